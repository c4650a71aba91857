"""Independent model of Tracking::UpdateLocalMap's two loops (ref: src/Tracking.cc:2377-2400 UpdateLocalPoints, :2411-2429 the
vote of UpdateLocalKeyFrames), written from the reference on dicts and lists: every map point carries its observation map
(key frame -> feature index) as MapPoint::mObservations does, the vote walks those maps, and the union stamps the points it
has taken as mnTrackReferenceForFrame does.  It does not sum over key-frame rows: that is the formulation of the kernel under
test.  Keys stand for pointers; 0 is NULL."""


class World:
    """Map points and key frames kept consistent the way the reference's mutators keep them: (KF, idx) is an observation of a
    point iff KF's mvpMapPoints[idx] is that point."""

    def __init__(self):
        self.points = {}     # key -> {"bad": bool, "obs": {kf_key: idx}}
        self.kfs = {}        # kf_key -> list of point keys (mvpMapPoints), 0 = NULL

    def add_point(self, key, bad=False):
        assert key and key not in self.points
        self.points[key] = {"bad": bool(bad), "obs": {}}

    def set_bad(self, key, bad=True):
        self.points[key]["bad"] = bool(bad)

    def put_kf(self, kf, row):
        """KeyFrame construction / a whole new mvpMapPoints: AddObservation for every point of it."""
        self.erase_kf(kf)
        row = [int(k) for k in row]
        assert len(set(k for k in row if k)) == len([k for k in row if k]), "a point twice in one key frame"
        self.kfs[kf] = row
        for idx, k in enumerate(row):
            if k:
                self.points[k]["obs"][kf] = idx

    def set_entry(self, kf, idx, key):
        """AddMapPoint + AddObservation (key != 0) / EraseMapPointMatch + EraseObservation (key == 0)."""
        old = self.kfs[kf][idx]
        if old and old in self.points:
            del self.points[old]["obs"][kf]
        self.kfs[kf][idx] = int(key)
        if key:
            assert kf not in self.points[key]["obs"]
            self.points[key]["obs"][kf] = idx

    def erase_kf(self, kf):
        for k in self.kfs.pop(kf, []):
            if k and k in self.points:
                del self.points[k]["obs"][kf]

    def erase_point(self, key):
        """SetBadFlag to its end: every key frame that observed the point forgets it, the point leaves the map."""
        for kf, idx in self.points.pop(key)["obs"].items():
            self.kfs[kf][idx] = 0

    def clear_points(self):
        for key in list(self.points):
            self.erase_point(key)


def vote(world, frame_point_keys):
    """keyframeCounter of UpdateLocalKeyFrames as (kf_key, count) in ascending key order (the canonical order of the map)."""
    counter = {}
    for key in frame_point_keys:
        key = int(key)
        if not key:
            continue
        mp = world.points.get(key)
        if mp is None or mp["bad"]:      # (a bad point is set to NULL in the frame; a point the map forgot has no observations)
            continue
        for kf in mp["obs"]:
            counter[kf] = counter.get(kf, 0) + 1
    return sorted(counter.items())


def collect(world, kf_keys):
    """mvpLocalMapPoints of UpdateLocalPoints for mvpLocalKeyFrames = kf_keys."""
    stamped = set()                      # the points with mnTrackReferenceForFrame == mCurrentFrame.mnId
    out = []
    for kf in kf_keys:
        for key in world.kfs[int(kf)]:   # GetMapPointMatches()
            if not key:
                continue
            if key in stamped:
                continue
            if not world.points[key]["bad"]:
                out.append(key)
                stamped.add(key)
    return out


def skip_bytes(local_keys, seen_keys):
    """mnLastFrameSeen == mCurrentFrame.mnId for the points of the list: the frame's own matches."""
    seen = set(int(k) for k in seen_keys)
    return [1 if int(k) in seen else 0 for k in local_keys]
