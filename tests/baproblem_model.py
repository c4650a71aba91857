"""Independent model of the set-up of Optimizer::LocalBundleAdjustment (ref: src/Optimizer.cc:2786-2802 lLocalMapPoints,
:2804-2820 lFixedCameras, :2888 ff. one edge per observation), written on the observation maps of
tests/localmap_collect_model.py's World: the points are stamped as mnBALocalForKF stamps them, the fixed key frames are found by
walking every local point's own key frame -> index map, and the edges by walking it again.  It does not sweep key-frame rows and
counts nothing: that is the formulation of the kernels under test.  Keys stand for pointers; 0 is NULL.  The reference's
map<KeyFrame*, size_t> iterates by heap address; the canonical stand-in is ascending key (docs/parity.md).

`defect` names one deliberate mistake (tests/test_baproblem_model.py shows that each changes a scene):
  "row_order"       a point's observers in the order of `row_of` (the table's rows) instead of ascending key
  "keep_bad"        a bad point is taken
  "stale"           the observations in `ghosts` ((point key, key frame, index): what an entry that outlived its point would
                    name if the slot's generation were not compared) are observations
  "local_as_fixed"  the last local key frame is not recognised as local
  "fixed_by_key"    the fixed key frames in ascending key instead of first appearance
  "double_local"    a local key given twice is numbered by its last occurrence
  "local_only"      only local key frames observe"""

DEFECTS = ("row_order", "keep_bad", "stale", "local_as_fixed", "fixed_by_key", "double_local", "local_only")


def ba_problem(world, kf_keys, defect=None, row_of=None, ghosts=()):
    """(point_keys, edge_off, edges [(kf, idx)], fixed_keys) as orbhip_map_ba_problem returns them."""
    assert defect is None or defect in DEFECTS
    kf_keys = [int(k) for k in kf_keys]
    nkf = len(kf_keys)
    local = {}                                           # mnBALocalForKF == pKF->mnId, with the place in the caller's list
    for k, kf in enumerate(kf_keys):
        if kf not in local or defect == "double_local":
            local[kf] = k
    if defect == "local_as_fixed" and nkf > 1:
        del local[kf_keys[-1]]

    points, stamped = [], set()                          # :2786-2802
    for kf in kf_keys:
        for key in world.kfs[kf]:                        # GetMapPointMatches()
            if not key:
                continue
            mp = world.points.get(key)
            if mp is None or (mp["bad"] and defect != "keep_bad"):
                continue
            if key not in stamped:
                points.append(key)
                stamped.add(key)

    def observations(key):                               # GetObservations(), in the map's order
        obs = dict(world.points[key]["obs"])
        if defect == "stale":
            for gkey, gkf, gidx in ghosts:
                if gkey == key and gkf in world.kfs:
                    obs[gkf] = gidx
        if defect == "local_only":
            obs = {kf: i for kf, i in obs.items() if kf in local}
        order = sorted(obs, key=(lambda kf: row_of[kf]) if defect == "row_order" else None)
        return [(kf, obs[kf]) for kf in order]

    fixed, fixed_at = [], {}                             # :2804-2820
    for key in points:
        for kfi, _ in observations(key):
            if kfi not in local and kfi not in fixed_at:     # mnBALocalForKF != id && mnBAFixedForKF != id
                fixed_at[kfi] = len(fixed)
                fixed.append(kfi)
    if defect == "fixed_by_key":
        fixed = sorted(fixed)
        fixed_at = {kf: r for r, kf in enumerate(fixed)}

    edges, off = [], [0]                                 # :2888 ff.
    for key in points:
        for kfi, idx in observations(key):
            edges.append((local[kfi] if kfi in local else nkf + fixed_at[kfi], idx))
        off.append(len(edges))
    return points, off, edges, fixed
