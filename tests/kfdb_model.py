"""Plain-Python restatement of src/KeyFrameDatabase.cc and DBoW2's L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-67): the yardstick of the device key-frame database.  Lists for the inverted
file, key-frame objects with the six query fields, float32 narrowing exactly where the reference narrows (float si, float
accScore / bestScore / bestAccScore, 0.8f and 0.75f products).

Divergences of the port that the model states the same way (include/orbhip.h): every query is a fresh query (the query id is
a counter of the model), a key frame that was never scored has mRelocScore 0, excluded keys are honoured in both modes."""
import numpy as np

f32 = np.float32


class KF:
    def __init__(self, key, words, values):
        self.key = key
        self.bow = (list(int(w) for w in words), list(float(v) for v in values))
        self.covis = []                      # GetBestCovisibilityKeyFrames(10), as KF objects
        self.mnLoopQuery = self.mnLoopWords = 0
        self.mLoopScore = f32(0)
        self.mnRelocQuery = self.mnRelocWords = 0
        self.mRelocScore = f32(0)


def l1_score(v1, v2):
    """ScoringObject.cpp:23-67 -- double sum over the common words in ascending id, then -score/2.0."""
    (w1, x1), (w2, x2) = v1, v2
    i = j = 0
    score = 0.0
    while i < len(w1) and j < len(w2):
        if w1[i] == w2[j]:
            vi, wi = x1[i], x2[j]
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i += 1
        else:
            j += 1
    return -score / 2.0


def min_common(max_common):
    return int(f32(max_common) * f32(0.8))          # int minCommonWords = maxCommonWords*0.8f;


class Model:
    def __init__(self, nwords):
        self.nwords = nwords
        self.inv = [[] for _ in range(nwords)]
        self._qid = 0

    def add(self, kf):                              # :40-46
        for w in kf.bow[0]:
            self.inv[w].append(kf)

    def erase(self, kf):                            # :48-68
        for w in kf.bow[0]:
            lst = self.inv[w]
            for i, k in enumerate(lst):
                if k is kf:
                    del lst[i]
                    break

    def clear(self):                                # :70-74
        self.inv = [[] for _ in range(self.nwords)]

    def _next_id(self, qid=None):
        """the query id: Frame::mnId / KeyFrame::mnId when the caller gives one, else a fresh counter value"""
        if qid is not None:
            return qid
        self._qid += 1
        return self._qid

    def loop_shared(self, bow, connected, qid=None):
        """:82-104 -- the query id and lKFsSharingWords"""
        qid = self._next_id(qid)
        shared = []
        for w in bow[0]:
            for k in self.inv[w]:
                if k.mnLoopQuery != qid:
                    k.mnLoopWords = 0
                    if k not in connected:
                        k.mnLoopQuery = qid
                        shared.append(k)
                k.mnLoopWords += 1
        return qid, shared

    def detect_loop(self, bow, connected, min_score, qid=None):
        """DetectLoopCandidates (:78-197); connected: the query's GetConnectedKeyFrames() (KF objects)."""
        min_score = f32(min_score)
        qid, shared = self.loop_shared(bow, connected, qid)
        if not shared:
            return []
        maxc = max(k.mnLoopWords for k in shared)
        minc = min_common(maxc)
        lsm = []
        for k in shared:
            if k.mnLoopWords > minc:
                si = f32(l1_score(bow, k.bow))
                k.mLoopScore = si
                if si >= min_score:
                    lsm.append((si, k))
        if not lsm:
            return []
        acc_list = []
        best_acc = min_score
        for si, k in lsm:
            best_score = si
            acc = si
            best = k
            for k2 in k.covis[:10]:
                if k2.mnLoopQuery == qid and k2.mnLoopWords > minc:
                    acc = f32(acc + k2.mLoopScore)
                    if k2.mLoopScore > best_score:
                        best = k2
                        best_score = k2.mLoopScore
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return _retain(acc_list, best_acc)

    def reloc_shared(self, bow, qid=None):
        """:205-224 -- the query id and lKFsSharingWords"""
        qid = self._next_id(qid)
        shared = []
        for w in bow[0]:
            for k in self.inv[w]:
                if k.mnRelocQuery != qid:
                    k.mnRelocWords = 0
                    k.mnRelocQuery = qid
                    shared.append(k)
                k.mnRelocWords += 1
        return qid, shared

    def detect_reloc(self, bow, qid=None):
        """DetectRelocalizationCandidates (:199-311), including the stale mRelocScore of unscored neighbours (:251-256)."""
        qid, shared = self.reloc_shared(bow, qid)
        if not shared:
            return []
        maxc = max(k.mnRelocWords for k in shared)
        minc = min_common(maxc)
        lsm = []
        for k in shared:
            if k.mnRelocWords > minc:
                si = f32(l1_score(bow, k.bow))
                k.mRelocScore = si
                lsm.append((si, k))
        if not lsm:
            return []
        acc_list = []
        best_acc = f32(0)
        for si, k in lsm:
            best_score = si
            acc = si
            best = k
            for k2 in k.covis[:10]:
                if k2.mnRelocQuery != qid:
                    continue
                acc = f32(acc + k2.mRelocScore)
                if k2.mRelocScore > best_score:
                    best = k2
                    best_score = k2.mRelocScore
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return _retain(acc_list, best_acc)

    def score(self, mode, bow, excluded=()):
        """What orbhip_kfdb_score returns: [(key, count, score or 0)], minCommon; reloc mode writes mRelocScore."""
        if mode == 1:
            qid, shared = self.loop_shared(bow, excluded)
            met = []
            seen = set()
            for w in bow[0]:                       # excluded ones too, at the place they were first met
                for k in self.inv[w]:
                    if id(k) not in seen:
                        seen.add(id(k))
                        met.append(k)
            cnt = {id(k): sum(1 for w in bow[0] if w in set(k.bow[0])) for k in met}
        else:
            qid, shared = self.reloc_shared(bow)
            met = shared
            cnt = {id(k): k.mnRelocWords for k in met}
        cand = [k for k in met if k not in excluded]
        minc = min_common(max([cnt[id(k)] for k in cand], default=0))
        out = []
        for k in met:
            c = cnt[id(k)]
            s = f32(0)
            if k not in excluded and c > minc:
                s = f32(l1_score(bow, k.bow))
                if mode == 0:
                    k.mRelocScore = s
                else:
                    k.mLoopScore = s
            out.append((k.key, c, s))
        return out, minc


def _retain(acc_list, best_acc):
    """:174-196 / :269-307: accScore > 0.75f*bestAccScore, first occurrence of pBestKF."""
    th = f32(f32(0.75) * f32(best_acc))
    out, seen = [], set()
    for acc, k in acc_list:
        if acc > th and id(k) not in seen:
            out.append(k)
            seen.add(id(k))
    return out
