// KeyFrameDatabase.h -- drop-in for the reference's include/KeyFrameDatabase.h (src/KeyFrameDatabase.cc): the BoW inverted
// file that relocalisation (src/Tracking.cc:2573) and loop detection (src/LoopClosing.cc:193) query.  Same class name,
// namespace and public methods.  The inverted file, the shared-word counts and the L1 scores live in liborbhip.so
// (orbhip_kfdb_*, include/orbhip.h); the body (vi-orb-slam-icra2018_amd/host/kfdb/KeyFrameDatabase.cc) writes the query fields
// of the key frames it met (mnLoopQuery / mnLoopWords / mLoopScore, mnRelocQuery / mnRelocWords / mRelocScore) and runs the
// covisibility accumulation on the host over GetBestCovisibilityKeyFrames(10), as the reference does -- so inside the
// reference tree (ORBHIP_WITH_REFERENCE_HEADERS) the results equal the reference's, stale mRelocScore included.
//
// Divergences (include/orbhip.h, "key-frame database"): add of a key frame already present is refused (the reference would
// list it twice); a query id asked twice counts as a fresh query.  Key frames are named by KeyFrame::mnId.  A failed device
// call returns no candidates (include/orbhip/hiperror.h).
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <map>
#include <mutex>
#include <set>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"
#else
#include "slamlite.h"
#include "ORBVocabulary.h"
#endif

struct orbhip_ctx;

namespace ORB_SLAM2
{

class KeyFrame;
class Frame;

class KeyFrameDatabase
{
public:
    KeyFrameDatabase(const ORBVocabulary &voc);
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    void add(KeyFrame *pKF);

    void erase(KeyFrame *pKF);

    void clear();

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);

    // Relocalization
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);

    // device of the databases constructed from now on (default 0; no counterpart in the reference, as
    // ORBVocabulary::SetDevice)
    static void SetDevice(int device);

protected:
    // Associated vocabulary
    const ORBVocabulary *mpVoc;

    // the device database and the key frames it holds, by mnId.  The database has a context of its own (the smallest an
    // orbhip_create makes, a few MB): a context is not re-entrant, and Tracking queries the database while LocalMapping
    // and LoopClosing use the vocabulary's and the extractors' contexts on other threads.
    orbhip_ctx *mpCtx;
    std::map<long unsigned int, KeyFrame *> mmKFs;

    // Mutex
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
