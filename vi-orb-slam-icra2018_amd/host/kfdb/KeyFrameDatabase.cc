// KeyFrameDatabase.cc -- host side of the drop-in ORB_SLAM2::KeyFrameDatabase (include/orbhip/KeyFrameDatabase.h).
// orbhip_kfdb_score does the part of each query that walks the inverted file (ref: src/KeyFrameDatabase.cc:82-137 loop,
// :203-239 reloc); the rest below follows the reference line for line on the KeyFrame objects.
#include "KeyFrameDatabase.h"

#include <cstdint>

#include "hiperror.h"
#include "orbhip.h"

namespace ORB_SLAM2
{

namespace
{
const int kMaxKeyFrames = 1 << 20;
int g_kfdb_device = 0;

struct Shared {
    std::vector<uint64_t> keys;
    std::vector<int32_t> counts;
    std::vector<float> scores;
    int minCommon = 0;
};

void flatten(const DBoW2::BowVector &v, std::vector<uint32_t> &w, std::vector<double> &x)
{
    w.clear();
    x.clear();
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
        w.push_back((uint32_t)it->first);
        x.push_back(it->second);
    }
}
}  // namespace

void KeyFrameDatabase::SetDevice(int device) { g_kfdb_device = device; }

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc), mpCtx(NULL)
{
    // a context of its own (see the header): the smallest extractor configuration, whose buffers are never used here
    mpCtx = orbhip_create(g_kfdb_device, 50, 1.2f, 1, 20, 7, 128, 128, 1);
    if (!mpCtx) {
        hipdetail::Fail("KeyFrameDatabase (device context)", orbhip_last_error(NULL));
        return;
    }
    if (orbhip_kfdb_init(mpCtx, (int)voc.size(), kMaxKeyFrames, 0) != ORBHIP_OK) {
        hipdetail::Fail("KeyFrameDatabase (orbhip_kfdb_init)", orbhip_last_error(mpCtx));
        orbhip_destroy(mpCtx);
        mpCtx = NULL;
    }
}

KeyFrameDatabase::~KeyFrameDatabase()
{
    if (mpCtx) orbhip_destroy(mpCtx);
}

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    std::vector<uint32_t> w;
    std::vector<double> x;
    flatten(pKF->mBowVec, w, x);
    if (orbhip_kfdb_add(mpCtx, pKF->mnId, w.data(), x.data(), (int)w.size()) != ORBHIP_OK) {
        hipdetail::Fail("KeyFrameDatabase::add", orbhip_last_error(mpCtx));
        return;
    }
    mmKFs[pKF->mnId] = pKF;
}

void KeyFrameDatabase::erase(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    std::map<long unsigned int, KeyFrame *>::iterator it = mmKFs.find(pKF->mnId);
    if (it == mmKFs.end() || it->second != pKF) return;
    if (orbhip_kfdb_erase(mpCtx, pKF->mnId) != ORBHIP_OK) {
        hipdetail::Fail("KeyFrameDatabase::erase", orbhip_last_error(mpCtx));
        return;
    }
    mmKFs.erase(it);
}

void KeyFrameDatabase::clear()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    if (orbhip_kfdb_clear(mpCtx) != ORBHIP_OK) hipdetail::Fail("KeyFrameDatabase::clear", orbhip_last_error(mpCtx));
    mmKFs.clear();
}

// the device half of one query: every key frame met, in the reference's order, with its count and score
static bool query(orbhip_ctx *ctx, int mode, const DBoW2::BowVector &bow, const std::vector<uint64_t> &excluded, size_t nkfs,
                  Shared &S, const char *who)
{
    std::vector<uint32_t> w;
    std::vector<double> x;
    flatten(bow, w, x);
    const int cap = (int)nkfs + 1;
    S.keys.resize(cap);
    S.counts.resize(cap);
    S.scores.resize(cap);
    int n = 0;
    if (orbhip_kfdb_score(ctx, mode, w.data(), x.data(), (int)w.size(), excluded.data(), (int)excluded.size(), S.keys.data(),
                          S.counts.data(), S.scores.data(), cap, &n, &S.minCommon) != ORBHIP_OK)
        return hipdetail::Fail(who, orbhip_last_error(ctx));
    S.keys.resize(n);
    return true;
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectLoopCandidates(KeyFrame *pKF, float minScore)
{
    std::set<KeyFrame *> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::vector<KeyFrame *> lKFsSharingWords;
    Shared S;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!mpCtx) return std::vector<KeyFrame *>();
        std::vector<uint64_t> excluded;
        for (std::set<KeyFrame *>::iterator it = spConnectedKeyFrames.begin(); it != spConnectedKeyFrames.end(); ++it)
            excluded.push_back((*it)->mnId);
        if (!query(mpCtx, ORBHIP_KFDB_LOOP, pKF->mBowVec, excluded, mmKFs.size(), S, "KeyFrameDatabase::DetectLoopCandidates"))
            return std::vector<KeyFrame *>();
        // ref :88-103: a connected key frame met is reset and counted on every visit (mnLoopWords ends at 1); the others
        // are stamped with the query and counted
        for (size_t i = 0; i < S.keys.size(); i++) {
            KeyFrame *pKFi = mmKFs[S.keys[i]];
            if (spConnectedKeyFrames.count(pKFi)) {
                pKFi->mnLoopWords = 1;
                continue;
            }
            pKFi->mnLoopQuery = pKF->mnId;
            pKFi->mnLoopWords = S.counts[i];
            lKFsSharingWords.push_back(pKFi);
        }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame *>();

    // ref :114-135: scores of the key frames with more than minCommonWords shared words (computed on the device)
    const int minCommonWords = S.minCommon;
    std::vector<std::pair<float, KeyFrame *> > lScoreAndMatch;
    for (size_t i = 0, j = 0; i < S.keys.size(); i++) {
        KeyFrame *pKFi = mmKFs[S.keys[i]];
        if (j >= lKFsSharingWords.size() || lKFsSharingWords[j] != pKFi) continue;   // a connected key frame
        j++;
        if (pKFi->mnLoopWords > minCommonWords) {
            const float si = S.scores[i];
            pKFi->mLoopScore = si;
            if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
        }
    }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame *>();

    std::vector<std::pair<float, KeyFrame *> > lAccScoreAndMatch;
    float bestAccScore = minScore;
    for (size_t i = 0; i < lScoreAndMatch.size(); i++) {                     // ref :144-172
        KeyFrame *pKFi = lScoreAndMatch[i].second;
        std::vector<KeyFrame *> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
        float bestScore = lScoreAndMatch[i].first;
        float accScore = lScoreAndMatch[i].first;
        KeyFrame *pBestKF = pKFi;
        for (size_t k = 0; k < vpNeighs.size(); k++) {
            KeyFrame *pKF2 = vpNeighs[k];
            if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
                accScore += pKF2->mLoopScore;
                if (pKF2->mLoopScore > bestScore) {
                    pBestKF = pKF2;
                    bestScore = pKF2->mLoopScore;
                }
            }
        }
        lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        if (accScore > bestAccScore) bestAccScore = accScore;
    }

    const float minScoreToRetain = 0.75f * bestAccScore;                     // ref :174-196
    std::set<KeyFrame *> spAlreadyAddedKF;
    std::vector<KeyFrame *> vpLoopCandidates;
    vpLoopCandidates.reserve(lAccScoreAndMatch.size());
    for (size_t i = 0; i < lAccScoreAndMatch.size(); i++) {
        if (lAccScoreAndMatch[i].first > minScoreToRetain) {
            KeyFrame *pKFi = lAccScoreAndMatch[i].second;
            if (!spAlreadyAddedKF.count(pKFi)) {
                vpLoopCandidates.push_back(pKFi);
                spAlreadyAddedKF.insert(pKFi);
            }
        }
    }
    return vpLoopCandidates;
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)
{
    std::vector<KeyFrame *> lKFsSharingWords;
    Shared S;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (!mpCtx) return std::vector<KeyFrame *>();
        if (!query(mpCtx, ORBHIP_KFDB_RELOC, F->mBowVec, std::vector<uint64_t>(), mmKFs.size(), S,
                   "KeyFrameDatabase::DetectRelocalizationCandidates"))
            return std::vector<KeyFrame *>();
        for (size_t i = 0; i < S.keys.size(); i++) {                         // ref :209-224
            KeyFrame *pKFi = mmKFs[S.keys[i]];
            pKFi->mnRelocQuery = F->mnId;
            pKFi->mnRelocWords = S.counts[i];
            lKFsSharingWords.push_back(pKFi);
        }
    }
    if (lKFsSharingWords.empty()) return std::vector<KeyFrame *>();

    const int minCommonWords = S.minCommon;                                   // ref :226-239
    std::vector<std::pair<float, KeyFrame *> > lScoreAndMatch;
    for (size_t i = 0; i < lKFsSharingWords.size(); i++) {
        KeyFrame *pKFi = lKFsSharingWords[i];
        if (pKFi->mnRelocWords > minCommonWords) {
            const float si = S.scores[i];
            pKFi->mRelocScore = si;
            lScoreAndMatch.push_back(std::make_pair(si, pKFi));
        }
    }
    if (lScoreAndMatch.empty()) return std::vector<KeyFrame *>();

    std::vector<std::pair<float, KeyFrame *> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (size_t i = 0; i < lScoreAndMatch.size(); i++) {                     // ref :241-272
        KeyFrame *pKFi = lScoreAndMatch[i].second;
        std::vector<KeyFrame *> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
        float bestScore = lScoreAndMatch[i].first;
        float accScore = bestScore;
        KeyFrame *pBestKF = pKFi;
        for (size_t k = 0; k < vpNeighs.size(); k++) {
            KeyFrame *pKF2 = vpNeighs[k];
            if (pKF2->mnRelocQuery != F->mnId) continue;
            accScore += pKF2->mRelocScore;                                    // stale when pKF2 was not scored now
            if (pKF2->mRelocScore > bestScore) {
                pBestKF = pKF2;
                bestScore = pKF2->mRelocScore;
            }
        }
        lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        if (accScore > bestAccScore) bestAccScore = accScore;
    }

    const float minScoreToRetain = 0.75f * bestAccScore;                     // ref :274-307
    std::set<KeyFrame *> spAlreadyAddedKF;
    std::vector<KeyFrame *> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (size_t i = 0; i < lAccScoreAndMatch.size(); i++) {
        const float &si = lAccScoreAndMatch[i].first;
        if (si > minScoreToRetain) {
            KeyFrame *pKFi = lAccScoreAndMatch[i].second;
            if (!spAlreadyAddedKF.count(pKFi)) {
                vpRelocCandidates.push_back(pKFi);
                spAlreadyAddedKF.insert(pKFi);
            }
        }
    }
    return vpRelocCandidates;
}

}  // namespace ORB_SLAM2
