// ref_bowcand.h -- what LocalMapSearch::SearchByBoWCandidates must reproduce, written out on the slamlite.h objects: the two
// ORBmatcher::SearchByBoW loops (ref: src/ORBmatcher.cc:159-288, :522-655) with the rotation check and ComputeThreeMaxima
// (:1629-1670), and the walk of the PnPsolver constructor with the mvMaxError loop of SetRansacParameters (ref:
// src/PnPsolver.cc:78-101, :154-156).  Host code only; test_bowcand.cpp runs it on the twin map.
#ifndef TESTS_REF_BOWCAND_H
#define TESTS_REF_BOWCAND_H

#include <cmath>
#include <vector>

#include "LocalMap.h"

namespace refbow
{
using namespace ORB_SLAM2;

const int HISTO_LENGTH = 30;

inline int distance(const unsigned char *a, const unsigned char *b)
{
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

inline void three_maxima(const std::vector<int> *histo, int L, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) {
            max3 = max2, max2 = max1, max1 = s;
            ind3 = ind2, ind2 = ind1, ind1 = i;
        } else if (s > max2) {
            max3 = max2, max2 = s;
            ind3 = ind2, ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1)
        ind2 = -1, ind3 = -1;
    else if (max3 < 0.1f * (float)max1)
        ind3 = -1;
}

inline int rot_bin(float a1, float a2)
{
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// one node of either loop: the best and the second best distance of d1 among the open features of the list
template <class Open>
inline void best_two(const unsigned char *d1, const cv::Mat &D2, const std::vector<unsigned int> &list, Open open, int &b1, int &b2, int &bi)
{
    b1 = 256, b2 = 256, bi = -1;
    for (size_t k = 0; k < list.size(); k++) {
        const int i2 = (int)list[k];
        if (!open(i2)) continue;
        const int d = distance(d1, D2.ptr(i2));
        if (d < b1)
            b2 = b1, b1 = d, bi = i2;
        else if (d < b2)
            b2 = d;
    }
}

struct OpenInFrame {
    const std::vector<MapPoint *> *m;
    bool operator()(int i) const { return !(*m)[i]; }
};
struct OpenInKeyFrame {
    const std::vector<bool> *matched;
    const std::vector<MapPoint *> *pts;
    bool operator()(int i) const { return !(*matched)[i] && (*pts)[i] && !(*pts)[i]->isBad(); }
};

inline int SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint *> &vpMapPointMatches, float nnratio, bool checkOri, int TH_LOW = 50)
{
    const std::vector<MapPoint *> vpMapPointsKF = pKF->GetMapPointMatches();
    vpMapPointMatches = std::vector<MapPoint *>(F.N, static_cast<MapPoint *>(NULL));
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    DBoW2::FeatureVector::const_iterator KFit = pKF->mFeatVec.begin(), Fit = F.mFeatVec.begin();
    while (KFit != pKF->mFeatVec.end() && Fit != F.mFeatVec.end()) {
        if (KFit->first == Fit->first) {
            for (size_t iKF = 0; iKF < KFit->second.size(); iKF++) {
                const unsigned int realIdxKF = KFit->second[iKF];
                MapPoint *pMP = vpMapPointsKF[realIdxKF];
                if (!pMP || pMP->isBad()) continue;
                int b1, b2, bi;
                const OpenInFrame open = {&vpMapPointMatches};
                best_two(pKF->mDescriptors.ptr((int)realIdxKF), F.mDescriptors, Fit->second, open, b1, b2, bi);
                if (b1 <= TH_LOW && (float)b1 < nnratio * (float)b2) {
                    vpMapPointMatches[bi] = pMP;
                    if (checkOri) rotHist[rot_bin(pKF->mvKeysUn[realIdxKF].angle, F.mvKeys[bi].angle)].push_back(bi);
                    nmatches++;
                }
            }
            ++KFit, ++Fit;
        } else if (KFit->first < Fit->first)
            KFit = pKF->mFeatVec.lower_bound(Fit->first);
        else
            Fit = F.mFeatVec.lower_bound(KFit->first);
    }
    if (checkOri) {
        int i1, i2, i3;
        three_maxima(rotHist, HISTO_LENGTH, i1, i2, i3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == i1 || i == i2 || i == i3) continue;
            for (size_t j = 0; j < rotHist[i].size(); j++) vpMapPointMatches[rotHist[i][j]] = static_cast<MapPoint *>(NULL), nmatches--;
        }
    }
    return nmatches;
}

inline int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, float nnratio, bool checkOri, int TH_LOW = 50)
{
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    vpMatches12 = std::vector<MapPoint *>(vpMapPoints1.size(), static_cast<MapPoint *>(NULL));
    std::vector<bool> vbMatched2(vpMapPoints2.size(), false);
    std::vector<int> rotHist[HISTO_LENGTH];
    int nmatches = 0;
    DBoW2::FeatureVector::const_iterator f1it = pKF1->mFeatVec.begin(), f2it = pKF2->mFeatVec.begin();
    while (f1it != pKF1->mFeatVec.end() && f2it != pKF2->mFeatVec.end()) {
        if (f1it->first == f2it->first) {
            for (size_t i1 = 0; i1 < f1it->second.size(); i1++) {
                const size_t idx1 = f1it->second[i1];
                MapPoint *pMP1 = vpMapPoints1[idx1];
                if (!pMP1 || pMP1->isBad()) continue;
                int b1, b2, bi;
                const OpenInKeyFrame open = {&vbMatched2, &vpMapPoints2};
                best_two(pKF1->mDescriptors.ptr((int)idx1), pKF2->mDescriptors, f2it->second, open, b1, b2, bi);
                if (b1 < TH_LOW && (float)b1 < nnratio * (float)b2) {
                    vpMatches12[idx1] = vpMapPoints2[bi];
                    vbMatched2[bi] = true;
                    if (checkOri) rotHist[rot_bin(pKF1->mvKeysUn[idx1].angle, pKF2->mvKeysUn[bi].angle)].push_back((int)idx1);
                    nmatches++;
                }
            }
            ++f1it, ++f2it;
        } else if (f1it->first < f2it->first)
            f1it = pKF1->mFeatVec.lower_bound(f2it->first);
        else
            f2it = pKF2->mFeatVec.lower_bound(f1it->first);
    }
    if (checkOri) {
        int i1, i2, i3;
        three_maxima(rotHist, HISTO_LENGTH, i1, i2, i3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == i1 || i == i2 || i == i3) continue;
            for (size_t j = 0; j < rotHist[i].size(); j++) vpMatches12[rotHist[i][j]] = static_cast<MapPoint *>(NULL), nmatches--;
        }
    }
    return nmatches;
}

// PnPsolver::PnPsolver(F, vpMapPointMatches) and mvMaxError[i] = mvSigma2[i] * th2
inline void PnPSetup(Frame &F, const std::vector<MapPoint *> &vpMapPointMatches, float th2, RelocCorrespondences &out)
{
    out = RelocCorrespondences();
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeysUn[i];
        out.mvP2D.push_back(kp.pt);
        out.mvMaxError.push_back(F.mvLevelSigma2[kp.octave] * th2);
        const cv::Mat Pos = pMP->GetWorldPos();
        out.mvP3Dw.push_back(cv::Point3f(Pos.at<float>(0, 0), Pos.at<float>(1, 0), Pos.at<float>(2, 0)));
        out.mvKeyPointIndices.push_back(i);
    }
}
}  // namespace refbow

#endif
