// LocalMapCorrect.cc -- LocalMapSearch::CorrectLoopPoints and ApplyGlobalBA (include/orbhip/LocalMap.h): the point loops of
// LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-568) and LoopClosing::RunGlobalBundleAdjustment (ref: :762-797) as one
// orbhip_map_correct_sim3 / orbhip_map_correct_se3 call each on the resident store, the results assigned to
// the caller's objects.  Points the calls cannot serve go the way that existed before them: the arithmetic on the host, at the
// point's turn in the sequence, then one Put.  A file of its own: programs that link the other LocalMap*.cc files alone do not need
// the entry points.
#include <algorithm>
#include <cstring>
#include <map>
#include <unordered_map>
#include <unordered_set>

#include "LocalMapDetail.h"
#include "../MatcherDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::key_of;

namespace
{
// g2o::Sim3::map (ref: Thirdparty/g2o/g2o/types/sim3.h:144), s*(r*xyz)+t with Eigen 3's Quaternion::_transformVector, every
// operation rounded on its own (docs/parity.md, "CorrectLoop"; this file is built with -ffp-contract=off)
void sim3_map(const LocalMapSearch::Sim3d &S, double v[3])
{
    const double qx = S.q[0], qy = S.q[1], qz = S.q[2], qw = S.q[3], x = v[0], y = v[1], z = v[2];
    double ux = qy * z - qz * y, uy = qz * x - qx * z, uz = qx * y - qy * x;
    ux += ux, uy += uy, uz += uz;
    const double rx = (x + qw * ux) + (qy * uz - qz * uy);
    const double ry = (y + qw * uy) + (qz * ux - qx * uz);
    const double rz = (z + qw * uz) + (qx * uy - qy * ux);
    v[0] = S.s * rx + S.t[0], v[1] = S.s * ry + S.t[1], v[2] = S.s * rz + S.t[2];
}

cv::Mat vec3(const float *p)
{
    cv::Mat m(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) m.at<float>(c, 0) = p[c];
    return m;
}

// the reference's lines :544-552 for one point, on the objects as they stand
void correct_on_host(MapPoint *p, const LocalMapSearch::LoopCorrection &L)
{
    const cv::Mat P = p->GetWorldPos();
    double v[3] = {(double)P.at<float>(0, 0), (double)P.at<float>(1, 0), (double)P.at<float>(2, 0)};
    sim3_map(L.Siw, v);
    sim3_map(L.correctedSwi, v);
    const float f[3] = {(float)v[0], (float)v[1], (float)v[2]};
    p->SetWorldPos(vec3(f));
    p->UpdateNormalAndDepth();
}

void copy_sim3(const LocalMapSearch::Sim3d &S, orbhip_sim3d *out)
{
    memcpy(out->q, S.q, sizeof out->q);
    memcpy(out->t, S.t, sizeof out->t);
    out->s = S.s;
}
}  // namespace

int LocalMapSearch::CorrectLoopPoints(const std::vector<LoopCorrection> &v, unsigned long nCurrentKFid)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx || v.empty()) return 0;
    localmapdetail::Stopwatch watch;
    const int K = (int)v.size();
    // the points in the sequence's order, each owned by the first key frame to reach it
    std::vector<MapPoint *> pts;
    std::vector<int> owner;
    std::unordered_map<KeyFrame *, int> rankOf;
    for (int j = 0; j < K; j++) {
        KeyFrame *pKFi = v[j].pKF;
        rankOf.insert(std::make_pair(pKFi, j));
        const std::vector<MapPoint *> vpMPsi = pKFi->GetMapPointMatches();
        for (size_t i = 0; i < vpMPsi.size(); i++) {
            MapPoint *p = vpMPsi[i];
            if (!p || p->isBad() || p->mnCorrectedByKF == nCurrentKFid) continue;
            p->mnCorrectedByKF = nCurrentKFid;
            p->mnCorrectedReference = pKFi->mnId;
            pts.push_back(p);
            owner.push_back(j);
        }
    }
    if (pts.empty()) {
        for (int j = 0; j < K; j++) v[j].pKF->SetPose(v[j].correctedTiw);
        return 0;
    }

    // what goes to the device: lists in ascending mnId, the observers with their centre now and after their SetPose
    KeyFrame *pyramid = v[0].pKF;
    const bool levelsOk = pyramid->mnScaleLevels >= 1 && pyramid->mnScaleLevels <= 16 && (int)pyramid->mvScaleFactors.size() >= pyramid->mnScaleLevels;
    std::unordered_map<KeyFrame *, int> kfIndex;
    std::vector<orbhip_correct_kf> kfs;
    std::vector<int> way(pts.size(), -1);   // position in the device batch, or -1: the host way
    std::vector<MapPoint *> dev;
    std::vector<uint64_t> keys;
    std::vector<int32_t> corr, off(1, 0), obsKf, refPos;
    std::vector<uint8_t> refLevel;
    for (size_t i = 0; i < pts.size() && levelsOk; i++) {
        MapPoint *p = pts[i];
        if (!Known(p)) continue;
        const localmapdetail::ObservationList l = localmapdetail::observations_by_mnid(p);
        int ref = -1, level = 0;
        for (size_t j = 0; j < l.size(); j++)
            if (l[j].first == p->mpRefKF) ref = (int)j;
        if (!l.empty()) {
            if (ref < 0 || l[ref].second >= p->mpRefKF->mvKeysUn.size()) continue;
            level = p->mpRefKF->mvKeysUn[l[ref].second].octave;
            if (level < 0 || level >= pyramid->mnScaleLevels) continue;
        }
        for (size_t j = 0; j < l.size(); j++) {
            KeyFrame *kf = l[j].first;
            std::unordered_map<KeyFrame *, int>::iterator it = kfIndex.find(kf);
            if (it == kfIndex.end()) {
                orbhip_correct_kf r;
                memset(&r, 0, sizeof r);
                const cv::Mat O = kf->GetCameraCenter();
                for (int c = 0; c < 3; c++) r.Ow_before[c] = r.Ow_after[c] = O.at<float>(c, 0);
                r.rank = -1;
                std::unordered_map<KeyFrame *, int>::const_iterator rk = rankOf.find(kf);
                if (rk != rankOf.end()) {
                    r.rank = rk->second;
                    const cv::Mat &T = v[rk->second].correctedTiw;   // Ow = -Rcw.t()*tcw, as SetPose will compute it
                    const float t[3] = {T.at<float>(0, 3), T.at<float>(1, 3), T.at<float>(2, 3)};
                    hipdetail::affine3(T.rowRange(0, 3).colRange(0, 3), t, NULL, r.Ow_after, true, -1.0);
                }
                it = kfIndex.insert(std::make_pair(kf, (int)kfs.size())).first;
                kfs.push_back(r);
            }
            obsKf.push_back(it->second);
        }
        way[i] = (int)dev.size();
        dev.push_back(p);
        keys.push_back(key_of(p));
        corr.push_back(owner[i]);
        off.push_back((int32_t)obsKf.size());
        refPos.push_back(std::max(ref, 0));
        refLevel.push_back((uint8_t)level);
    }

    std::vector<uint8_t> status;
    std::vector<float> pos, nrm, mn, mx;
    watch.lap(&CorrectTimes().prepare);
    if (!dev.empty()) {
        const int P = (int)dev.size();
        orbhip_refresh_params prm;
        localmapdetail::fill_refresh_params(pyramid, &prm);
        std::vector<orbhip_correct_xf> xf(K);
        for (int j = 0; j < K; j++) copy_sim3(v[j].Siw, &xf[j].Siw), copy_sim3(v[j].correctedSwi, &xf[j].corrected_Swi);
        status.resize(P), pos.resize((size_t)P * 3), nrm.resize((size_t)P * 3), mn.resize(P), mx.resize(P);
        if (orbhip_map_correct_sim3(mpCtx, &prm, K, xf.data(), (int)kfs.size(), kfs.data(), P, keys.data(), corr.data(), off.data(),
                                    obsKf.data(), refPos.data(), refLevel.data(), status.data(), pos.data(), nrm.data(), mn.data(),
                                    mx.data()) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::CorrectLoopPoints", orbhip_last_error(mpCtx));
            std::fill(way.begin(), way.end(), -1);   // the map stays right: these go the host way as well
        }
    }

    watch.lap(&CorrectTimes().device);
    // the sequence: key frame j's points, then its SetPose.  Device results do not depend on when they are assigned; a host point
    // reads the centres as they stand at its turn
    std::vector<MapPoint *> host;
    size_t i = 0;
    for (int j = 0; j < K; j++) {
        for (; i < pts.size() && owner[i] == j; i++) {
            MapPoint *p = pts[i];
            const int d = way[i];
            if (d < 0 || !(status[d] & 1)) {             // (status 0: the store holds the point as bad, the object is not)
                correct_on_host(p, v[j]);
                host.push_back(p);
                continue;
            }
            p->SetWorldPos(vec3(&pos[(size_t)d * 3]));
            if (status[d] & 2) AssignNormalDepth(p, &nrm[(size_t)d * 3], mn[d], mx[d]);
        }
        v[j].pKF->SetPose(v[j].correctedTiw);
    }
    if (!host.empty()) PutLocked(host);
    watch.lap(&CorrectTimes().apply);
    CorrectCounts().device += (long)(pts.size() - host.size());
    CorrectCounts().host += (long)host.size();
    return (int)pts.size();
}

int LocalMapSearch::ApplyGlobalBA(const std::vector<MapPoint *> &vpMPs, unsigned long nLoopKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return 0;
    localmapdetail::Stopwatch watch;
    std::unordered_set<MapPoint *> seen;
    seen.reserve(vpMPs.size());
    std::unordered_map<KeyFrame *, int> xfIndex;
    std::vector<orbhip_correct_se3> xf;
    std::vector<cv::Mat> before, inverse;     // per entry of xf, for the host way
    std::vector<MapPoint *> dev, host;
    std::vector<int> hostXf;
    std::vector<uint64_t> keys;
    std::vector<int32_t> corr;
    std::vector<float> posSet;
    bool given = false;
    long nDevice = 0;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *p = vpMPs[i];
        if (!p || p->isBad() || !seen.insert(p).second) continue;
        int c = -1;
        if (p->mnBAGlobalForKF != nLoopKF) {
            KeyFrame *pRefKF = p->GetReferenceKeyFrame();
            if (!pRefKF || pRefKF->mnBAGlobalForKF != nLoopKF) continue;
            std::unordered_map<KeyFrame *, int>::iterator it = xfIndex.find(pRefKF);
            if (it == xfIndex.end()) {
                orbhip_correct_se3 r;
                const cv::Mat Tb = pRefKF->mTcwBefGBA, Twc = pRefKF->GetPoseInverse();
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) r.Rcw_before[3 * a + b] = Tb.at<float>(a, b), r.Rwc[3 * a + b] = Twc.at<float>(a, b);
                    r.tcw_before[a] = Tb.at<float>(a, 3), r.twc[a] = Twc.at<float>(a, 3);
                }
                it = xfIndex.insert(std::make_pair(pRefKF, (int)xf.size())).first;
                xf.push_back(r);
                before.push_back(Tb), inverse.push_back(Twc);
            }
            c = it->second;
        }
        if (!Known(p)) {
            host.push_back(p), hostXf.push_back(c);
            continue;
        }
        dev.push_back(p);
        keys.push_back(key_of(p));
        corr.push_back(c);
        float g[3] = {0.f, 0.f, 0.f};
        if (c < 0) {
            for (int a = 0; a < 3; a++) g[a] = p->mPosGBA.at<float>(a, 0);
            given = true;
        }
        posSet.insert(posSet.end(), g, g + 3);
    }
    watch.lap(&CorrectTimes().prepare);
    if (!dev.empty()) {
        const int P = (int)dev.size();
        std::vector<uint8_t> status(P);
        std::vector<float> pos((size_t)P * 3);
        if (orbhip_map_correct_se3(mpCtx, (int)xf.size(), xf.data(), P, keys.data(), corr.data(), given ? posSet.data() : NULL, status.data(),
                                   pos.data()) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::ApplyGlobalBA", orbhip_last_error(mpCtx));
            for (int i = 0; i < P; i++) host.push_back(dev[i]), hostXf.push_back(corr[i]);
            watch.lap(&CorrectTimes().device);
        } else {
            watch.lap(&CorrectTimes().device);
            for (int i = 0; i < P; i++) {
                if (status[i] & 1) dev[i]->SetWorldPos(vec3(&pos[(size_t)i * 3])), nDevice++;
                else host.push_back(dev[i]), hostXf.push_back(corr[i]);   // (the store holds the point as bad, the object is not)
            }
        }
    }
    for (size_t i = 0; i < host.size(); i++) {   // the reference's lines :772-796 on the objects
        MapPoint *p = host[i];
        if (hostXf[i] < 0) {
            p->SetWorldPos(p->mPosGBA);
            continue;
        }
        const cv::Mat Tb = before[hostXf[i]], Twc = inverse[hostXf[i]], X = p->GetWorldPos();
        const float xw[3] = {X.at<float>(0, 0), X.at<float>(1, 0), X.at<float>(2, 0)};
        const float tcw[3] = {Tb.at<float>(0, 3), Tb.at<float>(1, 3), Tb.at<float>(2, 3)}, twc[3] = {Twc.at<float>(0, 3), Twc.at<float>(1, 3), Twc.at<float>(2, 3)};
        float xc[3], out[3];
        hipdetail::affine3(Tb.rowRange(0, 3).colRange(0, 3), xw, tcw, xc);       // Xc = Rcw*Xw + tcw
        hipdetail::affine3(Twc.rowRange(0, 3).colRange(0, 3), xc, twc, out);     // Rwc*Xc + twc
        p->SetWorldPos(vec3(out));
    }
    if (!host.empty()) PutLocked(host);
    watch.lap(&CorrectTimes().apply);
    CorrectCounts().device += nDevice;
    CorrectCounts().host += (long)host.size();
    return (int)(nDevice + (long)host.size());
}

}  // namespace ORB_SLAM2
