// k_bowcand.hip -- ORBmatcher::SearchByBoW of one fixed frame / key frame against K candidate key frames, every one a resident
// set whose "has a map point that is not bad" comes from its row of the key-frame table.
//   k_bow_match_cands   the grid runs over the shared vocabulary nodes of ALL candidates, one wave per {fixed-side node, candidate
//                       node, candidate}, four waves per block; the node body is bow_match_node (bow_match_dev.h), the one
//                       k_bow_match runs.  What differs from candidate to candidate sits in a table in device memory
//                       (BowCandDev) and comes in through scalar loads: the candidate index is wave-uniform (readfirstlane).
//                       MODE 0, SearchByBoW(pKF_k, F) (ref: src/ORBmatcher.cc:159-288): the candidate is side 1, the frame side 2
//                       (every feature counts), dist <= th.  MODE 1, SearchByBoW(pCurrentKF, pKF_k) (:522-655): the fixed key
//                       frame is side 1, the candidate side 2, both valid through their rows, dist < th.
//   k_bow_rot_cands     one wave per candidate: the 30-bin histogram of angle1 - angle2, ComputeThreeMaxima, the losers cleared,
//                       the count (bow_rot_dev.h, shared with k_bowseq.hip); writes the final row to the result block as well
//   k_pnp_gather_cands  MODE 0: one wave per candidate, the PnPsolver constructor's walk (ref: src/PnPsolver.cc:78-101) and the
//                       mvMaxError loop of SetRansacParameters (:154-156) as an ordered compaction by ballot and prefix
// Two arrays per candidate, both -1 on entry (a device memset): `out`, its row of [K][nFixed], indexed by the fixed side's
// features -- match21 in MODE 0, match12 in MODE 1, the row the caller gets --, and `scratch`, indexed by the candidate's
// features, the reverse.  Matches are a bijection between the two, so the rotation and gather kernels read `out` alone.
#include "orbhip_internal.h"
#include "bow_match_dev.h"
#include "bow_rot_dev.h"

template <int MODE>
__global__ __launch_bounds__(256) void k_bow_match_cands(const uint8_t *__restrict__ descF, const int32_t *__restrict__ offF,
                                                         const int32_t *__restrict__ idxF, const int2 *__restrict__ rowF,
                                                         const int nF, const BowCandDev *__restrict__ cands,
                                                         const BowCandPair *__restrict__ pairs, const int npairs,
                                                         const uint32_t *__restrict__ mflags, const int maxPoints, const int th,
                                                         const float nnratio, int32_t *__restrict__ out,
                                                         int32_t *__restrict__ scratch)
{
    __shared__ uint32_t s_claim[4][BOW_CLAIM_BITS / 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 4 + wave;
    if (pi >= npairs) return;
    const BowCandPair pr = pairs[pi];
    const int gF = __builtin_amdgcn_readfirstlane((int)pr.gFixed);
    const uint32_t gk = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr.gk);
    const BowCandDev *cd = cands + (gk >> BOW_CAND_NODE_BITS);
    const int gC = (int)(gk & ((1u << BOW_CAND_NODE_BITS) - 1u));
    const int32_t *offC = cd->off;
    const int f0 = offF[gF], f1 = offF[gF + 1];
    const int c0 = offC[gC], c1 = offC[gC + 1];
    if (f1 <= f0 || c1 <= c0) return;
    int32_t *outRow = out + (size_t)cd->outRow * nF, *scr = scratch + cd->scratchOff;
    const BowValid vC = {nullptr, (const int2 *)cd->row, mflags, maxPoints};
    if (MODE == 0) {
        const BowValid vF = {nullptr, nullptr, nullptr, 0};
        bow_match_node<BOW_V_ROW, BOW_V_BYTES_OR_ALL>(cd->desc, vC, cd->idx, c0, c1, descF, vF, idxF, f0, f1 - f0, th, 0, nnratio, scr,
                                                      outRow, s_claim[wave], lane);
    } else {
        const BowValid vF = {nullptr, rowF, mflags, maxPoints};
        bow_match_node<BOW_V_ROW, BOW_V_ROW>(descF, vF, idxF, f0, f1, cd->desc, vC, cd->idx, c0, c1 - c0, th, 1, nnratio, outRow, scr,
                                             s_claim[wave], lane);
    }
}

// out [K][nF] as the match kernel left it -> the rows after the rotation check, in place and in hostRows; nm / hostNm [K]
__global__ __launch_bounds__(256) void k_bow_rot_cands(const int mode, const BowCandDev *__restrict__ cands, const int K,
                                                       const orbhip_keypoint *__restrict__ kpsF, const int nF, const int check_ori,
                                                       int32_t *__restrict__ out, int32_t *__restrict__ hostRows,
                                                       int32_t *__restrict__ nm, int32_t *__restrict__ hostNm)
{
    __shared__ int s_hist[4][32];
    __shared__ int s_keep[4][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wave;
    if (k >= K) return;   // wave-uniform
    const BowCandDev *cd = cands + k;
    const orbhip_keypoint *kpsC = cd->kps;
    const int nC = cd->n;
    int32_t *row = out + (size_t)cd->outRow * nF, *hrow = hostRows + (size_t)k * nF;
    int *hist = s_hist[wave], *keep = s_keep[wave];
    // the bin of the match (fixed feature i, candidate feature j): side 1 is the candidate in mode 0, the fixed key frame in mode 1
    auto bin_of = [&](int i, int j) {
        const float aF = kpsF[i].angle, aC = kpsC[j].angle;
        return mode == 0 ? bow_rot_bin(aC, aF) : bow_rot_bin(aF, aC);
    };
    if (check_ori) {
        if (lane < 32) hist[lane] = 0;
        WAVE_LDS_SYNC();
        for (int i = lane; i < nF; i += 64) {
            const int j = row[i];
            if (j >= 0 && j < nC) {
                const int bin = bin_of(i, j);
                if (bin >= 0 && bin < BS_HISTO) atomicAdd(&hist[bin], 1);
            }
        }
        WAVE_LDS_SYNC();
        if (lane == 0) bow_three_maxima(hist, keep);
        WAVE_LDS_SYNC();
    }
    int local = 0;
    for (int i = lane; i < nF; i += 64) {
        int j = row[i];
        if (j >= nC) j = -1;
        if (j >= 0 && check_ori && !bow_rot_keeps(bin_of(i, j), keep)) j = -1;
        row[i] = j;     // (the lane's own entry: no other lane reads it in this kernel)
        hrow[i] = j;
        local += j >= 0 ? 1 : 0;
    }
    local = wave_sum(local);
    if (lane == 0) {
        nm[k] = local;
        hostNm[k] = local;
    }
}

// The correspondences of every candidate with nm[k] >= minMatches, one segment per candidate in candidate order, the frame's
// features in ascending index inside a segment.  off [K + 1], *ntotal = off[K]; nothing else is written when *ntotal > cap.
__global__ __launch_bounds__(256) void k_pnp_gather_cands(const BowCandDev *__restrict__ cands, const int K,
                                                          const int32_t *__restrict__ nm, const int minMatches,
                                                          const orbhip_keypoint *__restrict__ kpsF, const int nF,
                                                          const int32_t *__restrict__ out, const float *__restrict__ levelSigma2,
                                                          const int nlevels, const float th2, const float4 *__restrict__ geoA,
                                                          const uint32_t *__restrict__ mflags, const int maxPoints, const int cap,
                                                          int32_t *__restrict__ off, int32_t *__restrict__ ntotal,
                                                          int32_t *__restrict__ kpIdx, int32_t *__restrict__ kfIdx,
                                                          float *__restrict__ P3Dw, float *__restrict__ P2D,
                                                          float *__restrict__ maxErr)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wave;
    if (k >= K) return;   // wave-uniform
    int before = 0, all = 0;
    for (int base = 0; base < K; base += 64) {   // (K <= 4095: at most 64 rounds)
        const int kk = base + lane;
        int c = kk < K ? nm[kk] : 0;
        if (c < minMatches) c = 0;
        all += c;
        if (kk < k) before += c;
    }
    before = wave_sum(before);
    all = wave_sum(all);
    if (lane == 0) {
        off[k] = before;
        if (k == 0) {
            off[K] = all;
            *ntotal = all;
        }
    }
    if (all > cap) return;
    const int mine = nm[k];
    if (mine < minMatches || mine <= 0) return;
    const BowCandDev *cd = cands + k;
    const int2 *rowC = (const int2 *)cd->row;
    const int nC = cd->n;
    const int32_t *row = out + (size_t)cd->outRow * nF;
    int pos = before;
    for (int base = 0; base < nF; base += 64) {   // (wave-uniform trip count: every lane reaches the ballot)
        const int i = base + lane;
        const int j = i < nF ? row[i] : -1;
        const bool has = j >= 0 && j < nC;
        const unsigned long long m = __ballot(has);
        const int at = pos + __popcll(m & ((1ull << lane) - 1ull));
        if (has && at < cap) {
            const orbhip_keypoint kp = kpsF[i];
            kpIdx[at] = i;
            kfIdx[at] = j;
            P2D[2 * at] = kp.x;
            P2D[2 * at + 1] = kp.y;
            maxErr[at] = (kp.octave >= 0 && kp.octave < nlevels) ? __fmul_rn(levelSigma2[kp.octave], th2) : 0.f;
            const int s = kf_entry_slot(rowC[1 + j], mflags, maxPoints);   // (resolves: the match kernel asked the same question)
            const float4 g = s >= 0 ? geoA[s] : make_float4(0.f, 0.f, 0.f, 0.f);
            P3Dw[3 * at] = g.x;
            P3Dw[3 * at + 1] = g.y;
            P3Dw[3 * at + 2] = g.z;
        }
        pos += __popcll(m);
    }
}

void launch_bow_match_cands(hipStream_t s, int mode, const uint8_t *descF, const int32_t *offF, const int32_t *idxF, const void *rowF,
                            int nF, const BowCandDev *cands, const BowCandPair *pairs, int npairs, const uint32_t *mflags,
                            int maxPoints, int th, float nnratio, int32_t *out, int32_t *scratch)
{
    if (npairs <= 0) return;
    const dim3 grid((npairs + 3) / 4, 1, 1), blk(256, 1, 1);
    if (mode == 0)
        hipLaunchKernelGGL(k_bow_match_cands<0>, grid, blk, 0, s, descF, offF, idxF, (const int2 *)rowF, nF, cands, pairs, npairs, mflags,
                           maxPoints, th, nnratio, out, scratch);
    else
        hipLaunchKernelGGL(k_bow_match_cands<1>, grid, blk, 0, s, descF, offF, idxF, (const int2 *)rowF, nF, cands, pairs, npairs, mflags,
                           maxPoints, th, nnratio, out, scratch);
}

void launch_bow_rot_cands(hipStream_t s, int mode, const BowCandDev *cands, int K, const orbhip_keypoint *kpsF, int nF, int check_ori,
                          int32_t *out, int32_t *hostRows, int32_t *nm, int32_t *hostNm)
{
    if (K <= 0) return;
    hipLaunchKernelGGL(k_bow_rot_cands, dim3((K + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, mode, cands, K, kpsF, nF, check_ori, out, hostRows,
                       nm, hostNm);
}

void launch_pnp_gather_cands(hipStream_t s, const BowCandDev *cands, int K, const int32_t *nm, int minMatches,
                             const orbhip_keypoint *kpsF, int nF, const int32_t *out, const float *levelSigma2, int nlevels, float th2,
                             const void *geoA, const uint32_t *mflags, int maxPoints, int cap, int32_t *off, int32_t *ntotal,
                             int32_t *kpIdx, int32_t *kfIdx, float *P3Dw, float *P2D, float *maxErr)
{
    if (K <= 0) return;
    hipLaunchKernelGGL(k_pnp_gather_cands, dim3((K + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, cands, K, nm, minMatches, kpsF, nF, out,
                       levelSigma2, nlevels, th2, (const float4 *)geoA, mflags, maxPoints, cap, off, ntotal, kpIdx, kfIdx, P3Dw, P2D,
                       maxErr);
}
