// k_initscore.hip -- the scoring loops of the monocular initialiser's RANSAC (ref: src/Initializer.cc:305-468, CheckHomography
// and CheckFundamental) for every hypothesis of an attempt at once.
//
// The score of a hypothesis is a float sum over the matches in ascending order, two terms per match: the terms are independent,
// the sum is not associative.  Three launches, B problems in each grid:
//   k_init_pairs  one workgroup per problem: matches12 -> the matched pairs' coordinates {u1, v1, u2, v2} in ascending order of the
//                 frame-1 index (the reference's mvMatches12) and their number N;
//   k_init_score  one workgroup per IS_HPB hypotheses.  Waves 1-3 compute the two terms of (hypothesis, pair) for a tile of
//                 IS_TILE pairs into LDS while wave 0, one lane per hypothesis, adds the terms of the tile before in order;
//   k_init_pick   one workgroup per (problem, model): the first hypothesis of largest score > 0, then that hypothesis's inlier
//                 flags evaluated again per frame-1 feature (nothing of size hypotheses x matches is ever stored).
// Every float operation is rounded on its own (__fmul_rn ...; the file is built with -ffp-contract=off as well) and written in
// the source's left-to-right order.  An excluded term (chiSquare > th) is written as +0.0f: every term is >= +0.0f or NaN, so the
// running sum is >= +0.0f or NaN, and x + (+0.0f) has the bits of x for both -- adding it is skipping it.
#include "orbhip_internal.h"
#include "wave_ops.h"

#define IS_THREADS 256
#define IS_HPB 8                          // hypotheses per workgroup of k_init_score = summing lanes of wave 0
#define IS_TILE (IS_THREADS - 64)         // pairs per tile: one per lane of waves 1-3
#define IS_ROW (2 * IS_TILE + 4)          // floats per hypothesis row of a tile: 16 bytes of padding spread the eight summing lanes' b128 reads over the banks
#define IS_HYP 20                         // floats per staged hypothesis: H21 | H12 (F: F21 | unused), rows 16-byte aligned

#define IS_TH_H 5.991f                    // :333
#define IS_TH_F 3.841f                    // :408
#define IS_TH_SCORE 5.991f                // :409

// (x, y) of keypoint i of an array whose elements are `stride` bytes apart (orbhip_keypoint: 28, packed float2: 8)
__device__ __forceinline__ float2 is_xy(const uint8_t *base, int stride, int i)
{
    const float *p = (const float *)(base + (size_t)i * stride);
    return make_float2(p[0], p[1]);
}

// chiSquare of (us, vs) carried through the 3x3 homography M against (ud, vd) (:352-358, :368-374)
__device__ __forceinline__ float is_chi_h(const float *M, float us, float vs, float ud, float vd, float invSigmaSquare)
{
    const float winv = __fdiv_rn(1.0f, __fadd_rn(__fadd_rn(__fmul_rn(M[6], us), __fmul_rn(M[7], vs)), M[8]));
    const float x = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[0], us), __fmul_rn(M[1], vs)), M[2]), winv);
    const float y = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[3], us), __fmul_rn(M[4], vs)), M[5]), winv);
    const float dx = __fsub_rn(ud, x), dy = __fsub_rn(vd, y);
    return __fmul_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), invSigmaSquare);
}

// chiSquare of (ud, vd) against the line {a, b, c} = {fa, fb, fc} . (us, vs, 1) (:428-436 with the rows of F21, :446-454 with its
// columns)
__device__ __forceinline__ float is_chi_f(float fa0, float fa1, float fa2, float fb0, float fb1, float fb2, float fc0, float fc1,
                                          float fc2, float us, float vs, float ud, float vd, float invSigmaSquare)
{
    const float a = __fadd_rn(__fadd_rn(__fmul_rn(fa0, us), __fmul_rn(fa1, vs)), fa2);
    const float b = __fadd_rn(__fadd_rn(__fmul_rn(fb0, us), __fmul_rn(fb1, vs)), fb2);
    const float c = __fadd_rn(__fadd_rn(__fmul_rn(fc0, us), __fmul_rn(fc1, vs)), fc2);
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(a, ud), __fmul_rn(b, vd)), c);
    const float sq = __fdiv_rn(__fmul_rn(num, num), __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
    return __fmul_rn(sq, invSigmaSquare);
}

// the two chiSquares of a pair, in the order the reference adds them.  hyp: H21 | H12 (isF: F21)
__device__ __forceinline__ void is_chi2(const float *hyp, bool isF, float4 p, float invSigmaSquare, float &chi1, float &chi2)
{
    if (isF) {
        const float *F = hyp;
        chi1 = is_chi_f(F[0], F[1], F[2], F[3], F[4], F[5], F[6], F[7], F[8], p.x, p.y, p.z, p.w, invSigmaSquare);
        chi2 = is_chi_f(F[0], F[3], F[6], F[1], F[4], F[7], F[2], F[5], F[8], p.z, p.w, p.x, p.y, invSigmaSquare);
    } else {
        chi1 = is_chi_h(hyp + 9, p.z, p.w, p.x, p.y, invSigmaSquare);   // image 1, through H12
        chi2 = is_chi_h(hyp, p.x, p.y, p.z, p.w, invSigmaSquare);       // image 2, through H21
    }
}

// `chiSquare > th` as the reference writes it: a NaN is not excluded
__device__ __forceinline__ float is_term(float chi, float th, float thScore) { return chi > th ? 0.0f : __fsub_rn(thScore, chi); }

// the hypothesis g (H first) of problem b into 18 floats
__device__ __forceinline__ void is_load_hyp(const float *H21, const float *H12, const float *F21, int nH, int nF, int b, int g, int k,
                                            float *dst)
{
    if (g < nH)
        dst[k] = k < 9 ? H21[((size_t)b * nH + g) * 9 + k] : H12[((size_t)b * nH + g) * 9 + (k - 9)];
    else
        dst[k] = k < 9 ? F21[((size_t)b * nF + (g - nH)) * 9 + k] : 0.0f;
}

// a feature's match: an index into frame 2, or -1 for none (an entry outside [0, n2) counts as none)
__device__ __forceinline__ int is_match(const int32_t *match12, int i, int n2)
{
    const int m = match12[i];
    return (m >= 0 && m < n2) ? m : -1;
}

__global__ __launch_bounds__(IS_THREADS) void k_init_pairs(const uint8_t *kps1, int stride1, const int32_t *cnt1, int cap1,
                                                           const uint8_t *kps2, int stride2, const int32_t *cnt2, int cap2,
                                                           const int32_t *match12, float4 *pairs, int32_t *npairs)
{
    __shared__ int waveTotal[IS_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int n1 = min(max(cnt1[b], 0), cap1), n2 = min(max(cnt2[b], 0), cap2);
    kps1 += (size_t)b * cap1 * stride1, kps2 += (size_t)b * cap2 * stride2;
    match12 += (size_t)b * cap1, pairs += (size_t)b * cap1;
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += IS_THREADS) {   // (uniform trip count: every lane takes part in the scans)
        const int i = i0 + tid;
        const int m = i < n1 ? is_match(match12, i, n2) : -1;
        const int incl = wave_incl_scan(m >= 0 ? 1 : 0);
        if ((tid & 63) == 63) waveTotal[wave] = incl;
        __syncthreads();
        int at = base + incl - 1;
        for (int w = 0; w < wave; w++) at += waveTotal[w];
        if (m >= 0) {
            const float2 a = is_xy(kps1, stride1, i), c = is_xy(kps2, stride2, m);
            pairs[at] = make_float4(a.x, a.y, c.x, c.y);   // at < n1 <= cap1
        }
        base += waveTotal[0] + waveTotal[1] + waveTotal[2] + waveTotal[3];
        __syncthreads();
    }
    if (tid == 0) npairs[b] = base;
}

__global__ __launch_bounds__(IS_THREADS) void k_init_score(const float4 *pairs, const int32_t *npairs, int cap1, const float *H21,
                                                           const float *H12, int nH, const float *F21, int nF, float invSigmaSquare,
                                                           float *scores)
{
    __shared__ __attribute__((aligned(16))) float sHyp[IS_HPB][IS_HYP];
    __shared__ __attribute__((aligned(16))) float sTerm[2][IS_HPB][IS_ROW];
    const int b = blockIdx.y, g0 = blockIdx.x * IS_HPB, tid = threadIdx.x;
    const int nHyp = nH + nF, nh = min(IS_HPB, nHyp - g0);
    const int N = npairs[b];
    pairs += (size_t)b * cap1;
    if (tid < nh * 18) is_load_hyp(H21, H12, F21, nH, nF, b, g0 + tid / 18, tid % 18, sHyp[tid / 18]);
    __syncthreads();
    const int ntiles = (N + IS_TILE - 1) / IS_TILE;
    const bool producer = tid >= 64;
    const int j = tid - 64;                                   // a producer's pair within the tile
    float s = 0.0f;                                           // (wave 0, lane h: the score of hypothesis g0 + h)
    for (int k = -1; k < ntiles; k++) {
        if (producer) {
            if (k + 1 < ntiles) {
                const int p = (k + 1) * IS_TILE + j;
                const bool live = p < N;
                const float4 q = live ? pairs[p] : make_float4(0.f, 0.f, 0.f, 0.f);
                float(*dst)[IS_ROW] = sTerm[(k + 1) & 1];
                for (int h = 0; h < nh; h++) {
                    const bool isF = g0 + h >= nH;
                    float chi1, chi2;
                    is_chi2(sHyp[h], isF, q, invSigmaSquare, chi1, chi2);
                    const float th = isF ? IS_TH_F : IS_TH_H;
                    const float t1 = live ? is_term(chi1, th, IS_TH_SCORE) : 0.0f, t2 = live ? is_term(chi2, th, IS_TH_SCORE) : 0.0f;
                    *(float2 *)&dst[h][2 * j] = make_float2(t1, t2);
                }
            }
        } else if (k >= 0 && tid < nh) {
            // the tile's terms in order, four (two pairs) per read; a last odd pair is followed by a dead lane's two zeros
            const int cnt = min(IS_TILE, N - k * IS_TILE);
            const float4 *row = (const float4 *)sTerm[k & 1][tid];
#pragma unroll 4
            for (int q = 0; q < (cnt + 1) / 2; q++) {
                const float4 t = row[q];
                s = __fadd_rn(s, t.x);
                s = __fadd_rn(s, t.y);
                s = __fadd_rn(s, t.z);
                s = __fadd_rn(s, t.w);
            }
        }
        __syncthreads();
    }
    if (tid < nh) scores[(size_t)b * nHyp + g0 + tid] = s;
}

struct IsBest {
    float score;
    int32_t it, ninliers;
};

// `currentScore > score` from score = 0 over the hypotheses in index order: the first hypothesis of largest score, if that is > 0
__device__ __forceinline__ bool is_better(float s, int i, float bs, int bi) { return s > bs || (s == bs && bi >= 0 && i < bi); }

__global__ __launch_bounds__(IS_THREADS) void k_init_pick(const uint8_t *kps1, int stride1, const int32_t *cnt1, int cap1,
                                                          const uint8_t *kps2, int stride2, const int32_t *cnt2, int cap2,
                                                          const int32_t *match12, const float *H21, const float *H12, int nH,
                                                          const float *F21, int nF, float invSigmaSquare, const float *scores,
                                                          IsBest *best, uint8_t *inliers)
{
    __shared__ float sScore[IS_THREADS];
    __shared__ int sIdx[IS_THREADS];
    __shared__ float sHyp[IS_HYP];
    __shared__ int sCount[IS_THREADS / 64];
    const int model = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const bool isF = model == 1;
    const int nHyp = nH + nF, first = isF ? nH : 0, n = isF ? nF : nH;
    const int n1 = min(max(cnt1[b], 0), cap1), n2 = min(max(cnt2[b], 0), cap2);
    scores += (size_t)b * nHyp + first;
    float bs = 0.0f;
    int bi = -1;
    for (int i = tid; i < n; i += IS_THREADS) {
        const float s = scores[i];
        if (is_better(s, i, bs, bi)) bs = s, bi = i;   // (a NaN compares false: it never wins)
    }
    sScore[tid] = bs, sIdx[tid] = bi;
    __syncthreads();
    for (int step = IS_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step && is_better(sScore[tid + step], sIdx[tid + step], sScore[tid], sIdx[tid]) && sIdx[tid + step] >= 0)
            sScore[tid] = sScore[tid + step], sIdx[tid] = sIdx[tid + step];
        __syncthreads();
    }
    bs = sScore[0], bi = sIdx[0];
    if (bi >= 0 && tid < 18) is_load_hyp(H21, H12, F21, nH, nF, b, first + bi, tid, sHyp);
    __syncthreads();
    kps1 += (size_t)b * cap1 * stride1, kps2 += (size_t)b * cap2 * stride2;
    match12 += (size_t)b * cap1;
    inliers += ((size_t)b * 2 + model) * cap1;
    const float th = isF ? IS_TH_F : IS_TH_H;
    int mine = 0;
    for (int i0 = 0; i0 < n1; i0 += IS_THREADS) {
        const int i = i0 + tid;
        if (i >= n1) continue;
        uint8_t in = 0;
        const int m = bi >= 0 ? is_match(match12, i, n2) : -1;
        if (m >= 0) {
            const float2 a = is_xy(kps1, stride1, i), c = is_xy(kps2, stride2, m);
            float chi1, chi2;
            is_chi2(sHyp, isF, make_float4(a.x, a.y, c.x, c.y), invSigmaSquare, chi1, chi2);
            in = !(chi1 > th) && !(chi2 > th);
        }
        inliers[i] = in;
        mine += in;
    }
    const int total = wave_sum(mine);   // (every lane is back here)
    if ((tid & 63) == 0) sCount[tid >> 6] = total;
    __syncthreads();
    if (tid == 0) {
        IsBest r;
        r.score = bs, r.it = bi, r.ninliers = sCount[0] + sCount[1] + sCount[2] + sCount[3];
        best[(size_t)b * 2 + model] = r;
    }
}

void launch_init_score(hipStream_t s, const void *kps1, int stride1, const int32_t *cnt1, int cap1, const void *kps2, int stride2,
                       const int32_t *cnt2, int cap2, int B, const int32_t *match12, const float *H21, const float *H12, int nH,
                       const float *F21, int nF, float invSigmaSquare, float *scores, void *best, uint8_t *inliers, void *scratch)
{
    float4 *pairs = (float4 *)scratch;
    int32_t *npairs = (int32_t *)((uint8_t *)scratch + (size_t)B * cap1 * sizeof(float4));
    hipLaunchKernelGGL(k_init_pairs, dim3(B), dim3(IS_THREADS), 0, s, (const uint8_t *)kps1, stride1, cnt1, cap1, (const uint8_t *)kps2,
                       stride2, cnt2, cap2, match12, pairs, npairs);
    if (nH + nF > 0)
        hipLaunchKernelGGL(k_init_score, dim3((nH + nF + IS_HPB - 1) / IS_HPB, B), dim3(IS_THREADS), 0, s, pairs, npairs, cap1, H21, H12,
                           nH, F21, nF, invSigmaSquare, scores);
    hipLaunchKernelGGL(k_init_pick, dim3(2, B), dim3(IS_THREADS), 0, s, (const uint8_t *)kps1, stride1, cnt1, cap1,
                       (const uint8_t *)kps2, stride2, cnt2, cap2, match12, H21, H12, nH, F21, nF, invSigmaSquare, scores,
                       (IsBest *)best, inliers);
}

size_t init_score_scratch_bytes(int B, int cap1) { return (size_t)B * cap1 * sizeof(float4) + (size_t)B * sizeof(int32_t); }
