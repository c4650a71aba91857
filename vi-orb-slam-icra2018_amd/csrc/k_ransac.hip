// k_ransac.hip -- the inlier checks of the relocalisation and loop-closing RANSACs (ref: src/PnPsolver.cc:308-339 CheckInliers;
// src/Sim3Solver.cc:340-403 CheckInliers + Project) for M hypotheses of each of B problems at once, and the bookkeeping around
// them (PnPsolver.cc:209-225, Sim3Solver.cc:183-200) in hypothesis order.
//
// The result of a hypothesis is an integer count, so nothing depends on a summation order.  Two launches, B problems in each grid:
//   k_ransac_count  one workgroup per RS_HPB hypotheses of a problem.  Their matrices are staged in LDS and read as broadcasts;
//                   lanes run over the points, a lane keeps its point in registers across the group's hypotheses; a count is the
//                   population of the wave's ballot added to one LDS word per wave and hypothesis, one plain store per count;
//   k_ransac_pick   one workgroup per problem: one lane walks the M counts in order -- M integer compares, 300 at most in the
//                   reference's schedule -- and applies the solver's rule with the carried best_in; the flags of the <= R records
//                   (PnP) or of the winner (Sim3) are then evaluated again per point.  Nothing of size hypotheses x points is stored.
// Arithmetic (the contract; include/orbhip.h restates it): every operation is rounded on its own (__d*_rn / __f*_rn; the file is
// built with -ffp-contract=off as well), in the source's left-to-right order.
//   PnP   R, t, fu, fv, uc, vc double; X, Y, Z, u, v, max_err float.
//         Xc = (float)(((r00*X + r01*Y) + r02*Z) + t0) in double, Yc alike; invZc = (float)(1.0 / (((r20*X + r21*Y) + r22*Z) + t2)),
//         a double division rounded to float; ue = uc + ((fu * (double)Xc) * (double)invZc), ve alike; distX = (float)((double)u - ue);
//         error2 = (distX*distX) + (distY*distY) in float; inlier iff error2 < max_err (NaN and inf fail; no test on the depth's sign).
//   Sim3  everything float.  Project(X, T, K): Pc[r] = (float)(s + (double)t[r]) with s accumulated in double from 0.0 over
//         k = 0, 1, 2 of (double)R[r][k] * (double)X[k] (one gemm, as host/ORBmatcher.cc affine3); invz = 1.0f / Pc[2];
//         x = Pc[0] * invz; u = (fx * x) + cx, v alike.  dist1 = P1im1 - Project(X3Dc2, T12, K1), dist2 = Project(X3Dc1, T21, K2) -
//         P2im2; err = (float)(((double)d0*d0) + ((double)d1*d1)), cv::Mat::dot's double accumulator; inlier iff
//         err1 < max_err1 && err2 < max_err2.
#include "orbhip_internal.h"

#define RS_THREADS 256
#define RS_HPB 8                          // hypotheses per workgroup of k_ransac_count

namespace
{
// what k_ransac_pick knows of a problem: off[b], off[b + 1] | min_inliers[b] | best_in[b], as launch_ransac's `par` lays them out
struct RsProblem {
    int first, N, minInliers, bestIn;
};
__device__ __forceinline__ RsProblem rs_problem(const int32_t *par, int B, int b)
{
    RsProblem p;
    p.first = par[b], p.N = par[b + 1] - par[b];
    p.minInliers = par[B + 1 + b], p.bestIn = par[2 * B + 1 + b];
    return p;
}

struct RsPnp {
    typedef double hyp_t;
    static constexpr int HYP = 12;        // R[9] row-major | t[3]
    typedef OrbPnpPoints Points;
    struct Point {
        float X, Y, Z, u, v, maxErr;
    };
    static __device__ __forceinline__ Point load(const Points &P, size_t i)
    {
        Point p;
        p.X = P.X[3 * i], p.Y = P.X[3 * i + 1], p.Z = P.X[3 * i + 2];
        p.u = P.uv[2 * i], p.v = P.uv[2 * i + 1];
        p.maxErr = P.maxErr[i];
        return p;
    }
    // one row of R . X + t, in double, left to right
    static __device__ __forceinline__ double row(const double *h, int r, const Point &p)
    {
        return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(h[3 * r], (double)p.X), __dmul_rn(h[3 * r + 1], (double)p.Y)),
                                   __dmul_rn(h[3 * r + 2], (double)p.Z)),
                         h[9 + r]);
    }
    static __device__ __forceinline__ bool inlier(const double *h, const Points &P, const Point &p)
    {
        const float Xc = __double2float_rn(row(h, 0, p)), Yc = __double2float_rn(row(h, 1, p));
        const float invZc = __double2float_rn(__ddiv_rn(1.0, row(h, 2, p)));
        const double ue = __dadd_rn(P.uc, __dmul_rn(__dmul_rn(P.fu, (double)Xc), (double)invZc));
        const double ve = __dadd_rn(P.vc, __dmul_rn(__dmul_rn(P.fv, (double)Yc), (double)invZc));
        const float distX = __double2float_rn(__dsub_rn((double)p.u, ue)), distY = __double2float_rn(__dsub_rn((double)p.v, ve));
        const float error2 = __fadd_rn(__fmul_rn(distX, distX), __fmul_rn(distY, distY));
        return error2 < p.maxErr;
    }
};

struct RsSim3 {
    typedef float hyp_t;
    static constexpr int HYP = 24;        // the 3x4 block of T12 | the 3x4 block of T21, row-major
    typedef OrbSim3Points Points;
    struct Point {
        float X1[3], X2[3], p1[2], p2[2], maxErr1, maxErr2;
    };
    static __device__ __forceinline__ Point load(const Points &P, size_t i)
    {
        Point p;
        for (int k = 0; k < 3; k++) p.X1[k] = P.X1[3 * i + k], p.X2[k] = P.X2[3 * i + k];
        for (int k = 0; k < 2; k++) p.p1[k] = P.p1[2 * i + k], p.p2[k] = P.p2[2 * i + k];
        p.maxErr1 = P.maxErr1[i], p.maxErr2 = P.maxErr2[i];
        return p;
    }
    // Project(X, T, K) -> (u, v); K = {fx, fy, cx, cy}
    static __device__ __forceinline__ void project(const float *T, const float *X, const float *K, float &u, float &v)
    {
        float Pc[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) s = __dadd_rn(s, __dmul_rn((double)T[4 * r + k], (double)X[k]));
            Pc[r] = __double2float_rn(__dadd_rn(s, (double)T[4 * r + 3]));
        }
        const float invz = __fdiv_rn(1.0f, Pc[2]);
        const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
        u = __fadd_rn(__fmul_rn(K[0], x), K[2]);
        v = __fadd_rn(__fmul_rn(K[1], y), K[3]);
    }
    static __device__ __forceinline__ float dot2(float d0, float d1)
    {
        return __double2float_rn(__dadd_rn(__dmul_rn((double)d0, (double)d0), __dmul_rn((double)d1, (double)d1)));
    }
    static __device__ __forceinline__ bool inlier(const float *h, const Points &P, const Point &p)
    {
        float u, v;
        project(h, p.X2, P.K1, u, v);                                      // vP2im1
        const float err1 = dot2(__fsub_rn(p.p1[0], u), __fsub_rn(p.p1[1], v));
        project(h + 12, p.X1, P.K2, u, v);                                 // vP1im2
        const float err2 = dot2(__fsub_rn(u, p.p2[0]), __fsub_rn(v, p.p2[1]));
        return err1 < p.maxErr1 && err2 < p.maxErr2;
    }
};

template <class S>
__global__ __launch_bounds__(RS_THREADS) void k_ransac_count(typename S::Points P, const typename S::hyp_t *hyp, int M, const int32_t *par,
                                                             int B, int32_t *counts)
{
    __shared__ __attribute__((aligned(16))) typename S::hyp_t sHyp[RS_HPB * S::HYP];
    __shared__ int sPart[RS_THREADS / 64][RS_HPB];
    const int b = blockIdx.y, g0 = blockIdx.x * RS_HPB, tid = threadIdx.x, wave = tid >> 6;
    const int nh = min(RS_HPB, M - g0);                                    // >= 1: the grid has ceil(M / RS_HPB) groups
    const int first = par[b], N = par[b + 1] - first;
    hyp += ((size_t)b * M + g0) * S::HYP;
    for (int k = tid; k < nh * S::HYP; k += RS_THREADS) sHyp[k] = hyp[k];
    if (tid < RS_HPB) sPart[0][tid] = sPart[1][tid] = sPart[2][tid] = sPart[3][tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += RS_THREADS) {                           // (uniform trip count: every lane votes)
        const bool live = i0 + tid < N;
        const typename S::Point p = S::load(P, (size_t)first + (live ? i0 + tid : 0));
        // (not unrolled: unrolled, the compiler keeps all RS_HPB matrices in registers across the outer loop, 256 VGPRs + AGPRs)
#pragma unroll 1
        for (int h = 0; h < nh; h++) {
            const bool in = live && S::inlier(sHyp + h * S::HYP, P, p);
            const int c = __popcll(__ballot(in));
            if ((tid & 63) == 0) sPart[wave][h] += c;
        }
    }
    __syncthreads();
    if (tid < nh) counts[(size_t)b * M + g0 + tid] = sPart[0][tid] + sPart[1][tid] + sPart[2][tid] + sPart[3][tid];
}

// the flags of hypothesis h (wave-uniform) of the problem's N points -> dst[0 .. N)
template <class S>
__device__ __forceinline__ void rs_flags(const typename S::Points &P, const typename S::hyp_t *hyp, int first, int N, uint8_t *dst,
                                         typename S::hyp_t *sHyp)
{
    __syncthreads();                                                       // (the last reader of sHyp is done)
    if (threadIdx.x < S::HYP) sHyp[threadIdx.x] = hyp[threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += RS_THREADS) dst[i] = S::inlier(sHyp, P, S::load(P, (size_t)first + i)) ? 1 : 0;
}

// PnP (ref: src/PnPsolver.cc:209-225): from best = best_in, hypothesis h is a record iff count[h] >= min_inliers && count[h] > best,
// and then best = count[h].  res = {n_records, best_out}; the first min(n_records, R) records' indices, counts and flag rows.
// The counts are taken RS_THREADS at a time into LDS, where lane 0 walks them; the flags of that stretch's records follow.
__global__ __launch_bounds__(RS_THREADS) void k_ransac_pick_pnp(OrbPnpPoints P, const double *hyp, int M, const int32_t *par, int B,
                                                                const int32_t *counts, int32_t *countsCopy, int R, int32_t *res,
                                                                int32_t *recIdx, int32_t *recCnt, uint8_t *flags)
{
    __shared__ int sCount[RS_THREADS], sRec[RS_THREADS], sNew, sStored;
    __shared__ __attribute__((aligned(16))) double sHyp[RsPnp::HYP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const RsProblem pr = rs_problem(par, B, b);
    counts += (size_t)b * M, hyp += (size_t)b * M * RsPnp::HYP;
    recIdx += (size_t)b * R, recCnt += (size_t)b * R;
    flags += (size_t)R * pr.first;                                         // the problem's R rows of N bytes
    int best = pr.bestIn, nrec = 0;                                        // (lane 0's)
    for (int h0 = 0; h0 < M; h0 += RS_THREADS) {
        const int n = min(RS_THREADS, M - h0);
        if (tid < n) {
            const int c = counts[h0 + tid];
            sCount[tid] = c;
            if (countsCopy) countsCopy[(size_t)b * M + h0 + tid] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int k = 0;
            const int before = min(nrec, R);
            for (int j = 0; j < n; j++) {
                const int c = sCount[j];
                if (c >= pr.minInliers && c > best) {
                    best = c;
                    if (nrec < R) sRec[k++] = h0 + j, recIdx[nrec] = h0 + j, recCnt[nrec] = c;
                    nrec++;
                }
            }
            sNew = k, sStored = before;
        }
        __syncthreads();
        const int nNew = sNew, stored = sStored;
        for (int k = 0; k < nNew; k++) {
            const int h = __builtin_amdgcn_readfirstlane(sRec[k]);
            rs_flags<RsPnp>(P, hyp + (size_t)h * RsPnp::HYP, pr.first, pr.N, flags + (size_t)(stored + k) * pr.N, sHyp);
        }
        __syncthreads();                                                   // (sCount, sRec, sNew are free again)
    }
    if (tid == 0) res[2 * b] = nrec, res[2 * b + 1] = best;
}

// Sim3 (ref: src/Sim3Solver.cc:183-200): from best = best_in, for each h: count[h] >= best makes best = count[h], best_it = h, and
// if count[h] > min_inliers as well h is the winner and nothing after it is looked at.  res = {winner, ninliers, best_it, best_out}.
__global__ __launch_bounds__(RS_THREADS) void k_ransac_pick_sim3(OrbSim3Points P, const float *hyp, int M, const int32_t *par, int B,
                                                                 const int32_t *counts, int32_t *countsCopy, int32_t *res, uint8_t *flags)
{
    __shared__ int sCount[RS_THREADS], sWinner;
    __shared__ __attribute__((aligned(16))) float sHyp[RsSim3::HYP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const RsProblem pr = rs_problem(par, B, b);
    counts += (size_t)b * M, hyp += (size_t)b * M * RsSim3::HYP;
    flags += pr.first;
    int best = pr.bestIn, bestIt = -1, winner = -1, ninl = 0;              // (lane 0's)
    for (int h0 = 0; h0 < M; h0 += RS_THREADS) {
        const int n = min(RS_THREADS, M - h0);
        if (tid < n) {
            const int c = counts[h0 + tid];
            sCount[tid] = c;
            if (countsCopy) countsCopy[(size_t)b * M + h0 + tid] = c;
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < n && winner < 0; j++) {
                const int c = sCount[j];
                if (c >= best) {
                    best = c, bestIt = h0 + j;
                    if (c > pr.minInliers) winner = h0 + j, ninl = c;
                }
            }
        __syncthreads();
    }
    if (tid == 0) {
        res[4 * b] = winner, res[4 * b + 1] = ninl, res[4 * b + 2] = bestIt, res[4 * b + 3] = best;
        sWinner = winner;
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(sWinner);
    if (w >= 0)
        rs_flags<RsSim3>(P, hyp + (size_t)w * RsSim3::HYP, pr.first, pr.N, flags, sHyp);
    else
        for (int i = tid; i < pr.N; i += RS_THREADS) flags[i] = 0;
}
}  // namespace

void launch_pnp_score(hipStream_t s, const OrbPnpPoints &P, const double *Rt, int M, const int32_t *par, int B, int32_t *counts,
                      int32_t *countsCopy, int R, int32_t *res, int32_t *recIdx, int32_t *recCnt, uint8_t *flags)
{
    if (B <= 0) return;
    if (M > 0)
        hipLaunchKernelGGL(k_ransac_count<RsPnp>, dim3((M + RS_HPB - 1) / RS_HPB, B), dim3(RS_THREADS), 0, s, P, Rt, M, par, B, counts);
    hipLaunchKernelGGL(k_ransac_pick_pnp, dim3(B), dim3(RS_THREADS), 0, s, P, Rt, M, par, B, (const int32_t *)counts, countsCopy, R, res,
                       recIdx, recCnt, flags);
}

void launch_sim3_score(hipStream_t s, const OrbSim3Points &P, const float *T, int M, const int32_t *par, int B, int32_t *counts,
                       int32_t *countsCopy, int32_t *res, uint8_t *flags)
{
    if (B <= 0) return;
    if (M > 0)
        hipLaunchKernelGGL(k_ransac_count<RsSim3>, dim3((M + RS_HPB - 1) / RS_HPB, B), dim3(RS_THREADS), 0, s, P, T, M, par, B, counts);
    hipLaunchKernelGGL(k_ransac_pick_sim3, dim3(B), dim3(RS_THREADS), 0, s, P, T, M, par, B, (const int32_t *)counts, countsCopy, res,
                       flags);
}
