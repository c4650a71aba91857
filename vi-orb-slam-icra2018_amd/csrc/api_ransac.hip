// api_ransac.hip -- C ABI, part 13: the inlier checks of the PnP and Sim3 RANSACs for M hypotheses at once
// (orbhip_pnp_score[_device], orbhip_sim3_score[_device]; kernels in k_ransac.hip).  The caller draws the
// minimal sets and solves them (compute_pose / ComputeSim3 stay on the host) and gets back what the M calls of CheckInliers (ref:
// src/PnPsolver.cc:308-339, src/Sim3Solver.cc:340-403) and the bookkeeping behind them (:209-225, :183-200) would have left.
#include "api_common.h"

#include <vector>

static bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// what all four forms ask of the counts; off: B + 1 offsets into the concatenated points (host memory)
static int ransac_args_ok(orbhip_ctx *c, const char *who, const int32_t *off, int B, int M, const int32_t *minInliers)
{
    if (B < 0 || M < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": negative count");
    if (M > 65535) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65535 hypotheses");
    if (B > 65535) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65535 problems");
    if (B > 0 && off[0] < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": negative count");
    for (int b = 0; b < B; b++) {
        if (off[b + 1] < off[b]) return fail(c, ORBHIP_E_ARG, std::string(who) + ": off is not non-decreasing");
        if (minInliers[b] < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": min_inliers < 0");
    }
    return ORBHIP_OK;
}

// off | min_inliers | best_in of the device forms -> the matching scratch, where the kernels read them.  The copy leaves host
// memory before this returns (pageable source), so the vector may go.
static int ransac_upload_par(orbhip_ctx *c, const int32_t *off, int B, const int32_t *minInliers, const int32_t *bestIn, size_t extra,
                             const int32_t **par, int32_t **scratch)
{
    std::vector<int32_t> h((size_t)3 * B + 1);
    memcpy(h.data(), off, ((size_t)B + 1) * 4);
    memcpy(h.data() + B + 1, minInliers, (size_t)B * 4);
    if (bestIn)
        memcpy(h.data() + 2 * B + 1, bestIn, (size_t)B * 4);
    else
        std::fill(h.begin() + 2 * B + 1, h.end(), 0);
    const size_t parBytes = align_up(h.size() * 4, 256);
    int rc;
    if ((rc = orb_match_scratch(c, parBytes + extra))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_match.as<void>(), h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream));
    *par = c->d_match.as<int32_t>();
    if (scratch) *scratch = (int32_t *)(c->d_match.as<uint8_t>() + parBytes);
    return ORBHIP_OK;
}

extern "C" int orbhip_pnp_score_device(orbhip_ctx *c, const void *d_P3Dw, const void *d_P2D, const void *d_max_err, const int32_t *off,
                                       int B, double fu, double fv, double uc, double vc, const void *d_Rt, int M,
                                       const int32_t *min_inliers, const int32_t *best_in, int R, void *d_counts, void *d_res,
                                       void *d_rec_idx, void *d_rec_cnt, void *d_rec_flags)
{
    if (!c || (B > 0 && (!off || !min_inliers || !d_res || !d_rec_idx || !d_rec_cnt)) || (B > 0 && M > 0 && (!d_Rt || !d_counts)))
        return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score_device: bad argument");
    if (R < 1) return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score_device: R < 1");
    if (const int rc = ransac_args_ok(c, "orbhip_pnp_score_device", off, B, M, min_inliers)) return rc;
    if (B == 0) return ORBHIP_OK;
    if (off[B] > 0 && (!d_P3Dw || !d_P2D || !d_max_err || !d_rec_flags))
        return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score_device: bad argument");
    if (!aligned_to(d_P3Dw, 4) || !aligned_to(d_P2D, 4) || !aligned_to(d_max_err, 4) || !aligned_to(d_Rt, 8) || !aligned_to(d_counts, 4) ||
        !aligned_to(d_res, 4) || !aligned_to(d_rec_idx, 4) || !aligned_to(d_rec_cnt, 4))
        return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score_device: a pointer is not aligned to its element");
    HIPCHK(c, orb_enter(c));
    const int32_t *par;
    if (const int rc = ransac_upload_par(c, off, B, min_inliers, best_in, 0, &par, nullptr)) return rc;
    const OrbPnpPoints P = {(const float *)d_P3Dw, (const float *)d_P2D, (const float *)d_max_err, fu, fv, uc, vc};
    launch_pnp_score(c->stream, P, (const double *)d_Rt, M, par, B, (int32_t *)d_counts, nullptr, R, (int32_t *)d_res,
                     (int32_t *)d_rec_idx, (int32_t *)d_rec_cnt, (uint8_t *)d_rec_flags);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_sim3_score_device(orbhip_ctx *c, const void *d_X3Dc1, const void *d_X3Dc2, const void *d_P1im1, const void *d_P2im2,
                                        const void *d_max_err1, const void *d_max_err2, const int32_t *off, int B, const float *K1,
                                        const float *K2, const void *d_T, int M, const int32_t *min_inliers, const int32_t *best_in,
                                        void *d_counts, void *d_res, void *d_flags)
{
    if (!c || !K1 || !K2 || (B > 0 && (!off || !min_inliers || !d_res)) || (B > 0 && M > 0 && (!d_T || !d_counts)))
        return fail(c, ORBHIP_E_ARG, "orbhip_sim3_score_device: bad argument");
    if (const int rc = ransac_args_ok(c, "orbhip_sim3_score_device", off, B, M, min_inliers)) return rc;
    if (B == 0) return ORBHIP_OK;
    if (off[B] > 0 && (!d_X3Dc1 || !d_X3Dc2 || !d_P1im1 || !d_P2im2 || !d_max_err1 || !d_max_err2 || !d_flags))
        return fail(c, ORBHIP_E_ARG, "orbhip_sim3_score_device: bad argument");
    if (!aligned_to(d_X3Dc1, 4) || !aligned_to(d_X3Dc2, 4) || !aligned_to(d_P1im1, 4) || !aligned_to(d_P2im2, 4) ||
        !aligned_to(d_max_err1, 4) || !aligned_to(d_max_err2, 4) || !aligned_to(d_T, 4) || !aligned_to(d_counts, 4) || !aligned_to(d_res, 4))
        return fail(c, ORBHIP_E_ARG, "orbhip_sim3_score_device: a pointer is not 4-byte aligned");
    HIPCHK(c, orb_enter(c));
    const int32_t *par;
    if (const int rc = ransac_upload_par(c, off, B, min_inliers, best_in, 0, &par, nullptr)) return rc;
    OrbSim3Points P = {(const float *)d_X3Dc1,    (const float *)d_X3Dc2,    (const float *)d_P1im1, (const float *)d_P2im2,
                       (const float *)d_max_err1, (const float *)d_max_err2, {0, 0, 0, 0},           {0, 0, 0, 0}};
    memcpy(P.K1, K1, 16), memcpy(P.K2, K2, 16);
    launch_sim3_score(c->stream, P, (const float *)d_T, M, par, B, (int32_t *)d_counts, nullptr, (int32_t *)d_res, (uint8_t *)d_flags);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

// The host forms: one block up (the points, the hypotheses, off | min_inliers | best_in), the counts in device memory between the
// two kernels, and the results -- the copy of the counts, the record, the lists and the flag rows -- stored by k_ransac_pick
// straight into the page-locked block: one upload, two launches, one synchronisation.
extern "C" int orbhip_pnp_score(orbhip_ctx *c, const float *P3Dw, const float *P2D, const float *max_err, int N, double fu, double fv,
                                double uc, double vc, const double *Rt, int M, int min_inliers, int best_in, int R, int32_t *counts,
                                orbhip_pnp_result *res, int32_t *rec_idx, int32_t *rec_cnt, uint8_t *rec_flags)
{
    if (!c || !res || !rec_idx || !rec_cnt || (N > 0 && (!P3Dw || !P2D || !max_err || !rec_flags)) || (M > 0 && !Rt))
        return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score: bad argument");
    if (N < 0) return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score: negative count");
    if (R < 1) return fail(c, ORBHIP_E_ARG, "orbhip_pnp_score: R < 1");
    const int32_t off[2] = {0, N};
    int rc;
    if ((rc = ransac_args_ok(c, "orbhip_pnp_score", off, 1, M, &min_inliers))) return rc;
    HIPCHK(c, orb_enter(c));
    const int Reff = std::min(R, std::max(M, 1));                           // no more records than hypotheses
    Packed P(c);
    if ((rc = P.begin((size_t)N * 24 + (size_t)M * (96 + 8) + (size_t)Reff * (8 + (size_t)N) + 16 * 256))) return rc;
    const int32_t parH[4] = {0, N, min_inliers, best_in};
    const int32_t *par = (const int32_t *)P.in(parH, 16);
    OrbPnpPoints D = {(const float *)P.in(P3Dw, (size_t)N * 12), (const float *)P.in(P2D, (size_t)N * 8),
                      (const float *)P.in(max_err, (size_t)N * 4), fu, fv, uc, vc};
    const double *dRt = (const double *)P.in(Rt, (size_t)M * 96);
    int32_t *dCounts = (int32_t *)P.out((size_t)M * 4);                     // device only: read back by k_ransac_pick
    int32_t *hCounts = (int32_t *)P.out_host((size_t)M * 4);
    int32_t *hRes = (int32_t *)P.out_host(sizeof(orbhip_pnp_result));
    int32_t *hIdx = (int32_t *)P.out_host((size_t)Reff * 4), *hCnt = (int32_t *)P.out_host((size_t)Reff * 4);
    uint8_t *hFlags = (uint8_t *)P.out_host((size_t)Reff * N);
    if ((rc = P.upload())) return rc;
    launch_pnp_score(c->stream, D, dRt, M, par, 1, dCounts, hCounts, Reff, hRes, hIdx, hCnt, hFlags);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (counts) memcpy(counts, hCounts, (size_t)M * 4);
    memcpy(res, hRes, sizeof(orbhip_pnp_result));
    const int n = std::min(res->n_records, Reff);
    memcpy(rec_idx, hIdx, (size_t)n * 4);
    memcpy(rec_cnt, hCnt, (size_t)n * 4);
    if (N > 0) memcpy(rec_flags, hFlags, (size_t)n * N);
    return ORBHIP_OK;
}

extern "C" int orbhip_sim3_score(orbhip_ctx *c, const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2,
                                 const float *max_err1, const float *max_err2, int N, const float *K1, const float *K2, const float *T,
                                 int M, int min_inliers, int best_in, int32_t *counts, orbhip_sim3_result *res, uint8_t *flags)
{
    if (!c || !res || !K1 || !K2 || (N > 0 && (!X3Dc1 || !X3Dc2 || !P1im1 || !P2im2 || !max_err1 || !max_err2 || !flags)) || (M > 0 && !T))
        return fail(c, ORBHIP_E_ARG, "orbhip_sim3_score: bad argument");
    if (N < 0) return fail(c, ORBHIP_E_ARG, "orbhip_sim3_score: negative count");
    const int32_t off[2] = {0, N};
    int rc;
    if ((rc = ransac_args_ok(c, "orbhip_sim3_score", off, 1, M, &min_inliers))) return rc;
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    if ((rc = P.begin((size_t)N * (48 + 1) + (size_t)M * (96 + 8) + 16 * 256))) return rc;
    const int32_t parH[4] = {0, N, min_inliers, best_in};
    const int32_t *par = (const int32_t *)P.in(parH, 16);
    OrbSim3Points D = {(const float *)P.in(X3Dc1, (size_t)N * 12),  (const float *)P.in(X3Dc2, (size_t)N * 12),
                       (const float *)P.in(P1im1, (size_t)N * 8),   (const float *)P.in(P2im2, (size_t)N * 8),
                       (const float *)P.in(max_err1, (size_t)N * 4), (const float *)P.in(max_err2, (size_t)N * 4),
                       {0, 0, 0, 0},                                {0, 0, 0, 0}};
    memcpy(D.K1, K1, 16), memcpy(D.K2, K2, 16);
    const float *dT = (const float *)P.in(T, (size_t)M * 96);
    int32_t *dCounts = (int32_t *)P.out((size_t)M * 4);                     // device only
    int32_t *hCounts = (int32_t *)P.out_host((size_t)M * 4);
    int32_t *hRes = (int32_t *)P.out_host(sizeof(orbhip_sim3_result));
    uint8_t *hFlags = (uint8_t *)P.out_host((size_t)N);
    if ((rc = P.upload())) return rc;
    launch_sim3_score(c->stream, D, dT, M, par, 1, dCounts, hCounts, hRes, hFlags);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (counts) memcpy(counts, hCounts, (size_t)M * 4);
    memcpy(res, hRes, sizeof(orbhip_sim3_result));
    if (N > 0) memcpy(flags, hFlags, (size_t)N);
    return ORBHIP_OK;
}
