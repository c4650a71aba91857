// api_initscore.hip -- C ABI, part 12: the monocular initialiser's RANSAC hypotheses scored in one call (orbhip_init_score[_device];
// kernels in k_initscore.hip).  The caller computes the H21i / H12i / F21i of all iterations first -- they
// depend on mvSets alone -- and gets back what the 2 x 200 calls of CheckHomography / CheckFundamental (ref: src/Initializer.cc:305-468)
// and the `currentScore > score` updates around them (:148-171, :199-222) would have left.
#include "api_common.h"

static bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

// what both forms ask of the counts and of sigma; invSigmaSquare as the reference forms it (:335, :411): the product in float,
// the quotient in double, rounded to float
static int score_args_ok(orbhip_ctx *c, const char *who, int nH, int nF, float sigma, float *invSigmaSquare)
{
    if (nH < 0 || nF < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": negative count");
    if ((long long)nH + nF > 65535) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65535 hypotheses");
    if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": sigma must be finite and > 0");
    const float sigma2 = sigma * sigma;
    *invSigmaSquare = (float)(1.0 / (double)sigma2);
    return ORBHIP_OK;
}

extern "C" int orbhip_init_score_device(orbhip_ctx *c, const void *d_kps1_un, const void *d_cnt1, int cap1, const void *d_kps2_un,
                                        const void *d_cnt2, int cap2, int B, const void *d_match12, const void *d_H21,
                                        const void *d_H12, int nH, const void *d_F21, int nF, float sigma, void *d_scores,
                                        void *d_best, void *d_inliers)
{
    if (!c || !d_kps1_un || !d_cnt1 || !d_kps2_un || !d_cnt2 || !d_match12 || !d_scores || !d_best || !d_inliers || cap1 <= 0 ||
        cap2 <= 0 || B <= 0 || B > 65535 || (nH > 0 && (!d_H21 || !d_H12)) || (nF > 0 && !d_F21))
        return fail(c, ORBHIP_E_ARG, "orbhip_init_score_device: bad argument");
    float inv;
    if (const int rc = score_args_ok(c, "orbhip_init_score_device", nH, nF, sigma, &inv)) return rc;
    if (!aligned4(d_kps1_un) || !aligned4(d_cnt1) || !aligned4(d_kps2_un) || !aligned4(d_cnt2) || !aligned4(d_match12) ||
        !aligned4(d_H21) || !aligned4(d_H12) || !aligned4(d_F21) || !aligned4(d_scores) || !aligned4(d_best))
        return fail(c, ORBHIP_E_ARG, "orbhip_init_score_device: a pointer is not 4-byte aligned");
    HIPCHK(c, orb_enter(c));
    int rc;
    if ((rc = orb_match_scratch(c, init_score_scratch_bytes(B, cap1)))) return rc;
    launch_init_score(c->stream, d_kps1_un, (int)sizeof(orbhip_keypoint), (const int32_t *)d_cnt1, cap1, d_kps2_un,
                      (int)sizeof(orbhip_keypoint), (const int32_t *)d_cnt2, cap2, B, (const int32_t *)d_match12, (const float *)d_H21,
                      (const float *)d_H12, nH, (const float *)d_F21, nF, inv, (float *)d_scores, d_best, (uint8_t *)d_inliers,
                      c->d_match.as<void>());
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_init_score(orbhip_ctx *c, const orbhip_keypoint *kps1_un, int n1, const orbhip_keypoint *kps2_un, int n2,
                                 const int32_t *match12, const float *H21, const float *H12, int nH, const float *F21, int nF,
                                 float sigma, float *scores, orbhip_init_best *best, uint8_t *inliers)
{
    if (!c || n1 < 0 || n2 < 0 || !best || (n1 > 0 && (!kps1_un || !match12 || !inliers)) || (n2 > 0 && !kps2_un) ||
        (nH > 0 && (!H21 || !H12)) || (nF > 0 && !F21))
        return fail(c, ORBHIP_E_ARG, "orbhip_init_score: bad argument");
    float inv;
    int rc;
    if ((rc = score_args_ok(c, "orbhip_init_score", nH, nF, sigma, &inv))) return rc;
    for (int i = 0; i < n1; i++)
        if (match12[i] >= n2) return fail(c, ORBHIP_E_ARG, "orbhip_init_score: a match is not a feature of frame 2");
    HIPCHK(c, orb_enter(c));
    // One block up: the (x, y) of both frames' keypoints, the counts, the matches and the hypotheses.  The kernels store the
    // scores, the two records and the inlier bytes straight into the page-locked block (a few KB of plain stores; no copy node
    // behind the last kernel), so the call is one upload, three launches and one synchronisation.
    const int cap1 = std::max(n1, 1), cap2 = std::max(n2, 1), nHyp = nH + nF;
    Packed P(c);
    if ((rc = P.begin((size_t)cap1 * (8 + 4 + 2) + (size_t)cap2 * 8 + (size_t)nH * 72 + (size_t)nF * 36 + (size_t)nHyp * 4 +
                      init_score_scratch_bytes(1, cap1) + 16 * 256)))
        return rc;
    float *h1, *h2;
    const void *d1 = P.in_reserve((size_t)cap1 * 8, (void **)&h1), *d2 = P.in_reserve((size_t)cap2 * 8, (void **)&h2);
    for (int i = 0; i < n1; i++) h1[2 * i] = kps1_un[i].x, h1[2 * i + 1] = kps1_un[i].y;
    for (int i = 0; i < n2; i++) h2[2 * i] = kps2_un[i].x, h2[2 * i + 1] = kps2_un[i].y;
    const int32_t cnts[4] = {n1, n2, 0, 0};
    const int32_t *dc = (const int32_t *)P.in(cnts, 16);
    const int32_t *dm = (const int32_t *)P.in(match12, (size_t)n1 * 4);
    const float *dH21 = (const float *)P.in(H21, (size_t)nH * 36), *dH12 = (const float *)P.in(H12, (size_t)nH * 36);
    const float *dF21 = (const float *)P.in(F21, (size_t)nF * 36);
    void *scratch = P.out(init_score_scratch_bytes(1, cap1));   // device only: the compacted pairs
    float *hs = (float *)P.out_host((size_t)nHyp * 4);
    orbhip_init_best *hb = (orbhip_init_best *)P.out_host(2 * sizeof(orbhip_init_best));
    uint8_t *hi = (uint8_t *)P.out_host((size_t)2 * cap1);
    if ((rc = P.upload())) return rc;
    launch_init_score(c->stream, d1, 8, dc, cap1, d2, 8, dc + 1, cap2, 1, dm, dH21, dH12, nH, dF21, nF, inv, hs, hb, hi, scratch);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (scores) memcpy(scores, hs, (size_t)nHyp * 4);
    memcpy(best, hb, 2 * sizeof(orbhip_init_best));
    if (n1 > 0) memcpy(inliers, hi, (size_t)2 * n1);   // (cap1 == n1)
    return ORBHIP_OK;
}
