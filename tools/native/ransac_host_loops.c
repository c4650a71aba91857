/* What orbhip_pnp_score / orbhip_sim3_score replace, as it runs on a host core: the two iterate() loops of
 * tests/native_ransac/host_loops.h with external linkage.  tools/ransac_latency.py compiles this file (g++ -O3 -march=native
 * -ffp-contract=off) and times the loops in the process that times the device calls. */
#include "../../tests/native_ransac/host_loops.h"

#ifdef __cplusplus
extern "C" {
#endif
int host_pnp_iterate(const double *Rt, int M, const float *P3Dw, const float *P2D, const float *maxErr, int N, const double *cam,
                     int minInliers, int bestIn, int *counts, int *recIdx, int *recCnt, unsigned char *cur, unsigned char *bestFlags,
                     int *bestOut)
{
    int best = bestIn;
    const int n = pnp_iterate(Rt, M, P3Dw, P2D, maxErr, N, cam[0], cam[1], cam[2], cam[3], minInliers, &best, counts, recIdx, recCnt, cur,
                              bestFlags);
    *bestOut = best;
    return n;
}

int host_sim3_iterate(const float *T, int M, const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2,
                      const float *maxErr1, const float *maxErr2, int N, const float *K1, const float *K2, int minInliers, int bestIn,
                      int *counts, unsigned char *cur, unsigned char *bestFlags, int *bestIt, int *bestOut)
{
    int best = bestIn;
    const int w = sim3_iterate(T, M, X3Dc1, X3Dc2, P1im1, P2im2, maxErr1, maxErr2, N, K1, K2, minInliers, &best, bestIt, counts, cur,
                               bestFlags);
    *bestOut = best;
    return w;
}
#ifdef __cplusplus
}
#endif
