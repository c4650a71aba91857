/* The loops orbhip_pnp_score / orbhip_sim3_score replace, as they run on a host core: one walk over all N correspondences per
 * hypothesis (ref: src/PnPsolver.cc:308-339; src/Sim3Solver.cc:340-403, restated without OpenCV: the 3x3 gemm of Project accumulates
 * in double and rounds once, Mat::dot accumulates in double) and the bookkeeping of the two iterate() loops around them (:209-225,
 * :183-200).  Plain C, so that tools/native/ransac_host_loops.c can time the same text.  Build with -ffp-contract=off. */
#ifndef ORBHIP_TESTS_RANSAC_HOST_LOOPS_H
#define ORBHIP_TESTS_RANSAC_HOST_LOOPS_H

/* Rt: R[9] row-major | t[3].  in[N] <- the flags; returns their number. */
static int pnp_check_inliers(const double *Rt, const float *P3Dw, const float *P2D, const float *maxErr, int N, double fu, double fv,
                             double uc, double vc, unsigned char *in)
{
    int n = 0;
    for (int i = 0; i < N; i++) {
        const float X = P3Dw[3 * i], Y = P3Dw[3 * i + 1], Z = P3Dw[3 * i + 2];
        const float Xc = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9];
        const float Yc = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10];
        const float invZc = 1 / (Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11]);
        const double ue = uc + fu * Xc * invZc;
        const double ve = vc + fv * Yc * invZc;
        const float distX = P2D[2 * i] - ue;
        const float distY = P2D[2 * i + 1] - ve;
        const float error2 = distX * distX + distY * distY;
        in[i] = error2 < maxErr[i];
        n += in[i];
    }
    return n;
}

/* T: a 3x4 block, row-major; K: fx, fy, cx, cy */
static void sim3_project(const float *T, const float *X, const float *K, float *uv)
{
    float Pc[3];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T[4 * r + k] * (double)X[k];
        Pc[r] = (float)(s + (double)T[4 * r + 3]);
    }
    const float invz = 1 / Pc[2];
    const float x = Pc[0] * invz;
    const float y = Pc[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}

static float sim3_dot(const float *d)
{
    double s = 0;
    for (int k = 0; k < 2; k++) s += (double)d[k] * d[k];
    return (float)s;
}

/* T: the 3x4 block of T12 | of T21 */
static int sim3_check_inliers(const float *T, const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2,
                              const float *maxErr1, const float *maxErr2, int N, const float *K1, const float *K2, unsigned char *in)
{
    int n = 0;
    for (int i = 0; i < N; i++) {
        float p2im1[2], p1im2[2];
        sim3_project(T, X3Dc2 + 3 * i, K1, p2im1);
        sim3_project(T + 12, X3Dc1 + 3 * i, K2, p1im2);
        const float dist1[2] = {P1im1[2 * i] - p2im1[0], P1im1[2 * i + 1] - p2im1[1]};
        const float dist2[2] = {p1im2[0] - P2im2[2 * i], p1im2[1] - P2im2[2 * i + 1]};
        const float err1 = sim3_dot(dist1), err2 = sim3_dot(dist2);
        in[i] = err1 < maxErr1[i] && err2 < maxErr2[i];
        n += in[i];
    }
    return n;
}

/* PnPsolver::iterate's bookkeeping over M hypotheses: cur / bestFlags are N bytes each; recIdx / recCnt take every record (M
 * entries at most).  Returns the number of records; *best: in best_in, out best_out. */
static int pnp_iterate(const double *Rt, int M, const float *P3Dw, const float *P2D, const float *maxErr, int N, double fu, double fv,
                       double uc, double vc, int minInliers, int *best, int *counts, int *recIdx, int *recCnt, unsigned char *cur,
                       unsigned char *bestFlags)
{
    int nrec = 0;
    for (int h = 0; h < M; h++) {
        const int n = pnp_check_inliers(Rt + 12 * h, P3Dw, P2D, maxErr, N, fu, fv, uc, vc, cur);
        if (counts) counts[h] = n;
        if (n >= minInliers) {
            if (n > *best) {
                for (int i = 0; i < N; i++) bestFlags[i] = cur[i];
                *best = n;
                recIdx[nrec] = h, recCnt[nrec] = n;
                nrec++;
            }
        }
    }
    return nrec;
}

/* Sim3Solver::iterate's bookkeeping: returns the winner or -1; *best in / out, *bestIt the last hypothesis that reached best (-1:
 * none); bestFlags: mvbBestInliers.  Stops at the winner: counts beyond it are not written. */
static int sim3_iterate(const float *T, int M, const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2,
                        const float *maxErr1, const float *maxErr2, int N, const float *K1, const float *K2, int minInliers, int *best,
                        int *bestIt, int *counts, unsigned char *cur, unsigned char *bestFlags)
{
    *bestIt = -1;
    for (int h = 0; h < M; h++) {
        const int n = sim3_check_inliers(T + 24 * h, X3Dc1, X3Dc2, P1im1, P2im2, maxErr1, maxErr2, N, K1, K2, cur);
        if (counts) counts[h] = n;
        if (n >= *best) {
            for (int i = 0; i < N; i++) bestFlags[i] = cur[i];
            *best = n;
            *bestIt = h;
            if (n > minInliers) return h;
        }
    }
    return -1;
}

#endif
