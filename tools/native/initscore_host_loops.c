/* What orbhip_init_score replaces, as it runs on a host core: for each of n hypotheses a walk over all N matches with two
 * chi-square terms per match and a running float score (ref: src/Initializer.cc:305-468, restated).  tools/initscore_latency.py
 * compiles this file (g++ -O3 -march=native -ffp-contract=off) and times the two loops, one thread each. */
typedef struct { float u1, v1, u2, v2; } pair_t;

static float chi_transfer(const float *m, float su, float sv, float tu, float tv, float inv)
{
    const float w = 1.0 / (m[6] * su + m[7] * sv + m[8]);
    const float x = (m[0] * su + m[1] * sv + m[2]) * w, y = (m[3] * su + m[4] * sv + m[5]) * w;
    return ((tu - x) * (tu - x) + (tv - y) * (tv - y)) * inv;
}

static float chi_line(float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2, float su, float sv,
                      float tu, float tv, float inv)
{
    const float a = a0 * su + a1 * sv + a2, b = b0 * su + b1 * sv + b2, c = c0 * su + c1 * sv + c2;
    const float num = a * tu + b * tv + c;
    return num * num / (a * a + b * b) * inv;
}

/* scores[h] and, for the best hypothesis so far, the inlier flags: the loop FindHomography runs */
int host_score_h(const pair_t *p, int N, const float *H21, const float *H12, int n, float sigma, float *scores, unsigned char *inl,
                 unsigned char *cur)
{
    const float th = 5.991, inv = 1.0 / (sigma * sigma);
    float best = 0;
    int it = -1;
    for (int h = 0; h < n; h++) {
        float s = 0;
        for (int k = 0; k < N; k++) {
            const float c1 = chi_transfer(H12 + 9 * h, p[k].u2, p[k].v2, p[k].u1, p[k].v1, inv);
            const float c2 = chi_transfer(H21 + 9 * h, p[k].u1, p[k].v1, p[k].u2, p[k].v2, inv);
            unsigned char in = 1;
            if (c1 > th) in = 0; else s += th - c1;
            if (c2 > th) in = 0; else s += th - c2;
            cur[k] = in;
        }
        scores[h] = s;
        if (s > best) {
            best = s, it = h;
            for (int k = 0; k < N; k++) inl[k] = cur[k];
        }
    }
    return it;
}

/* the loop FindFundamental runs */
int host_score_f(const pair_t *p, int N, const float *F21, int n, float sigma, float *scores, unsigned char *inl, unsigned char *cur)
{
    const float th = 3.841, thScore = 5.991, inv = 1.0 / (sigma * sigma);
    float best = 0;
    int it = -1;
    for (int h = 0; h < n; h++) {
        const float *F = F21 + 9 * h;
        float s = 0;
        for (int k = 0; k < N; k++) {
            const float c1 = chi_line(F[0], F[1], F[2], F[3], F[4], F[5], F[6], F[7], F[8], p[k].u1, p[k].v1, p[k].u2, p[k].v2, inv);
            const float c2 = chi_line(F[0], F[3], F[6], F[1], F[4], F[7], F[2], F[5], F[8], p[k].u2, p[k].v2, p[k].u1, p[k].v1, inv);
            unsigned char in = 1;
            if (c1 > th) in = 0; else s += thScore - c1;
            if (c2 > th) in = 0; else s += thScore - c2;
            cur[k] = in;
        }
        scores[h] = s;
        if (s > best) {
            best = s, it = h;
            for (int k = 0; k < N; k++) inl[k] = cur[k];
        }
    }
    return it;
}
