// mock_correct.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch::CorrectLoopPoints / ApplyGlobalBA call, for the
// programs that run them without a device (test_correct_mock, test_correct_mock_asan): the store and everything else the class
// links is the model of tests/native_refresh/mock_refresh.cc, included here as it stands; orbhip_map_correct_sim3 and
// orbhip_map_correct_se3 are restated over that store as include/orbhip.h states them -- the rank rule, not the sequence -- with the
// library's argument checks.  Built with -ffp-contract=off: every operation is rounded on its own.
#include "../native_refresh/mock_refresh.cc"

namespace
{
void sim3_map(const orbhip_sim3d &S, double v[3])
{
    const double *q = S.q;
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int i = 0; i < 3; i++) uv[i] += uv[i];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int i = 0; i < 3; i++) v[i] = S.s * ((v[i] + q[3] * uv[i]) + c[i]) + S.t[i];
}

void gemm3(const float *R, const float *t, const float x[3], float out[3])
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)R[3 * r + k] * (double)x[k];
        out[r] = (float)(s + (double)t[r]);
    }
}

bool keys_ok(int P, const uint64_t *point_keys)
{
    std::set<uint64_t> seen;
    for (int p = 0; p < P; p++)
        if (!g.points.count(point_keys[p]) || !seen.insert(point_keys[p]).second) return false;
    return true;
}
}  // namespace

extern "C" {
int orbhip_map_correct_sim3(orbhip_ctx *, const orbhip_refresh_params *prm, int K, const orbhip_correct_xf *xf, int nkf,
                            const orbhip_correct_kf *kfs, int P, const uint64_t *point_keys, const int32_t *corr, const int32_t *off,
                            const int32_t *obs_kf, const int32_t *ref_pos, const uint8_t *ref_level, uint8_t *status, float *pos_out,
                            float *normal_out, float *min_dist_out, float *max_dist_out)
{
    if (!prm || nkf < 0 || P < 0 || K < 0) return ORBHIP_E_ARG;
    if (P == 0) return ORBHIP_OK;
    if (K < 1 || prm->nlevels < 1 || prm->nlevels > 16 || off[0] != 0) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++)
        if (off[p + 1] < off[p]) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++)
        if (off[p + 1] - off[p] >= (1 << 20)) return ORBHIP_E_SIZE;
    if (!keys_ok(P, point_keys)) return ORBHIP_E_ARG;
    std::set<int> ranks;
    for (int k = 0; k < nkf; k++)
        if (kfs[k].rank < -1 || kfs[k].rank >= K || (kfs[k].rank >= 0 && !ranks.insert(kfs[k].rank).second)) return ORBHIP_E_ARG;
    for (int j = 0; j < off[P]; j++)
        if (obs_kf[j] < 0 || obs_kf[j] >= nkf) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++) {
        const int N = off[p + 1] - off[p];
        if (corr[p] < 0 || corr[p] >= K || ref_level[p] >= prm->nlevels || (N > 0 && (ref_pos[p] < 0 || ref_pos[p] >= N))) return ORBHIP_E_ARG;
    }

    for (int p = 0; p < P; p++) {
        Point &Q = g.points[point_keys[p]];
        const int s = off[p], N = off[p + 1] - s, c = corr[p];
        int st = 0;
        if (!(Q.flags & ORBHIP_MP_BAD)) {
            double v[3] = {Q.pos[0], Q.pos[1], Q.pos[2]};
            sim3_map(xf[c].Siw, v);
            sim3_map(xf[c].corrected_Swi, v);
            for (int i = 0; i < 3; i++) Q.pos[i] = (float)v[i];
            st = 1;
            if (N > 0) {
                float normal[3] = {0.f, 0.f, 0.f}, dist = 0.f;
                for (int j = 0; j < N; j++) {
                    const orbhip_correct_kf &F = kfs[obs_kf[s + j]];
                    const float *O = (F.rank >= 0 && F.rank < c) ? F.Ow_after : F.Ow_before;
                    const float d[3] = {Q.pos[0] - O[0], Q.pos[1] - O[1], Q.pos[2] - O[2]};
                    const float a = (float)(1.0 / norm3(d));
                    for (int i = 0; i < 3; i++) {
                        const float t = d[i] * a;
                        normal[i] = t + normal[i];
                    }
                    if (j == ref_pos[p]) dist = (float)norm3(d);
                }
                const float inv = (float)(1.0 / (double)N);
                Q.mx = dist * prm->scale_factors[ref_level[p]];
                Q.mn = Q.mx / prm->scale_factors[prm->nlevels - 1];
                for (int i = 0; i < 3; i++) Q.nrm[i] = normal[i] * inv;
                st = 3;
            }
        }
        status[p] = (uint8_t)st;
        if (pos_out) memcpy(pos_out + 3 * (size_t)p, Q.pos, 12);
        if (normal_out) memcpy(normal_out + 3 * (size_t)p, Q.nrm, 12);
        if (min_dist_out) min_dist_out[p] = Q.mn;
        if (max_dist_out) max_dist_out[p] = Q.mx;
    }
    return ORBHIP_OK;
}

int orbhip_map_correct_se3(orbhip_ctx *, int K, const orbhip_correct_se3 *xf, int P, const uint64_t *point_keys, const int32_t *corr,
                           const float *pos_set, uint8_t *status, float *pos_out)
{
    if (P < 0 || K < 0) return ORBHIP_E_ARG;
    if (P == 0) return ORBHIP_OK;
    for (int p = 0; p < P; p++)
        if (corr[p] < -1 || corr[p] >= K || (corr[p] == -1 && !pos_set)) return ORBHIP_E_ARG;
    if (!keys_ok(P, point_keys)) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++) {
        Point &Q = g.points[point_keys[p]];
        status[p] = 0;
        if (!(Q.flags & ORBHIP_MP_BAD)) {
            if (corr[p] < 0) {
                memcpy(Q.pos, pos_set + 3 * (size_t)p, 12);
            } else {
                float xc[3], out[3];
                gemm3(xf[corr[p]].Rcw_before, xf[corr[p]].tcw_before, Q.pos, xc);
                gemm3(xf[corr[p]].Rwc, xf[corr[p]].twc, xc, out);
                memcpy(Q.pos, out, 12);
            }
            status[p] = 1;
        }
        if (pos_out) memcpy(pos_out + 3 * (size_t)p, Q.pos, 12);
    }
    return ORBHIP_OK;
}
}
