// The reference's two inlier loops and the bookkeeping around them, restated (host_loops.h), on a scene file: what the independent
// numpy model (tests/ransac_model.py) is compared with on the CPU.  No device.
//   ransac_host_loops <scene.bin> <out.bin>
// out.bin: int32 kind, N, M; counts [M] int32; flags [M][N] bytes (CheckInliers of every hypothesis on its own); then
// PnP: int32 n_records, best_out, the n_records indices, the n_records counts; Sim3: int32 winner, ninliers, best_it, best_out.
#include <cstdio>
#include <vector>

#include "host_loops.h"
#include "scene_io.h"

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]); return 2; }
    Scene s;
    if (!read_scene(argv[1], s)) return 2;
    const int N = s.N, M = s.M;
    std::vector<int> counts(M), tail;
    std::vector<unsigned char> flags((size_t)M * N), cur(N), bestFlags(N);
    for (int h = 0; h < M; h++)
        counts[h] = s.kind == 0 ? pnp_check_inliers(s.Rt.data() + 12 * h, s.P3Dw.data(), s.P2D.data(), s.maxErr.data(), N, s.cam[0], s.cam[1],
                                                    s.cam[2], s.cam[3], flags.data() + (size_t)h * N)
                                : sim3_check_inliers(s.T.data() + 24 * h, s.X1.data(), s.X2.data(), s.p1.data(), s.p2.data(), s.maxErr1.data(),
                                                     s.maxErr2.data(), N, s.K1, s.K2, flags.data() + (size_t)h * N);
    int best = s.bestIn;
    if (s.kind == 0) {
        std::vector<int> idx(M), cnt(M);
        const int n = pnp_iterate(s.Rt.data(), M, s.P3Dw.data(), s.P2D.data(), s.maxErr.data(), N, s.cam[0], s.cam[1], s.cam[2], s.cam[3],
                                  s.minInliers, &best, NULL, idx.data(), cnt.data(), cur.data(), bestFlags.data());
        tail.push_back(n), tail.push_back(best);
        tail.insert(tail.end(), idx.begin(), idx.begin() + n);
        tail.insert(tail.end(), cnt.begin(), cnt.begin() + n);
    } else {
        int bestIt;
        const int w = sim3_iterate(s.T.data(), M, s.X1.data(), s.X2.data(), s.p1.data(), s.p2.data(), s.maxErr1.data(), s.maxErr2.data(), N,
                                   s.K1, s.K2, s.minInliers, &best, &bestIt, NULL, cur.data(), bestFlags.data());
        const int r[4] = {w, w >= 0 ? counts[w] : 0, bestIt, best};
        tail.assign(r, r + 4);
    }
    const int head[3] = {s.kind, N, M};
    FILE *o = fopen(argv[2], "wb");
    const bool ok = o && put(o, head, 12) && put(o, counts.data(), (size_t)M * 4) && put(o, flags.data(), flags.size()) &&
                    put(o, tail.data(), tail.size() * 4);
    if (!ok || fclose(o)) { perror(argv[2]); return 2; }
    printf("ok %d %d %d\n", s.kind, N, M);
    return 0;
}
