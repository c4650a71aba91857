// The scene file of the RANSAC-scoring tests (tests/ransac_scenes.py scene_bytes): int32 kind (0 PnP, 1 Sim3), N, M, min_inliers,
// best_in; PnP: P3Dw [N][3], P2D [N][2], max_err [N] float, cam {fu, fv, uc, vc} double, Rt [M][12] double; Sim3: X3Dc1, X3Dc2
// [N][3], P1im1, P2im2 [N][2], max_err1, max_err2 [N], K1, K2 {fx, fy, cx, cy}, T [M][24], all float.
#ifndef ORBHIP_TESTS_RANSAC_SCENE_IO_H
#define ORBHIP_TESTS_RANSAC_SCENE_IO_H
#include <cstdio>
#include <vector>

struct Scene {
    int kind, N, M, minInliers, bestIn;
    std::vector<float> P3Dw, P2D, maxErr;                             // PnP
    double cam[4];
    std::vector<double> Rt;
    std::vector<float> X1, X2, p1, p2, maxErr1, maxErr2, T;          // Sim3
    float K1[4], K2[4];
};

template <typename V> static bool get(FILE *f, std::vector<V> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(V), n, f) == n;
}

static bool read_scene(const char *path, Scene &s)
{
    FILE *f = fopen(path, "rb");
    int hdr[5];
    if (!f || fread(hdr, 4, 5, f) != 5) { perror(path); return false; }
    s.kind = hdr[0], s.N = hdr[1], s.M = hdr[2], s.minInliers = hdr[3], s.bestIn = hdr[4];
    const size_t N = s.N, M = s.M;
    bool ok;
    if (s.kind == 0)
        ok = get(f, s.P3Dw, 3 * N) && get(f, s.P2D, 2 * N) && get(f, s.maxErr, N) && fread(s.cam, 8, 4, f) == 4 && get(f, s.Rt, 12 * M);
    else
        ok = get(f, s.X1, 3 * N) && get(f, s.X2, 3 * N) && get(f, s.p1, 2 * N) && get(f, s.p2, 2 * N) && get(f, s.maxErr1, N) &&
             get(f, s.maxErr2, N) && fread(s.K1, 4, 4, f) == 4 && fread(s.K2, 4, 4, f) == 4 && get(f, s.T, 24 * M);
    fclose(f);
    if (!ok) fprintf(stderr, "short scene file\n");
    return ok;
}

static bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

#endif
