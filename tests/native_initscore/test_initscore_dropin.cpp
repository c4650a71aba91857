// ORB_SLAM2::InitializerScore (one device call) against the loops it replaces, restated here on the host: for every hypothesis the
// symmetric transfer error / the two epipolar distances over the matches in order, the chi-square gates, the running float score,
// and the first-largest-score-above-zero rule around them (ref: src/Initializer.cc:148-171, :199-222, :305-468).
//   test_initscore_dropin <scene.bin> <out.bin>
// scene.bin: int32 n1, n2, nH, nF; float sigma; n1 + n2 keypoints (28 bytes each); n1 int32 matches; nH x 9 H21, nH x 9 H12,
// nF x 9 F21 floats.
// out.bin: int32 N, itH, itF; float SH, SF; N bytes vbMatchesInliersH, N bytes vbMatchesInliersF (mvMatches12 order), as the
// class returned them -- after this program found them equal to its own restatement.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "InitializerScore.h"
#include "hiperror.h"

using namespace ORB_SLAM2;

namespace
{
struct Match { float u1, v1, u2, v2; };

// squared distance between (tu, tv) and the image of (su, sv) under the 3x3 matrix m, over sigma^2
float transfer_chi(const float *m, float su, float sv, float tu, float tv, float invSigma2)
{
    const float winv = 1.0 / (m[6] * su + m[7] * sv + m[8]);
    const float pu = (m[0] * su + m[1] * sv + m[2]) * winv;
    const float pv = (m[3] * su + m[4] * sv + m[5]) * winv;
    const float d2 = (tu - pu) * (tu - pu) + (tv - pv) * (tv - pv);
    return d2 * invSigma2;
}

// squared distance of (tu, tv) to the line l = (r0, r1, r2) . (su, sv, 1), each r a triple of matrix entries, over sigma^2
float line_chi(const float *r0, const float *r1, const float *r2, int step, float su, float sv, float tu, float tv, float invSigma2)
{
    const float a = r0[0] * su + r0[step] * sv + r0[2 * step];
    const float b = r1[0] * su + r1[step] * sv + r1[2 * step];
    const float c = r2[0] * su + r2[step] * sv + r2[2 * step];
    const float num = a * tu + b * tv + c;
    const float d2 = num * num / (a * a + b * b);
    return d2 * invSigma2;
}

// one hypothesis: its score, and per match whether both gates let it through
float score_one(bool fundamental, const float *A, const float *Ainv, const std::vector<Match> &ms, float sigma, std::vector<bool> &in)
{
    const float gate = fundamental ? 3.841 : 5.991, reward = 5.991;
    const float invSigma2 = 1.0 / (sigma * sigma);
    float total = 0;
    in.assign(ms.size(), false);
    for (size_t k = 0; k < ms.size(); k++) {
        const Match &q = ms[k];
        float first, second;
        if (fundamental) {
            first = line_chi(A, A + 3, A + 6, 1, q.u1, q.v1, q.u2, q.v2, invSigma2);        // rows of F21 on x1, measured in image 2
            second = line_chi(A, A + 1, A + 2, 3, q.u2, q.v2, q.u1, q.v1, invSigma2);       // columns of F21 on x2, measured in image 1
        } else {
            first = transfer_chi(Ainv, q.u2, q.v2, q.u1, q.v1, invSigma2);                  // x2 into image 1
            second = transfer_chi(A, q.u1, q.v1, q.u2, q.v2, invSigma2);                    // x1 into image 2
        }
        bool good = true;
        if (first > gate) good = false; else total += reward - first;
        if (second > gate) good = false; else total += reward - second;
        in[k] = good;
    }
    return total;
}

bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int hdr[4];
    float sigma;
    if (!f || fread(hdr, 4, 4, f) != 4 || fread(&sigma, 4, 1, f) != 1) { perror(argv[1]); return 2; }
    const int n1 = hdr[0], n2 = hdr[1], nH = hdr[2], nF = hdr[3];
    std::vector<cv::KeyPoint> keys1(n1), keys2(n2);
    std::vector<int> matches(n1);
    std::vector<float> h21(9 * nH), h12(9 * nH), f21(9 * nF);
    static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");
    if (fread(keys1.data(), 28, n1, f) != (size_t)n1 || fread(keys2.data(), 28, n2, f) != (size_t)n2 ||
        fread(matches.data(), 4, n1, f) != (size_t)n1 || fread(h21.data(), 4, h21.size(), f) != h21.size() ||
        fread(h12.data(), 4, h12.size(), f) != h12.size() || fread(f21.data(), 4, f21.size(), f) != f21.size())
    { fprintf(stderr, "short scene file\n"); return 2; }
    fclose(f);

    // the integrator's side: cv::Mat hypotheses, one call
    std::vector<cv::Mat> vH21, vH12, vF21;
    for (int i = 0; i < nH; i++) {
        vH21.push_back(cv::Mat(3, 3, CV_32F, h21.data() + 9 * i).clone());
        vH12.push_back(cv::Mat(3, 3, CV_32F, h12.data() + 9 * i).clone());
    }
    for (int i = 0; i < nF; i++) vF21.push_back(cv::Mat(3, 3, CV_32F, f21.data() + 9 * i).clone());
    InitializerScore scorer;
    InitializerScore::Result R;
    if (!scorer.Score(keys1, keys2, matches, vH21, vH12, vF21, sigma, R) || OrbHipErrorCount())
    { fprintf(stderr, "InitializerScore::Score failed: %s\n", OrbHipLastError()); return 1; }

    // the restatement: the matched pairs in frame-1 order, then hypothesis after hypothesis
    std::vector<Match> ms;
    for (int i = 0; i < n1; i++)
        if (matches[i] >= 0) {
            const Match q = {keys1[i].pt.x, keys1[i].pt.y, keys2[matches[i]].pt.x, keys2[matches[i]].pt.y};
            ms.push_back(q);
        }
    const size_t N = ms.size();
    if (R.vbMatchesInliersH.size() != N || R.vbMatchesInliersF.size() != N || R.vScoresH.size() != (size_t)nH || R.vScoresF.size() != (size_t)nF)
    { fprintf(stderr, "result sizes: %zu / %zu flags for %zu matches\n", R.vbMatchesInliersH.size(), R.vbMatchesInliersF.size(), N); return 1; }
    for (int model = 0; model < 2; model++) {
        const int n = model ? nF : nH;
        float bestScore = 0;
        int bestIt = -1;
        std::vector<bool> bestIn(N, false), in;
        for (int it = 0; it < n; it++) {
            const float s = model ? score_one(true, f21.data() + 9 * it, nullptr, ms, sigma, in)
                                  : score_one(false, h21.data() + 9 * it, h12.data() + 9 * it, ms, sigma, in);
            const float got = model ? R.vScoresF[it] : R.vScoresH[it];
            if (!same_bits(s, got) && !(s != s && got != got))
            { fprintf(stderr, "model %d iteration %d: score %.9g, the class returned %.9g\n", model, it, s, got); return 1; }
            if (s > bestScore) bestScore = s, bestIt = it, bestIn = in;
        }
        const float gotScore = model ? R.SF : R.SH;
        const int gotIt = model ? R.itF : R.itH;
        const std::vector<bool> &gotIn = model ? R.vbMatchesInliersF : R.vbMatchesInliersH;
        if (!same_bits(bestScore, gotScore) || bestIt != gotIt || bestIn != gotIn)
        { fprintf(stderr, "model %d: winner %d (%.9g), the class returned %d (%.9g)%s\n", model, bestIt, bestScore, gotIt, gotScore, bestIn != gotIn ? ", other inliers" : ""); return 1; }
    }

    std::vector<unsigned char> inH(N), inF(N);
    for (size_t k = 0; k < N; k++) inH[k] = R.vbMatchesInliersH[k], inF[k] = R.vbMatchesInliersF[k];
    const int head[3] = {(int)N, R.itH, R.itF};
    const float sc[2] = {R.SH, R.SF};
    FILE *o = fopen(argv[2], "wb");
    const bool ok = o && put(o, head, 12) && put(o, sc, 8) && put(o, inH.data(), N) && put(o, inF.data(), N);
    if (!ok || fclose(o)) { perror(argv[2]); return 2; }
    printf("ok %zu %d %d\n", N, R.itH, R.itF);
    return 0;
}
