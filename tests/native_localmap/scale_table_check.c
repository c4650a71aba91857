/* scale_table_check LOGS_BITS NLEVELS LO_BITS HI_BITS T0_BITS ... : for every float r in [lo, hi] (bit patterns of positive
 * floats, inclusive) compares the table-based level -- the number of k < nlevels - 1 with r >= T[k] -- with MapPoint::PredictScale,
 * ceil(logf(r) / logS) clamped to [0, nlevels - 1] (ref: src/MapPoint.cc:417-432).  Prints "checked mismatches transitions
 * downward". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float from_bits(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const float logS = from_bits((uint32_t)strtoul(argv[1], 0, 0));
    const int nlevels = atoi(argv[2]);
    const uint32_t lo = (uint32_t)strtoul(argv[3], 0, 0), hi = (uint32_t)strtoul(argv[4], 0, 0);
    if (argc != 5 + nlevels - 1 || nlevels < 1 || nlevels > 16) return 2;
    float T[16];
    for (int k = 0; k < nlevels - 1; k++) T[k] = from_bits((uint32_t)strtoul(argv[5 + k], 0, 0));
    unsigned long long checked = 0, bad = 0, trans = 0, down = 0;
    int prev = -1;
    for (uint32_t b = lo;; b++) {
        const float r = from_bits(b);
        int want = (int)ceilf(logf(r) / logS);
        if (want < 0) want = 0; else if (want >= nlevels) want = nlevels - 1;
        int got = 0;
        for (int k = 0; k < nlevels - 1; k++) got += r >= T[k] ? 1 : 0;
        if (got != want) bad++;
        if (prev >= 0 && want != prev) {
            trans++;
            if (want < prev) down++;
        }
        prev = want;
        checked++;
        if (b == hi) break;
    }
    printf("%llu %llu %llu %llu\n", checked, bad, trans, down);
    return 0;
}
