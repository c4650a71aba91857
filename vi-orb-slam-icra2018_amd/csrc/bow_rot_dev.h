// bow_rot_dev.h -- the rotation-consistency check of the matchers on the device (SearchByBoW, ref: src/ORBmatcher.cc:236-246,
// :267-285; SearchByProjection, :1458-1494; SearchForInitialization, :473-507; ComputeThreeMaxima :1629-1670): the bin of a match
// and the three bins that survive.  One copy for k_bow_seq, k_bow_lane (k_bowseq.hip), k_bow_rot_cands (k_bowcand.hip) and
// k_proj_assign, k_proj_assign_par, k_init_assign (k_guided.hip).  The name is the first user's.  Device code only.
#ifndef ORBHIP_BOW_ROT_DEV_H
#define ORBHIP_BOW_ROT_DEV_H
#include <hip/hip_runtime.h>

#define BS_HISTO 30

// the histogram bin of a match whose side-1 / side-2 keypoints have these angles (degrees); float operations as in the reference
__device__ __forceinline__ int bow_rot_bin(float angle1, float angle2)
{
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / BS_HISTO));
    if (bin == BS_HISTO) bin = 0;
    return bin;
}

// ComputeThreeMaxima over hist[BS_HISTO] by one thread: keep[0..2] = ind1, ind2, ind3 (-1: none)
__device__ __forceinline__ void bow_three_maxima(const int *hist, int *keep)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < BS_HISTO; i++) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            i3 = i2; i2 = i1; i1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            i3 = i2; i2 = i;
        } else if (s > max3) {
            max3 = s;
            i3 = i;
        }
    }
    if ((float)max2 < 0.1f * (float)max1) {
        i2 = -1;
        i3 = -1;
    } else if ((float)max3 < 0.1f * (float)max1) {
        i3 = -1;
    }
    keep[0] = i1;
    keep[1] = i2;
    keep[2] = i3;
}

// does a match of this bin survive?  (a bin outside [0, BS_HISTO) was never entered in the histogram and is never cleared)
__device__ __forceinline__ bool bow_rot_keeps(int bin, const int *keep)
{
    return !(bin >= 0 && bin < BS_HISTO && bin != keep[0] && bin != keep[1] && bin != keep[2]);
}

#endif
