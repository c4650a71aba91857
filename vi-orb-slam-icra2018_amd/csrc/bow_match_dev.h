// bow_match_dev.h -- one shared vocabulary node of ORBmatcher::SearchByBoW by one wave (ref: src/ORBmatcher.cc:159-288, :522-655).
// The matching arithmetic of SearchByBoW exists here once: k_bow_match (k_hamming.hip: one pair of key frames) and
// k_bow_match_cands (k_bowcand.hip: one fixed side against K candidates) both call it.  Device code only.
#ifndef ORBHIP_BOW_MATCH_DEV_H
#define ORBHIP_BOW_MATCH_DEV_H
#include "localmap_dev.h"   // kf_entry_slot
#include "wave_ops.h"

#define BOW_CLAIM_BITS 4096  // claimed-flags kept in LDS per wave (side-2 features of one node)

// How a side says "feature i has a map point that is not bad": a byte per feature, a byte per feature or no array at all
// (every feature counts), or the key frame's row of the resident table (orbhip_map_kf_*), asked through kf_entry_slot.
enum { BOW_V_BYTES = 0, BOW_V_BYTES_OR_ALL = 1, BOW_V_ROW = 2 };
struct BowValid {
    const uint8_t *bytes;      // BOW_V_BYTES, BOW_V_BYTES_OR_ALL
    const int2 *row;           // BOW_V_ROW: row[0].x = length, row[1 + i] = {slot, generation}
    const uint32_t *mflags;    // BOW_V_ROW: the store's flag words
    int maxPoints;
};
template <int V>
__device__ __forceinline__ bool bow_valid(const BowValid &v, int i)
{
    if (V == BOW_V_ROW) return kf_entry_slot(v.row[1 + i], v.mflags, v.maxPoints) >= 0;
    if (V == BOW_V_BYTES_OR_ALL) return !v.bytes || v.bytes[i];
    return v.bytes[i];
}

// Side-1 list entries [a0, a1) of idx1 against the n2 > 0 entries of idx2 from b0; claim: BOW_CLAIM_BITS / 32 words of LDS of this
// wave's own.  Three paths by n2: <= 128 in registers, <= BOW_CLAIM_BITS with the claimed flags in LDS, above that polling match21.
template <int V1, int V2>
__device__ __forceinline__ void bow_match_node(const uint8_t *__restrict__ desc1, const BowValid &valid1,
                                               const int32_t *__restrict__ idx1, const int a0, const int a1,
                                               const uint8_t *__restrict__ desc2, const BowValid &valid2,
                                               const int32_t *__restrict__ idx2, const int b0, const int n2, const int th,
                                               const int th_mode, const float nnratio, int32_t *__restrict__ match12,
                                               int32_t *__restrict__ match21, uint32_t *claim, const int lane)
{
    if (n2 <= 128) {
        // The usual node (a dozen features a side): the side-2 descriptors and the node's side-1 indices are loaded ONCE into
        // registers (lane p holds candidates p and p + 64), the claimed flags are lane-local, and the descriptor of the next
        // side-1 feature is requested while the current one is reduced -- a side-1 feature then costs one 6-step wave
        // reduction instead of two dependent trips to memory (a single SearchByBoW(KF, F) call: 97 -> ~25 us).
        uint32_t R[2][8];
        int I2[2];
        bool live[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int p = c * 64 + lane;
            live[c] = p < n2;
            I2[c] = idx2[b0 + min(p, n2 - 1)];
            if (!bow_valid<V2>(valid2, I2[c])) live[c] = false;
            const uint4 r0 = reinterpret_cast<const uint4 *>(desc2 + (size_t)I2[c] * 32)[0];
            const uint4 r1 = reinterpret_cast<const uint4 *>(desc2 + (size_t)I2[c] * 32)[1];
            R[c][0] = r0.x; R[c][1] = r0.y; R[c][2] = r0.z; R[c][3] = r0.w;
            R[c][4] = r1.x; R[c][5] = r1.y; R[c][6] = r1.z; R[c][7] = r1.w;
        }
        for (int abase = a0; abase < a1; abase += 64) {
            const int n1c = min(64, a1 - abase);
            const int myI1 = idx1[abase + min(lane, n1c - 1)];
            const int myV1 = bow_valid<V1>(valid1, myI1);
            // descriptor of the chunk's first feature, then always one ahead
            int i1n = __builtin_amdgcn_readlane(myI1, 0);
            uint4 q0n = reinterpret_cast<const uint4 *>(desc1 + (size_t)i1n * 32)[0];
            uint4 q1n = reinterpret_cast<const uint4 *>(desc1 + (size_t)i1n * 32)[1];
            for (int k = 0; k < n1c; k++) {
                const int i1 = i1n;
                const uint32_t Q[8] = {q0n.x, q0n.y, q0n.z, q0n.w, q1n.x, q1n.y, q1n.z, q1n.w};
                const int v1 = __builtin_amdgcn_readlane(myV1, k);   // (k is wave-uniform: v_readlane, not a trip through ds_bpermute)
                if (k + 1 < n1c) {
                    i1n = __builtin_amdgcn_readlane(myI1, k + 1);
                    q0n = reinterpret_cast<const uint4 *>(desc1 + (size_t)i1n * 32)[0];
                    q1n = reinterpret_cast<const uint4 *>(desc1 + (size_t)i1n * 32)[1];
                }
                if (!v1) continue;   // wave-uniform
                int bd1 = 256, bpos = 0x7FFFFFFF, bd2 = 256;
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    if (live[c]) {
                        const int d = hamming256(Q, R[c]);
                        if (d < bd1) {
                            bd2 = bd1;
                            bd1 = d;
                            bpos = c * 64 + lane;
                        } else if (d < bd2) {
                            bd2 = d;
                        }
                    }
                }
                {
                    // (best distance, lowest position) and the second smallest distance of the whole node: two wave minima --
                    // the winner by (distance, position), then every lane's best, the winner lane's second (r04: the butterfly
                    // of three shuffled values and six tie-aware merges was two thirds of a side-1 feature's instructions, and this
                    // loop is the serial chain the call waits for)
                    const int key = bpos != 0x7FFFFFFF ? ((bd1 << 8) | bpos) : 0x7FFFFFFF;
                    const int k1 = wave_min(key);
                    const int k2 = wave_min(key == k1 ? bd2 : bd1);
                    bd1 = k1 != 0x7FFFFFFF ? k1 >> 8 : 256;
                    bpos = k1 != 0x7FFFFFFF ? (k1 & 255) : 0x7FFFFFFF;
                    bd2 = k2;
                }
                const bool pass = th_mode ? (bd1 < th) : (bd1 <= th);
                if (pass && (float)bd1 < nnratio * (float)bd2) {  // ref: :228-230 / :598-600
#pragma unroll
                    for (int c = 0; c < 2; c++)
                        if (bpos == c * 64 + lane) {
                            live[c] = false;            // claimed (:233 / :603)
                            match12[i1] = I2[c];
                            match21[I2[c]] = i1;
                        }
                }
            }
        }
        return;
    }
    const bool useLds = n2 <= BOW_CLAIM_BITS;
    if (useLds)
        for (int k = lane; k < (n2 + 31) / 32; k += 64) claim[k] = 0;
    WAVE_LDS_SYNC();

    for (int a = a0; a < a1; a++) {
        const int i1 = idx1[a];
        if (!bow_valid<V1>(valid1, i1)) continue;  // wave-uniform
        uint32_t Q[8];
        {
            const uint32_t *row = reinterpret_cast<const uint32_t *>(desc1 + (size_t)i1 * 32);
#pragma unroll
            for (int k = 0; k < 8; k++) Q[k] = row[k];
        }
        int bd1 = 256, bpos = 0x7FFFFFFF, bd2 = 256;
        for (int p = lane; p < n2; p += 64) {
            const int i2 = idx2[b0 + p];
            bool skip;
            if (useLds)
                skip = (claim[p >> 5] >> (p & 31)) & 1u;
            else
                skip = __atomic_load_n(&match21[i2], __ATOMIC_RELAXED) >= 0;
            if (!bow_valid<V2>(valid2, i2)) skip = true;
            if (skip) continue;
            const uint4 r0 = reinterpret_cast<const uint4 *>(desc2 + (size_t)i2 * 32)[0];
            const uint4 r1 = reinterpret_cast<const uint4 *>(desc2 + (size_t)i2 * 32)[1];
            const uint32_t R[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            const int d = hamming256(Q, R);
            if (d < bd1) {
                bd2 = bd1;
                bd1 = d;
                bpos = p;
            } else if (d < bd2) {
                bd2 = d;
            }
        }
        {
            const int key = bpos != 0x7FFFFFFF ? ((bd1 << 20) | bpos) : 0x7FFFFFFF;   // (a FeatureVector of < 2^20 entries: the entry points check)
            const int k1 = wave_min(key);
            const int k2 = wave_min(key == k1 ? bd2 : bd1);
            bd1 = k1 != 0x7FFFFFFF ? k1 >> 20 : 256;
            bpos = k1 != 0x7FFFFFFF ? (k1 & 0xFFFFF) : 0x7FFFFFFF;
            bd2 = k2;
        }
        const bool pass = th_mode ? (bd1 < th) : (bd1 <= th);
        if (pass && (float)bd1 < nnratio * (float)bd2) {  // ref: :228-230 / :598-600
            const int i2 = idx2[b0 + bpos];
            if (lane == 0) {
                match12[i1] = i2;
                if (useLds)
                    claim[bpos >> 5] |= 1u << (bpos & 31);
                __atomic_store_n(&match21[i2], i1, __ATOMIC_RELAXED);
            }
            if (!useLds) __threadfence();
            WAVE_LDS_SYNC();
        }
    }
}

#endif
