// kfdb_dev.h -- what k_kfdb.hip (device) and api_kfdb.hip (host) share: limits, status bits and the view of one key-frame
// database plus one batch of queries that every query kernel takes by value.
#ifndef ORBHIP_KFDB_DEV_H
#define ORBHIP_KFDB_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define KFDB_MAX_QWORDS 8192     // words of one BowVector (query or key frame)
#define KFDB_MAX_NEIGH 10        // GetBestCovisibilityKeyFrames(10)
#define KFDB_MAX_BATCH 1024
#define KFDB_PHASES 6          // walk | max | score | order | accumulate | retain + emit (orbhip_kfdb_phase_times)
#define KFDB_MODE_RELOC 0
#define KFDB_MODE_LOOP 1
#define KFDB_ST_QLEN 1           // a query has more than KFDB_MAX_QWORDS words
#define KFDB_ST_QWORD 2          // a query's word ids are not strictly ascending or not below nwords

struct KfdbView {
    // the database
    int nwords = 0, maxKfs = 0;
    const uint32_t *row = nullptr;      // [nwords + 1] CSR over word ids
    const uint32_t *post = nullptr;     // slots, sorted by (word, add sequence)
    const uint32_t *tomb = nullptr;     // erased slots, one bit each
    const uint4 *meta = nullptr;        // per slot: pool offset, word count, add sequence, 0
    const uint32_t *poolW = nullptr;    // BowVectors: word ids ascending | values
    const double *poolV = nullptr;
    const int32_t *delta = nullptr;     // slots added since the last rebuild, in add order
    int ndelta = 0;
    const uint64_t *nbKey = nullptr;    // [maxKfs * KFDB_MAX_NEIGH] covisibility neighbours (keys), best first
    const uint8_t *nbN = nullptr;       // [maxKfs]
    const uint64_t *mapKey = nullptr;   // sorted keys of the live key frames | their slots
    const uint32_t *mapSlot = nullptr;
    int nmap = 0;
    const uint64_t *slotKey = nullptr;  // [maxKfs]
    float *lastReloc = nullptr;         // [maxKfs] KeyFrame::mRelocScore of the last reloc query that scored the slot
    // the batch
    int B = 0;
    const int32_t *qoff = nullptr;      // [B + 1] query BowVectors as CSR
    const uint32_t *qw = nullptr;
    const double *qv = nullptr;
    const int32_t *xoff = nullptr;      // [B + 1] excluded keys per query
    const uint64_t *xkey = nullptr;
    // per (query, slot): B x maxKfs
    int32_t *cnt = nullptr;             // shared words (0 between calls)
    uint32_t *rank = nullptr;           // rank of the first shared query word (all ones between calls)
    float *score = nullptr;
    uint8_t *excl = nullptr;            // 0 between calls
    int32_t *firstPos = nullptr;        // INT_MAX between calls
    int32_t *touched = nullptr;         // per query: the slots met, in no particular order
    int32_t *ordered = nullptr;         // per query: the same slots in the reference's order
    float *accScore = nullptr;          // per query, by ordered position
    int32_t *accBest = nullptr;
    int32_t *cand = nullptr;
    // per (query, query word): B x KFDB_MAX_QWORDS
    int32_t *cntFirst = nullptr;        // key frames per first rank, then the start of each rank's run
    int32_t *csrFirst = nullptr;
    // per query
    int32_t *tcount = nullptr, *maxc = nullptr, *minc = nullptr, *outCnt = nullptr;
    int32_t *outOff = nullptr;          // [B + 1]
    uint64_t *outKeys = nullptr;
    int outCap = 0;
    int32_t *status = nullptr;
};

// k_kfdb.hip
void kfdb_scan(hipStream_t s, int32_t *a, int n, int32_t *scratch);
int kfdb_radix_sort(hipStream_t s, uint32_t *keys, uint32_t *vals, uint32_t *keys2, uint32_t *vals2, int n, int nwords,
                    int32_t *th, int32_t *scanScratch);
void kfdb_rows(hipStream_t s, const uint32_t *keys, int n, int nwords, uint32_t *row);
void kfdb_fold_expand(hipStream_t s, const int4 *items, int nitems, const uint32_t *oldW, const double *oldV, uint32_t *newW,
                      double *newV, uint32_t *keys, uint32_t *vals);
hipError_t kfdb_query_launch(hipStream_t s, const KfdbView &V, int ntotal, int nx, int mode, float minScore,
                             int stop_after_order, hipEvent_t *ev);
void kfdb_gather(hipStream_t s, const KfdbView &V, int32_t *counts, float *scores);
hipError_t kfdb_keep_reloc(hipStream_t s, const KfdbView &V);
hipError_t kfdb_query_reset(hipStream_t s, const KfdbView &V, int nx);

#endif
