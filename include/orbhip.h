/*
 * orbhip.h -- C ABI of liborbhip.so: the MI355X (gfx950) ORB front end and Hamming matcher.
 *
 * This is the drop-in boundary for ONE hot path of hwb0314/VI-ORB-SLAM-ICRA2018:
 * ORBextractor::operator() and ORBmatcher's descriptor matching.  The C++ classes
 * ORB_SLAM2::ORBextractor / ORB_SLAM2::ORBmatcher in include/orbhip/ keep the reference's
 * signatures and forward to these entry points (INTEGRATION.md shows the binding).
 *
 * Plain pointers and sizes only; no C++/torch types.  Unless a name ends in _device every
 * pointer is a HOST pointer and the call is synchronous.  *_device entry points take device
 * pointers, enqueue on the context's HIP stream and return without synchronising; call
 * orbhip_sync() before reading results.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).
 *
 * Errors: 0 = ok, negative = error (see ORBHIP_E_*); orbhip_last_error() gives the text.
 * There is no CPU fallback: without a usable HIP device orbhip_create() fails.
 * Threading: one context = one extractor instance = one HIP stream; a context is not
 * re-entrant (same as the reference class, which mutates mvImagePyramid), different contexts
 * may be used concurrently from different host threads (src/Frame.cc:422-425 does this for
 * stereo).
 */
#ifndef ORBHIP_H
#define ORBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBHIP_OK 0
#define ORBHIP_E_ARG (-1)       /* bad argument */
#define ORBHIP_E_SIZE (-2)      /* image larger than the context or too small for the cell grid */
#define ORBHIP_E_CAPACITY (-3)  /* output capacity too small */
#define ORBHIP_E_HIP (-4)       /* HIP runtime error */
#define ORBHIP_E_NODEVICE (-5)  /* no HIP device / wrong architecture */
#define ORBHIP_E_COMM (-6)      /* RCCL error */

#define ORBHIP_MAX_LEVELS 16

typedef struct orbhip_ctx orbhip_ctx;

/* Binary layout of cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave,
 * class_id.  Replaces std::vector<cv::KeyPoint>& of include/ORBextractor.h:77-79. */
typedef struct orbhip_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbhip_keypoint;

/* A FAST candidate before quadtree distribution (debug/parity access): coordinates relative
 * to (16,16) of the level as in src/ORBextractor.cc:822-827, and the FAST score. */
typedef struct orbhip_cand {
    int32_t x, y, score;
} orbhip_cand;

/* Number of visible HIP devices (0 if none). */
int orbhip_device_count(void);

/* Replaces ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels,
 * int iniThFAST, int minThFAST) (include/ORBextractor.h:69-70, src/ORBextractor.cc:412-472).
 * max_w/max_h bound the image size, max_batch the frames per batched call; all device
 * buffers are allocated here, none in the per-frame calls.  Returns NULL on failure
 * (orbhip_last_error(NULL) has the reason).  Limits (ORBHIP_E_SIZE): every pyramid level must hold at least one
 * 30-pixel cell and one quadtree root (the reference divides by zero there); levels up to 4128 x 4128; scaleFactor > 1.
 * There is no bound on a level's feature quota (node tables beyond the LDS move to a device scratch block). */
orbhip_ctx *orbhip_create(int device, int nfeatures, float scaleFactor, int nlevels,
                          int iniThFAST, int minThFAST, int max_w, int max_h, int max_batch);
void orbhip_destroy(orbhip_ctx *ctx);
const char *orbhip_last_error(const orbhip_ctx *ctx);
int orbhip_sync(orbhip_ctx *ctx);
/* The context's hipStream_t (as void*), so a caller can order its own work against it. */
void *orbhip_stream(orbhip_ctx *ctx);

/* Replaces GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/GetScaleSigmaSquares/
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:81-101) and exposes
 * mnFeaturesPerLevel/umax (:122,:124).  Any output pointer may be NULL.  Arrays need nlevels
 * entries (umax: 16). */
int orbhip_get_tables(const orbhip_ctx *ctx, int *nlevels, double *scaleFactor, float *mvScaleFactor,
                      float *mvInvScaleFactor, float *mvLevelSigma2, float *mvInvLevelSigma2,
                      int *mnFeaturesPerLevel, int *umax);
/* The same tables without a context or a device (pure host arithmetic of
 * src/ORBextractor.cc:417-471), for constructing the C++ class before the first image arrives.
 * Arrays need nlevels entries (umax: 16); any output pointer may be NULL. */
int orbhip_tables(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                  float *mvScaleFactor, float *mvInvScaleFactor, float *mvLevelSigma2,
                  float *mvInvLevelSigma2, int *mnFeaturesPerLevel, int *umax);
/* Upper bound on keypoints per frame (nfeatures plus the quadtree's overshoot); use as `cap`. */
int orbhip_max_keypoints(const orbhip_ctx *ctx);
/* Size of pyramid level `level` for a w x h input (src/ORBextractor.cc:1132-1133). */
int orbhip_level_size(const orbhip_ctx *ctx, int w, int h, int level, int *lw, int *lh);

/* Replaces ORBextractor::operator()(InputArray image, InputArray mask, vector<KeyPoint>&,
 * OutputArray descriptors) (include/ORBextractor.h:77-79, src/ORBextractor.cc:1045-1126).
 * img: 8-bit single channel, `stride` bytes per row.  kps/desc: capacity `cap` keypoints
 * (desc is cap x 32 bytes, row i = descriptor of keypoint i).  timings_ms (may be NULL)
 * receives {pyramid, keypoints, descriptors} in ms = GetTimeOfComputePyramid /
 * GetTimeOfComputeKeyPointsOctTree / GetTImeOfComputeDescriptor (include/ORBextractor.h:51-53). */
int orbhip_extract(orbhip_ctx *ctx, const uint8_t *img, int w, int h, int stride,
                   orbhip_keypoint *kps, uint8_t *desc, int cap, int *n_out, float timings_ms[3]);

/* Batched mode (new; the reference processes one image per call): B independent frames of the
 * same size per call, one launch per stage.  imgs[b] are host pointers; outputs are
 * kps[b*cap + i], desc[(b*cap + i)*32], n_out[b]. */
int orbhip_extract_batch(orbhip_ctx *ctx, const uint8_t *const *imgs, int B, int w, int h,
                         int stride, orbhip_keypoint *kps, uint8_t *desc, int cap, int *n_out);

/* Same with everything resident in device memory: d_imgs = B frames, frame b at
 * d_imgs + b*frame_stride, rows `stride` bytes apart (stride % 4 == 0 and 4-byte aligned
 * base required).  d_kps [B*cap] orbhip_keypoint, d_desc [B*cap*32] bytes, d_counts [B]
 * int32.  Asynchronous on the context stream.  Level 0 of the pyramid aliases d_imgs until the
 * next extract call on this context. */
int orbhip_extract_batch_device(orbhip_ctx *ctx, const void *d_imgs, int B, int w, int h,
                                int stride, size_t frame_stride, void *d_kps, void *d_desc, int cap,
                                void *d_counts);

/* ---- host-fed pipeline (new; the reference's frames always arrive from host memory: cv::imread at
 * Examples/Monocular/mono_euroc.cc:73, then ORBextractor::operator() via src/Frame.cc:591-597) ----
 * A ring of `depth` (2..8) slots per context: batch n + 1 is copied to the device and batch n - 1's keypoints /
 * descriptors are copied back while batch n computes (one copy-in stream, the context's compute stream, one copy-out
 * stream; the results land in pinned host memory owned by the context).  Frames of w x h, up to B per batch.
 *   orbhip_pipe_submit  enqueues one batch and returns at once.  `frames`: B images, image b at frames + b * frame_stride,
 *                       rows `stride` bytes apart.  The copy is one asynchronous DMA when the memory is pinned
 *                       (orbhip_host_alloc, or the caller's own hipHostMalloc / hipHostRegister); pageable memory works
 *                       but is staged by the driver.  The caller must leave the frames alone until the batch's wait returns.
 *                       ORBHIP_E_CAPACITY when `depth` batches are in flight and none was collected.
 *   orbhip_pipe_wait    blocks until the OLDEST outstanding batch is complete and returns pointers into that slot's pinned
 *                       result block: kps[b * cap + i], desc[(b * cap + i) * 32], n_out[b].  They stay valid until the
 *                       NEXT orbhip_pipe_wait (or orbhip_pipe_destroy) on this context, however many batches are submitted
 *                       in between: the ring has depth + 1 host result blocks, and no submit it admits reuses the block
 *                       the last wait returned.
 * Results are those of orbhip_extract_batch for the same frames (same kernels, same order). */
void *orbhip_host_alloc(size_t nbytes);
void orbhip_host_free(void *p);
int orbhip_pipe_create(orbhip_ctx *ctx, int depth, int B, int w, int h);
int orbhip_pipe_destroy(orbhip_ctx *ctx);
int orbhip_pipe_submit(orbhip_ctx *ctx, const uint8_t *frames, int B, int stride, size_t frame_stride);
int orbhip_pipe_wait(orbhip_ctx *ctx, const orbhip_keypoint **kps, const uint8_t **desc, const int32_t **n_out, int *B,
                     int *cap);
/* Optional matching stage of the pipeline: after the extraction of a batch, Frame::ComputeBoW (src/Frame.cc:739-746,
 * orbhip_vocab_transform_device with `levelsup`) and ORBmatcher(nnratio, check_ori)::SearchByBoW of every frame b >= 1
 * against frame b - 1 of the same batch (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:1881-1885;
 * orbhip_search_by_bow_seq_device with lag 1, th_mode 0) run on the device-resident outputs and their results travel back
 * with the keypoints.  Needs a vocabulary in the context.  orbhip_pipe_matches returns, for the batch the last
 * orbhip_pipe_wait returned, match12[b * cap + i1] (feature of frame b matched by feature i1 of frame b - 1, or -1),
 * match21[b * cap + i2] and nmatches[b] (frame 0 of a batch: all -1 / 0). */
int orbhip_pipe_enable_bow(orbhip_ctx *ctx, int levelsup, float nnratio, int check_ori);
int orbhip_pipe_matches(orbhip_ctx *ctx, const int32_t **match12, const int32_t **match21, const int32_t **nmatches);

/* Replaces reads of the public member std::vector<cv::Mat> mvImagePyramid
 * (include/ORBextractor.h:103; read by src/Frame.cc:817,907,919,924).  Copies level `level`
 * of frame `frame` of the last extract call to dst (rows dst_stride apart). */
int orbhip_get_pyramid_level(orbhip_ctx *ctx, int frame, int level, uint8_t *dst, int dst_stride,
                             int *w, int *h);

/* The same member without a copy per level: with orbhip_set_host_pyramid(ctx, 1) every following orbhip_extract /
 * orbhip_extract_batch also lands levels 1.. of its frames in page-locked host memory (one device-to-host copy that runs
 * beside the kernels), and orbhip_host_pyramid_level returns a pointer into that block (rows *stride apart); level 0 is
 * the page-locked copy of the caller's frame that the single-frame path uploads from.  The pointers stay valid until the
 * next extract call on this context or orbhip_destroy -- the drop-in's mvImagePyramid[level] are headers on them, read
 * right after the extraction as src/Frame.cc:817 does.  Returns ORBHIP_E_ARG when a level is not staged (host pyramid
 * off, device-pointer entry points, or level 0 of a batch of 8 or more frames: use the caller's image). */
int orbhip_set_host_pyramid(orbhip_ctx *ctx, int on);
int orbhip_host_pyramid_level(orbhip_ctx *ctx, int frame, int level, const uint8_t **ptr, int *stride, int *w, int *h);

/* ---- parity/debug access to stage outputs of the last extract call ---- */
/* blurred level (cv::GaussianBlur at src/ORBextractor.cc:1103-1104) */
int orbhip_debug_get_blurred_level(orbhip_ctx *ctx, int frame, int level, uint8_t *dst,
                                   int dst_stride, int *w, int *h);
/* FAST candidates of one level in the reference's order (cells row-major, raster inside a
 * cell; src/ORBextractor.cc:791-831). */
int orbhip_debug_get_candidates(orbhip_ctx *ctx, int frame, int level, orbhip_cand *out, int cap,
                                int *n_out);
/* keypoints of one level after DistributeOctTree + orientation, level coordinates
 * (src/ORBextractor.cc:833-854). */
int orbhip_debug_get_level_keypoints(orbhip_ctx *ctx, int frame, int level, orbhip_keypoint *out,
                                     int cap, int *n_out);

/* ---- matching ---- */
/* Replaces ORBmatcher::DescriptorDistance (include/ORBmatcher.h:47, src/ORBmatcher.cc:1675-1691)
 * applied to a whole query set against a whole database with the best / second-best
 * bookkeeping of every search routine (src/ORBmatcher.cc:205-226 etc.): for each query the
 * lowest-index minimum (strict '<'), its distance and the second smallest distance; initial
 * values 256 / -1 / 256.  Descriptors are rows of 32 bytes.  Device pointers of any alignment are accepted; the matrix-pipe
 * kernels want d_q 16-byte and d_db 4-byte aligned (what hipMalloc and rows of 32 bytes give) and hand other pointers to
 * the scalar kernels (same results, about a third of the rate). */
int orbhip_hamming_knn2(orbhip_ctx *ctx, const uint8_t *q, int nq, const uint8_t *db, int ndb,
                        int32_t *best_idx, int32_t *best_d, int32_t *second_d);
int orbhip_hamming_knn2_device(orbhip_ctx *ctx, const void *d_q, int nq, const void *d_db, int ndb,
                               void *d_best_idx, void *d_best_d, void *d_second_d);

/* Batched form for a sequence held on the device (new; the reference matches one frame pair per
 * call): descriptor sets laid out as the outputs of orbhip_extract_batch_device (set b at
 * d_desc + b*cap*32 with d_counts[b] rows).  For b >= lag the queries are set b and the database
 * is set b-lag; outputs at [b*cap + i]; for b < lag the outputs are -1 / 256 / 256.  One launch for
 * all B sets. */
int orbhip_hamming_knn2_seq_device(orbhip_ctx *ctx, const void *d_desc, const void *d_counts, int cap,
                                   int B, int lag, void *d_best_idx, void *d_best_d, void *d_second_d);

/* Same bookkeeping over explicit candidate lists in CSR form (query i examines
 * cand[off[i] .. off[i+1])), the shape of SearchByProjection / SearchForInitialization /
 * Fuse / SearchBySim3 inner loops (src/ORBmatcher.cc:76-125, 432-461, 901-949, 1199-1224). */
int orbhip_hamming_knn2_lists(orbhip_ctx *ctx, const uint8_t *q, int nq, const uint8_t *db, int ndb,
                              const int32_t *off, const int32_t *cand, int32_t *best_idx,
                              int32_t *best_d, int32_t *second_d);

/* Replaces the matching core of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)
 * (src/ORBmatcher.cc:159-288; th_mode 0: accept best <= th) and
 * SearchByBoW(KeyFrame*, KeyFrame*, ...) (:522-655; th_mode 1: accept best < th, valid2 given).
 * Side 1/2 FeatureVectors in CSR form: sorted node ids, offsets [ng+1], feature indices.
 * valid1[i] != 0 <=> feature i has a good MapPoint; valid2 may be NULL.
 * match12[n1] / match21[n2] receive the matched index on the other side or -1, after the
 * rotation histogram filter (ComputeThreeMaxima, :1629-1670) when check_ori != 0.
 * *nmatches receives the return value of the reference routine. */
int orbhip_search_by_bow(orbhip_ctx *ctx, const uint8_t *desc1, int n1, const uint8_t *valid1,
                         const float *angle1, const int32_t *node1, const int32_t *off1,
                         const int32_t *idx1, int ng1, const uint8_t *desc2, int n2,
                         const uint8_t *valid2, const float *angle2, const int32_t *node2,
                         const int32_t *off2, const int32_t *idx2, int ng2, int th, int th_mode,
                         float nnratio, int check_ori, int32_t *match12, int32_t *match21,
                         int *nmatches);

/* ---- ORB vocabulary ----
 * Replaces ORBVocabulary::loadFromBinaryFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1680-1721,
 * called from src/System.cc:336-339): parses the binary vocabulary (header u32 nb_nodes, u32 size_node=41,
 * i32 k, L, scoring, weighting; then per node i32 parent, u8 desc[32], f32 weight, u8 is_leaf) and keeps
 * it as device tables in the context.  _device: the blob is already in device memory (e.g. after
 * orbhip_bcast_blob_device); it is copied back once for parsing. */
int orbhip_vocab_load(orbhip_ctx *ctx, const void *blob, size_t nbytes);
int orbhip_vocab_load_device(orbhip_ctx *ctx, const void *d_blob, size_t nbytes);
/* The vocabulary tables of `src` serve `dst` too (contexts of one device; borrowed, not copied -- 58 MB for the stock tree).
 * What lets the extractor's context run the transform inside orbhip_frame_build on the vocabulary the ORBVocabulary drop-in
 * loaded into its own context.  The device block is reference-counted: src may load another vocabulary or be destroyed while
 * dst still uses what it borrowed -- dst then keeps running on the OLD tables until it shares again.
 * orbhip_vocab_generation: a process-wide counter of orbhip_vocab_load calls as seen by this context's tables (0 = no
 * vocabulary); a borrower compares it with the lender's to learn that it should share again (no counterpart in the reference:
 * System.cc:336-339 loads the vocabulary once).  orbhip_vocab_share / orbhip_vocab_generation on `src` may run on another
 * thread than an orbhip_vocab_load on it: the (block, tables) pair is swapped under a lock, the borrower sees the old pair or
 * the new one.  Work already queued on src's OWN stream against the old tables is the caller's to order, as with any two
 * calls on one context. */
int orbhip_vocab_share(orbhip_ctx *dst, const orbhip_ctx *src);
unsigned long long orbhip_vocab_generation(const orbhip_ctx *ctx);
/* Replaces ORBVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1564-1647; chosen by
 * src/System.cc:335-336 for a ".txt" vocabulary such as the stock ORBvoc.txt): host-only conversion of the text (first
 * line "k L scoring weighting", then per node "parent is_leaf d0 .. d31 weight") to the binary layout above, which
 * orbhip_vocab_load takes.  Call with blob = NULL to get *blob_bytes = 24 + 41 * nodes, then with a buffer.  node_weight
 * (may be NULL; (*blob_bytes - 24) / 41 entries, node ids 1..n) receives the weights as the doubles the reference's text
 * loader keeps (Node::weight is a double; the binary format narrows it to float, so BowVector values of a text-loaded
 * vocabulary come from this array).  Lines without a token are skipped (the reference turns the empty line after the final
 * newline into a node built from uninitialised memory).  ORBHIP_E_ARG for a malformed text, ORBHIP_E_CAPACITY for a
 * buffer that is too small. */
int orbhip_vocab_text_to_binary(const char *text, size_t nbytes, void *blob, size_t blob_cap, size_t *blob_bytes,
                                double *node_weight, size_t weight_cap);
int orbhip_vocab_info(const orbhip_ctx *ctx, int *k, int *L, int *scoring, int *weighting, int *nnodes,
                      int *nwords);
/* Replaces the per-feature ORBVocabulary::transform (TemplatedVocabulary.h:1443-1485) as used by
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:739-746, src/KeyFrame.cc:392-400): word id and
 * weight of the leaf reached, node id at level L - levelsup; node id 0 if that level is <= 0 and -- canonical, the
 * reference leaves the value unset -- if the leaf lies above level L - levelsup (a built vocabulary has leaves at every
 * depth).  The caller builds
 * BowVector (sum of weights per word, normalised) and FeatureVector (indices per node, weight > 0 only)
 * from these arrays. */
int orbhip_vocab_transform(orbhip_ctx *ctx, const uint8_t *desc, int n, int levelsup, int32_t *word_id,
                           float *weight, int32_t *node_id);
int orbhip_vocab_transform_device(orbhip_ctx *ctx, const void *d_desc, int n, int levelsup, void *d_word_id,
                                  void *d_weight, void *d_node_id);
/* Batched SearchByBoW (src/ORBmatcher.cc:159-288 / :522-655 with th_mode 0 / 1) for a sequence on the
 * device, laid out like the outputs of orbhip_extract_batch_device; d_node / d_weight [B*cap] from
 * orbhip_vocab_transform_device; d_valid [B*cap] bytes ("has a good MapPoint") or NULL = all valid.
 * For b >= lag side 1 is set b-lag (the key frame) and side 2 is set b; d_match12[b*cap + i1] = matched
 * side-2 feature or -1, d_match21[b*cap + i2] = matched side-1 feature or -1, d_nmatches[b] = the
 * reference routine's return value.  TH_LOW = 50.  One launch for all B pairs.  cap <= 4096 (ORBHIP_E_SIZE beyond: the
 * per-pair tables live in LDS). */
int orbhip_search_by_bow_seq_device(orbhip_ctx *ctx, const void *d_desc, const void *d_kps, const void *d_counts,
                                    const void *d_node, const void *d_weight, const void *d_valid, int cap,
                                    int B, int lag, int th_mode, float nnratio, int check_ori, void *d_match12,
                                    void *d_match21, void *d_nmatches);

/* ---- stereo ----
 * Replaces Frame::ComputeStereoMatches (src/Frame.cc:810-984): for every left keypoint the best right
 * keypoint in its row band (octave +-1, u in [uL - mbf/mb, uL], distance < 75), refined by the 11-shift SAD
 * on the pyramid level of the keypoint and a parabola fit; outputs mvuRight / mvDepth (-1 = none) after the
 * median-based outlier cut.  `left` and `right` are the two extractor contexts that have just extracted the
 * left / right image(s) of the same size: their device-resident pyramids are read in place (the reference
 * reads mpORBextractorLeft/Right->mvImagePyramid, :817,:907,:919,:924).  *nmatch = matches before the cut. */
int orbhip_stereo_match(orbhip_ctx *left, orbhip_ctx *right, const orbhip_keypoint *kpsL, const uint8_t *descL,
                        int nL, const orbhip_keypoint *kpsR, const uint8_t *descR, int nR, float mb, float mbf,
                        float *mvuRight, float *mvDepth, int *nmatch);
/* Batched, device-resident form (B stereo pairs; arrays laid out like orbhip_extract_batch_device outputs). */
int orbhip_stereo_match_device(orbhip_ctx *left, orbhip_ctx *right, const void *d_kpsL, const void *d_descL,
                               const void *d_cntL, const void *d_kpsR, const void *d_descR, const void *d_cntR,
                               int cap, int B, float mb, float mbf, void *d_uRight, void *d_depth, void *d_nmatch);

/* ---- frame grid and guided search ----
 * The 64 x 48 grid of include/Frame.h:41-42 as CSR: cell id = ix * 48 + iy (the order
 * Frame::GetFeaturesInArea visits cells in), feature indices ascending inside a cell (the push_back
 * order of Frame::AssignFeaturesToGrid, src/Frame.cc:574-589; cell of a feature by PosInGrid,
 * :726-736).  min_x, min_y, inv_w, inv_h are Frame::mnMinX, mnMinY, mfGridElementWidthInv,
 * mfGridElementHeightInv (:556-557).  d_cell_off [B][ORBHIP_GRID_CELLS + 1], d_cell_idx [B][cap]. */
#define ORBHIP_GRID_COLS 64
#define ORBHIP_GRID_ROWS 48
#define ORBHIP_GRID_CELLS (ORBHIP_GRID_COLS * ORBHIP_GRID_ROWS)
int orbhip_grid_build_device(orbhip_ctx *ctx, const void *d_kps_un, const void *d_counts, int cap, int B, float min_x,
                             float min_y, float inv_w, float inv_h, void *d_cell_off, void *d_cell_idx);
int orbhip_grid_build(orbhip_ctx *ctx, const orbhip_keypoint *kps_un, int n, float min_x, float min_y, float inv_w,
                      float inv_h, int32_t *cell_off, int32_t *cell_idx);

/* One projected point of a guided search: where it falls in the frame (u, v), the window half-size, the
 * octave range GetFeaturesInArea filters on (min_level <= 0 and max_level < 0: no filter, :693-707), the
 * projected right coordinate (compared with mvuRight when that is > 0) and the orientation of the source
 * keypoint.  flags: ORBHIP_Q_ACTIVE = the point takes part (mbTrackInView && !isBad(), :55-59; or the
 * LastFrame point is valid, not an outlier and projects inside the image, :1371-1398);
 * ORBHIP_Q_OBSERVED = its MapPoint has Observations() > 0, so a feature it takes is closed to later points. */
#define ORBHIP_Q_ACTIVE 1
#define ORBHIP_Q_OBSERVED 2
typedef struct {
    float u, v, radius, proj_xr;
    int32_t min_level, max_level;
    float angle;
    int32_t flags;
} orbhip_proj_query;

/* Replaces Frame::GetFeaturesInArea (src/Frame.cc:671-724) for nq windows at once (only u, v, radius,
 * min_level, max_level of a query are read): out_off[nq + 1], out_idx[out_off[nq]] in the reference's
 * order.  Returns ORBHIP_E_ARG if out_cap is too small (out_off is still filled). */
int orbhip_features_in_area(orbhip_ctx *ctx, const orbhip_keypoint *kps_un, int n, float min_x, float min_y,
                            float inv_w, float inv_h, const orbhip_proj_query *queries, int nq, int32_t *out_off,
                            int32_t *out_idx, int out_cap);

/* Replaces the search loops of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:45-129; use_ratio = 1: second best and the ratio test when best and second lie on the
 * same octave) and SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (:1341-1498;
 * use_ratio = 0: best only, rotation histogram when check_ori).  Queries are processed in index order, as
 * the reference processes its points: occupied[i] != 0 marks frame features that already hold a MapPoint
 * with observations (:88-90, :1413-1415).  match[i] = index of the query assigned to frame feature i (the
 * last one, as in the reference), -1 if none was, -2 if one was and the rotation check removed it (the
 * reference stores NULL there, :1489); *nmatches = the reference routine's return value.  The caller
 * projects the points (pose arithmetic stays on the host) and fills the queries.  TH_HIGH = th_high. */
int orbhip_search_by_projection(orbhip_ctx *ctx, const orbhip_keypoint *kps_un, const uint8_t *desc, int n,
                                const float *u_right, const uint8_t *occupied, float min_x, float min_y,
                                float inv_w, float inv_h, const orbhip_proj_query *queries, const uint8_t *qdesc,
                                int nq, int use_ratio, float nnratio, int check_ori, int th_high, int32_t *match,
                                int *nmatches);
/* Batched, device-resident form: B frames laid out like orbhip_extract_batch_device outputs, the grid from
 * orbhip_grid_build_device, d_queries [B][cap_q], d_qdesc [B][cap_q][32], d_nq [B]; d_u_right / d_occupied
 * [B][cap] or NULL; d_match [B][cap], d_nmatches [B]. */
int orbhip_search_by_projection_device(orbhip_ctx *ctx, const void *d_kps_un, const void *d_desc,
                                       const void *d_counts, int cap, int B, const void *d_u_right,
                                       const void *d_occupied, float min_x, float min_y, float inv_w, float inv_h,
                                       const void *d_cell_off, const void *d_cell_idx, const void *d_queries,
                                       const void *d_qdesc, const void *d_nq, int cap_q, int use_ratio,
                                       float nnratio, int check_ori, int th_high, void *d_match, void *d_nmatches);

/* Replaces the body of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:283-349; the remaining caller of
 * ORBmatcher::DescriptorDistance, run by LocalMapping on every point of a new key frame and after every fusion) for P map
 * points at once: point p's observed descriptors (rows of the key frames that see it, in the order of its observation map)
 * are rows off[p] .. off[p + 1] of desc; off[0] = 0.  best[p] = the row within that list with the least median distance
 * to the list (the reference's sorted_row[0.5 * (N - 1)], self-distance included; the first such row), -1 for an empty
 * list; best_median[p] (may be NULL in the host form) = that median, INT_MAX for an empty list. */
int orbhip_distinctive_descriptors(orbhip_ctx *ctx, const uint8_t *desc, const int32_t *off, int P, int32_t *best,
                                   int32_t *best_median);
int orbhip_distinctive_descriptors_device(orbhip_ctx *ctx, const void *d_desc, const void *d_off, int P, void *d_best,
                                          void *d_best_median);

/* Replaces the per-point inner loop of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:887-950), Fuse(KeyFrame*, cv::Mat Scw, ...) (:1044-1075) and both directions of SearchBySim3
 * (:1190-1224, :1270-1304): for every projected point, KeyFrame::GetFeaturesInArea(u, v, radius) (src/KeyFrame.cc:1138-1177),
 * features on levels outside [min_level, max_level] (= [predicted - 1, predicted]) skipped, the first feature of smallest
 * Hamming distance wins.  inv_level_sigma2 != NULL (host array, nlevels <= 16 entries = KeyFrame::mvInvLevelSigma2) turns on
 * the first Fuse's chi-square gate on the reprojection error: 7.8 over (u, v, proj_xr) when u_right[idx] >= 0, else 5.99
 * over (u, v) (:908-934).  Points do not close features to each other here, so best_idx[q] / best_dist[q] are per query:
 * -1 / 256 when the query is not ORBHIP_Q_ACTIVE or no feature is closer than 256; the caller applies <= TH_LOW (50) /
 * TH_HIGH (100) and the map updates.  Only u, v, radius, proj_xr, min_level, max_level and flags of a query are read. */
int orbhip_window_best(orbhip_ctx *ctx, const orbhip_keypoint *kps_un, const uint8_t *desc, int n, const float *u_right,
                       const float *inv_level_sigma2, int nlevels, float min_x, float min_y, float inv_w, float inv_h,
                       const orbhip_proj_query *queries, const uint8_t *qdesc, int nq, int32_t *best_idx,
                       int32_t *best_dist);
/* Batched, device-resident form (layouts as orbhip_search_by_projection_device); d_best_idx / d_best_dist [B][cap_q]. */
int orbhip_window_best_device(orbhip_ctx *ctx, const void *d_kps_un, const void *d_desc, int cap, int B,
                              const void *d_u_right, const float *inv_level_sigma2, int nlevels, float min_x, float min_y,
                              float inv_w, float inv_h, const void *d_cell_off, const void *d_cell_idx,
                              const void *d_queries, const void *d_qdesc, const void *d_nq, int cap_q, void *d_best_idx,
                              void *d_best_dist);

/* Replaces the body of ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched,
 * vector<int> &vnMatches12, int windowSize) (src/ORBmatcher.cc:405-520; the monocular initialiser, called at
 * src/Tracking.cc MonocularInitialization with nnratio 0.9, windowSize 100).  kps1_un / kps2_un are mvKeysUn of the two
 * frames; only octave-0 features of frame 1 search (:420-421), in index order, among the octave-0 features of frame 2
 * inside the window around prev_matched[i1] (:424); a feature of frame 2 that is already matched at a distance <= the
 * new one is skipped (:443-444), a better match displaces the earlier owner (:462-466); TH_LOW = 50 and
 * bestDist < bestDist2 * nnratio (:458-460); rotation histogram and three maxima when check_ori (:471-509).
 * matches12[i1] = feature of frame 2 or -1; prev_matched (n1 x 2 floats, in/out) is updated for the matched
 * features (:512-515); *nmatches = the reference's return value. */
int orbhip_search_for_initialization(orbhip_ctx *ctx, const orbhip_keypoint *kps1_un, const uint8_t *desc1, int n1,
                                     const orbhip_keypoint *kps2_un, const uint8_t *desc2, int n2, float min_x, float min_y,
                                     float inv_w, float inv_h, float *prev_matched, int window_size, float nnratio,
                                     int check_ori, int32_t *matches12, int *nmatches);
/* Batched, device-resident form: B frame pairs; frame 1 arrays [B][cap1], frame 2 arrays [B][cap2] with the grid
 * of frame 2 from orbhip_grid_build_device; d_prev_matched [B][cap1][2] floats (in/out), d_matches12 [B][cap1],
 * d_nmatches [B]. */
int orbhip_search_for_initialization_device(orbhip_ctx *ctx, const void *d_kps1_un, const void *d_desc1,
                                            const void *d_counts1, int cap1, const void *d_kps2_un, const void *d_desc2,
                                            const void *d_counts2, int cap2, int B, float min_x, float min_y, float inv_w,
                                            float inv_h, const void *d_cell_off2, const void *d_cell_idx2,
                                            void *d_prev_matched, int window_size, float nnratio, int check_ori,
                                            void *d_matches12, void *d_nmatches);

/* Replaces the matching core of ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12,
 * vector<pair<size_t,size_t>> &vMatchedPairs, bool bOnlyStereo) (src/ORBmatcher.cc:657-827, with
 * CheckDistEpipolarLine :140-157; called by LocalMapping::CreateNewMapPoints).  Both key frames as mvKeysUn,
 * descriptors, skip[i] != 0 <=> GetMapPoint(i) != NULL, mvuRight (NULL = monocular) and their FeatureVectors in CSR
 * form; F12 3x3 row-major float; (ex, ey) the epipole in the second image (:664-671, computed by the caller);
 * scale_factors2 / level_sigma2_2 = pKF2->mvScaleFactors / mvLevelSigma2.  TH_LOW = 50.  matches12[i1] = feature of
 * key frame 2 or -1 after the rotation histogram; *nmatches = the reference's return value.  (This fork does not mark
 * matched features of key frame 2, so one of them can be matched by several features of key frame 1.) */
int orbhip_search_for_triangulation(orbhip_ctx *ctx, const orbhip_keypoint *kps1_un, const uint8_t *desc1, int n1,
                                    const uint8_t *skip1, const float *u_right1, const int32_t *node1, const int32_t *off1,
                                    const int32_t *idx1, int ng1, const orbhip_keypoint *kps2_un, const uint8_t *desc2, int n2,
                                    const uint8_t *skip2, const float *u_right2, const int32_t *node2, const int32_t *off2,
                                    const int32_t *idx2, int ng2, const float F12[9], float ex, float ey,
                                    const float *scale_factors2, const float *level_sigma2_2, int nlevels2, int only_stereo,
                                    int check_ori, int32_t *matches12, int *nmatches);

/* ---- undistortion and rectification ----
 * Replaces the body of Frame::UndistortKeyPoints (src/Frame.cc:748-778): cv::undistortPoints(mat, mat, mK,
 * mDistCoef, cv::Mat(), mK) on the keypoint coordinates; every other field of a keypoint is copied.  K, P: 3x3
 * row-major float (P = NULL: normalised coordinates are returned, as OpenCV does without P; the reference passes
 * mK); dist: ndist in {0, 4, 5, 8} coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]).  The caller keeps the
 * reference's shortcut "mDistCoef(0) == 0 -> mvKeysUn = mvKeys" (:750-754).  d_counts may be NULL (= cap points
 * per set).  Also serves Frame::ComputeImageBounds (:780-808: the four image corners as keypoints). */
int orbhip_undistort_keypoints(orbhip_ctx *ctx, const orbhip_keypoint *kps, int n, const float K[9], const float *dist,
                               int ndist, const float *P, orbhip_keypoint *kps_un);
int orbhip_undistort_keypoints_device(orbhip_ctx *ctx, const void *d_kps, const void *d_counts, int cap, int B,
                                      const float K[9], const float *dist, int ndist, const float *P, void *d_kps_un);
/* Replaces cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3).colRange(0,3), size, CV_32F, M1, M2)
 * (Examples/Stereo/stereo_euroc.cc:96-98): a once-per-run table built on the host in double. */
int orbhip_init_undistort_rectify_map(const double K[9], const double *dist, int ndist, const double R[9],
                                      const double P[9], int w, int h, float *map_x, float *map_y);
/* Replaces cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) (stereo_euroc.cc:136-137; 8-bit single channel,
 * BORDER_CONSTANT 0).  The maps (w x h floats each) are uploaded once per context; every call rectifies B images
 * with them.  The destination has the maps' size. */
int orbhip_remap_set_maps(orbhip_ctx *ctx, const float *map_x, const float *map_y, int w, int h);
int orbhip_remap(orbhip_ctx *ctx, const uint8_t *src, int src_w, int src_h, int src_stride, uint8_t *dst,
                 int dst_stride);
int orbhip_remap_device(orbhip_ctx *ctx, const void *d_src, int B, int src_w, int src_h, int src_stride,
                        size_t src_frame_stride, void *d_dst, int dst_stride, size_t dst_frame_stride);

/* Device time of the stages of the last extract call on this context, in ms:
 * {pyramid, FAST, quadtree, blur, describe} and, at [5], of the last orbhip_hamming_knn2*_device
 * call.  Measured with HIP events on the context's stream; synchronises the stream.  A batch of 16 frames or more runs
 * the quadtree in two halves, the second on another stream: [2] is the first half only.  [3] is 0 when the blur ran
 * inside the describe kernel (the default for batches). */
int orbhip_get_stage_times(orbhip_ctx *ctx, float ms[6]);
/* Which of those events the extract / match calls record: 2 (default) all of them, 1 only the pair around the FAST launch
 * (the other entries read 0), 0 none.  An event between two kernels of a stream costs a few microseconds of device time;
 * a loop that only wants its throughput (and bench.py, which wants the FAST launch time) narrows the set. */
int orbhip_set_stage_timing(orbhip_ctx *ctx, int mode);

/* ---- resident feature sets (new) ----
 * A key frame's descriptors, keypoints, FeatureVector and feature grid never change after KeyFrame::KeyFrame / ComputeBoW
 * (ref: src/KeyFrame.cc:53-87, 392-400), but the reference's matcher entry points take the KeyFrame itself, so a per-call
 * C entry point has to upload that data again on every call.  A set keeps it on the device under a caller-chosen key
 * (non-zero; the drop-in classes use the KeyFrame's / Frame's mnId); at most 96 sets per context, least recently used out.
 *   orbhip_set_put   kps[n] / desc[n * 32]; the FeatureVector as CSR over ascending node ids (node[ng], off[ng + 1], idx[off[ng]];
 *                    ng may be 0); inv_w, inv_h > 0: the 64 x 48 grid of Frame::AssignFeaturesToGrid is built too (needed
 *                    by orbhip_window_best_set).  Replaces a set of the same key.
 *   orbhip_set_has   1 if a set with this key and this number of features is resident, else 0.
 *   orbhip_set_drop  key 0: all sets. */
int orbhip_set_put(orbhip_ctx *ctx, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *node,
                   const int32_t *off, const int32_t *idx, int ng, float min_x, float min_y, float inv_w, float inv_h);
int orbhip_set_has(orbhip_ctx *ctx, uint64_t key, int n);
int orbhip_set_drop(orbhip_ctx *ctx, uint64_t key);
/* Bounds the table: at most max_sets sets (clamped to 4 .. 96, the default) stay resident in this context, least recently used
 * out -- ~90 KB of device memory per set of 1000 features.  Returns the limit in force.  (The reference keeps every KeyFrame's
 * descriptors in host memory for the life of the map, src/KeyFrame.cc:55-89; this is the device-side counterpart's budget.) */
int orbhip_set_limit(orbhip_ctx *ctx, int max_sets);
/* Is the set what the caller thinks it is?  Ids are not identities: Tracking::Reset restarts KeyFrame::nNextId and
 * Frame::nNextId (ref: src/Tracking.cc:2758-2759), and a key frame met before KeyFrame::ComputeBoW (ref: src/KeyFrame.cc:392-400)
 * has an empty FeatureVector.
 *   orbhip_set_info         1 and the set's feature count, FeatureVector nodes and fingerprint when `key` is resident, else 0
 *                           (any of the three pointers may be NULL).  The wrappers of the *_sets entry points size their
 *                           buffers from it.
 *   orbhip_set_fingerprint  the fingerprint orbhip_set_put / orbhip_set_put_from_frame store: a hash of n, the first
 *                           keypoint's position and the first and last descriptor.  A caller compares the one of its own
 *                           data with the resident one and puts the set again when they differ.
 * The integration calls orbhip_set_drop(ctx, 0) from Tracking::Reset. */
int orbhip_set_info(orbhip_ctx *ctx, uint64_t key, int *n, int *ng, uint64_t *fingerprint);
uint64_t orbhip_set_fingerprint(const orbhip_keypoint *kps, const uint8_t *desc, int n);
/* the same from the three things it hashes (descriptor rows that are not contiguous: a cv::Mat with a step) */
uint64_t orbhip_set_fingerprint_rows(const orbhip_keypoint *first_kp, const uint8_t *first_desc, const uint8_t *last_desc, int n);
/* orbhip_search_by_bow (above) between two resident sets: valid1[n1] (and valid2[n2] or NULL) are the only per-feature
 * inputs that travel.  Same results as orbhip_search_by_bow on the sets' data. */
int orbhip_search_by_bow_sets(orbhip_ctx *ctx, uint64_t key1, const uint8_t *valid1, uint64_t key2, const uint8_t *valid2, int th,
                              int th_mode, float nnratio, int check_ori, int32_t *match12, int32_t *match21, int *nmatches);
/* orbhip_window_best (above) into a resident set (with a grid): the projected points travel, the key frame does not. */
int orbhip_window_best_set(orbhip_ctx *ctx, uint64_t key, const float *u_right, const float *inv_level_sigma2, int nlevels,
                           const orbhip_proj_query *queries, const uint8_t *qdesc, int nq, int32_t *best_idx, int32_t *best_dist);
/* orbhip_search_for_triangulation (above) of key frame 1 against K neighbours in ONE call, every key frame a resident set
 * (LocalMapping::CreateNewMapPoints calls SearchForTriangulation once per neighbour of the new key frame, 20 of them in the
 * monocular case: ref src/LocalMapping.cc:2226-2298).  Row k of matches12 ([K][n1], n1 = the features of set key1) and
 * nmatches[k] equal what orbhip_search_for_triangulation returns for neighbour k on the sets' data.
 *   skip1[n1], u_right1[n1]   of key frame 1, shared by all neighbours (u_right1 NULL: monocular)
 *   nb[K]                     per neighbour: its set, F12 (row-major) and the epipole in its image; a key may appear several
 *                             times, and key2 == key1 is allowed
 *   skip2, u_right2           the K per-neighbour arrays one after the other in neighbour order, each as long as its set
 *                             (orbhip_set_info); u_right2 NULL: monocular
 * Only these, the shared nodes and the K parameter records travel.  K == 0 returns ORBHIP_OK and writes nothing.
 * ORBHIP_E_ARG, with nothing written: a key that is not resident, K < 0, more distinct keys than the set limit in force
 * (orbhip_set_limit), nlevels2 outside 1..64, a set of more than 65535 features on side 2, a side-2 set with an octave
 * outside [0, nlevels2). */
typedef struct orbhip_tri_neighbour {
    uint64_t key2;      /* resident set of pKF2 */
    float F12[9];       /* row-major, as for orbhip_search_for_triangulation */
    float ex, ey;       /* epipole in image 2 */
} orbhip_tri_neighbour;
int orbhip_search_for_triangulation_sets(orbhip_ctx *ctx, uint64_t key1, const uint8_t *skip1, const float *u_right1,
                                         const orbhip_tri_neighbour *nb, int K, const uint8_t *skip2, const float *u_right2,
                                         const float *scale_factors2, const float *level_sigma2_2, int nlevels2,
                                         int only_stereo, int check_ori, int32_t *matches12 /* [K][n1] */, int32_t *nmatches /* [K] */);

/* ---- the Frame constructor's device work as one launch (new) ----
 * Frame::Frame (ref: src/Frame.cc:518-572) runs ExtractORB (:591-597), UndistortKeyPoints (:748-778) and AssignFeaturesToGrid
 * (:574-589) one after the other, and Tracking asks for Frame::ComputeBoW (:739-746) before the frame's first SearchByBoW
 * (ref: src/Tracking.cc, TrackReferenceKeyFrame).  As four entry points that is four launch + synchronise round trips for
 * one dependency chain; orbhip_frame_build runs the chain as ONE captured graph with one synchronisation and one packed
 * result block -- the kernels are those of orbhip_extract, orbhip_undistort_keypoints, orbhip_grid_build and
 * orbhip_vocab_transform, the results are theirs.
 *   fp->K, dist, ndist  mK / mDistCoef as for orbhip_undistort_keypoints (P = K); ndist == 0 or dist[0] == 0: kps_un = kps, the
 *                       reference's shortcut (:750-754)
 *   fp->min_x ... inv_h the grid of Frame::AssignFeaturesToGrid (mnMinX, mnMinY, mfGridElementWidthInv, ...HeightInv);
 *                       inv_w <= 0: no grid (cell_off / cell_idx may be NULL) -- the first frame of a run, whose image
 *                       bounds Frame::ComputeImageBounds derives after the extraction
 *   fp->levelsup        >= 0: ORBVocabulary::transform of the descriptors with this levelsup (a vocabulary must be
 *                       loaded); < 0: none (word_id / weight / node_id may be NULL)
 * Outputs: kps, kps_un, desc (capacity `cap` features), n_out; cell_off[3073] / cell_idx[n] as orbhip_grid_build;
 * word_id / weight / node_id [n] as orbhip_vocab_transform.  The result block stays on the device until the context's
 * next orbhip_frame_build: orbhip_set_put_from_frame makes it a resident set of any context of the same device (the
 * matcher's per-thread context in the drop-in classes) without the keypoints and descriptors travelling again;
 * orbhip_frame_fingerprint is the orbhip_set_fingerprint of the frame it holds (0: none).  The graph is captured at the first
 * call of an (image size, parameters) pair and replayed afterwards; ORBHIP_NO_GRAPH=1 keeps the eager sequence. */
typedef struct orbhip_frame_params {
    float K[9];
    float dist[8];
    int ndist;
    float min_x, min_y, inv_w, inv_h;
    int levelsup;
} orbhip_frame_params;
int orbhip_frame_build(orbhip_ctx *ctx, const uint8_t *img, int w, int h, int stride, const orbhip_frame_params *fp,
                       orbhip_keypoint *kps, orbhip_keypoint *kps_un, uint8_t *desc, int cap, int *n_out, int32_t *cell_off,
                       int32_t *cell_idx, int32_t *word_id, float *weight, int32_t *node_id);
uint64_t orbhip_frame_fingerprint(const orbhip_ctx *ctx);
/* orbhip_set_put with the frame that `src` built last: the FeatureVector (CSR as for orbhip_set_put; ng may be 0) is all
 * that travels.  ctx and src must be contexts of the same device (they may be the same context).  Several contexts may copy
 * the same frame, each from its own thread: src's next orbhip_frame_build waits for every one of the copies.  What the caller
 * orders itself, as with any two calls on one context: a copy of src's frame must not START (this call) while another thread
 * is inside orbhip_frame_build on src -- in the reference the thread that builds a Frame is the one that makes it a KeyFrame
 * (src/Tracking.cc, CreateNewKeyFrame). */
int orbhip_set_put_from_frame(orbhip_ctx *ctx, uint64_t key, orbhip_ctx *src, const int32_t *node, const int32_t *off,
                              const int32_t *idx, int ng);

/* The floor under a per-call entry point, in microseconds per call on this context's stream: mode 0 = an empty kernel and
 * one synchronisation; 1 = 4 KB copied in, the kernel, 4 KB copied out, one synchronisation; 2 = the kernel stores its
 * result to page-locked memory, one synchronisation.  (Measurement aid: tools/percall_latency.py.) */
int orbhip_debug_roundtrip(orbhip_ctx *ctx, int mode, int iters, double *us_per_call);

/* Which kernel variants this PROCESS has launched since the last reset (test aid: a test that claims to reach a fallback path
 * checks the bit).  Bits: 0 k_fast_fix, 1 k_fast (generic grid), 2 k_resize_fit, 3 k_resize<32> / <8>, 4 k_pyramid_chain,
 * 5 k_quadtree (tables in LDS), 6 k_quadtree (tables and candidates in LDS, a frame or two), 7 k_quadtree (tables in global
 * memory), 8 k_bow_lane, 9 k_bow_seq (descriptors in LDS), 10 k_bow_seq (descriptors in global memory), 11 k_fast_fix on the
 * tall-cell instance, 12 k_describe, 13 k_describe_blur, 14 k_blur, 15 k_tri_match_sets with a node of at most 128 side-2
 * features (held in registers), 16 k_tri_match_sets with a node of more than 128 (strided), 17 k_grid_build (cell entries sorted
 * in LDS, 1024 threads: fewer than 8 frames), 18 k_grid_build (LDS, 256 threads: 8 frames or more), 19 k_grid_build (cell
 * entries sorted in place in global memory: more than 12288 slots per frame).  Returns the mask; reset != 0 clears it. */
unsigned orbhip_debug_path_mask(int reset);

/* ---- multi-GPU (one process per GPU) ----
 * The reference is a single process (no distributed back end); these entry points are what a
 * multi-GPU host adds around the unchanged per-frame path: frames or whole sequences are sharded over ranks with no
 * per-frame collective, the vocabulary travels once, and database-sharded brute force has one exchange step. */
/* RCCL communicator over the ranks of one node.  uid: 128-byte ncclUniqueId produced by
 * orbhip_comm_unique_id() on rank 0 and distributed by the caller (file, env, torch store).  nranks = 1 is valid (the
 * collectives then run on a one-rank communicator).  The communicator is destroyed by orbhip_comm_destroy or
 * orbhip_destroy. */
int orbhip_comm_unique_id(uint8_t uid[128]);
int orbhip_comm_init(orbhip_ctx *ctx, int rank, int nranks, const uint8_t uid[128]);
int orbhip_comm_destroy(orbhip_ctx *ctx);
/* Rank and size as the communicator reports them (ncclCommUserRank / ncclCommCount); 0 and 1 without a communicator. */
int orbhip_comm_info(orbhip_ctx *ctx, int *rank, int *nranks);
/* Broadcast of the ORB vocabulary blob (binary format of
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1727-1751, loaded at src/System.cc:331-346)
 * from `root` to every rank over xGMI.  d_buf: device pointer, nbytes on every rank.  Asynchronous on the context
 * stream. */
int orbhip_bcast_blob_device(orbhip_ctx *ctx, void *d_buf, size_t nbytes, int root);
/* Database-sharded brute force (the bookkeeping of src/ORBmatcher.cc:205-226 over a database
 * split by rows): every rank runs orbhip_hamming_knn2_device of the same nq queries against ITS rows (shard_offset =
 * global index of its first row; ranks hold increasing row ranges), then this call all-gathers the nq x 3 int32 results
 * (ncclAllGather, 12 bytes per query per rank) and min-merges them on the device with the reference's tie rule (strict
 * '<': lowest global row wins).  Outputs as orbhip_hamming_knn2_device, global indices, identical on every rank.
 * Asynchronous on the context stream.  Without a communicator (nranks = 1) it reduces to the index shift. */
int orbhip_knn2_allgather_merge_device(orbhip_ctx *ctx, const void *d_best_idx_local, const void *d_best_d_local,
                                       const void *d_second_d_local, int nq, int shard_offset, void *d_best_idx,
                                       void *d_best_d, void *d_second_d);
/* The merge alone, for hosts that exchange through their own collective (torch.distributed in bench.py / the tests):
 * d_parts = nshards consecutive parts of 3 * nq + 1 int32 each: best_idx[nq] | best_d[nq] | second_d[nq] | shard_offset,
 * in order of increasing shard_offset. */
int orbhip_knn2_merge_device(orbhip_ctx *ctx, const void *d_parts, int nshards, int nq, void *d_best_idx, void *d_best_d,
                             void *d_second_d);

/* ---- key-frame database (ref: src/KeyFrameDatabase.cc) ----
 * The BoW inverted file that picks the key frames relocalisation (src/Tracking.cc:2573) and loop detection
 * (src/LoopClosing.cc:193) match against, resident on the device (DESIGN.md "Key-frame database").  Key frames are named by a
 * caller-chosen 64-bit key (the drop-in uses KeyFrame::mnId).  BowVectors are (word[n] ascending, value[n]) pairs as
 * ORBVocabulary::transform returns them; n <= 8192 words per BowVector.  Results are bit for bit those of the reference:
 * candidate order, the (int)(max * 0.8f) threshold, the L1 score summed in double over the common words in ascending id
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-67) and narrowed to float, the float covisibility sums in list order.
 * Divergences from the reference, by design:
 *   - adding a key that is already present returns ORBHIP_E_ARG (the reference would insert the key frame twice);
 *   - every query is a fresh query: no query id is taken (the reference would double-count mnRelocWords when asked twice
 *     with the same Frame::mnId);
 *   - the stale score of a reloc query (a covisible key frame that shares a word but was not scored adds its mRelocScore of
 *     an earlier query, ref :241-268) is kept per key; a key frame never scored has 0 (the reference reads an uninitialised
 *     field, src/KeyFrame.cc:58); erase or clear forget it;
 *   - excluded keys (the loop query's GetConnectedKeyFrames(), ref :82-104) are honoured in both modes.
 * Limits: max_kfs <= 4194304 key frames (ORBHIP_E_CAPACITY when full), 8192 words per BowVector (ORBHIP_E_SIZE), B <= 1024
 * queries per batch (ORBHIP_E_SIZE), word ids below nwords and strictly ascending (ORBHIP_E_ARG).  Nothing is truncated.
 * Memory: the database holds ~60 bytes per key frame plus 12 per BowVector word (twice while a rebuild runs); a query call
 * keeps dense per-(query, key frame) state of B x max_kfs x 37 bytes plus B x 64 KB, allocated on the first call of that
 * batch size and kept: 2.4 GB for B = 1024 at max_kfs = 65536.  A batch that does not fit returns ORBHIP_E_HIP.
 * A query call that fails (invalid query, output too small) leaves the database as it was -- the stale reloc scores
 * included -- so the same call with a larger output returns what it would have returned the first time. */
#define ORBHIP_KFDB_RELOC 0   /* DetectRelocalizationCandidates (ref :199-311) */
#define ORBHIP_KFDB_LOOP 1    /* DetectLoopCandidates (ref :78-197) */
/* Replaces KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary&) (ref :33-37): an empty database over `nwords` words
 * (ORBVocabulary::size()) for at most max_kfs key frames.  delta_max: key frames added between two rebuilds of the inverted
 * file (0 = 128).  Calling it again drops the old database. */
int orbhip_kfdb_init(orbhip_ctx *ctx, int nwords, int max_kfs, int delta_max);
/* Replaces KeyFrameDatabase::add (ref :40-46): the key frame's BowVector joins every word's list after the key frames added
 * before it. */
int orbhip_kfdb_add(orbhip_ctx *ctx, uint64_t key, const uint32_t *word, const double *value, int n);
/* Replaces KeyFrameDatabase::erase (ref :48-68); an absent key is not an error.  clear (ref :70-74) empties the database. */
int orbhip_kfdb_erase(orbhip_ctx *ctx, uint64_t key);
int orbhip_kfdb_clear(orbhip_ctx *ctx);
/* The key frame's KeyFrame::GetBestCovisibilityKeyFrames(10) as keys, best first (n <= 10); read by orbhip_kfdb_detect*.
 * Neighbours need not be in the database. Reset by add. */
int orbhip_kfdb_set_covis(orbhip_ctx *ctx, uint64_t key, const uint64_t *neigh, int n);
/* Key frames in the database, in the delta region, erased but not yet folded out; rebuilds so far.  Any pointer may be NULL. */
int orbhip_kfdb_info(orbhip_ctx *ctx, int *live, int *delta, int *tombs, long long *rebuilds);
/* The first half of one query (ref :82-137 loop, :203-239 reloc), for the C++ drop-in, which runs the covisibility step on its
 * own KeyFrame objects: every key frame that shares a word with the BowVector, excluded ones included, in the reference's
 * order (lKFsSharingWords, excluded ones at the place they were first met), with its shared-word count and its score (0 when
 * it was not scored: excluded, or count <= *min_common).  *nout = number of such key frames; ORBHIP_E_CAPACITY when it
 * exceeds cap (the first cap are filled).  A reloc-mode call also updates the stale scores. */
int orbhip_kfdb_score(orbhip_ctx *ctx, int mode, const uint32_t *word, const double *value, int n, const uint64_t *excluded,
                      int nx, uint64_t *keys, int32_t *counts, float *scores, int cap, int *nout, int *min_common);
/* Replaces DetectLoopCandidates(pKF, minScore) / DetectRelocalizationCandidates(F) (ref :78-311) for B queries at once,
 * exactly as B calls in batch order (stale reloc scores pass from query b to b + 1).  Queries as CSR (qoff[B + 1], qword,
 * qvalue), excluded keys per query as CSR (xoff[B + 1], xkey; xoff may be NULL on the host entry point), min_score for the
 * loop mode.  Candidates as CSR: out_off[B + 1], out_keys[out_off[B]]; ORBHIP_E_CAPACITY when out_off[B] > out_cap (out_off
 * is still filled, nothing changed: call again with out_cap >= out_off[B]).  orbhip_kfdb_detect_device takes device pointers
 * (xoff not NULL) and, unlike other *_device entry points, synchronises: it reads qoff[0], qoff[B], xoff[0], xoff[B] before the
 * launches (ORBHIP_E_ARG unless both start at 0) and the status word and out_off[B] after them (limits are checked on the
 * device); ORBHIP_E_CAPACITY as the host entry point. */
int orbhip_kfdb_detect(orbhip_ctx *ctx, int mode, int B, const int32_t *qoff, const uint32_t *qword, const double *qvalue,
                       const int32_t *xoff, const uint64_t *xkey, float min_score, int32_t *out_off, uint64_t *out_keys,
                       int out_cap);
int orbhip_kfdb_detect_device(orbhip_ctx *ctx, int mode, int B, const void *d_qoff, const void *d_qword, const void *d_qvalue,
                              const void *d_xoff, const void *d_xkey, float min_score, void *d_out_off, void *d_out_keys,
                              int out_cap);
/* Phase timing of the query calls (no counterpart in the reference): with timing on, every orbhip_kfdb_score / _detect /
 * _detect_device records HIP events at its phase boundaries; orbhip_kfdb_phase_times gives the last call's six phase times in
 * ms: 0 inverted-file walk (with validation, exclusion and the delta region), 1 max count, 2 scores, 3 reference order,
 * 4 covisibility accumulation, 5 retention + output (4 and 5 are 0 for orbhip_kfdb_score). */
int orbhip_kfdb_set_timing(orbhip_ctx *ctx, int on);
int orbhip_kfdb_phase_times(orbhip_ctx *ctx, float *ms);

/* ---- resident local map and Tracking::SearchLocalPoints (ref: src/Tracking.cc:2315-2365) ----
 * What Frame::isInFrustum (src/Frame.cc:613-669) and ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:45-129) read from a MapPoint lives on the device under a caller-chosen non-zero 64-bit key (the drop-in
 * uses MapPoint::mnId + 1) and changes only when LocalMapping touches the point; a search sends a camera, a list of keys and
 * one skip byte per point.  Results are bit for bit those of the reference's loops.
 * Limits: max_points <= 16777216; a put that would exceed max_points returns ORBHIP_E_CAPACITY and leaves the store as it
 * was; a key twice in one put / update_flags / erase call is ORBHIP_E_ARG; nlevels <= 16.  Nothing is truncated.  A put that
 * fails with ORBHIP_E_HIP part way (points travel 4096 at a time) may leave keys in the store whose data never arrived: they are
 * reported not in view until they are put again.  put / update_flags / erase synchronise the context's stream once per 4096 points.
 * Divergences from the reference, by design: a point at the camera centre (dist == 0), one with a non-finite position,
 * distance or mfMaxDistance / dist is reported not in view (the reference's int(ceil(inf)) is undefined); a key the store does
 * not know is reported not in view.  The scale level comes from a threshold table built with the host's logf (below). */
#define ORBHIP_MP_OBSERVED 1   /* MapPoint::Observations() > 0 */
#define ORBHIP_MP_BAD 2        /* MapPoint::isBad() */
/* A store for at most max_points map points; calling it again drops the old store.  clear forgets every point. */
int orbhip_map_init(orbhip_ctx *ctx, int max_points);
int orbhip_map_clear(orbhip_ctx *ctx);
int orbhip_map_info(orbhip_ctx *ctx, int *live, int *capacity);
/* Batched upsert: pos / normal = mWorldPos / mNormalVector [3n], min_dist / max_dist = the RAW mfMinDistance / mfMaxDistance
 * (0.8f * / 1.2f * of GetMin/MaxDistanceInvariance are applied on the device: PredictScale reads the raw value),
 * desc = GetDescriptor() [32n], flags = ORBHIP_MP_* [n]. */
int orbhip_map_put(orbhip_ctx *ctx, int n, const uint64_t *keys, const float *pos, const float *normal, const float *min_dist,
                   const float *max_dist, const uint8_t *desc, const uint8_t *flags);
/* Flags of points already in the store (ORBHIP_E_ARG for a key that is not); erase forgets points (absent keys are no error). */
int orbhip_map_update_flags(orbhip_ctx *ctx, int n, const uint64_t *keys, const uint8_t *flags);
int orbhip_map_erase(orbhip_ctx *ctx, int n, const uint64_t *keys);
/* The slots of keys, for orbhip_search_local_points_device: -1 for a key the store does not know.  A slot stays a point's
 * until it is erased or the store is cleared. */
int orbhip_map_slots(orbhip_ctx *ctx, int n, const uint64_t *keys, int32_t *slots);

/* The frame's side of isInFrustum as the caller's Frame holds it: mRcw (row-major), mtcw, mOw; fx fy cx cy, mbf; mnMinX, mnMaxX,
 * mnMinY, mnMaxY; mvScaleFactors[nlevels], mfLogScaleFactor, mnScaleLevels; the viewingCosLimit of the call (Tracking passes 0.5)
 * and th.  level_ratio is the library's: T[k] = the smallest float r with logf(r) / log_scale_factor > (float)k, so that
 * PredictScale's ceil(logf(ratio) / mfLogScaleFactor), clamped, is the number of k < nlevels - 1 with ratio >= T[k].
 * orbhip_search_local_points fills it itself; for the _device form orbhip_local_camera_prepare does. */
typedef struct {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float scale_factors[16];
    float log_scale_factor;
    int32_t nlevels;
    float viewing_cos_limit, th;
    float level_ratio[15];
    int32_t reserved;
} orbhip_local_camera;
/* What isInFrustum leaves in the MapPoint: mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel,
 * mTrackViewCos; all 0 for a point that is not in view (skipped, bad, unknown or rejected). */
typedef struct {
    float u, v, proj_xr, view_cos;
    int32_t level, in_view;
} orbhip_local_point;
/* Fills cam->level_ratio from cam->log_scale_factor and cam->nlevels (cached per pair in the context).  The table builder
 * checks what it assumes -- the predicate is false for the 4096 floats below T[k] and true for the 4096 from it -- and returns
 * ORBHIP_E_ARG otherwise, or when log_scale_factor is not a positive finite number or nlevels is outside [1, 16]. */
int orbhip_local_camera_prepare(orbhip_ctx *ctx, orbhip_local_camera *cam);
/* The table alone (host only, no device needed; for tests): table[nlevels - 1]. */
int orbhip_debug_predict_scale_table(float log_scale_factor, int nlevels, float *table);
/* Replaces the second loop of Tracking::SearchLocalPoints and the SearchByProjection behind it.  The frame is the resident set
 * frame_key, put with a grid (orbhip_set_put, orbhip_set_put_from_frame); frame_key 0 = a frame without features (the frustum
 * test alone; match may be NULL).  u_right [n] or NULL, occupied [n] or NULL as in orbhip_search_by_projection.  keys [nq] in the
 * order of mvpLocalMapPoints, skip[k] != 0 = mnLastFrameSeen == mCurrentFrame.mnId.  points [nq]; *n_to_match = the number of
 * points in view; match [n] and *nmatches as orbhip_search_by_projection defines them (use_ratio = 1, check_ori = 0,
 * TH_HIGH = 100): match[i] = index into keys.  One synchronisation per call; 5 bytes per local point cross the bus. */
int orbhip_search_local_points(orbhip_ctx *ctx, uint64_t frame_key, const float *u_right, const uint8_t *occupied,
                               const orbhip_local_camera *cam, const uint64_t *keys, const uint8_t *skip, int nq, float nnratio,
                               orbhip_local_point *points, int *n_to_match, int32_t *match, int *nmatches);
/* B frames laid out as for orbhip_search_by_projection_device, all against the one store: d_cam [B] (prepared),
 * d_slots [B][cap_q] (orbhip_map_slots), d_skip [B][cap_q], d_nq [B]; d_points [B][cap_q], d_n_to_match [B], d_match [B][cap],
 * d_nmatches [B].  No synchronisation.  Every d_cam record must have passed orbhip_local_camera_prepare (the kernel reads at
 * most 16 levels whatever nlevels says). */
int orbhip_search_local_points_device(orbhip_ctx *ctx, const void *d_kps_un, const void *d_desc, const void *d_counts, int cap,
                                      int B, const void *d_u_right, const void *d_occupied, float min_x, float min_y, float inv_w,
                                      float inv_h, const void *d_cell_off, const void *d_cell_idx, const void *d_cam,
                                      const void *d_slots, const void *d_skip, const void *d_nq, int cap_q, float nnratio,
                                      void *d_points, void *d_n_to_match, void *d_match, void *d_nmatches);

/* ---- Tracking::UpdateLocalMap on the resident store (ref: src/Tracking.cc:2367-2429) ----
 * What the two loops of UpdateLocalMap read beside the points: KeyFrame::mvpMapPoints of every key frame, as a table of
 * fixed-stride rows on the device under a caller-chosen non-zero 64-bit key (the drop-in uses KeyFrame::mnId + 1).  A row entry
 * is a point key of the store above or 0 (no point); the table keeps the point's slot and the slot's generation, so an entry
 * whose point was erased, cleared away, or whose slot went to another point resolves to nothing until it is set again.
 *   orbhip_map_vote     the first loop of UpdateLocalKeyFrames (:2411-2429): how many of the frame's points each key frame holds;
 *   orbhip_map_collect  UpdateLocalPoints (:2377-2400): the points of the given key frames, each once, in the reference's order;
 *   orbhip_track_local_points  collect and orbhip_search_local_points as one call, the list never leaving the device.
 * The graph step between vote and collect (:2431-2530: isBad, the maximum, neighbours, children, parents, the limit of 80) stays
 * with the caller, on its own KeyFrame objects.  Everything is integer work: results are exact.
 * Limits: max_kfs <= 65536, max_row <= 8192, max_kfs * (max_row + 1) <= 2^26 entries (8 bytes each; ORBHIP_E_ARG beyond);
 * a full table is ORBHIP_E_CAPACITY; at most 2^24 row entries per collect (ORBHIP_E_SIZE).  A point key the store does not
 * know, a point twice within one row, n > max_row, an index outside the row (its length is that of the last put) and a key
 * frame the table does not know (put excepted) are ORBHIP_E_ARG.  A failed call changes nothing.  Nothing is truncated.
 * kf_put / kf_set / kf_erase synchronise the context's stream once; vote, collect and the fused call once.
 * Divergences from the reference, by design: the vote counts a key frame through its own row (equal to the observation map
 * under the reference's invariant that (KF, idx) is an observation iff KF->mvpMapPoints[idx] is the point); key frames come
 * back in ascending key order (the reference's map<KeyFrame*, int> iterates by heap address; docs/parity.md); a slot that has
 * been freed 2^24 times is retired, so the store's usable capacity can fall below max_points by such slots. */
/* A table of at most max_kfs rows of at most max_row entries; needs orbhip_map_init (which drops the table with the store);
 * calling it again drops the old table.  Nothing is allocated afterwards but the grow-only scratch of collect (4 bytes per row
 * entry of the largest call).  clear forgets every key frame. */
int orbhip_map_kf_init(orbhip_ctx *ctx, int max_kfs, int max_row);
int orbhip_map_kf_clear(orbhip_ctx *ctx);
int orbhip_map_kf_info(orbhip_ctx *ctx, int *live, int *capacity, int *max_row);
/* The whole row of a key frame (upsert): point_keys [n] = mvpMapPoints as keys, 0 = no point. */
int orbhip_map_kf_put(orbhip_ctx *ctx, uint64_t kf_key, int n, const uint64_t *point_keys);
/* Single entries of a row: AddMapPoint / EraseMapPointMatch (key 0) / ReplaceMapPointMatch.  idx [m], point_keys [m]. */
int orbhip_map_kf_set(orbhip_ctx *ctx, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys);
/* Forgets a key frame; an absent key is no error. */
int orbhip_map_kf_erase(orbhip_ctx *ctx, uint64_t kf_key);
/* frame_point_keys [n] = mCurrentFrame.mvpMapPoints as keys (0 = NULL, repeats count as often as they occur; unknown, erased
 * and ORBHIP_MP_BAD points vote for nothing).  kf_keys_out / counts_out [cap]: the key frames with a non-zero count in
 * ascending key order; *nout = their number, ORBHIP_E_CAPACITY when it exceeds cap (the first cap are filled). */
int orbhip_map_vote(orbhip_ctx *ctx, int n, const uint64_t *frame_point_keys, uint64_t *kf_keys_out, int32_t *counts_out, int cap,
                    int *nout);
/* kf_keys [nkf] in the order of mvpLocalKeyFrames (a key twice: its second copy adds nothing).  local_keys_out [cap] = the keys
 * of mvpLocalMapPoints element for element: rows in the given order, each in feature-index order, empty, stale and
 * ORBHIP_MP_BAD entries dropped, the first occurrence of a point kept.  *nlocal = their number, ORBHIP_E_CAPACITY when it
 * exceeds cap (the first cap are filled). */
int orbhip_map_collect(orbhip_ctx *ctx, int nkf, const uint64_t *kf_keys, uint64_t *local_keys_out, int cap, int *nlocal);
/* orbhip_map_collect, then orbhip_search_local_points over that list with skip[k] = (local_keys_out[k] is in seen_keys [nseen]:
 * the frame's own matches, mnLastFrameSeen == mCurrentFrame.mnId; keys the store does not know are ignored).  frame_key,
 * u_right, occupied, cam, nnratio, n_to_match, match, nmatches as there; points [cap]; match[i] indexes local_keys_out.  One
 * dependency chain, one result block, one synchronisation; 8 * nkf + 4 * nseen bytes, the camera and the frame's u_right /
 * occupied go up.  ORBHIP_E_CAPACITY when *nlocal exceeds cap: the first cap keys are filled, nothing else is. */
int orbhip_track_local_points(orbhip_ctx *ctx, uint64_t frame_key, const float *u_right, const uint8_t *occupied,
                              const orbhip_local_camera *cam, int nkf, const uint64_t *kf_keys, int nseen, const uint64_t *seen_keys,
                              float nnratio, uint64_t *local_keys_out, int cap, int *nlocal, orbhip_local_point *points,
                              int *n_to_match, int32_t *match, int *nmatches);

/* ---- Tracking's other two guided searches on the resident map ----
 * orbhip_search_last_frame        ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) of TrackWithMotionModel
 *                                 (ref: src/ORBmatcher.cc:1341-1498): every point the last frame holds, projected with the current
 *                                 pose and searched in a window on the octaves `motion` allows;
 * orbhip_search_keyframe_points   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) of Relocalization
 *                                 (ref: :1500-1627): the key frame's points that are not in found_keys.
 * Points come from the store (orbhip_map_*), the key frame's mvpMapPoints from the key-frame table (orbhip_map_kf_*), octaves and
 * angles of the source features from their resident sets: a camera, the key list, u_right / occupied of the current frame and 16
 * bytes of counts go up in one block, one block comes back, one synchronisation.
 *   cur_key       resident set of the current frame, put with a grid; last_key / kf_set_key: resident sets of the source frame
 *                 (no grid needed; 0 = a frame without features, which no set can hold: n_last == 0 or an empty row then);
 *                 kf_row_key: the key frame's row in the table, as long as its set
 *   cam           Rcw, tcw, intrinsics, mbf, bounds, scale_factors / nlevels of the CURRENT frame, th = the th of the call;
 *                 viewing_cos_limit is not read; the key-frame form also reads Ow and log_scale_factor (PredictScale)
 *   last_point_keys [n_last]  LastFrame.mvpMapPoints as keys: 0 for NULL and for mvbOutlier; a key the store does not know is
 *                 inactive.  A point flagged ORBHIP_MP_BAD takes part, as in the reference, which does not test isBad() there
 *   motion        0 same: octaves [o - 1, o + 1]; 1 forward: [o, ...]; 2 backward: [0, o] (:1351-1365, :1407-1412)
 *   u_right [n] or NULL (monocular), occupied [n] or NULL as in orbhip_search_by_projection (key-frame form: every feature
 *                 that holds a point, :1565-1566; it has no u_right because the reference does not test it there)
 *   queries_out   [n_last] / [row length] or NULL: the queries as the kernel wrote them; inactive ones are all zero
 *   match [n], *nmatches   as orbhip_search_by_projection defines them with use_ratio = 0 (-1, -2); match[i] indexes the source
 *                 feature; *n_active = the number of ORBHIP_Q_ACTIVE queries
 * The arithmetic is the reference's: the camera point is one gemm (double sums, one rounding), invz = (float)(1.0 / (double)z)
 * -- a double division, not the float division of isInFrustum -- and every other operation an individually rounded float one.
 * ORBHIP_E_ARG (ORBHIP_E_SIZE for the last), with no output touched: no store (key-frame form: no table), an unknown set, cur_key
 * without a grid, n_last different from the last set's size, a row whose length differs from its set's, motion outside 0..2,
 * nlevels outside 1..16, a th that is not finite, a last-frame set with an octave outside [0, nlevels), a current frame too
 * large for the match table in LDS.  n_last == 0 or an empty row: match all -1, counts 0, nothing is launched.
 * Divergences from the reference, by design (it reaches undefined behaviour there): a point is inactive when its position, the
 * reciprocal depth (z == 0), u or v is not finite, when dist3D is 0 or not finite, when mfMaxDistance / dist3D is not finite, or
 * when the store does not know its key. */
int orbhip_search_last_frame(orbhip_ctx *ctx, uint64_t cur_key, uint64_t last_key, const uint64_t *last_point_keys, int n_last,
                             const orbhip_local_camera *cam, int motion, const float *u_right, const uint8_t *occupied,
                             int check_ori, int th_high, orbhip_proj_query *queries_out, int *n_active, int32_t *match,
                             int *nmatches);
int orbhip_search_keyframe_points(orbhip_ctx *ctx, uint64_t cur_key, uint64_t kf_set_key, uint64_t kf_row_key,
                                  const uint64_t *found_keys, int n_found, const orbhip_local_camera *cam, const uint8_t *occupied,
                                  int check_ori, int th_high, orbhip_proj_query *queries_out, int *n_active, int32_t *match,
                                  int *nmatches);
/* The last-frame form for B frames, laid out as for orbhip_search_local_points_device: d_cam [B], d_slots [B][cap_q]
 * (orbhip_map_slots; -1 = no point), d_last_kps [B][cap_q] (orbhip_keypoint: octave and angle are read), d_motion [B] (int32),
 * d_nq [B]; d_queries [B][cap_q] or NULL, d_n_active [B], d_match [B][cap], d_nmatches [B].  No synchronisation.  A source
 * keypoint whose octave is outside [0, min(nlevels, 16)) is inactive (the host form refuses such a set). */
int orbhip_search_last_frame_device(orbhip_ctx *ctx, const void *d_kps_un, const void *d_desc, const void *d_counts, int cap, int B,
                                    const void *d_u_right, const void *d_occupied, float min_x, float min_y, float inv_w,
                                    float inv_h, const void *d_cell_off, const void *d_cell_idx, const void *d_cam,
                                    const void *d_slots, const void *d_last_kps, const void *d_motion, const void *d_nq, int cap_q,
                                    int check_ori, int th_high, void *d_queries, void *d_n_active, void *d_match, void *d_nmatches);

/* ---- ORBmatcher::Fuse for LocalMapping::SearchInNeighbors on the resident map ----
 * SearchInNeighbors (ref: src/LocalMapping.cc:2514-2594) calls Fuse(pKFi, vpMapPointMatches) (ref: src/ORBmatcher.cc:825-975) once
 * per target key frame -- 40 to 100 calls -- and then Fuse(mpCurrentKeyFrame, vpFuseCandidates) once.  Everything those loops read
 * is resident: the points in the store, mvpMapPoints of every key frame in the key-frame table, the targets' features in their sets.
 *   orbhip_fuse_row      the first pass: the entries of key frame src_row_key's row, in feature order, projected into K targets and
 *                        searched in each target's window, in one call;
 *   orbhip_fuse_collect  the second pass: orbhip_map_collect over kf_keys (= vpFuseCandidates element for element), every candidate
 *                        that the row of cur_row_key already holds inactive (IsInKeyFrame), projected and searched in the one target.
 * Both return, per (target, point), what the loop of :887-950 finds: best_idx / best_dist as orbhip_window_best defines them with
 * the chi-square gate on (-1 / 256: inactive, or no feature closer than 256).  The caller applies <= TH_LOW and the map edits in
 * the reference's order, re-reading isBad() and IsInKeyFrame() there (the drop-in: LocalMapSearch::FuseInTargets / FuseCandidates).
 * Row k equals what the host projection followed by orbhip_window_best_set gives for target k on the store as it stands at the call.
 *   targets [K]   a key may repeat; cam.viewing_cos_limit is not read, cam.level_ratio is filled by the call
 *   skip          [K][n] or NULL: skip[k][i] != 0 = IsInKeyFrame(target k) as the caller knows it; n = the length of the source row
 *   u_right       the targets' mvuRight one after the other, each as long as its set (fuse_collect: the one target's), or NULL
 *                 for monocular key frames; a feature with u_right >= 0 takes the 7.8 gate over (u, v, proj_xr), else 5.99
 *   queries_out   [K][n] / [cap] or NULL: the queries as the kernel wrote them; inactive ones are all zero
 *   best_idx, best_dist [K][n] / [cap]; n_active [K] / one int: the number of ORBHIP_Q_ACTIVE queries per target
 *   keys_out [cap], *ncand   as orbhip_map_collect.  ORBHIP_E_CAPACITY when *ncand exceeds cap: the first cap keys are filled, *ncand
 *                 has the number and *n_active is 0; nothing else is written
 * The arithmetic is Fuse's, not the frame searches': invz = 1 / z in float, x = xc * invz and then u = fx * x + cx (each operation
 * rounded), KeyFrame::IsInImage's half-open bounds (u < max_x), PO . normal in double against 0.5 * (double)dist3D.
 * K == 0 returns ORBHIP_OK and writes nothing.  An empty source row / no candidates: counts 0, nothing is launched.
 * ORBHIP_E_ARG, with no output touched: no store or table, an unknown row or set, a target without a grid, K < 0, more distinct set
 * keys than the set limit in force (orbhip_set_limit), nlevels outside 1..16, a th that is not finite.  ORBHIP_E_SIZE, likewise:
 * K above 65535, K * n beyond 2^24, a target set of 2^20 features or more, more than 2^24 row entries among kf_keys.
 * Divergences from the reference, by design: a point with dist3D == 0 or not finite, with a non-finite mfMaxDistance / dist3D, or
 * whose entry does not resolve (empty, erased, re-used slot, ORBHIP_MP_BAD) is inactive. */
typedef struct orbhip_fuse_target {
    uint64_t set_key;            /* resident set of the target key frame, put with a grid */
    orbhip_local_camera cam;     /* the TARGET key frame: Rcw, tcw, Ow, intrinsics, mbf, bounds, scale_factors,
                                    log_scale_factor, nlevels, th; level_ratio is filled by the call */
    float inv_level_sigma2[16];  /* KeyFrame::mvInvLevelSigma2 */
} orbhip_fuse_target;
int orbhip_fuse_row(orbhip_ctx *ctx, uint64_t src_row_key, const orbhip_fuse_target *targets, int K, const uint8_t *skip,
                    const float *u_right, orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist, int32_t *n_active);
int orbhip_fuse_collect(orbhip_ctx *ctx, const orbhip_fuse_target *target, uint64_t cur_row_key, int nkf, const uint64_t *kf_keys,
                        const float *u_right, uint64_t *keys_out, int cap, int *ncand, orbhip_proj_query *queries_out,
                        int32_t *best_idx, int32_t *best_dist, int32_t *n_active);

/* ---- LoopClosing's two projection searches on the resident map ----
 * LoopClosing::ComputeSim3 (ref: src/LoopClosing.cc:404-427) gathers the points of the matched key frame and its covisibles and calls
 * SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) (ref: src/ORBmatcher.cc:290-403);
 * LoopClosing::SearchAndFuse (ref: :647-673) calls Fuse(pKF, Scw, mvpLoopMapPoints, 4, vpReplacePoints) (ref: :977-1100) once per
 * corrected key frame, each time with the whole list.  Everything both read is resident.
 *   orbhip_fuse_sim3           the search half of Fuse(pKF, Scw, ...) (:977-1080) for K targets in one call;
 *   orbhip_search_loop_points  orbhip_map_collect over kf_keys (= mvpLoopMapPoints element for element), the list projected from
 *                              where it lies on the device and matched by the sequential claim of orbhip_search_by_projection;
 *   orbhip_map_kf_set_batch    orbhip_map_kf_set for entries of many key frames: one upload, one launch, one synchronisation.
 * targets [K] / target: cam holds Rcw, tcw, Ow as the reference's decomposition of Scw gives them (:986-990: Rcw = sRcw / s,
 * tcw = t / s, Ow = -Rcw' tcw; the caller decomposes on the host), the target's intrinsics, bounds, scale tables and th; mbf,
 * viewing_cos_limit, inv_level_sigma2 are not read and there is no u_right; level_ratio is filled by the call.  A set key may repeat.
 * orbhip_fuse_sim3:
 *   point_keys [n]      mvpLoopMapPoints as store keys; 0 = no point
 *   target_row_keys [K] or NULL: the target's row in the key-frame table, 0 = none.  Point i is inactive for target k when the store
 *                       does not know its key, when it is ORBHIP_MP_BAD, or when a live entry of row k resolves to its slot
 *                       (spAlreadyFound = pKF->GetMapPoints(), :993, :1005; an entry resolves when its generation is the slot's and
 *                       the point is not bad, so a stale entry whose slot went to another point of the list closes nothing)
 *   queries_out [K][n] or NULL; best_idx, best_dist [K][n]; n_active [K]: per (target, point) what the loop of :1062-1079 finds, as
 *                       orbhip_window_best_set defines them with inv_level_sigma2 == NULL (no chi-square gate; -1 / 256: inactive,
 *                       or no feature closer than 256).  proj_xr of a query is 0.
 *   Row k equals, bit for bit, the host projection followed by orbhip_window_best_set on the store as it stands at the call.
 *   The projection is that of orbhip_fuse_row operation for operation (:1012-1049 is :850-888 line for line).
 *   K == 0: ORBHIP_OK, nothing is written.  n == 0: n_active all 0, nothing is launched.
 *   ORBHIP_E_ARG, with no output touched: no store; no table while a row key is non-zero; an unknown row or set; a target without a
 *   grid; K < 0 or n < 0; more distinct set keys than the set limit in force; nlevels outside 1..16; a th that is not finite; a
 *   non-zero key twice in point_keys.  ORBHIP_E_SIZE, likewise: K above 65535, K * n beyond 2^24, a target set of 2^20 features or more.
 * orbhip_search_loop_points:
 *   kf_keys [nkf], keys_out [cap], *npoints   as orbhip_map_collect.  ORBHIP_E_CAPACITY when *npoints exceeds cap: the first cap keys
 *                       are filled, *npoints has the number, *n_active and *nmatches are 0 and match is all -1
 *   matched_keys [size of target->set_key] or NULL: vpMatched as keys, 0 = NULL.  A feature with a non-zero entry is closed (:375); a
 *                       point whose key occurs there is inactive (:306-317)
 *   th_high             the bound on the best distance (:394; the drop-in passes TH_LOW)
 *   queries_out [cap] or NULL (flags ORBHIP_Q_ACTIVE | ORBHIP_Q_OBSERVED); match [size of the set], *nmatches as
 *                       orbhip_search_by_projection defines them with use_ratio = 0 and check_ori = 0; match[i] indexes keys_out
 *   The result equals orbhip_search_by_projection fed with the host projection's queries.
 *   ORBHIP_E_ARG / ORBHIP_E_SIZE with no output touched: those of orbhip_fuse_collect (it has no cur_row_key), and a target set too
 *   large for the match table in LDS.  No key frames or only empty rows: counts 0, match all -1, nothing is launched.
 * orbhip_map_kf_set_batch: kf_keys, idx, point_keys [m]; entry j sets index idx[j] of key frame kf_keys[j]'s row.  ORBHIP_E_ARG, the
 *   table unchanged: an unknown key frame or point, an index outside its row, a point twice within one row after the edits, a
 *   (key frame, index) pair twice in the call.  The table afterwards equals the table after orbhip_map_kf_set per key frame.
 * Divergences from the reference, by design: as orbhip_fuse_row. */
int orbhip_fuse_sim3(orbhip_ctx *ctx, const orbhip_fuse_target *targets, const uint64_t *target_row_keys, int K,
                     const uint64_t *point_keys, int n, orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist,
                     int32_t *n_active);
int orbhip_search_loop_points(orbhip_ctx *ctx, const orbhip_fuse_target *target, int nkf, const uint64_t *kf_keys,
                              const uint64_t *matched_keys, int th_high, uint64_t *keys_out, int cap, int *npoints,
                              orbhip_proj_query *queries_out, int *n_active, int32_t *match, int *nmatches);
int orbhip_map_kf_set_batch(orbhip_ctx *ctx, int m, const uint64_t *kf_keys, const int32_t *idx, const uint64_t *point_keys);

/* ---- ORBmatcher::SearchBySim3 on the resident map ----
 * LoopClosing::ComputeSim3 calls SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, 7.5) (ref: src/ORBmatcher.cc:1102-1326,
 * src/LoopClosing.cc:375) after every successful solver iteration: the points of each key frame are carried into the other camera,
 * searched there, and a pair counts when the two directions name each other.  Everything it reads is resident: the points in the
 * store, mvpMapPoints of both key frames in the key-frame table, both feature sets with their grids.  One pair of key frames per call.
 *   sides [2]       side 1, side 2: set_key = the key frame's resident set, put with a grid; cam = its Rcw / tcw (world -> camera),
 *                   intrinsics, image bounds, scale_factors, log_scale_factor, nlevels.  Ow, mbf, viewing_cos_limit, th and
 *                   inv_level_sigma2 are not read; level_ratio is filled by the call.
 *   row_keys [2]    the sides' rows in the key-frame table; each row must be as long as its set has features (the matches index both)
 *   sR21, t21       [9] row-major, [3]: carry a point of camera 1 into camera 2 (the reference's (1.0/s12)*R12.t() and -sR21*t12);
 *   sR12, t12       the other way (s12*R12, t12).  The caller composes them on the host, as it decomposes Scw for orbhip_fuse_sim3.
 *   th, th_high     the window factor (ComputeSim3 passes 7.5) and the bound on the best distance (TH_HIGH = 100)
 *   taken1 [n1], taken2 [n2] or NULL: vbAlreadyMatched1 / vbAlreadyMatched2 (:1129-1142), non-zero = the entry stays out
 *   match12 [n1]    the feature of key frame 2 of every agreed pair (:1310-1323), -1 elsewhere; *nfound = their number
 *   n_active [2]    the ORBHIP_Q_ACTIVE queries of direction 0 (row 1 into set 2) and direction 1 (row 2 into set 1)
 *   queries1_out, best1, dist1 [n1]; queries2_out, best2, dist2 [n2], each may be NULL: the queries as the kernel wrote them (an
 *                   inactive one is all zero; proj_xr is 0) and what the loops of :1196-1219 / :1276-1299 find, as
 *                   orbhip_window_best_set defines them with inv_level_sigma2 == NULL (no chi-square gate; -1 / 256: inactive, or
 *                   no feature closer than 256).  match12[i1] = best1[i1] if dist1[i1] <= th_high and, with i2 = best1[i1],
 *                   dist2[i2] <= th_high and best2[i2] == i1.
 * An entry is active when it resolves (live, not ORBHIP_MP_BAD, the entry's generation), its taken byte is 0, z >= 0 (`< 0.0`
 * skips), the projection lies inside the DESTINATION's half-open IsInImage bounds and 0.8f * mfMinDistance <= dist3D <=
 * 1.2f * mfMaxDistance.  The arithmetic is the reference's: p = Rsw * Xw + tsw rounded to float, then sR * p + t, one gemm each
 * (double sums, one rounding); invz = 1 / z in float; x = X * invz and then u = fx * x + cx, each operation rounded (Fuse's
 * association); dist3D = cv::norm of the CAMERA point (there is no P - Ow here); no viewing-angle test; PredictScale(dist3D,
 * destination), radius = th * scale_factors[level], levels [level - 1, level], the first feature of smallest distance.
 * One quirk of the reference is kept: fx, fy, cx, cy are SIDE 1's in both directions (:1105-1108, used at :1170 and :1250); bounds,
 * scale tables and grid are the destination's.  sides[1].cam's intrinsics are therefore not read.
 * row_keys[0] == row_keys[1] (with the same set) is legal.  Two rows without a point: counts 0, match12 all -1, nothing is launched.
 * One upload (two camera records, the similarity, the taken bytes), one result block, one synchronisation.
 * ORBHIP_E_ARG, with no output touched: no store or table, an unknown row or set, a set without a grid, a row whose length is not
 * its set's feature count, nlevels outside 1..16, a th that is not finite, more distinct sets than the set limit in force.
 * ORBHIP_E_SIZE, likewise: a set of 2^20 features or more.
 * Divergences from the reference, by design: as orbhip_fuse_row (dist3D == 0 or not finite, a non-finite mfMaxDistance / dist3D,
 * an entry that does not resolve: inactive). */
int orbhip_search_by_sim3(orbhip_ctx *ctx, const orbhip_fuse_target *sides, const uint64_t *row_keys, const float *sR21,
                          const float *t21, const float *sR12, const float *t12, float th, int th_high, const uint8_t *taken1,
                          const uint8_t *taken2, int32_t *match12, int *nfound, int32_t *n_active, orbhip_proj_query *queries1_out,
                          int32_t *best1, int32_t *dist1, orbhip_proj_query *queries2_out, int32_t *best2, int32_t *dist2);

/* ---- map points refreshed in place on the resident store ----
 * MapPoint::ComputeDistinctiveDescriptors (ref: src/MapPoint.cc:257-322) and MapPoint::UpdateNormalAndDepth (ref: :345-386) for a
 * batch of points, from their observation lists: the observers' descriptors and octaves are read from the resident feature sets, the
 * position from the store, the camera centres from kfs.  The store's descriptor, normal and distance range are written in place and
 * come back for the host objects as well.  One upload (8 B per point and 4 B of ref_pos, 8 B per observation, 32 B per key
 * frame; no descriptors), one launch, one synchronisation.
 *   prm        mvScaleFactors[nlevels], mnScaleLevels of the key frames; what = ORBHIP_REFRESH_DESC | ORBHIP_REFRESH_NORMAL
 *   kfs [nkf]  the key frames the lists name: resident set, GetCameraCenter(), ORBHIP_KF_BAD = isBad()
 *   point_keys [P]; off [P + 1] ascending from 0; obs_kf / obs_idx [off[P]]: observation j of point p is feature obs_idx[j] of key
 *              frame kfs[obs_kf[j]], the list in ascending KeyFrame::mnId (docs/parity.md; the call never reorders it);
 *              ref_pos [P]: the position of mpRefKF inside the point's list (read for ORBHIP_REFRESH_NORMAL only)
 *   Descriptor half: observers with ORBHIP_KF_BAD are left out; if none remain the descriptor stays; otherwise the first row with the
 *              least median sorted_row[(size_t)(0.5 * (N - 1))] wins.  best_pos [P] = its position in the list, or -1.
 *   Normal and depth half: bad observers are NOT left out (the reference has no such test); arithmetic in docs/parity.md.
 *   status [P] bit 0: descriptor set, bit 1: normal and depth set.  A point with ORBHIP_MP_BAD in the store, or with an empty list, is
 *              left untouched: status 0.  desc_out [32 P], normal_out [3 P], min_dist_out, max_dist_out [P] hold the store's values
 *              after the call, also for an untouched half.  Every output but status may be NULL.
 *   ORBHIP_E_ARG, checked before any device work, nothing changed: an unknown point key or a key twice; a set that is not resident;
 *   more distinct sets than the set limit in force; obs_kf / obs_idx out of range; ref_pos outside a non-empty list when
 *   ORBHIP_REFRESH_NORMAL is asked; nlevels outside 1..16 or a set with an octave outside [0, nlevels); off not ascending from 0; what
 *   outside 1..3.  ORBHIP_E_SIZE: a list of 2^20 rows or more.  P == 0: ORBHIP_OK.  Nothing is truncated.
 * orbhip_map_get: read-back of n store entries; any output may be NULL; an unknown key is ORBHIP_E_ARG.  flags = ORBHIP_MP_*. */
#define ORBHIP_REFRESH_DESC 1     /* ComputeDistinctiveDescriptors */
#define ORBHIP_REFRESH_NORMAL 2   /* UpdateNormalAndDepth */
#define ORBHIP_KF_BAD 1
typedef struct {
    uint64_t set_key;
    float Ow[3];
    uint32_t flags;
} orbhip_refresh_kf;
typedef struct {
    float scale_factors[16];
    int32_t nlevels;
    int32_t what;
} orbhip_refresh_params;
int orbhip_map_refresh(orbhip_ctx *ctx, const orbhip_refresh_params *prm, int nkf, const orbhip_refresh_kf *kfs, int P,
                       const uint64_t *point_keys, const int32_t *off, const int32_t *obs_kf, const int32_t *obs_idx,
                       const int32_t *ref_pos, uint8_t *status, int32_t *best_pos, uint8_t *desc_out, float *normal_out,
                       float *min_dist_out, float *max_dist_out);
int orbhip_map_get(orbhip_ctx *ctx, int n, const uint64_t *keys, float *pos, float *normal, float *min_dist, float *max_dist,
                   uint8_t *desc, uint8_t *flags);

/* ---- map points moved in place on the resident store ----
 * orbhip_map_correct_sim3: the point loop of LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-568) for the points of K corrected
 * key frames.  Per point that is not ORBHIP_MP_BAD in the store: the store's position, widened to double, goes through
 * xf[corr].Siw and then xf[corr].corrected_Swi (g2o::Sim3::map, s*(r*xyz)+t, every operation rounded on its own; docs/parity.md,
 * "CorrectLoop"), is rounded to float once and written back (status bit 0).  A point with a non-empty list then gets
 * MapPoint::UpdateNormalAndDepth as orbhip_map_refresh computes it (status bit 1), with the camera centre of observer o taken as
 * kfs[o].Ow_after when 0 <= kfs[o].rank < corr[p] and as kfs[o].Ow_before otherwise: in the reference the points of key frame j are
 * refreshed after SetPose of key frames 0 .. j - 1 and before its own.  The same rule gives the reference observer's centre.
 *   prm          scale_factors, nlevels as for orbhip_map_refresh; what is ignored
 *   xf [K]       per corrected key frame, in the loop's order; kfs [nkf] the key frames the lists name, rank = position in that
 *                order or -1 for a key frame that is not corrected
 *   point_keys [P]; corr [P] in [0, K); off [P + 1] ascending from 0; obs_kf [off[P]] into kfs, each list in ascending KeyFrame::mnId;
 *   ref_pos [P]  position of mpRefKF in the list; ref_level [P] the octave of mpRefKF's feature.  No feature set has to be resident.
 *   status [P]; pos_out, normal_out [3 P], min_dist_out, max_dist_out [P]: the store's values after the call.  Any output but
 *   status may be NULL.  A bad point keeps everything (status 0); an empty list moves the position only (status 1).  Flags,
 *   generation and descriptor are never touched.
 *   ORBHIP_E_ARG, checked before any device work, nothing changed: an unknown point key or a key twice; corr, obs_kf out of range;
 *   ref_pos outside a non-empty list; ref_level >= nlevels; nlevels outside 1..16; off not ascending from 0; a rank outside [-1, K);
 *   a non-negative rank twice; K < 1 with P > 0.  ORBHIP_E_SIZE: a list of 2^20 rows or more.  P == 0: ORBHIP_OK.
 *   One packed upload (128 B per corrected key frame, 28 B per listed key frame, 17 B per point, 4 B per observation), one launch,
 *   one result block, one synchronisation.
 * orbhip_map_correct_se3: the point loop of LoopClosing::RunGlobalBundleAdjustment (ref: :762-797).  corr[p] >= 0: Xc =
 *   Rcw_before*Xw + tcw_before, Xw' = Rwc*Xc + twc of xf[corr[p]], each one gemm (products and sums in double from 0.0, t added, one
 *   rounding to float); corr[p] == -1: the position becomes pos_set[3 p] (SetWorldPos(mPosGBA)).  Position only: status bit 0.  Bad
 *   points are untouched, status 0.  ORBHIP_E_ARG: an unknown point key or a key twice; corr outside [-1, K); K < 0; a corr of -1
 *   with pos_set == NULL.  pos_out [3 P] may be NULL. */
typedef struct {
    double q[4]; /* x y z w, unit */
    double t[3];
    double s;
} orbhip_sim3d;
typedef struct {
    orbhip_sim3d Siw, corrected_Swi;
} orbhip_correct_xf;
typedef struct {
    float Ow_before[3], Ow_after[3];
    int32_t rank;
} orbhip_correct_kf;
typedef struct {
    float Rcw_before[9], tcw_before[3], Rwc[9], twc[3];
} orbhip_correct_se3;
int orbhip_map_correct_sim3(orbhip_ctx *ctx, const orbhip_refresh_params *prm, int K, const orbhip_correct_xf *xf, int nkf,
                            const orbhip_correct_kf *kfs, int P, const uint64_t *point_keys, const int32_t *corr, const int32_t *off,
                            const int32_t *obs_kf, const int32_t *ref_pos, const uint8_t *ref_level, uint8_t *status, float *pos_out,
                            float *normal_out, float *min_dist_out, float *max_dist_out);
int orbhip_map_correct_se3(orbhip_ctx *ctx, int K, const orbhip_correct_se3 *xf, int P, const uint64_t *point_keys, const int32_t *corr,
                           const float *pos_set, uint8_t *status, float *pos_out);

/* ---- the covisibility graph from the resident key-frame table ----
 * KeyFrame::UpdateConnections (ref: src/KeyFrame.cc:731-812) for a batch of key frames.  w(q, j) = the number of points that are
 * resolving entries (live, not ORBHIP_MP_BAD, of the entry's generation) of both row q and row j of the table above.
 *   kf_keys [nq]   the key frames to update, nq <= 65536; a key twice gives the same answer twice; th >= 1 (the reference uses 15)
 *   off_out [nq + 1]; entries off_out[q] .. off_out[q + 1] - 1 of nbr_keys_out / weights_out [cap] are the key frames j != q with
 *                  w(q, j) > 0 in ascending key order: KFcounter, and so mConnectedKeyFrameWeights (docs/parity.md)
 *   order_out [cap], nordered_out [nq]: order_out[off_out[q] + r], r < nordered_out[q], is the position within q's segment of the
 *                  r-th element of mvpOrderedConnectedKeyFrames: the links of weight >= th, or, when there are none, the single
 *                  link of greatest weight (the first maximum in ascending key order), in descending weight, ties by descending key
 *   A query whose row is empty, or that shares nothing, has an empty segment and nordered_out[q] = 0.  *ntotal = off_out[nq].
 * ORBHIP_E_ARG: a key the table does not know, th < 1, nq > 65536.  ORBHIP_E_CAPACITY: more than cap links; *ntotal has the number
 * and nothing else is written.  ORBHIP_E_SIZE: nq times the number of key frames in the table above 2^30.  nq == 0: ORBHIP_OK,
 * off_out[0] = 0.  A failed call changes nothing.  The queries go through the table 32 to a sweep, all sweeps in one call: one upload
 * (4 B per query), one result block (8 B per link), one synchronisation.  Integer work: results are exact. */
int orbhip_map_covis(orbhip_ctx *ctx, int nq, const uint64_t *kf_keys, int th, int32_t *off_out, uint64_t *nbr_keys_out,
                     int32_t *weights_out, int32_t *order_out, int32_t *nordered_out, int cap, int *ntotal);

/* ---- the counts of KeyFrameCulling from the resident key-frame table ----
 * LocalMapping::KeyFrameCulling and KeyFrameCullingForMonoVI (ref: src/LocalMapping.cc:2692-2756, :1477-1584) count, for every
 * covisible key frame, the map points it sees and those of them that at least th_obs other key frames see at the same or a finer
 * scale.  Three facts about feature i of a key frame that the rows do not hold travel once, as one level byte per row entry:
 *   bits 0..3  mvKeysUn[i].octave (0..15)       bit 6  mvuRight[i] >= 0: the observation counts twice in MapPoint::nObs
 *   bit 7      mvDepth[i] > mThDepth || mvDepth[i] < 0: a far stereo point      bits 4, 5  must be 0
 * orbhip_map_kf_levels: the levels of m key frames in one upload, bytes [off[m]], row q = bytes[off[q] .. off[q + 1]) covers features
 * 0 .. off[q + 1] - off[q] - 1.  The device array ([max_kfs][max_row] bytes) is allocated by the first call.  A row keeps its levels
 * through orbhip_map_kf_put / _set of the same key (a key frame's features do not change) and loses them when it is erased, when
 * its row goes to another key, and in orbhip_map_kf_clear / orbhip_map_kf_init / orbhip_map_init.  A row longer than its levels
 * counts as without.  ORBHIP_E_ARG, nothing changed: an unknown key, a key twice in the call, a segment longer than max_row, off
 * not ascending from 0, a byte with bit 4 or 5 set.  m == 0: ORBHIP_OK.
 * orbhip_map_kf_levels_missing: the keys of the live rows whose levels are missing or shorter than the row, ascending; *nout = their
 * number, ORBHIP_E_CAPACITY when it exceeds cap (the first cap are written).  Host state only, no device work. */
int orbhip_map_kf_levels(orbhip_ctx *ctx, int m, const uint64_t *kf_keys, const int32_t *off, const uint8_t *bytes);
int orbhip_map_kf_levels_missing(orbhip_ctx *ctx, uint64_t *kf_keys_out, int cap, int *nout);
/* orbhip_map_cull counts on the map as it is and applies nothing: culling a key frame changes the counts of every other one, so a
 * caller that culls counts again for the candidates behind (ORB_SLAM2::LocalMapSearch::KeyFrameCulling does).  An entry resolves
 * as above: live, not ORBHIP_MP_BAD, of the entry's generation.  For candidate k, entry i of its row resolving to point p, l its octave:
 *   !monocular and the far bit set: the entry is skipped (the reference's continue).  Otherwise n_mps++.
 *   obs(p)       = the sum of 1 + stereo bit over all resolving entries of all live rows that hold p, k's own included: Observations()
 *   others(p, l) = the number of resolving entries of rows other than k that hold p with octave <= l + 1 (far and stereo bits play
 *                  no part: the reference's inner loop tests neither)
 *   the entry is redundant iff obs(p) > th_obs && others(p, l) >= th_obs; n_redundant counts those
 *   redundant[k]      = (double)n_redundant > 0.9 * (double)n_mps, formed on the host: nRedundantObservations>0.9*nMPs
 *   entry_state[k][i] (NULL to skip; [K][max_row], 0 beyond the row) 0 = not counted, 1 = counted, 2 = counted and redundant
 * th_obs: the reference's 3.  A key twice gives the same answer twice.  K == 0: ORBHIP_OK.  Precondition for equality with the
 * reference's loop over observation maps: every observer's row is in the table and current, flags are current (docs/parity.md).
 * ORBHIP_E_ARG, checked before any device work, nothing written: a key the table does not know, th_obs < 1, K > 65536, any live
 * row of the table (candidate or not) whose levels are missing.  ORBHIP_E_SIZE: more than 2^24 candidate row entries in one call.
 * One upload (8 B per candidate), one result block, one synchronisation; scratch only grows.  Integer work: results are exact. */
typedef struct orbhip_cull_count {
    int32_t n_mps, n_redundant;
} orbhip_cull_count;
int orbhip_map_cull(orbhip_ctx *ctx, int K, const uint64_t *kf_keys, int monocular, int th_obs, orbhip_cull_count *counts /* [K] */,
                    uint8_t *redundant /* [K] */, uint8_t *entry_state /* [K][max_row] or NULL */);

/* ---- the structure of local bundle adjustment's problem from the resident key-frame table ----
 * Optimizer::LocalBundleAdjustment (ref: src/Optimizer.cc:2763-2960; the windowed forms at :980 ff. and :1720 ff., BundleAdjustment
 * at :2358 ff. over the whole map) forms, before the solver sees a vertex, lLocalMapPoints from the local key frames' mvpMapPoints,
 * lFixedCameras from every local point's observation map, and one edge per observation.  All three are functions of the rows.
 * An entry resolves as above: live, not ORBHIP_MP_BAD, of the entry's generation.
 *   kf_keys [nkf]          the local key frames in the caller's order, nkf <= 65536; the second copy of a key adds nothing
 *   point_keys_out [0 .. *npoints)   exactly what orbhip_map_collect returns for the same kf_keys, element for element
 *   edge_off_out [*npoints + 1], edges_out [*nedges]: the observers of point j are edges_out[edge_off_out[j] .. edge_off_out[j + 1]),
 *                          one per resolving entry of ANY live row of the table that names the point, in ascending key-frame key
 *                          (the canonical stand-in for map<KeyFrame*, size_t>'s order by address, docs/parity.md).  Every point
 *                          has at least one edge; edge_off_out[*npoints] == *nedges.
 *   edges_out[e].kf        < nkf: the observer is kf_keys[kf], the key's first occurrence; otherwise fixed_keys_out[kf - nkf]
 *   edges_out[e].idx       the feature index in that key frame's row
 *   fixed_keys_out [0 .. *nfixed)    the observers that are no local key frame, each once, in the order of their first edge in
 *                          edges_out: the order in which the reference's walk pushes to lFixedCameras.  A key frame that shares
 *                          nothing with the local points is not listed.
 * nkf == 0, or local rows without entries: ORBHIP_OK, all counts 0, edge_off_out[0] = 0, nothing launched.  ORBHIP_E_ARG, checked
 * before any device work, nothing written: no store or table, a key the table does not know, nkf > 65536.  ORBHIP_E_SIZE: more
 * than 2^24 local row entries.  ORBHIP_E_CAPACITY: any of the three caps is too small; all three counts are written with the true
 * numbers and no array is.  A failed call changes nothing.  One upload (8 B per local key frame and per table row), one result
 * block, one synchronisation; scratch only grows.  Integer work: results are exact and two runs give identical bytes.
 * Precondition for equality with the reference's walk over observation maps: every observer's row is in the table and current,
 * flags are current. */
typedef struct orbhip_ba_edge {
    int32_t kf, idx;
} orbhip_ba_edge;
int orbhip_map_ba_problem(orbhip_ctx *ctx, int nkf, const uint64_t *kf_keys, uint64_t *point_keys_out, int cap_points, int *npoints,
                          int32_t *edge_off_out /* [cap_points + 1] */, orbhip_ba_edge *edges_out, int cap_edges, int *nedges,
                          uint64_t *fixed_keys_out, int cap_fixed, int *nfixed);

/* ---- SearchByBoW against all candidate key frames in one call ----
 * Tracking::Relocalization (ref: src/Tracking.cc:2595-2616) and LoopClosing::ComputeSim3 (ref: src/LoopClosing.cc:304-332) call
 * ORBmatcher::SearchByBoW once per candidate key frame.  Here one call matches the fixed side against K candidates: every key frame
 * is a resident set (orbhip_set_put), and "feature i has a map point that is not bad" is what the key frame's row of the table
 * above answers -- entry i resolves (live, not ORBHIP_MP_BAD, of the entry's generation) -- so no validity bytes travel.
 *   mode 0   SearchByBoW(pKF_k, F) (ref: src/ORBmatcher.cc:159-288): the fixed set is the frame and takes side 2, every feature of it
 *            counts, fixed_row_key is ignored; candidate k takes side 1; a match needs dist <= th.  matches[k][iF] = the key frame's
 *            feature matched to frame feature iF, or -1: vpMapPointMatches of call k as indices.
 *   mode 1   SearchByBoW(pCurrentKF, pKF_k) (:522-655): the fixed set is the current key frame and takes side 1, valid through
 *            fixed_row_key; candidate k takes side 2; dist < th.  matches[k][i1] = the candidate's feature, or -1: vpMatches12.
 *   matches [K][n_fixed], nmatches [K] (after the rotation check when check_ori != 0).  Row k and nmatches[k] equal what
 *   orbhip_search_by_bow_sets returns for that pair (match21 in mode 0, match12 in mode 1) with validity bytes derived from the same
 *   rows at the same moment and th_mode = mode.  A candidate may appear twice (two equal rows); a candidate may be the fixed set.
 * Mode 0 only, all of level_sigma2 .. max_err and ntotal NULL to skip: what PnPsolver::PnPsolver (ref: src/PnPsolver.cc:78-101) and
 * the mvMaxError loop of SetRansacParameters (:154-156) build, for every candidate with nmatches[k] >= min_matches, in the layout
 * orbhip_pnp_score takes.  Candidate k owns entries off[k] .. off[k + 1] - 1 (off [K + 1]; an empty segment below min_matches), the
 * frame's features in ascending index: kp_idx = the frame feature i (mvKeyPointIndices), kf_idx = the matched key-frame feature j,
 * P2D [.][2] = the frame set's keypoint position, max_err = level_sigma2[octave_i] * th2 (a float product), P3Dw [.][3] = the store's
 * position of the point row entry j resolves to.  *ntotal = off[K]; cap = the capacity of the five arrays in entries,
 * K * n_fixed always suffices.
 * Limits: K <= 4095 (the pair record keeps the candidate in 12 bits, its FeatureVector node in 20); K * n_fixed < 2^31.
 * Errors, checked before any device work -- a failed call writes nothing and leaves the context usable.  ORBHIP_E_ARG: an unknown
 * set or row key, a row whose length differs from its set's n, more distinct sets than orbhip_set_limit allows, K < 0 or > 4095, a
 * mode other than 0 / 1, gather outputs in mode 1 or only some of them, nlevels outside 1..64, a frame octave outside [0, nlevels).
 * ORBHIP_E_SIZE: a side-2 FeatureVector of 2^20 entries or more.  ORBHIP_E_CAPACITY: cap < *ntotal; *ntotal is set and nothing else
 * is written.  K == 0: ORBHIP_OK, nothing is written.  Integer work but for the histogram's float bin and max_err: exact. */
typedef struct orbhip_bow_candidate {
    uint64_t set_key, row_key;
} orbhip_bow_candidate;
int orbhip_search_by_bow_candidates(orbhip_ctx *ctx, int mode, uint64_t fixed_set_key, uint64_t fixed_row_key,
                                    const orbhip_bow_candidate *cand, int K, int th, float nnratio, int check_ori,
                                    int32_t *matches /* [K][n_fixed] */, int32_t *nmatches /* [K] */,
                                    /* mode 0 only, all NULL to skip: */ int min_matches, const float *level_sigma2, int nlevels,
                                    float th2, int32_t *off /* [K+1] */, int32_t *kp_idx, int32_t *kf_idx, float *P3Dw, float *P2D,
                                    float *max_err, int cap, int *ntotal);

/* ---- colour frames in, depth at the keypoints out: the RGB-D sensor path (new) ----
 * Every Tracking::GrabImage* converts a 3- or 4-channel image to grey with cvtColor before the extractor sees it (ref:
 * src/Tracking.cc:869-894, 909-922, 939-952), and GrabImageRGBD converts the whole depth map with
 * imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (:924-925) before Frame::ComputeStereoFromRGBD (ref: src/Frame.cc:987-1008)
 * reads it at the keypoints.  Here the colour frame travels as it is and a kernel in front of the pyramid makes it grey; the
 * depth map is read at the keypoints only and converted there.
 *   grey   = (4899 R + 9617 G + 1868 B + 8192) >> 14, OpenCV 2.4's 8-bit RGB2Gray; alpha is ignored; packed pixels, R first
 *            (ORBHIP_FMT_RGB, _RGBA) or B first (_BGR, _BGRA)
 *   depth  d = raw * factor (ORBHIP_DEPTH_U16; ORBHIP_DEPTH_F32 when |factor - 1| > 1e-5, else d = raw) at
 *            ((int)kps[i].x, (int)kps[i].y) -- the DISTORTED keypoint, truncated; d > 0: depth_out[i] = d,
 *            u_right[i] = kps_un[i].x - mbf / d, otherwise both -1.  Each operation rounded to float on its own.
 *            Divergence: a keypoint outside the depth map has no depth (the reference reads out of bounds).
 * Errors (ORBHIP_E_ARG, nothing is written): an unknown format or depth type, stride < w * channels, a device pointer or stride
 * that is not aligned as stated, a factor that is not finite. */
enum { ORBHIP_FMT_GREY = 0, ORBHIP_FMT_RGB, ORBHIP_FMT_BGR, ORBHIP_FMT_RGBA, ORBHIP_FMT_BGRA };
enum { ORBHIP_DEPTH_NONE = 0, ORBHIP_DEPTH_U16, ORBHIP_DEPTH_F32 };
/* Replaces cvtColor(im, im, CV_RGB2GRAY) and its three siblings.  src: rows `stride` bytes apart, any alignment; dst: w bytes of
 * each of h rows are written, nothing else.  format: one of the four colour formats. */
int orbhip_grey(orbhip_ctx *ctx, const uint8_t *src, int w, int h, int stride, int format, uint8_t *dst, int dst_stride);
/* B resident frames, frame b at d_src + b * frame_stride / d_dst + b * dst_frame_stride.  Both bases 4-byte aligned, all four
 * strides multiples of 4: the output can feed orbhip_extract_batch_device.  Asynchronous on the context's stream. */
int orbhip_grey_device(orbhip_ctx *ctx, const void *d_src, int B, int w, int h, int stride, size_t frame_stride, int format,
                       void *d_dst, int dst_stride, size_t dst_frame_stride);
/* orbhip_extract on a colour frame: the frame is staged and copied in as it is (3 or 4 bytes per pixel), the conversion is the
 * first node of the same graph, the results are those of orbhip_extract on the grey image.  ORBHIP_FMT_GREY: orbhip_extract.
 * With orbhip_set_host_pyramid on, level 0 of the host pyramid is the grey image (copied back: the caller never had it). */
int orbhip_extract_color(orbhip_ctx *ctx, const uint8_t *img, int w, int h, int stride, int format, orbhip_keypoint *kps,
                         uint8_t *desc, int cap, int *n_out, float timings_ms[3]);
/* Replaces Frame::ComputeStereoFromRGBD and the convertTo in front of it.  Host arithmetic, n reads of the caller's map: ctx is
 * used for the error text only and may be NULL.  depth: dw x dh, rows depth_stride bytes apart, ORBHIP_DEPTH_U16 or _F32. */
int orbhip_rgbd_depth(orbhip_ctx *ctx, const orbhip_keypoint *kps, const orbhip_keypoint *kps_un, int n, const void *depth,
                      int depth_type, int dw, int dh, int depth_stride, float factor, float mbf, float *u_right,
                      float *depth_out);
/* The same for B resident frames: d_kps / d_kps_un [B][cap], d_counts [B] (NULL: cap per frame), map b at
 * d_depth + b * depth_frame_stride; d_u_right / d_depth_out [B][cap], rows from d_counts[b] on are left alone.  d_depth,
 * depth_stride and depth_frame_stride aligned to the element (2 or 4 bytes).  Asynchronous on the context's stream, behind
 * orbhip_grey_device, orbhip_extract_batch_device and orbhip_undistort_keypoints_device. */
int orbhip_rgbd_depth_device(orbhip_ctx *ctx, const void *d_kps, const void *d_kps_un, const void *d_counts, int cap, int B,
                             const void *d_depth, int depth_type, int dw, int dh, int depth_stride, size_t depth_frame_stride,
                             float factor, float mbf, void *d_u_right, void *d_depth_out);
/* orbhip_frame_build for an RGB-D frame: one graph, one synchronisation.  The colour frame is converted on the device as in
 * orbhip_extract_color; the depth (a w x h map; ORBHIP_DEPTH_NONE: none, u_right / depth_out read -1 and may be NULL) is gathered on the host
 * after the synchronisation -- n reads of the caller's map, where an upload would move the whole map.  Every other output, the
 * resident block and orbhip_frame_fingerprint are those of orbhip_frame_build on the grey image. */
typedef struct orbhip_frame_input {
    const uint8_t *img;
    int w, h, stride, format;
    const void *depth;
    int depth_type, depth_stride;
    float depth_factor, mbf;
} orbhip_frame_input;
int orbhip_frame_build_rgbd(orbhip_ctx *ctx, const orbhip_frame_input *in, const orbhip_frame_params *fp, orbhip_keypoint *kps,
                            orbhip_keypoint *kps_un, uint8_t *desc, int cap, int *n_out, int32_t *cell_off, int32_t *cell_idx,
                            int32_t *word_id, float *weight, int32_t *node_id, float *u_right, float *depth_out);

/* ---- the monocular initialiser's RANSAC hypotheses scored in one call (ref: src/Initializer.cc:305-468) ----
 * Initializer::FindHomography / FindFundamental (:124-223) run mMaxIterations times "eight-point solve, then CheckHomography /
 * CheckFundamental over all N matches" and keep the first iteration of largest score.  The hypotheses depend on mvSets alone, not
 * on each other's scores: the caller computes all H21i / H12i / F21i first (the solves stay on the host, with the integrator's
 * own SVD) and one call scores them all and names the two winners.
 *   match12[n1]   what orbhip_search_for_initialization returns: a feature of frame 2, or a negative value for none.  The k-th
 *                 non-negative entry is the reference's mvMatches12[k]; this ascending order is the order of every sum.
 *   H21, H12      [nH][9] row-major float, the matrices CheckHomography is given; F21 [nF][9], CheckFundamental's.  Either count
 *                 may be 0 and its pointers NULL.
 *   sigma         the reference's mSigma (1.0); invSigmaSquare = (float)(1.0 / (double)(sigma * sigma)), the product in float.
 *   scores        [nH + nF], H first (host form: may be NULL): each the float sum from 0.0f over the matches in ascending
 *                 order, the term of image 1 before the term of image 2 (F: the l2 term before the l1 term), a term with
 *                 chiSquare > th (H 5.991f, F 3.841f; both score with 5.991f - chiSquare) skipped.  A NaN chiSquare is not
 *                 greater than th: it is added, as in the reference.  Every operation is rounded to float on its own, in the
 *                 source's left-to-right order; 1.0 / x is one correctly rounded float division.
 *   best[2]       H then F: `currentScore > score` from score = 0 in index order, i.e. the first hypothesis of largest score
 *                 if that score is > 0 -- otherwise it = -1, score = 0.0f, ninliers = 0.  A NaN score never wins.
 *   inliers       [2][n1] bytes, H then F: the winner's vbMatchesInliers scattered to frame-1 feature indices (0 for an unmatched
 *                 feature and when there is no winner).
 * N == 0 matches: every score 0.0f, no winner.  Limits: nH + nF <= 65535; device form B <= 65535.
 * Errors (ORBHIP_E_ARG, nothing is written): a negative count, sigma not finite or not > 0, nH + nF > 65535, and in the host form
 * a match12[i] >= n2 (divergence: the reference would read mvKeys2 out of bounds).  In the device form such an entry -- anything
 * outside [0, d_cnt2[b]) -- counts as unmatched. */
typedef struct orbhip_init_best {
    float score;
    int32_t it;
    int32_t ninliers;
} orbhip_init_best;
/* One upload, three launches on the context's stream, one synchronisation. */
int orbhip_init_score(orbhip_ctx *ctx, const orbhip_keypoint *kps1_un, int n1, const orbhip_keypoint *kps2_un, int n2,
                      const int32_t *match12, const float *H21, const float *H12, int nH, const float *F21, int nF, float sigma,
                      float *scores, orbhip_init_best *best, uint8_t *inliers);
/* B problems, asynchronous on the context's stream: d_kps1_un [B][cap1] / d_kps2_un [B][cap2] keypoints with d_cnt1 / d_cnt2 [B]
 * and d_match12 [B][cap1], laid out like the arguments and the output of orbhip_search_for_initialization_device, which it can
 * follow without a copy; d_H21 / d_H12 [B][nH][9], d_F21 [B][nF][9]; d_scores [B][nH + nF] (required), d_best [B][2] records,
 * d_inliers [B][2][cap1] bytes, of which the entries from d_cnt1[b] on are left untouched.  The same three launches with B in
 * the grid.  Pointers 4-byte aligned (d_inliers: any). */
int orbhip_init_score_device(orbhip_ctx *ctx, const void *d_kps1_un, const void *d_cnt1, int cap1, const void *d_kps2_un,
                             const void *d_cnt2, int cap2, int B, const void *d_match12, const void *d_H21, const void *d_H12,
                             int nH, const void *d_F21, int nF, float sigma, void *d_scores, void *d_best, void *d_inliers);

/* ---- the inlier checks of the PnP and Sim3 RANSACs for M hypotheses at once (ref: src/PnPsolver.cc:308-339, :209-225;
 * src/Sim3Solver.cc:340-403, :183-200) ----
 * Tracking::Relocalization and LoopClosing::ComputeSim3 run, per candidate key frame, "draw a minimal set, solve it (EPnP / Horn),
 * CheckInliers over all N correspondences, keep the best".  The solves stay on the host with the integrator's own SVD / eigen; the
 * caller hands over the M hypotheses it has and gets every count and what the solver's bookkeeping would have kept.  The
 * reference leaves its loop early, so a call only pays with the hypotheses the caller has: the calls are chunkable (best_in).
 * Arithmetic, every operation rounded on its own in the source's left-to-right order:
 *   PnP   R, t, fu, fv, uc, vc double; X, Y, Z, u, v, max_err float (max_err[i] = sigma2[i] * th2, a float product, the caller's).
 *         Xc = (float)(((r00*X + r01*Y) + r02*Z) + t0) in double, Yc alike; invZc = (float)(1.0 / (((r20*X + r21*Y) + r22*Z) + t2)):
 *         a double division rounded to float, not one float division; ue = uc + ((fu * (double)Xc) * (double)invZc), ve alike;
 *         distX = (float)((double)u - ue), distY alike; error2 = (distX*distX) + (distY*distY) in float; inlier iff
 *         error2 < max_err[i].  NaN and inf fail; there is no test on the sign of the depth.
 *   Sim3  everything float; the caller prepares X3Dc1, X3Dc2, P1im1, P2im2 and max_err1 / max_err2 as Sim3Solver's constructor does
 *         ((float)(9.210 * (double)sigma2); a fork that keeps them in a vector<size_t> passes (float)mvnMaxError1[i]).
 *         Project(X, T, K): Pc[r] = (float)(s + (double)t[r]), s accumulated in double from 0.0 over k = 0, 1, 2 of
 *         (double)R[r][k] * (double)X[k]; invz = 1.0f / Pc[2], one float division; x = Pc[0] * invz; u = (fx * x) + cx; y, v alike.
 *         dist1 = P1im1[i] - Project(X3Dc2[i], T12, K1), dist2 = Project(X3Dc1[i], T21, K2) - P2im2[i] (float subtractions);
 *         err = (float)(((double)d0*d0) + ((double)d1*d1)); inlier iff err1 < max_err1[i] && err2 < max_err2[i].
 * Hypotheses: PnP Rt [M][12] double, R row-major then t; Sim3 T [M][24] float, the 3x4 block of mT12i then of mT21i, row-major.
 * K1 / K2: {fx, fy, cx, cy}.  counts [M] (host forms: may be NULL): the inliers of every hypothesis.
 * PnP rule: from best = best_in (0 on the first call), hypothesis h is a record iff counts[h] >= min_inliers && counts[h] > best,
 * and then best = counts[h].  res = {n_records, best_out}; rec_idx / rec_cnt: the first min(n_records, R) records' indices
 * (ascending) and counts, rec_flags [R][N] their inlier bytes; entries and rows from min(n_records, R) on are left untouched.
 * Sim3 rule: from best = best_in, for each h: counts[h] >= best makes best = counts[h], best_it = h; if counts[h] > min_inliers as
 * well, h is the winner and nothing after it is looked at.  res = {winner, ninliers, best_it, best_out}: winner -1 and ninliers 0
 * when there is none, best_it -1 when no hypothesis of this call reached best_in; flags [N]: the winner's bytes, all 0 without one.
 * Carry: one call over M hypotheses and the same hypotheses in consecutive chunks, best_out fed back as best_in and the indices
 * offset, give the same records / winner (Sim3: the chunks end with the first that has a winner).
 * N == 0: every count 0.  N < min_inliers is no error.  M == 0: no record / winner, best_out = best_in.
 * Errors (ORBHIP_E_ARG, nothing is written): a negative count, off not non-decreasing, M > 65535, B > 65535, R < 1,
 * min_inliers < 0. */
typedef struct orbhip_pnp_result {
    int32_t n_records, best_out;
} orbhip_pnp_result;
typedef struct orbhip_sim3_result {
    int32_t winner, ninliers, best_it, best_out;
} orbhip_sim3_result;
/* One upload through the context's page-locked block, two launches, one synchronisation. */
int orbhip_pnp_score(orbhip_ctx *ctx, const float *P3Dw, const float *P2D, const float *max_err, int N, double fu, double fv, double uc,
                     double vc, const double *Rt, int M, int min_inliers, int best_in, int R, int32_t *counts, orbhip_pnp_result *res,
                     int32_t *rec_idx, int32_t *rec_cnt, uint8_t *rec_flags);
int orbhip_sim3_score(orbhip_ctx *ctx, const float *X3Dc1, const float *X3Dc2, const float *P1im1, const float *P2im2,
                      const float *max_err1, const float *max_err2, int N, const float *K1, const float *K2, const float *T, int M,
                      int min_inliers, int best_in, int32_t *counts, orbhip_sim3_result *res, uint8_t *flags);
/* B problems of different sizes with M hypotheses each, asynchronous on the context's stream.  off [B + 1], min_inliers [B] and
 * best_in [B] (NULL: all 0) are host arrays, read before the call returns; problem b owns the points off[b] .. off[b + 1] of the
 * concatenated device arrays.  d_Rt [B][M][12] / d_T [B][M][24]; d_counts [B][M] (required), d_res [B] records, d_rec_idx /
 * d_rec_cnt [B][R]; problem b's R flag rows of off[b + 1] - off[b] bytes start at byte R * off[b] of d_rec_flags; d_flags is
 * indexed like the points.  All problems share the camera(s).  Pointers aligned to their elements (flags: any). */
int orbhip_pnp_score_device(orbhip_ctx *ctx, const void *d_P3Dw, const void *d_P2D, const void *d_max_err, const int32_t *off, int B,
                            double fu, double fv, double uc, double vc, const void *d_Rt, int M, const int32_t *min_inliers,
                            const int32_t *best_in, int R, void *d_counts, void *d_res, void *d_rec_idx, void *d_rec_cnt,
                            void *d_rec_flags);
int orbhip_sim3_score_device(orbhip_ctx *ctx, const void *d_X3Dc1, const void *d_X3Dc2, const void *d_P1im1, const void *d_P2im2,
                             const void *d_max_err1, const void *d_max_err2, const int32_t *off, int B, const float *K1,
                             const float *K2, const void *d_T, int M, const int32_t *min_inliers, const int32_t *best_in,
                             void *d_counts, void *d_res, void *d_flags);

#ifdef __cplusplus
}
#endif
#endif /* ORBHIP_H */
