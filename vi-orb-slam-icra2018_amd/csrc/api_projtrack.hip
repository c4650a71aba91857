// api_projtrack.hip -- C ABI, part 10: Tracking's two other guided searches on the resident map:
// orbhip_search_last_frame[_device] (TrackWithMotionModel, ref: src/ORBmatcher.cc:1341-1498) and orbhip_search_keyframe_points
// (Relocalization, ref: :1500-1627).  The projection kernels (k_projtrack.hip) write the queries, the window search of
// k_guided.hip reads the points' descriptors from the store by slot.  As orbhip_search_local_points: one packed upload, one
// dependency chain, one result block, one synchronisation.
#include "localmap_store.h"   // fuse_camera_ok: the per-level table of a camera record as both searches need it

// projection -> queries (the caller's block, or the matching scratch behind what the window search carves from it) -> window
// search.  d_n_active must be zero (zeroIt: a memset node in front).
static int last_frame_enqueue(orbhip_ctx *c, OrbLocalMap *M, const void *d_kps, const void *d_desc, const void *d_counts, int cap, int B,
                              const void *d_u_right, const void *d_occupied, float min_x, float min_y, float inv_w, float inv_h,
                              const void *d_cell_off, const void *d_cell_idx, const void *d_cam, const void *d_slots,
                              const void *d_last_kps, const void *d_motion, const void *d_nq, int cap_q, int check_ori, int th_high,
                              void *d_queries, void *d_n_active, void *d_match, void *d_nmatches, bool zeroIt)
{
    const bool search = d_kps != nullptr;
    const size_t searchBytes = search ? align_up(proj_scratch_bytes(B, cap_q, cap), 256) : 0;
    int rc;
    if ((rc = orb_match_scratch(c, searchBytes + (d_queries ? 0 : (size_t)B * cap_q * sizeof(orbhip_proj_query)) + 256))) return rc;
    orbhip_proj_query *dq = d_queries ? (orbhip_proj_query *)d_queries : (orbhip_proj_query *)(c->d_match.as<uint8_t>() + searchBytes);
    if (zeroIt) HIPCHK(c, hipMemsetAsync(d_n_active, 0, (size_t)B * 4, c->stream));
    launch_project_last_frame(c->stream, M->geoA.as<void>(), M->flags.as<uint32_t>(), M->maxPoints, (const orbhip_local_camera *)d_cam,
                              (const int32_t *)d_slots, (const orbhip_keypoint *)d_last_kps, (const int32_t *)d_motion,
                              (const int32_t *)d_nq, cap_q, B, dq, (int32_t *)d_n_active);
    HIPCHK(c, hipGetLastError());
    if (!search) return ORBHIP_OK;
    launch_search_by_projection(c->stream, (const orbhip_keypoint *)d_kps, (const uint8_t *)d_desc, (const int32_t *)d_counts, cap, B,
                                (const float *)d_u_right, (const uint8_t *)d_occupied, min_x, min_y, inv_w, inv_h,
                                (const int32_t *)d_cell_off, (const int32_t *)d_cell_idx, dq, M->desc.as<uint8_t>(),
                                (const int32_t *)d_nq, cap_q, /*use_ratio*/ 0, 0.f, check_ori ? 1 : 0, th_high, (int32_t *)d_match,
                                (int32_t *)d_nmatches, c->d_match.as<void>(), (const int32_t *)d_slots);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_search_last_frame_device(orbhip_ctx *c, const void *d_kps, const void *d_desc, const void *d_counts, int cap,
                                               int B, const void *d_u_right, const void *d_occupied, float min_x, float min_y,
                                               float inv_w, float inv_h, const void *d_cell_off, const void *d_cell_idx,
                                               const void *d_cam, const void *d_slots, const void *d_last_kps, const void *d_motion,
                                               const void *d_nq, int cap_q, int check_ori, int th_high, void *d_queries,
                                               void *d_n_active, void *d_match, void *d_nmatches)
{
    if (!c || !d_kps || !d_desc || !d_counts || cap <= 0 || B <= 0 || !d_cell_off || !d_cell_idx || !d_cam || !d_slots || !d_last_kps ||
        !d_motion || !d_nq || cap_q <= 0 || !d_n_active || !d_match || !d_nmatches || !grid_params_ok(inv_w, inv_h) ||
        cap >= (1 << 19))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame_device: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame_device: no store (orbhip_map_init)");
    if (proj_assign_lds(cap) > 120 * 1024)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame_device: cap too large for the per-frame match table in LDS");
    HIPCHK(c, orb_enter(c));
    return last_frame_enqueue(c, M, d_kps, d_desc, d_counts, cap, B, d_u_right, d_occupied, min_x, min_y, inv_w, inv_h, d_cell_off,
                              d_cell_idx, d_cam, d_slots, d_last_kps, d_motion, d_nq, cap_q, check_ori, th_high, d_queries, d_n_active,
                              d_match, d_nmatches, true);
}

extern "C" int orbhip_search_last_frame(orbhip_ctx *c, uint64_t cur_key, uint64_t last_key, const uint64_t *last_point_keys, int n_last,
                                        const orbhip_local_camera *cam, int motion, const float *u_right, const uint8_t *occupied,
                                        int check_ori, int th_high, orbhip_proj_query *queries_out, int *n_active, int32_t *match,
                                        int *nmatches)
{
    if (!c || !cam || n_last < 0 || (n_last > 0 && !last_point_keys) || !match)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: no store (orbhip_map_init)");
    OrbSetView S = {};
    OrbSetKps L = {};
    if (!orb_set_grid_view(c, cur_key, &S))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: cur_key is an unknown set, or a set without a grid (orbhip_set_put)");
    if (last_key != 0 && !orb_set_kps_view(c, last_key, &L))   // (key 0: a frame without features, which no set can hold)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: last_key is an unknown set");
    if (n_last != L.n) return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: n_last differs from the size of the last frame's set");
    if (motion < 0 || motion > 2) return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: motion outside 0..2");
    if (!fuse_camera_ok(cam)) return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: nlevels outside 1..16, or th not finite");
    if (n_last > 0 && (L.octMin < 0 || L.octMax >= cam->nlevels))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_last_frame: the last frame's set has an octave outside [0, nlevels)");
    if (S.n >= (1 << 19) || proj_assign_lds(S.n) > 120 * 1024)
        return fail(c, ORBHIP_E_SIZE, "orbhip_search_last_frame: the frame has too many features for the match table in LDS");
    const int n = S.n, nq = n_last;
    if (n_active) *n_active = 0;
    if (nmatches) *nmatches = 0;
    for (int i = 0; i < n; i++) match[i] = -1;
    if (nq == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    int rc;
    if ((rc = P.begin(sizeof *cam + (size_t)nq * (4 + sizeof(orbhip_proj_query)) + (size_t)n * (4 + 1 + 4) + 8 * 256))) return rc;
    const void *dcam = P.in(cam, sizeof *cam);
    int32_t *hslots;
    const void *dslots = P.in_reserve((size_t)nq * 4, (void **)&hslots);
    kf_mark_slots(M, last_point_keys, nq, hslots);   // -1 for key 0 (no point, an outlier) and for keys the store does not know
    const float *dur = (n && u_right) ? (const float *)P.in(u_right, (size_t)n * 4) : nullptr;
    const uint8_t *docc = (n && occupied) ? (const uint8_t *)P.in(occupied, (size_t)n) : nullptr;
    const int32_t cnts[4] = {nq, 0, 0, motion};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // nq | active queries | matches | motion (come back with the matches and the queries)
    int32_t *dm = n ? (int32_t *)P.out((size_t)n * 4) : nullptr;
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out((size_t)nq * sizeof(orbhip_proj_query)) : nullptr;
    if ((rc = P.upload())) return rc;
    if ((rc = last_frame_enqueue(c, M, n ? S.d_kps : nullptr, S.d_desc, S.d_cnt, n, 1, dur, docc, S.minX, S.minY, S.invW, S.invH,
                                 S.d_cellOff, S.d_cellIdx, dcam, dslots, L.d_kps, dc + 3, dc, nq, check_ori, th_high, dq, dc + 1, dm,
                                 dc + 2, false)))
        return rc;
    if ((rc = P.download(dc))) return rc;   // counts | matches | queries are adjacent: one copy back, one synchronisation
    if (n) memcpy(match, P.host(dm), (size_t)n * 4);
    if (queries_out) memcpy(queries_out, P.host(dq), (size_t)nq * sizeof(orbhip_proj_query));
    const int32_t *hc = (const int32_t *)P.host(dc);
    if (n_active) *n_active = hc[1];
    if (nmatches) *nmatches = n ? hc[2] : 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_search_keyframe_points(orbhip_ctx *c, uint64_t cur_key, uint64_t kf_set_key, uint64_t kf_row_key,
                                             const uint64_t *found_keys, int n_found, const orbhip_local_camera *cam,
                                             const uint8_t *occupied, int check_ori, int th_high, orbhip_proj_query *queries_out,
                                             int *n_active, int32_t *match, int *nmatches)
{
    if (!c || !cam || n_found < 0 || (n_found > 0 && !found_keys) || !match)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: no store (orbhip_map_init)");
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: no table (orbhip_map_kf_init)");
    OrbSetView S = {};
    OrbSetKps F = {};
    if (!orb_set_grid_view(c, cur_key, &S))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: cur_key is an unknown set, or a set without a grid (orbhip_set_put)");
    if (kf_set_key != 0 && !orb_set_kps_view(c, kf_set_key, &F))   // (key 0: a key frame without features)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: kf_set_key is an unknown set");
    auto it = K->rowOf.find(kf_row_key);
    if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: unknown key frame (orbhip_map_kf_put)");
    const int row = it->second, nq = (int)K->entries[row].size();
    if (nq != F.n) return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: the key frame's row and its set differ in length");
    if (!fuse_camera_ok(cam)) return fail(c, ORBHIP_E_ARG, "orbhip_search_keyframe_points: nlevels outside 1..16, or th not finite");
    if (S.n >= (1 << 19) || proj_assign_lds(S.n) > 120 * 1024)
        return fail(c, ORBHIP_E_SIZE, "orbhip_search_keyframe_points: the frame has too many features for the match table in LDS");
    orbhip_local_camera cm = *cam;
    int rc;
    if ((rc = orbhip_local_camera_prepare(c, &cm))) return rc;
    const int n = S.n;
    if (n_active) *n_active = 0;
    if (nmatches) *nmatches = 0;
    for (int i = 0; i < n; i++) match[i] = -1;
    if (nq == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    // scratch: the window search's | the slot of every row entry | the queries, unless they go back to the caller
    const bool search = n > 0;
    const size_t searchBytes = search ? align_up(proj_scratch_bytes(1, nq, n), 256) : 0, slotBytes = align_up((size_t)nq * 4, 256);
    if ((rc = orb_match_scratch(c, searchBytes + slotBytes + (queries_out ? 0 : (size_t)nq * sizeof(orbhip_proj_query)) + 256))) return rc;
    int32_t *dslots = (int32_t *)(c->d_match.as<uint8_t>() + searchBytes);
    Packed P(c);
    if ((rc = P.begin(sizeof cm + (size_t)n_found * 4 + (size_t)nq * sizeof(orbhip_proj_query) + (size_t)n * (1 + 4) + 8 * 256))) return rc;
    const void *dcam = P.in(&cm, sizeof cm);
    int32_t *hfound;
    const int32_t *dfound = (const int32_t *)P.in_reserve((size_t)n_found * 4, (void **)&hfound);
    kf_mark_slots(M, found_keys, n_found, hfound);
    const uint8_t *docc = (n && occupied) ? (const uint8_t *)P.in(occupied, (size_t)n) : nullptr;
    const int32_t cnts[4] = {nq, 0, 0, row};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // row length | active queries | matches | row (come back with what follows)
    int32_t *dm = n ? (int32_t *)P.out((size_t)n * 4) : nullptr;
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out((size_t)nq * sizeof(orbhip_proj_query))
                                        : (orbhip_proj_query *)(c->d_match.as<uint8_t>() + searchBytes + slotBytes);
    if ((rc = P.upload())) return rc;
    uint32_t *marks = K->marks.as<uint32_t>();
    launch_mark_add(c->stream, dfound, n_found, M->maxPoints, marks);
    launch_project_keyframe_points(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints, marks,
                                   K->rows.as<void>(), K->maxKfs, K->stride, K->maxRow, dc + 3, (const orbhip_local_camera *)dcam,
                                   F.d_kps, dc, nq, 1, dq, dslots, dc + 1);
    launch_mark_clear(c->stream, dfound, n_found, M->maxPoints, marks);
    HIPCHK(c, hipGetLastError());
    if (search) {   // (no u_right: the reference does not test the right coordinate here)
        launch_search_by_projection(c->stream, S.d_kps, S.d_desc, S.d_cnt, n, 1, nullptr, docc, S.minX, S.minY, S.invW, S.invH,
                                    S.d_cellOff, S.d_cellIdx, dq, M->desc.as<uint8_t>(), dc, nq, /*use_ratio*/ 0, 0.f,
                                    check_ori ? 1 : 0, th_high, dm, dc + 2, c->d_match.as<void>(), dslots);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = P.download(dc))) return rc;   // counts | matches | queries: one copy back, one synchronisation
    if (n) memcpy(match, P.host(dm), (size_t)n * 4);
    if (queries_out) memcpy(queries_out, P.host(dq), (size_t)nq * sizeof(orbhip_proj_query));
    const int32_t *hc = (const int32_t *)P.host(dc);
    if (n_active) *n_active = hc[1];
    if (nmatches) *nmatches = n ? hc[2] : 0;
    return ORBHIP_OK;
}
