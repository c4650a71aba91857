// mock_localmap.cc -- the entry points ORB_SLAM2::LocalMapSearch calls, recording their arguments and answering from a script
// (tests/native_localmap/test_localmap_mock.cpp; no device, no liborbhip).
#include "mock_localmap.h"

#include <cstring>

MockLog g_mock;

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return g_mock.failCreate ? nullptr : (orbhip_ctx *)&g_mock; }
void orbhip_destroy(orbhip_ctx *) { g_mock.destroyed++; }
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g_mock.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *) { g_mock.cleared++; return ORBHIP_OK; }
int orbhip_set_limit(orbhip_ctx *, int n) { return n; }
int orbhip_set_drop(orbhip_ctx *, uint64_t key) { g_mock.dropped.push_back(key); return ORBHIP_OK; }
int orbhip_set_has(orbhip_ctx *, uint64_t key, int n) { return key == g_mock.setKey && n == g_mock.setN; }
int orbhip_set_put(orbhip_ctx *, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *, const int32_t *,
                   const int32_t *, int ng, float min_x, float min_y, float inv_w, float inv_h)
{
    g_mock.setPuts++;
    g_mock.setKey = key, g_mock.setN = n, g_mock.setNg = ng;
    g_mock.setKps.assign(kps, kps + n);
    g_mock.setDesc.assign(desc, desc + (size_t)n * 32);
    g_mock.grid[0] = min_x, g_mock.grid[1] = min_y, g_mock.grid[2] = inv_w, g_mock.grid[3] = inv_h;
    return ORBHIP_OK;
}
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *pos, const float *normal, const float *min_dist,
                   const float *max_dist, const uint8_t *desc, const uint8_t *flags)
{
    g_mock.putKeys.assign(keys, keys + n);
    g_mock.putPos.assign(pos, pos + 3 * n);
    g_mock.putNormal.assign(normal, normal + 3 * n);
    g_mock.putMin.assign(min_dist, min_dist + n);
    g_mock.putMax.assign(max_dist, max_dist + n);
    g_mock.putDesc.assign(desc, desc + 32 * n);
    g_mock.putFlags.assign(flags, flags + n);
    return ORBHIP_OK;
}
int orbhip_map_update_flags(orbhip_ctx *, int n, const uint64_t *keys, const uint8_t *flags)
{
    g_mock.flagKeys.assign(keys, keys + n);
    g_mock.flagVals.assign(flags, flags + n);
    return ORBHIP_OK;
}
int orbhip_map_erase(orbhip_ctx *, int n, const uint64_t *keys) { g_mock.erased.assign(keys, keys + n); return ORBHIP_OK; }
int orbhip_search_local_points(orbhip_ctx *, uint64_t frame_key, const float *u_right, const uint8_t *occupied,
                               const orbhip_local_camera *cam, const uint64_t *keys, const uint8_t *skip, int nq, float nnratio,
                               orbhip_local_point *points, int *n_to_match, int32_t *match, int *nmatches)
{
    g_mock.searches++;
    g_mock.frameKey = frame_key;
    g_mock.cam = *cam;
    g_mock.nnratio = nnratio;
    g_mock.keys.assign(keys, keys + nq);
    g_mock.skip.assign(skip, skip + nq);
    g_mock.hadURight = u_right != nullptr;
    if (u_right) g_mock.uRight.assign(u_right, u_right + g_mock.setN);
    g_mock.occupied.assign(occupied, occupied + g_mock.setN);
    if (g_mock.failSearch) return ORBHIP_E_HIP;
    for (int k = 0; k < nq; k++) points[k] = g_mock.answerPoints[k];
    for (int i = 0; i < g_mock.setN; i++) match[i] = g_mock.answerMatch[i];
    *n_to_match = g_mock.answerToMatch;
    *nmatches = g_mock.answerMatches;
    return ORBHIP_OK;
}
}

// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (this program links neither)
#include "slamlite.h"
namespace ORB_SLAM2
{
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
}
