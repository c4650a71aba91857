// mock_trisearch.cc -- host model of the entry points ORB_SLAM2::TriangulationSearch calls: a table of resident sets with the
// library's limit and least-recently-used eviction, and orbhip_search_for_triangulation_sets computed on the host from the
// sets' data (tri::flat_search).  No device, no liborbhip.
#include "mock_trisearch.h"

#include <algorithm>
#include <string>

#include "tri_scene.h"

namespace
{
struct Set {
    uint64_t key, fp;
    int n, ng;
    std::vector<tri::Kp> kps;
    std::vector<uint8_t> desc;
    std::vector<int32_t> node, off, idx;
    unsigned long stamp;
};
MockLog g_log;
int g_resident = 0;
}  // namespace

struct orbhip_ctx {
    std::vector<Set> sets;
    int limit = 96;
    unsigned long clock = 0;
    std::string err;
    Set *find(uint64_t key)
    {
        for (size_t i = 0; i < sets.size(); i++)
            if (sets[i].key == key) {
                sets[i].stamp = ++clock;
                return &sets[i];
            }
        return nullptr;
    }
};

MockLog &mock_log() { return g_log; }
int mock_resident() { return g_resident; }

static int fail(orbhip_ctx *c, const char *msg)
{
    if (c) c->err = msg;
    return ORBHIP_E_ARG;
}

extern "C" {

orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return new orbhip_ctx(); }
void orbhip_destroy(orbhip_ctx *c) { delete c; }
const char *orbhip_last_error(const orbhip_ctx *c) { return c ? c->err.c_str() : "no context"; }

uint64_t orbhip_set_fingerprint_rows(const orbhip_keypoint *first_kp, const uint8_t *first_desc, const uint8_t *last_desc, int n)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t bytes) {
        for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const uint8_t *>(p)[i]) * 1099511628211ull;
    };
    mix(&n, sizeof(n));
    mix(first_kp, 8);
    mix(first_desc, 32);
    mix(last_desc, 32);
    return h ? h : 1;
}
uint64_t orbhip_frame_fingerprint(const orbhip_ctx *) { return 0; }
int orbhip_set_put_from_frame(orbhip_ctx *c, uint64_t, orbhip_ctx *, const int32_t *, const int32_t *, const int32_t *, int)
{
    return fail(c, "mock: no frame build");
}

int orbhip_set_info(orbhip_ctx *c, uint64_t key, int *n, int *ng, uint64_t *fingerprint)
{
    Set *s = c->find(key);
    if (!s) return 0;
    *n = s->n; *ng = s->ng; *fingerprint = s->fp;
    return 1;
}

int orbhip_set_limit(orbhip_ctx *c, int max_sets)
{
    g_log.limits.push_back(max_sets);
    c->limit = max_sets < 4 ? 4 : max_sets > 96 ? 96 : max_sets;
    return c->limit;
}

int orbhip_set_drop(orbhip_ctx *c, uint64_t key)
{
    g_log.drops++;
    for (size_t i = 0; i < c->sets.size();)
        if (key == 0 || c->sets[i].key == key) c->sets.erase(c->sets.begin() + i);
        else i++;
    g_resident = (int)c->sets.size();
    return ORBHIP_OK;
}

int orbhip_set_put(orbhip_ctx *c, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *node,
                   const int32_t *off, const int32_t *idx, int ng, float, float, float, float)
{
    if (!c || key == 0 || n <= 0 || !kps || !desc || ng < 0 || ng > n) return fail(c, "orbhip_set_put: bad argument");
    g_log.puts.push_back(key);
    for (size_t i = 0; i < c->sets.size(); i++)
        if (c->sets[i].key == key) {
            c->sets.erase(c->sets.begin() + i);
            break;
        }
    while (c->sets.size() >= (size_t)c->limit) {   // least recently used out
        size_t lru = 0;
        for (size_t i = 1; i < c->sets.size(); i++)
            if (c->sets[i].stamp < c->sets[lru].stamp) lru = i;
        c->sets.erase(c->sets.begin() + lru);
    }
    Set s;
    s.key = key;
    s.n = n;
    s.ng = ng;
    s.kps.assign(reinterpret_cast<const tri::Kp *>(kps), reinterpret_cast<const tri::Kp *>(kps) + n);
    s.desc.assign(desc, desc + (size_t)n * 32);
    s.fp = orbhip_set_fingerprint_rows(kps, desc, desc + (size_t)(n - 1) * 32, n);
    if (ng > 0) {
        s.node.assign(node, node + ng);
        s.off.assign(off, off + ng + 1);
        s.idx.assign(idx, idx + off[ng]);
    } else
        s.off.assign(1, 0);
    s.stamp = ++c->clock;
    c->sets.push_back(s);
    g_resident = (int)c->sets.size();
    return ORBHIP_OK;
}

int orbhip_search_for_triangulation_sets(orbhip_ctx *c, uint64_t key1, const uint8_t *skip1, const float *u_right1,
                                         const orbhip_tri_neighbour *nb, int K, const uint8_t *skip2, const float *u_right2,
                                         const float *scale_factors2, const float *level_sigma2_2, int nlevels2, int only_stereo,
                                         int check_ori, int32_t *matches12, int32_t *nmatches)
{
    if (!c || K < 0) return fail(c, "orbhip_search_for_triangulation_sets: bad argument");
    if (K == 0) return ORBHIP_OK;
    if (nlevels2 < 1 || nlevels2 > 64) return fail(c, "orbhip_search_for_triangulation_sets: nlevels2 must be within 1..64");
    std::vector<uint64_t> keys(1, key1);
    for (int k = 0; k < K; k++)
        if (std::find(keys.begin(), keys.end(), nb[k].key2) == keys.end()) keys.push_back(nb[k].key2);
    if ((int)keys.size() > c->limit) return fail(c, "orbhip_search_for_triangulation_sets: more distinct sets than the set limit in force");
    for (size_t i = 0; i < keys.size(); i++)
        if (!c->find(keys[i])) return fail(c, "orbhip_search_for_triangulation_sets: unknown set (orbhip_set_put)");
    const Set s1 = *c->find(key1);
    g_log.searches++;
    g_log.nb.assign(nb, nb + K);
    g_log.skip1.assign(skip1, skip1 + s1.n);
    g_log.ur1Null = !u_right1;
    g_log.ur2Null = !u_right2;
    size_t at = 0;
    for (int k = 0; k < K; k++) {
        const Set s2 = *c->find(nb[k].key2);
        for (int i = 0; i < s2.n; i++)
            if (s2.kps[i].octave < 0 || s2.kps[i].octave >= nlevels2) return fail(c, "orbhip_search_for_triangulation_sets: octave of key frame 2 out of range");
        nmatches[k] = tri::flat_search(s1.kps.data(), s1.desc.data(), s1.n, skip1, u_right1, s1.node.data(), s1.off.data(), s1.idx.data(),
                                       s1.ng, s2.kps.data(), s2.desc.data(), skip2 + at, u_right2 ? u_right2 + at : nullptr,
                                       s2.node.data(), s2.off.data(), s2.idx.data(), s2.ng, nb[k].F12, nb[k].ex, nb[k].ey, scale_factors2,
                                       level_sigma2_2, only_stereo != 0, check_ori != 0, matches12 + (size_t)k * s1.n);
        at += (size_t)s2.n;
    }
    g_log.skip2.assign(skip2, skip2 + at);
    if (u_right2) g_log.ur2.assign(u_right2, u_right2 + at);
    return ORBHIP_OK;
}

}  // extern "C"
