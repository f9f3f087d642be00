// tirt_pvb.h -- what the list pass of the camera rays (k_pvb_cand, tirt_pvb.hip) and the fused first step of PT_RGB (k_pvb_cand_shade, tirt_render.hip)
// share: the view of the pixels' candidate lists and ONE walk of a camera ray over its pixel's list, so that the two kernels cannot drift apart.
#pragma once
#include "tirt_trace.h"

namespace tirt {

constexpr int PVB_CMAX = 24;                        // leaves on a pixel's list (12: 3 % of the headline's pixels without a list, -1.3 %; 48: no gain -- profiles/r05an_*)

struct PvbView { const int *count; const int2 *cand; const float *bound; };     // [P], [PVB_CMAX][P] (leaf code, bits of the nearest distance any ray of the pixel can reach the leaf's box at), [P]; count < 0: no list

// tirt_pvb.hip, for the test entries tirt_primary_beam_lists_download and tirt_kat_primary_list_walk (tirt_kat.hip): the current lists, made as a batch makes them
int pvb_lists_for_tests(tirt_ctx *c, const char *fn, bool &have);
PvbView pvb_current_view(const tirt_ctx *c);

// One camera ray (from `eye` along `d`, local pixel k of P) against its pixel's list: the hit (hit_t .. hit_prim) and whether it is k_trace's answer (see the
// header of tirt_pvb.hip); a ray that is not `resolved` is k_trace's.  Every lane of the wave calls it (the loop leaves on a ballot); a lane that is not `live`
// comes back unresolved.  `steps`, `trips`: leaf steps of this ray and loop trips of its wave (diagnostics, option "primary_beams_diag").
TD bool pvb_walk_list(const BvhView &b, const PvbView &pv, const int P, const int k, const bool live, const v3 eye, const v3 d,
                      float &hit_t, float &hit_u, float &hit_v, int &hit_prim, int &steps, int &trips)
{
    const RayCtx r = make_ray(eye, d);
    const bool par = ray_has_parallel_axis(r);
    int n = live ? pv.count[k] : 0;
    const float bound = live ? pv.bound[k] : 0.0f;
    bool resolved = live && n >= 0;
    // k_trace's first step for a camera ray: the root's exact box -- when the root is an inner node: in a one-primitive scene the root IS the leaf, k_trace
    // goes straight to the primitive test and a hit that fails the leaf's box has no ancestor to be refused by -- and a NaN ray misses
    bool dead = false;
    if (live) {
        float tn;
        if (b.root_qcode >= 0 && !slabs(r, b.root_min[0], b.root_min[1], b.root_min[2], b.root_max[0], b.root_max[1], b.root_max[2], tn)) dead = true;
        if (!((d.x == d.x) & (d.y == d.y) & (d.z == d.z))) dead = true;
    }
    if (dead) { n = 0; resolved = true; }
    if (!resolved) n = 0;
    hit_t = INF_VALUE; hit_u = 0.0f; hit_v = 0.0f; hit_prim = -1;
    int hit_leaf = -1;
    for (int c = 0; c < PVB_CMAX; c++) {
        // (the lists are sorted by the distance at which a ray of the pixel can reach the leaf's box at the earliest: beyond the hit so far, nothing on the rest of the list can win or tie)
        int2 en = make_int2(0, 0x7f800000);
        if (c < n) en = pv.cand[(size_t)c * P + k];
        const bool go = c < n && __int_as_float(en.y) <= hit_t;
        if (!go) n = 0;
        if (__ballot(go) == 0ull) break;
        trips++; if (go) steps++;
        if (go) (void)trace_leaf_step<true>(b, r, par, ~en.x, hit_t, hit_u, hit_v, hit_prim, hit_leaf);      // k_trace's leaf step itself (tirt_internal.h)
    }
    // within bound: k_trace's answer (a list made without a bound is complete: whatever it says holds)
    if (resolved && !dead && !(hit_t <= bound) && bound < INF_VALUE) resolved = false;
    return resolved;
}

}  // namespace tirt
