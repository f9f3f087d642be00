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

#define PVB_HD __host__ __device__ __forceinline__

// A triangle leaf against a pixel's pyramid (k_pvb_beam, tirt_pvb.hip; on the host: tirt_kat_beam_triangle_host, tirt_kat.hip): true = `off`, no ray of the pixel
// can hit the triangle and its leaf stays off the list.  All in grid units seen from the eye: g0, g1, g2 the corners (world - eye) / cell, dg[q] the pyramid's four
// corner directions / cell -- the pixel's own moved outward by a twentieth of a pixel --, nrm[q] = cross(dg[q], dg[q + 1]) turned inward, eps[q] the rounding bound
// of a face's plane expression.  Both tests look for a plane THROUGH THE EYE with the triangle strictly on one side and the pyramid on the other: a ray of the pixel
// is a non-negative combination of the dg, so it stays on the pyramid's side and meets no point of the triangle.
//   The four faces (round 5): all three corners outside one face, by eps[q] and a twentieth of a cell.
//   The triangle's three edge planes (`edges`): the plane of edge (a, b) and the eye has the normal m = cross(ga, gb) = cross(ga, gb - ga); with s = [g0, g1, g2] the
//   triple product of the corners, sign(s) m points to the side of the third corner for all three edges taken in the order (0, 1), (1, 2), (2, 0).  The triangle is
//   off if for one edge sign(s) dot(m, dg[q]) < -tol for all four q.  A point of the triangle seen from the eye has sign(s) dot(m, x) >= 0 for every edge (it is a
//   non-negative combination of the corners, two of which lie in the plane, the third on the inside), the pyramid's rays have it < 0: disjoint.
//   m is formed as cross(ga, gb - ga), not as cross(ga, gb): a triangle 15 pixels wide has corners that agree to 2 %, cross(ga, gb) cancels to a fiftieth of its
//   terms and its rounding, as an angle, would be a tenth of a pixel; gb - ga is exact or rounded once (relative 2^-24) and nothing cancels after it.
//   tol, the fp32 rounding of t = dot(cross(a, e), d) as the code forms it (no contraction: -ffp-contract=off), u = 2^-24:
//     m_i = fl(fl(a_j e_k) - fl(a_k e_j))             |m_i - exact| <= (2u + u^2) M_i,   M_i = |a_j e_k| + |a_k e_j|
//     t   = fl(fl(fl(m_x d_x) + fl(m_y d_y)) + fl(m_z d_z))   adds <= (3u + 3u^2) sum_i |m_i| |d_i| <= 3.01u sum_i M_i |d_i|
//     e_k = fl(b_k - a_k) is within u |e_k| of the exact difference: another u sum_i M_i |d_i|
//   together |t - exact| <= 6.1u T with T = sum_i M_i |d_i| <= (M_x + M_y + M_z) D, D the largest |component| of the four dg.  The code takes tol = 2^-20 (M_x + M_y +
//   M_z) D = 16u (..): the sums M, D are of non-negative terms, their own rounding is a few u of themselves, so tol > 2.6 x the bound.  As an angle that is ~1e-6 / sin
//   of the angle between the edge and the line of sight: a hundredth of a pixel at 850 pixels focal length, against the pyramid's twentieth.  PVB_EDGE_TINY covers
//   products that underflow (their error is absolute, below 1e-37).  The same bound with g_c - g_a in the place of d holds for s = dot(cross(g0, g1 - g0), g2 - g0).
//   What separates nothing stays listed: |s| <= its tolerance (a degenerate or edge-on triangle, or the eye in its plane: the sign of s is not known); an edge whose
//   plane passes within tol of a corner direction (among them an edge whose line passes through the eye: m = 0, tol >= 0, `<` is strict); NaN or infinity anywhere
//   (every comparison is false).
//   The rounding of g and dg themselves (a corner moved by 2u of its distance, 1e-7 rad; the primitive test's own slack is 1e-6 of the distance) is what the
//   pyramid's twentieth of a pixel (6e-5 rad at 850 pixels) is for, as it is for the faces.
constexpr float PVB_EDGE_TOL = 9.5367431640625e-7f;           // 2^-20
constexpr float PVB_EDGE_TINY = 1.0e-30f;
PVB_HD float pvb_abs(const float x) { return x < 0.0f ? -x : x; }
PVB_HD float pvb_max(const float a, const float b) { return a > b ? a : b; }
PVB_HD float pvb_l1(const v3 a) { return pvb_abs(a.x) + pvb_abs(a.y) + pvb_abs(a.z); }
PVB_HD bool pvb_beam_triangle_off(const v3 *nrm, const float *eps, const v3 *dg, const v3 g0, const v3 g1, const v3 g2, const bool edges)
{
    bool off = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float e = eps[q] + 0.05f * (pvb_abs(nrm[q].x) + pvb_abs(nrm[q].y) + pvb_abs(nrm[q].z));      // (+ a twentieth of a cell)
        off = off || (dot(nrm[q], g0) < -e && dot(nrm[q], g1) < -e && dot(nrm[q], g2) < -e);
    }
    if (off || !edges) return off;
    float D = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; q++) D = pvb_max(D, pvb_max(pvb_max(pvb_abs(dg[q].x), pvb_abs(dg[q].y)), pvb_abs(dg[q].z)));
    const v3 ga[3] = {g0, g1, g2}, ed[3] = {g1 - g0, g2 - g1, g0 - g2};
    // s = [g0, g1, g2] as dot(cross(g0, g1 - g0), g2 - g0)
    const v3 m0 = cross(ga[0], ed[0]);
    const v3 M0 = V(pvb_abs(ga[0].y * ed[0].z) + pvb_abs(ga[0].z * ed[0].y), pvb_abs(ga[0].z * ed[0].x) + pvb_abs(ga[0].x * ed[0].z), pvb_abs(ga[0].x * ed[0].y) + pvb_abs(ga[0].y * ed[0].x));
    const float s = -dot(m0, ed[2]);
    const float stol = PVB_EDGE_TOL * ((M0.x * pvb_abs(ed[2].x) + M0.y * pvb_abs(ed[2].y)) + M0.z * pvb_abs(ed[2].z)) + PVB_EDGE_TINY;
    if (!(pvb_abs(s) > stol)) return false;
    const float sg = s > 0.0f ? 1.0f : -1.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const v3 m = a == 0 ? m0 : cross(ga[a], ed[a]);
        const float Ms = a == 0 ? (M0.x + M0.y) + M0.z
                                : ((pvb_abs(ga[a].y * ed[a].z) + pvb_abs(ga[a].z * ed[a].y)) + (pvb_abs(ga[a].z * ed[a].x) + pvb_abs(ga[a].x * ed[a].z))) + (pvb_abs(ga[a].x * ed[a].y) + pvb_abs(ga[a].y * ed[a].x));
        const float tol = PVB_EDGE_TOL * (Ms * D) + PVB_EDGE_TINY;
        bool out = true;
#pragma unroll
        for (int q = 0; q < 4; q++) out = out && (sg * dot(m, dg[q]) < -tol);
        off = off || out;
    }
    return off;
}

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
