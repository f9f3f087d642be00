// tirt_triangle_query.h -- the closest points of ONE query triangle T and ONE scene triangle, as include/tirt.h defines them ("Triangle distance"):
// the 21 candidates of a pair in code order (vertex of T against the scene triangle, scene vertex against T, edge against edge, edge of T piercing the
// scene triangle, scene edge piercing T) and the rule by which one of them is the pair's answer.  One text for the scan (k_tq_scan), the walk (k_tq_walk)
// and the known-answer entries (tirt_kat_tri_tri on the device, tirt_kat_tri_tri_host on the host: every function here is __host__ __device__), so what
// they return can only differ in WHICH scene triangles they look at.  fp32 throughout, every operation and its order as written (the library is compiled
// with -ffp-contract=off); tests/triangle_query_expected.py restates the header's text in numpy.
//
// WHY THE WALK'S CULL IS CONSERVATIVE (k_tq_walk, tirt_triangle_query.hip).  The argument in the head of tirt_point_walk.h, with the query POINT p replaced
// by the query BOX [lo, hi] of T, lo_k = min(p0_k, p1_k, p2_k), hi_k = max(...), both exact (a minimum and a maximum round nothing).  The walk skips a
// subtree on lb2 > cut only, never on equality, so it suffices that lb2 <= D2 holds as computed fp32 numbers for every triangle t below the node, D2 the
// d2 of the pair's answer.  eps, E, C, M, m as there; M now the largest coordinate magnitude among T and the scene.
//  (1) The computed D2 = dot(P - Q, P - Q) of whichever candidate wins.  It suffices that P lies within k eps M of T's exact box and Q within k eps M of
//      the leaf's exact box, per coordinate, with the k of tirt_point_walk.h: then |P - Q| >= d_box - 2 sqrt(3) k eps M with d_box the exact distance
//      between the two exact boxes, which is where the point argument starts with p in the place of P.
//      codes 0..2: P = p_j is a vertex of T (in its box, exactly), Q = cp_triangle's Q: (1) of tirt_point_walk.h as it stands.
//      codes 3..5: the same with the roles exchanged: Q = s_j is a scene vertex, P = cp_triangle's Q on T.
//      codes 6..14: P = p1 + d1 * s, Q = p2 + d2v * t.  clamp() returns 0, 1 or its argument where that is in [0, 1], and t = (B s + F) / E is used
//      unclamped only where 0 <= t <= 1 held as computed -- so s, t are in [0, 1] or NaN (a NaN d2 is never a candidate).  The exact p1 + d1 s lies on
//      the segment, hence in the box of its triangle; the evaluated one differs by the roundings of q1 - p1, the product and the sum: <= 2 eps M per
//      coordinate, as for cp_triangle's edge regions.  WHICH s, t the formulas pick does not matter here: any pair of points of the two segments is at
//      least d_box apart.
//      codes 15..20: P = Q = X = (a + E1 u) + E2 v with u >= 0, v >= 0, u + v <= 1 as computed.  u + v <= 1 in fp32 puts the exact u + v below 1 + eps, so
//      the exact a + E1 u + E2 v lies within eps |E2| of the triangle it is formed on and the evaluated one within 4 eps M of that: within 5 eps M of
//      that triangle's box.  It is formed on ONE of the two triangles; d2 = 0 claims that the other one is there too, and the parameters alone cannot
//      vouch for that: with the segment in the triangle's plane (a wall's edge against a coplanar query, the everyday case) det is rounding noise,
//      1 / det amplifies without bound and u, v, t land in range by accident for triangles a scene apart.  So tq_seg_tri CONFIRMS a hit: the
//      segment's own point x0 + d t (t in [0, 1]: within 2 eps M of the segment's triangle's box) has to lie within g = 2^-19 max |vertex| <=
//      32 sqrt(3) eps M < 56 eps M of X.  An accepted piercing therefore has a point near each exact box that are g apart: d_box <= g + 7 sqrt(3) eps M
//      < 69 eps M, whatever det was.  With the roundings of (2) that is below the 140 eps M of the margin: every axis' gap is 0, lb2 = 0 <= D2.
//      No needle caveat is needed for these codes; the one of tirt_point_walk.h stays for cp_triangle's interior (codes 0..5).
//  (2) The computed lb2.  The per-axis gap is max(max(mn - hi_k, lo_k - mx) - m, 0): the two differences are off by eps M each at most, as mn - p and
//      p - mx were, and the decoded planes, squares and sums as there.
//  (3) The slack.  With x the exact per-axis distances between the two exact boxes (|x| = d_box) and e_a <= max(x_a - m, 0), |e| <= d_box - m as there:
//      the step never used that the query is a point.  rho_p is taken over all three vertices of T (the largest of the three margins: the expression
//      is monotone in rho_p), so M <= (rho_0 + max(rho_p, 1/2)) E bounds T's coordinates too, and d_box <= sqrt(3) (rho_p + 1/2) E.
//  Together: lb2 <= D2 under the same condition on m, with 2 k in the place of k: the 100 eps M that mc leaves cover k <= 50 per side.
// THE COST OF EQUALITY.  Several scene triangles may tie at D2 = 0 and the smallest id must win, so a subtree with lb2 == 0 is still visited when the
// answer is already 0: a query triangle deep inside a dense part of the scene tests every leaf whose grown box meets its box.  That is the price of
// the scan's bits; there is no early exit for "any contact".
#pragma once
#include "tirt_closest_point.h"

namespace tirt {

#define TQ_HD __host__ __device__ __forceinline__

struct TqSegSeg { float s, t, d2; v3 P, Q; };
struct TqSegTri { bool hit; float u, v, t; v3 X; };
struct TqPair { float d2; v3 P, Q; int code; };

TQ_HD float tq_clamp(const float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }      // a NaN passes through
TQ_HD v3 tq_pick(const int j, const v3 a, const v3 b, const v3 c) { return j == 0 ? a : (j == 1 ? b : c); }

// segment p1 -> q1 against segment p2 -> q2 (Ericson 5.1.9 with exact zero tests)
TQ_HD TqSegSeg tq_seg_seg(const v3 p1, const v3 q1, const v3 p2, const v3 q2)
{
    const v3 d1 = q1 - p1, d2v = q2 - p2, r = p1 - p2;
    const float A = dot(d1, d1), E = dot(d2v, d2v), F = dot(d2v, r);
    float s, t;
    if ((A <= 0.0f) & (E <= 0.0f)) { s = 0.0f; t = 0.0f; }
    else if (A <= 0.0f) { s = 0.0f; t = tq_clamp(F / E); }
    else {
        const float C = dot(d1, r);
        if (E <= 0.0f) { t = 0.0f; s = tq_clamp(-C / A); }
        else {
            const float B = dot(d1, d2v), den = A * E - B * B;
            s = den > 0.0f ? tq_clamp((B * F - C * E) / den) : 0.0f;
            t = (B * s + F) / E;
            if (t < 0.0f) { t = 0.0f; s = tq_clamp(-C / A); }
            else if (t > 1.0f) { t = 1.0f; s = tq_clamp((B - C) / A); }
        }
    }
    TqSegSeg o;
    o.s = s; o.t = t;
    o.P = p1 + d1 * s; o.Q = p2 + d2v * t;
    const v3 pq = o.P - o.Q;
    o.d2 = dot(pq, pq);
    return o;
}

// segment x0 -> x1 against the triangle a, b, c (Moeller-Trumbore): no hit, and u = v = t = 0, unless det < 0 or det > 0.  The parameters in range do
// not make a hit by themselves: where the segment runs in (or nearly in) the triangle's plane det is rounding noise and u, v, t are noise over noise, in
// range by accident for triangles that are far apart.  A hit is CONFIRMED by its two points: the segment's x0 + d t and the triangle's X have to agree
// within TQ_PIERCE_TOL2 of the largest squared vertex norm (2^-19 of the largest norm: 32 sqrt(3) eps M at most)
constexpr float TQ_PIERCE_TOL2 = 0x1p-38f;
TQ_HD float tq_max(const float x, const float y) { return x > y ? x : y; }
TQ_HD TqSegTri tq_seg_tri(const v3 x0, const v3 x1, const v3 a, const v3 b, const v3 c)
{
    const v3 d = x1 - x0, E1 = b - a, E2 = c - a, h = cross(d, E2);
    const float det = dot(E1, h);
    TqSegTri o;
    o.hit = false; o.u = 0.0f; o.v = 0.0f; o.t = 0.0f; o.X = V(0.0f, 0.0f, 0.0f);
    if ((det < 0.0f) | (det > 0.0f)) {
        const float inv = 1.0f / det;
        const v3 s = x0 - a;
        o.u = dot(s, h) * inv;
        const v3 q = cross(s, E1);
        o.v = dot(d, q) * inv;
        o.t = dot(E2, q) * inv;
        o.X = (a + E1 * o.u) + E2 * o.v;
        const v3 w = (x0 + d * o.t) - o.X;
        const float m2 = tq_max(tq_max(tq_max(tq_max(dot(x0, x0), dot(x1, x1)), dot(a, a)), dot(b, b)), dot(c, c));
        o.hit = (o.u >= 0.0f) & (o.v >= 0.0f) & (o.u + o.v <= 1.0f) & (o.t >= 0.0f) & (o.t <= 1.0f) & (dot(w, w) <= m2 * TQ_PIERCE_TOL2);
    }
    return o;
}

// The pair's answer: it starts as (d2 = +inf, code = -1, P = Q = 0) and a candidate replaces it iff its d2 is BELOW the answer's (so the first in code
// order wins at equal bits, and neither a NaN nor +inf ever stands).  Once a d2 of +0 stands nothing can replace it: the later groups are skipped.
TQ_HD TqPair tq_pair(const v3 p0, const v3 p1, const v3 p2, const v3 a, const v3 b, const v3 c)
{
    TqPair o;
    o.d2 = __builtin_inff(); o.P = V(0.0f, 0.0f, 0.0f); o.Q = o.P; o.code = -1;
#pragma unroll 1
    for (int j = 0; j < 3; j++) {                            // 0..2: a vertex of T against the scene triangle
        const v3 p = tq_pick(j, p0, p1, p2);
        const CpPoint r = cp_triangle(p, a, b, c);
        if (r.d2 < o.d2) { o.d2 = r.d2; o.P = p; o.Q = r.q; o.code = j; }
    }
    if (o.d2 == 0.0f) return o;
#pragma unroll 1
    for (int j = 0; j < 3; j++) {                            // 3..5: a scene vertex against T
        const v3 s = tq_pick(j, a, b, c);
        const CpPoint r = cp_triangle(s, p0, p1, p2);
        if (r.d2 < o.d2) { o.d2 = r.d2; o.P = r.q; o.Q = s; o.code = 3 + j; }
    }
    if (o.d2 == 0.0f) return o;
#pragma unroll 1
    for (int ef = 0; ef < 9; ef++) {                         // 6 + 3e + f: edge e of T against edge f of the scene triangle
        const int e = ef / 3, f = ef - 3 * e;
        const TqSegSeg r = tq_seg_seg(tq_pick(e, p0, p1, p2), tq_pick(e, p1, p2, p0), tq_pick(f, a, b, c), tq_pick(f, b, c, a));
        if (r.d2 < o.d2) { o.d2 = r.d2; o.P = r.P; o.Q = r.Q; o.code = 6 + ef; }
    }
    if (o.d2 == 0.0f) return o;
#pragma unroll 1
    for (int e = 0; e < 3; e++) {                            // 15..17: edge e of T pierces the scene triangle
        const TqSegTri r = tq_seg_tri(tq_pick(e, p0, p1, p2), tq_pick(e, p1, p2, p0), a, b, c);
        if (r.hit & (0.0f < o.d2)) { o.d2 = 0.0f; o.P = r.X; o.Q = r.X; o.code = 15 + e; }
    }
    if (o.d2 == 0.0f) return o;
#pragma unroll 1
    for (int f = 0; f < 3; f++) {                            // 18..20: edge f of the scene triangle pierces T
        const TqSegTri r = tq_seg_tri(tq_pick(f, a, b, c), tq_pick(f, b, c, a), p0, p1, p2);
        if (r.hit & (0.0f < o.d2)) { o.d2 = 0.0f; o.P = r.X; o.Q = r.X; o.code = 18 + f; }
    }
    return o;
}

// one known-answer row (include/tirt.h, tirt_kat_tri_tri): what = 0: 18 floats (T, a, b, c) -> d2, P3, Q3, code; 1: 12 floats (p1, q1, p2, q2) -> s, t, d2;
// 2: 15 floats (x0, x1, a, b, c) -> hit, u, v, t
constexpr int TQ_KAT_IN[3] = {18, 12, 15}, TQ_KAT_OUT[3] = {8, 3, 4};
TQ_HD v3 tq_v3(const float *r) { return V(r[0], r[1], r[2]); }
TQ_HD void tq_kat_row(const float *r, const int what, float *o)
{
    if (what == 0) {
        const TqPair a = tq_pair(tq_v3(r), tq_v3(r + 3), tq_v3(r + 6), tq_v3(r + 9), tq_v3(r + 12), tq_v3(r + 15));
        o[0] = a.d2; o[1] = a.P.x; o[2] = a.P.y; o[3] = a.P.z; o[4] = a.Q.x; o[5] = a.Q.y; o[6] = a.Q.z; o[7] = (float)a.code;
    } else if (what == 1) {
        const TqSegSeg a = tq_seg_seg(tq_v3(r), tq_v3(r + 3), tq_v3(r + 6), tq_v3(r + 9));
        o[0] = a.s; o[1] = a.t; o[2] = a.d2;
    } else {
        const TqSegTri a = tq_seg_tri(tq_v3(r), tq_v3(r + 3), tq_v3(r + 6), tq_v3(r + 9), tq_v3(r + 12));
        o[0] = a.hit ? 1.0f : 0.0f; o[1] = a.u; o[2] = a.v; o[3] = a.t;
    }
}

}  // namespace tirt
