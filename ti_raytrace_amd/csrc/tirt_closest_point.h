// tirt_closest_point.h -- the closest point of ONE primitive to a query point, as include/tirt.h defines it ("Closest point"): D2, Q, u, v of a
// triangle (Ericson, Real-Time Collision Detection 5.1.5, regions in the book's order) and of an analytic sphere, and the rule by which a candidate
// replaces the answer.  One text for the scan (k_cp_scan), the walk (k_cp_walk) and the known-answer entry (k_kat_closest_point), tirt_closest_point.hip:
// what the three return can only differ in WHICH primitives they look at.  fp32 throughout, every operation and its order as written (the library is
// compiled with -ffp-contract=off); tests/closest_point_expected.py restates it in numpy.
// Below them: the pieces of the signed distance (include/tirt.h "Signed distance"; tests/signed_distance_expected.py): the feature rule, sd_sign, and the per-triangle
// terms of the pseudo-normal table.  (What a point's WALK over `cnode` is made of -- the margin, the decode of a child's planes, the lane stack and its
// sizing -- is tirt_point_walk.h.)
#pragma once
#include "tirt_device.h"

namespace tirt {

struct CpPoint { float d2; v3 q; float u, v; };

// (u, v) in the hit record's convention: Q = a + u (b - a) + v (c - a).  A vertex region returns the vertex itself, not a + ab * 1.
__host__ TD CpPoint cp_triangle(const v3 p, const v3 a, const v3 b, const v3 c)
{
    const v3 ab = b - a, ac = c - a, ap = p - a;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const v3 bp = p - b;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const v3 cp = p - c;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    CpPoint r;
    if ((d1 <= 0.0f) & (d2 <= 0.0f)) { r.q = a; r.u = 0.0f; r.v = 0.0f; }                                  // A
    else if ((d3 >= 0.0f) & (d4 <= d3)) { r.q = b; r.u = 1.0f; r.v = 0.0f; }                               // B
    else if ((vc <= 0.0f) & (d1 >= 0.0f) & (d3 <= 0.0f)) { r.u = d1 / (d1 - d3); r.v = 0.0f; r.q = a + ab * r.u; }      // AB
    else if ((d6 >= 0.0f) & (d5 <= d6)) { r.q = c; r.u = 0.0f; r.v = 1.0f; }                               // C
    else if ((vb <= 0.0f) & (d2 >= 0.0f) & (d6 <= 0.0f)) { r.v = d2 / (d2 - d6); r.u = 0.0f; r.q = a + ac * r.v; }      // AC
    else if ((va <= 0.0f) & (e43 >= 0.0f) & (e56 >= 0.0f)) { const float w = e43 / (e43 + e56); r.q = b + (c - b) * w; r.u = 1.0f - w; r.v = w; }      // BC
    else { const float den = 1.0f / ((va + vb) + vc); r.u = vb * den; r.v = vc * den; r.q = (a + ab * r.u) + ac * r.v; }      // interior
    const v3 pq = p - r.q;
    r.d2 = dot(pq, pq);
    return r;
}

__host__ TD CpPoint cp_sphere(const v3 p, const v3 c, const float rad)      // (__host__ too: tirt_kat_sweep_host verifies a contact through it)
{
    const v3 pc = p - c;
    const float len = tm_sqrt(dot(pc, pc)), d = absf(len - rad);
    CpPoint r;
    r.d2 = d * d; r.u = 0.0f; r.v = 0.0f;
    r.q = (len == 0.0f) ? c + V(rad, 0.0f, 0.0f) : c + pc * (rad / len);
    return r;
}

// lim2 of a query: dmax * dmax, formed once; a negative or NaN dmax finds nothing (no D2 is <= -1)
TD float cp_limit2(const float dmax) { return dmax >= 0.0f ? dmax * dmax : -1.0f; }

// Does the candidate (d2, prim) replace the answer (best2, best_prim)?  The answer starts as (+inf, -1), "nothing": a NaN d2 fails every comparison, and
// d2 = +inf is neither below +inf nor, at equal bits, of a smaller id than -1 -- so neither is ever accepted.  A total order on (d2, prim): the
// result does not depend on the order in which the candidates come.  (__host__ too: tirt_kat_nearest_list runs the neighbour list, tirt_nearest.h, on the host)
__host__ TD bool cp_accept(const float d2, const int prim, const float lim2, const float best2, const int best_prim)
{ return (d2 <= lim2) & ((d2 < best2) | ((d2 == best2) & (prim < best_prim))); }

// ---- signed distance (include/tirt.h, "Signed distance") ----
// the feature of a closest point from its (u, v), as the row of the primitive's table entry: 0 interior, 1 A, 2 B, 3 C, 4 AB, 5 AC, 6 BC
TD int sd_feature(const float u, const float v)
{
    if (v == 0.0f) return u == 0.0f ? 1 : (u == 1.0f ? 2 : 4);
    if (u == 0.0f) return v == 1.0f ? 3 : 5;
    if (u == 1.0f - v) return 6;
    return 0;
}
// The signed distance of p to the closest point r of a TRIANGLE whose seven pseudo-normals `row(f)` hands out (a gather from the context's table in
// the walk and the scan, the operands themselves in the known-answer entry): one text for the three.  s == 0 and a NaN s are positive.
template <class Row>
TD float sd_sign(const v3 p, const CpPoint &r, Row row, int &feature)
{
    feature = sd_feature(r.u, r.v);
    const v3 pq = p - r.q;
    const float s = dot(pq, row(feature)), d = tm_sqrt(r.d2);
    return s < 0.0f ? -d : d;
}
// the same for an analytic sphere: inside iff len < rad, len as cp_sphere forms it
TD float sd_sign_sphere(const v3 p, const float d2, const v3 c, const float rad)
{
    const v3 pc = p - c;
    const float len = tm_sqrt(dot(pc, pc)), d = tm_sqrt(d2);
    return len < rad ? -d : d;
}
// what the table build forms per triangle: g = cross(b - a, c - a), l2 = dot(g, g); valid iff 0 < l2 < +inf
TD bool sd_triangle_normal(const v3 a, const v3 b, const v3 c, v3 &nh)
{
    const v3 g = cross(b - a, c - a);
    const float l2 = dot(g, g), l = tm_sqrt(l2);
    nh = V(g.x / l, g.y / l, g.z / l);
    return l2 > 0.0f && l2 < __int_as_float(0x7f800000);
}
// the angle between the edges e1, e2 that leave a corner
TD float sd_corner_angle(const v3 e1, const v3 e2)
{
    const v3 x = cross(e1, e2);
    return tm_atan2(tm_sqrt(dot(x, x)), dot(e1, e2));
}
__host__ TD long long sd_quant(const float x) {      // (__host__ too: tirt_kat_winding_host quantises a term through it)
 return (long long)__builtin_rintf(x * 1073741824.0f); }
constexpr int SD_ROWS = 7;                   // float4 per primitive id: interior, A, B, C, AB, AC, BC

}  // namespace tirt
