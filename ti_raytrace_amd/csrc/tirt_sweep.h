// tirt_sweep.h -- the first contact of ONE primitive with a sphere of radius r whose centre moves along c(t) = o + t d, as include/tirt.h defines it
// ("Sphere sweep"): the contact time T, the feature code and Q, u, v of a triangle (sw_triangle) and of an analytic sphere (sw_sphere), and the rule by
// which a contact replaces the answer (sw_accept).  One text for the scan (k_sw_scan), the walk (k_sw_walk), the known-answer entry on the device
// (k_kat_sweep) and the one on the host (tirt_kat_sweep_host), tirt_sweep.hip: every function here is __host__ __device__, and what the four return can only
// differ in WHICH primitives they look at.  fp32 throughout, every operation and its order as written (the library is compiled with
// -ffp-contract=off); tests/sweep_expected.py restates it in numpy.
//
// A triangle's candidates are the boundary pieces of its Minkowski sum with the ball: the two offset faces, the three cylinders about its edges, the
// three spheres about its corners.  Each piece lies inside the sum and the first contact lies on one of them, so in exact arithmetic the smallest
// candidate whose parameters are in range IS the first contact.  In fp32 a candidate may be cancellation noise (a nearly parallel edge, a far origin):
// none counts before cp_triangle itself has put c(t) within r + tol of the triangle -- k_trace's rule, "every accepted hit is re-checked".  The
// candidates are formed first and verified smallest first, so the usual case costs one verification, and the verifying call's Q, u, v are the attributes.
// (The one-shot alternative of Ericson 5.5.6 -- the closest point to the plane contact, then a ray cast back -- is not exact in general and is not used.)
//
// Square roots and divisions sit behind SW_ANY: a wave ballot on the device (a real branch, as cp_record's sphere branch), the predicate itself on the host.
#pragma once
#include "tirt_device.h"
#include "tirt_closest_point.h"

namespace tirt {

#define SW_HD __host__ __device__ __forceinline__
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define SW_ANY(p_) (__builtin_amdgcn_ballot_w64(p_) != 0ull)
#else
#define SW_ANY(p_) (p_)
#endif

constexpr float SW_TOL_REL = 1.0f / 65536.0f;      // the relative part of tol: 2^-16 of r
// T == 0 is kept for "overlap at the start by cp_triangle's / cp_sphere's own arithmetic" (code 0: exactly where PointQuery.count_within(o, r) > 0).  A
// start that the distance function puts an ulp OUTSIDE r can still have a candidate whose root rounds to 0 (a sphere resting on a floor and pushed into
// it): the contact lies ahead by less than any step, and it is given the smallest positive normal number -- never dropped, never 0.
constexpr float SW_T_MIN = 1.17549435e-38f;        // 2^-126
constexpr int SW_KAT_TRI = 18, SW_KAT_SPH = 13, SW_KAT_OUT = 8;      // floats per row of tirt_kat_sweep[_host]

// what a query hands to every primitive: formed once, the way lim2 is
struct SwQuery { v3 o, d; float r, r2, rhi2, nn; };      // r2 = r * r, rhi2 = (r + tol)^2, nn = dot(d, d)
struct SwHit { float t; int code; CpPoint cp; };         // cp: the verifying call's (code 0: the call at o); t = +inf, code = -1: no contact

SW_HD float sw_inf() { return __builtin_inff(); }
// m: the length of the query (the walk's margin, sw_margin in tirt_sweep.hip; a known-answer row carries its own)
SW_HD SwQuery sw_query(const v3 o, const v3 d, const float r, const float m)
{
    SwQuery q;
    q.o = o; q.d = d; q.r = r;
    q.r2 = r * r;
    const float tol = r * SW_TOL_REL + m, rh = r + tol;
    q.rhi2 = rh * rh;
    q.nn = dot(d, d);
    return q;
}
// a query that fails this gets the miss without a look at any primitive
SW_HD bool sw_valid(const v3 o, const v3 d, const float r, const float B)
{
    const float inf = sw_inf();
    return absf(o.x) < inf && absf(o.y) < inf && absf(o.z) < inf && absf(d.x) < inf && absf(d.y) < inf && absf(d.z) < inf && r >= 0.0f && r < inf && B >= 0.0f;
}
SW_HD v3 sw_at(const SwQuery &q, const float t) { return q.o + q.d * t; }
SW_HD float sw_ahead(const float t) { return t == 0.0f ? SW_T_MIN : t; }
SW_HD SwHit sw_miss()
{
    SwHit h;
    h.t = sw_inf(); h.code = -1;
    h.cp.d2 = sw_inf(); h.cp.q = V(0.0f, 0.0f, 0.0f); h.cp.u = 0.0f; h.cp.v = 0.0f;
    return h;
}

// a root of a t^2 + 2 b t + c = 0: (-b + sg sqrt(b b - a c)) / a with sg = -1 (the smaller) or +1; +inf where `ok` fails, a is not positive or the
// discriminant is negative or NaN
SW_HD float sw_root(const float a, const float b, const float c, const bool ok, const float sg)
{
    float t = sw_inf();
    const float disc = b * b - a * c;
    const bool go = ok & (a > 0.0f) & (disc >= 0.0f);
    if (SW_ANY(go)) { if (go) t = (-b + sg * tm_sqrt(disc)) / a; }
    return t;
}
// the candidate of the edge from P along e (Ericson 5.3.7: the ray against the infinite cylinder about the edge's line), m = o - P, mm = dot(m, m),
// md_ = dot(m, d): the smaller root, with t >= 0 and the axial parameter in [0, dot(e, e)]; a ray parallel to the edge and an edge of length 0 have A = 0: none
SW_HD float sw_edge(const SwQuery &q, const v3 m, const float mm, const float md_, const v3 e)
{
    const float me = dot(m, e), de = dot(q.d, e), ee = dot(e, e);
    const float A = ee * q.nn - de * de, k = mm - q.r2, C = ee * k - me * me, Bq = ee * md_ - de * me;
    const float t = sw_root(A, Bq, C, true, -1.0f);
    const float ax = me + t * de;
    return ((t >= 0.0f) & (ax >= 0.0f) & (ax <= ee)) ? t : sw_inf();
}
// the candidate of the corner: the smaller root against the sphere of radius r about it, with t >= 0
SW_HD float sw_corner(const SwQuery &q, const float mm, const float md_)
{
    const float t = sw_root(q.nn, md_, mm - q.r2, true, -1.0f);
    return t >= 0.0f ? t : sw_inf();
}

// T, code, Q, u, v of the triangle (a, b, c); candidates above tmax_c are not looked at (the caller accepts no T above it: B, or the walk's cut)
SW_HD SwHit sw_triangle(const SwQuery &q, const v3 a, const v3 b, const v3 c, const float tmax_c)
{
    const float inf = sw_inf();
    SwHit h = sw_miss();
    // code 0: overlap at the start
    const CpPoint c0 = cp_triangle(q.o, a, b, c);
    if (c0.d2 <= q.r2) { h.t = 0.0f; h.code = 0; h.cp = c0; return h; }
    const v3 ab = b - a, ac = c - a, bc = c - b, ca = a - c;
    const v3 ma = q.o - a, mb = q.o - b, mc = q.o - c;
    const float maa = dot(ma, ma), mbb = dot(mb, mb), mcc = dot(mc, mc);
    const float mad = dot(ma, q.d), mbd = dot(mb, q.d), mcd = dot(mc, q.d);
    // code 1: the plane offset by r on the side the centre starts from
    float t1 = inf;
    {
        const v3 n = cross(ab, ac);
        const float n2 = dot(n, n), s = dot(n, ma), nd = dot(n, q.d);
        const float sg = s < 0.0f ? -1.0f : 1.0f, hh = s * sg, vv = nd * sg;      // the height above the plane and its rate, both times |n|
        const bool go = (n2 > 0.0f) & (vv < 0.0f);
        if (SW_ANY(go)) {
            if (go) {
                const float rl = q.r * tm_sqrt(n2);
                if (hh >= rl) {
                    const float t = (hh - rl) / (-vv);
                    const v3 p = sw_at(q, t);
                    const float e0 = dot(cross(ab, p - a), n), e1 = dot(cross(bc, p - b), n), e2 = dot(cross(ca, p - c), n);
                    if ((e0 >= 0.0f) & (e1 >= 0.0f) & (e2 >= 0.0f)) t1 = t;
                }
            }
        }
    }
    // codes 2, 3, 4: the edges ab, bc, ca; codes 5, 6, 7: the corners a, b, c
    float t2 = sw_edge(q, ma, maa, mad, ab), t3 = sw_edge(q, mb, mbb, mbd, bc), t4 = sw_edge(q, mc, mcc, mcd, ca);
    float t5 = sw_corner(q, maa, mad), t6 = sw_corner(q, mbb, mbd), t7 = sw_corner(q, mcc, mcd);
#define SW_RANGE(t_) t_ = sw_ahead(t_); t_ = ((t_ >= 0.0f) & (t_ <= tmax_c)) ? t_ : inf
    SW_RANGE(t1); SW_RANGE(t2); SW_RANGE(t3); SW_RANGE(t4); SW_RANGE(t5); SW_RANGE(t6); SW_RANGE(t7);
#undef SW_RANGE
    // the smallest candidate that verifies, at equal bits the first in code order
    bool done = false;
#pragma nounroll
    for (int it = 0; it < 7; it++) {
        float tm = t1; int km = 1;
        if (t2 < tm) { tm = t2; km = 2; }
        if (t3 < tm) { tm = t3; km = 3; }
        if (t4 < tm) { tm = t4; km = 4; }
        if (t5 < tm) { tm = t5; km = 5; }
        if (t6 < tm) { tm = t6; km = 6; }
        if (t7 < tm) { tm = t7; km = 7; }
        const bool go = !done & (tm < inf);
        if (!SW_ANY(go)) break;
        if (go) {
            const CpPoint v = cp_triangle(sw_at(q, tm), a, b, c);
            if (v.d2 <= q.rhi2) { h.t = tm; h.code = km; h.cp = v; done = true; }
            t1 = km == 1 ? inf : t1; t2 = km == 2 ? inf : t2; t3 = km == 3 ? inf : t3; t4 = km == 4 ? inf : t4;
            t5 = km == 5 ? inf : t5; t6 = km == 6 ? inf : t6; t7 = km == 7 ? inf : t7;
        }
    }
    return h;
}

// T, code, Q of the analytic sphere (centre C, radius R): contact is defined on cp_sphere's distance to the SURFACE.  Code 8: the smaller root of radius
// R + r for a centre that starts outside it; code 9: the larger root of radius R - r for a centre that starts inside that; between the two: code 0
SW_HD SwHit sw_sphere(const SwQuery &q, const v3 C, const float R, const float tmax_c)
{
    SwHit h = sw_miss();
    const CpPoint c0 = cp_sphere(q.o, C, R);
    if (c0.d2 <= q.r2) { h.t = 0.0f; h.code = 0; h.cp = c0; return h; }
    const v3 m = q.o - C;
    const float mm = dot(m, m), md_ = dot(m, q.d);
    const float Ro = R + q.r, Ri = R - q.r;
    const float co = mm - Ro * Ro, ci = mm - Ri * Ri;
    const bool outside = co > 0.0f, inside = (Ri > 0.0f) & (ci < 0.0f);
    const float t = sw_ahead(sw_root(q.nn, md_, outside ? co : ci, outside | inside, outside ? -1.0f : 1.0f));
    const bool go = (t >= 0.0f) & (t <= tmax_c) & (t < sw_inf());
    if (SW_ANY(go)) {
        if (go) {
            const CpPoint v = cp_sphere(sw_at(q, t), C, R);
            if (v.d2 <= q.rhi2) { h.t = t; h.code = outside ? 8 : 9; h.cp = v; }
        }
    }
    return h;
}

// Does the contact (t, prim) replace the answer (best_t, best_prim)?  cp_accept's order on (T, prim) with the bound B in lim2's place: the answer starts as
// (+inf, -1), a NaN t fails every comparison and t = +inf is never accepted.  A total order: the result does not depend on the order of the visits.
SW_HD bool sw_accept(const float t, const int prim, const float B, const float best_t, const int best_prim)
{ return (t <= B) & ((t < best_t) | ((t == best_t) & (prim < best_prim))); }

// the unit vector from the contact point to the centre at the contact, (0, 0, 0) where they coincide (and for a miss)
SW_HD v3 sw_normal(const SwQuery &q, const SwHit &h)
{
    v3 n = V(0.0f, 0.0f, 0.0f);
    const bool hit = h.code >= 0;
    const v3 w = sw_at(q, hit ? h.t : 0.0f) - h.cp.q;
    const float l2 = dot(w, w);
    const bool go = hit & (l2 > 0.0f);
    if (SW_ANY(go)) { if (go) { const float inv = 1.0f / tm_sqrt(l2); n = w * inv; } }
    return n;
}

// one known-answer row: (o3, d3, r, m, B, a3, b3, c3) or (o3, d3, r, m, B, C3, R) -> (t, (float) code, Q3, u, v, the verifying call's D2); a miss: (+inf, -1, 0 ...)
SW_HD void sw_kat_row(const float *in, const int is_sphere, float *out)
{
    const v3 o = V(in[0], in[1], in[2]), d = V(in[3], in[4], in[5]);
    const float r = in[6], m = in[7], B = in[8];
    SwHit h = sw_miss();
    if (sw_valid(o, d, r, B)) {
        const SwQuery q = sw_query(o, d, r, m);
        h = is_sphere ? sw_sphere(q, V(in[9], in[10], in[11]), in[12], B)
                      : sw_triangle(q, V(in[9], in[10], in[11]), V(in[12], in[13], in[14]), V(in[15], in[16], in[17]), B);
    }
    const bool hit = h.code >= 0;
    out[0] = h.t; out[1] = (float)h.code;
    out[2] = hit ? h.cp.q.x : 0.0f; out[3] = hit ? h.cp.q.y : 0.0f; out[4] = hit ? h.cp.q.z : 0.0f;
    out[5] = hit ? h.cp.u : 0.0f; out[6] = hit ? h.cp.v : 0.0f; out[7] = hit ? h.cp.d2 : 0.0f;
}

}  // namespace tirt
