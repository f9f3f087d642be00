// tirt_winding.h -- the terms of the generalized winding number, as include/tirt.h defines them ("Winding number"): the signed solid angle of ONE triangle
// (Van Oosterom & Strackee 1983) and of an analytic sphere seen from a query point, the two far-field terms of a cluster of triangles from its moments
// (Barill et al. 2018, orders 0 and 1), the quantisation every term goes through before it is summed, and the result of a sum.  One text for the walk
// (k_wn_walk), the scan (k_wn_scan), the known-answer entry on the device (k_kat_winding) and the one on the host (tirt_kat_winding_host), tirt_winding.hip:
// every function of the first part is __host__ __device__, and what the four return can only differ in WHICH terms they add.  fp32 throughout, every
// operation and its order as written (the library is compiled with -ffp-contract=off); tests/winding_expected.py restates it in numpy.
// The second part is what the moment table is made of (k_wn_level, k_wn_convert): a triangle's sixteen integer moments and the fp32 row of a sum of them.
#pragma once
#include "tirt_device.h"
#include "tirt_closest_point.h"

namespace tirt {

#define WN_HD __host__ TD

constexpr float WN_FOUR_PI = 12.566370614359172f;           // fp32: 0x41490fdb
constexpr float WN_INV_FOUR_PI = 0.07957747154594767f;      // fp32: 0x3da2f983
constexpr float WN_UNIT = 9.313225746154785e-10f;           // 2^-30
constexpr float WN_QUANT_LIMIT = 4611686018427387904.0f;    // 2^62

// I(x) = (int64) rintf(x * 2^30), sd_quant's; a term that is NaN, or whose product reaches 2^62 in magnitude, counts as 0 (an exact term is at most 2 pi:
// only the far-field terms of a degenerate cluster, and operands that overflow fp32, get here)
WN_HD long long wn_quant(const float x) { return absf(x * 1073741824.0f) < WN_QUANT_LIMIT ? sd_quant(x) : 0ll; }

// valid as sd_triangle_normal has it: g = cross(b - a, c - a), 0 < dot(g, g) < +inf
WN_HD bool wn_valid(const v3 a, const v3 b, const v3 c, v3 &g, float &l2)
{
    g = cross(b - a, c - a);
    l2 = dot(g, g);
    return l2 > 0.0f && l2 < __builtin_inff();
}

// Omega of the triangle (A, B, C) from q; an invalid triangle: 0.  q on the triangle's plane: num is (nearly) 0 and den < 0 inside the triangle, > 0 outside:
// +-2 pi or 0, whatever these operations give
WN_HD float wn_triangle(const v3 q, const v3 A, const v3 B, const v3 C)
{
    v3 g; float l2;
    if (!wn_valid(A, B, C, g, l2)) return 0.0f;
    const v3 a = A - q, b = B - q, c = C - q;
    const float la = tm_sqrt(dot(a, a)), lb = tm_sqrt(dot(b, b)), lc = tm_sqrt(dot(c, c));
    const float num = dot(a, cross(b, c));
    const float den = (((la * lb) * lc + dot(a, b) * lc) + dot(a, c) * lb) + dot(b, c) * la;
    return 2.0f * tm_atan2(num, den);
}

// an analytic sphere: 4 pi inside (len < rad, len as sd_sign_sphere forms it), else 0
WN_HD float wn_sphere(const v3 q, const v3 centre, const float rad)
{
    const v3 pc = q - centre;
    const float len = tm_sqrt(dot(pc, pc));
    return len < rad ? WN_FOUR_PI : 0.0f;
}

// the two far-field terms of a cluster with summed area vector n and first-order tensor C (row-major, C[3 i + j]: i the centroid's axis, j the area
// vector's), d = p~ - q, d2 = dot(d, d) > 0:   t0 = n . d / |d|^3,   t1 = sum_ij C_ij (delta_ij / |d|^3 - 3 d_i d_j / |d|^5)
WN_HD void wn_far_terms(const v3 d, const float d2, const v3 n, const float *C, float &t0, float &t1)
{
    const float s = tm_sqrt(d2), d3 = d2 * s;
    t0 = dot(n, d) / d3;
    const float tr = (C[0] + C[4]) + C[8];
    const v3 cd = V(dot(V(C[0], C[1], C[2]), d), dot(V(C[3], C[4], C[5]), d), dot(V(C[6], C[7], C[8]), d));
    t1 = tr / d3 - (3.0f * dot(d, cd)) / (d2 * d3);
}

// the winding number of a sum of quantised terms
WN_HD float wn_result(const long long S) { return ((float)S * WN_UNIT) * WN_INV_FOUR_PI; }

// one known-answer row: (q3, a3, b3, c3) or (q3, centre3, r) -> four 32-bit words: the bits of Omega, the bits of wn_result(I(Omega)), I(Omega) low and high
constexpr int WN_KAT_TRI = 12, WN_KAT_SPH = 7, WN_KAT_OUT = 4;
WN_HD void wn_kat_row(const float *in, const int is_sphere, uint32_t *out)
{
    const v3 q = V(in[0], in[1], in[2]);
    const float om = is_sphere ? wn_sphere(q, V(in[3], in[4], in[5]), in[6])
                               : wn_triangle(q, V(in[3], in[4], in[5]), V(in[6], in[7], in[8]), V(in[9], in[10], in[11]));
    const long long I = wn_quant(om);
    out[0] = tm_f2u(om); out[1] = tm_f2u(wn_result(I));
    out[2] = (uint32_t)((unsigned long long)I & 0xffffffffull); out[3] = (uint32_t)((unsigned long long)I >> 32);
}

// ---- the moment table (include/tirt.h, "Winding number", the moment table) ----
// The scales of the integer moments: with the padded root extent ext = m 2^e, 0.5 <= m < 1 (WnScale::of), s2 = 2^(37 - 2 e) for areas and s3 = 2^(37 - 3 e)
// for area x length.  A position relative to grid_min is at most ext / 2 < 2^(e - 1) in magnitude, an edge at most sqrt(3) ext, so |g| / 2 < 1.5 * 2^(2 e):
// a scaled term stays below 1.5 * 2^37 (areas) and 0.75 * 2^37 (area x length), and 2^24 of them below 2^62.
struct WnScale {
    double s2, s3, inv_s2, inv_s3; int e;
    static WnScale of(const float ext)
    {
        WnScale w;
        w.e = (int)((tm_f2u(ext) >> 23) & 0xffu) - 126;
        w.s2 = tm_pow2i(37 - 2 * w.e); w.s3 = tm_pow2i(37 - 3 * w.e); w.inv_s2 = tm_pow2i(2 * w.e - 37); w.inv_s3 = tm_pow2i(3 * w.e - 37);
        return w;
    }
};
constexpr int WN_MOMENTS = 16;               // int64 per sum: area vector 3, area 1, area x centroid 3, centroid (x) area vector 9 (row-major, centroid first)
constexpr int WN_ROW_QUADS = 4;              // float4 per table row: (p~, r2) (N, C00) (C01, C02, C10, C11) (C12, C20, C21, C22)

TD long long wn_moment_quant(const float x, const double s)
{
    const double y = (double)x * s;
    return (y < 0.0 ? -y : y) < 4611686018427387904.0 ? (long long)__builtin_rint(y) : 0ll;
}
// adds the sixteen moments of the triangle (A, B, C) to m; an invalid triangle adds nothing
TD void wn_moment_add(long long *m, const v3 A, const v3 B, const v3 C, const v3 gm, const WnScale &w)
{
    v3 g; float l2;
    if (!wn_valid(A, B, C, g, l2)) return;
    const v3 h = V(0.5f * g.x, 0.5f * g.y, 0.5f * g.z);
    const float ar = 0.5f * tm_sqrt(l2);
    const v3 cen = (((A - gm) + (B - gm)) + (C - gm)) * 0.3333333432674408f;
    m[0] += wn_moment_quant(h.x, w.s2); m[1] += wn_moment_quant(h.y, w.s2); m[2] += wn_moment_quant(h.z, w.s2);
    m[3] += wn_moment_quant(ar, w.s2);
    m[4] += wn_moment_quant(ar * cen.x, w.s3); m[5] += wn_moment_quant(ar * cen.y, w.s3); m[6] += wn_moment_quant(ar * cen.z, w.s3);
    m[7] += wn_moment_quant(cen.x * h.x, w.s3); m[8] += wn_moment_quant(cen.x * h.y, w.s3); m[9] += wn_moment_quant(cen.x * h.z, w.s3);
    m[10] += wn_moment_quant(cen.y * h.x, w.s3); m[11] += wn_moment_quant(cen.y * h.y, w.s3); m[12] += wn_moment_quant(cen.y * h.z, w.s3);
    m[13] += wn_moment_quant(cen.z * h.x, w.s3); m[14] += wn_moment_quant(cen.z * h.y, w.s3); m[15] += wn_moment_quant(cen.z * h.z, w.s3);
}
// the fp32 row of the sums m for a slot whose decoded box is [mn, mx]: float64 with + - * / only, rounded once per word; r2 in fp32
TD void wn_moment_row(const long long *m, const v3 gm, const v3 mn, const v3 mx, const WnScale &w, float *row)
{
    const bool has = m[3] > 0;
    const double area = (double)m[3] * w.inv_s2;
    const double n0 = (double)m[0] * w.inv_s2, n1 = (double)m[1] * w.inv_s2, n2 = (double)m[2] * w.inv_s2;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (has) { p0 = ((double)m[4] * w.inv_s3) / area; p1 = ((double)m[5] * w.inv_s3) / area; p2 = ((double)m[6] * w.inv_s3) / area; }
    const float px = has ? (float)(p0 + (double)gm.x) : 0.5f * (mn.x + mx.x);
    const float py = has ? (float)(p1 + (double)gm.y) : 0.5f * (mn.y + mx.y);
    const float pz = has ? (float)(p2 + (double)gm.z) : 0.5f * (mn.z + mx.z);
    const float ax = absf(px - mn.x), bx = absf(mx.x - px), ay = absf(py - mn.y), by = absf(mx.y - py), az = absf(pz - mn.z), bz = absf(mx.z - pz);
    const float fx = ax > bx ? ax : bx, fy = ay > by ? ay : by, fz = az > bz ? az : bz;
    row[0] = px; row[1] = py; row[2] = pz; row[3] = (fx * fx + fy * fy) + fz * fz;
    row[4] = (float)n0; row[5] = (float)n1; row[6] = (float)n2;
    row[7] = (float)((double)m[7] * w.inv_s3 - p0 * n0); row[8] = (float)((double)m[8] * w.inv_s3 - p0 * n1); row[9] = (float)((double)m[9] * w.inv_s3 - p0 * n2);
    row[10] = (float)((double)m[10] * w.inv_s3 - p1 * n0); row[11] = (float)((double)m[11] * w.inv_s3 - p1 * n1); row[12] = (float)((double)m[12] * w.inv_s3 - p1 * n2);
    row[13] = (float)((double)m[13] * w.inv_s3 - p2 * n0); row[14] = (float)((double)m[14] * w.inv_s3 - p2 * n1); row[15] = (float)((double)m[15] * w.inv_s3 - p2 * n2);
}

}  // namespace tirt
