// tirt_sweep.hip -- the first contact of a moving sphere with the scene (tirt_query_sweep / tirt_sweep / tirt_kat_sweep / tirt_kat_sweep_host,
// include/tirt.h "Sphere sweep").  No reference counterpart: the reference only answers questions that start from a ray without a radius.
//
//   k_sw_scan<COUNT>        one query per lane against all n primitive records in primitive-id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick on the device
//   k_sw_walk<COUNT, ANY>   one query per lane, near to far over the quantised 4-wide nodes `cnode` (BvhView): the hot path.  ANY (only `blocked` is
//                           asked for): the walk stops at the first accepted contact -- whether some primitive has T <= B does not depend on the order
// Both call sw_triangle / sw_sphere / sw_accept (tirt_sweep.h) and nothing else decides an answer, and the answer is the minimum of a total order on
// (T, prim): the walk returns the scan's bits if and only if it never skips a primitive that would have been accepted.
//
// THE WALK has a loop of its own over the pieces of tirt_point_walk.h (the decode of a child's planes as CP_BOX_GAP does it, PointStack<CpEntry>, the
// margin's expressions, the grid sizing): a wave is a block (CP_BLOCK lanes, no barrier anywhere), lane l holds query base + l and the blocks stride over the
// chunk.  A node visit decodes the four children's planes, grows each box by G = (r + tol) + m on every side, takes the parameters tn, tf at which the
// segment c(t), t >= 0, enters and leaves the grown box by slabs, drops empty slots and children with tn > tf or tn > cut -- never on equality --, sorts
// the rest near to far (five compare-exchanges, as point_walk and k_trace), descends into the nearest and pushes the others far to near WITH their tn; a
// popped entry is tested against the cut of that moment again.  THE CUT is min(best T so far, B).  An axis on which d is 0 has no parameters: the child
// is dropped iff o lies outside the grown slab; an axis whose 1 / d overflows constrains nothing.
// The walk starts at root_qcode (a leaf code in a one-primitive scene).  Every analytic sphere is below it with a box that contains it (the head of
// tirt_closest_point.hip says why).  Spot and laser leaves are reached and skipped.
//
// WHY THE CULL IS CONSERVATIVE.  It suffices that tn <= T <= tf holds, as computed fp32 numbers, at every ancestor of the leaf of a primitive i whose
// T = T(i) could still be accepted.  Write eps = 2^-24, M = the largest coordinate magnitude among o, the scene and the scene grown by r.
//  (1) An accepted T(i) has p = fl(o + T d) with the computed D2(p, i) <= rhi2 = (r + tol)^2: sw_triangle / sw_sphere verified exactly that (code 0: p = o,
//      D2 <= r^2).  Argument (1) of tirt_point_walk.h puts p within sqrt(rhi2) (1 + 2 eps) + sqrt(3) (k + 1) eps M of the leaf's exact box (k "a few").
//  (2) Every ancestor's decoded box contains the leaf's exact box (tirt_internal.h: planes rounded outward), up to the eps E / 4 + eps M / 2 of the
//      decode.  So on every axis a, p_a lies in [mn_a - G', mx_a + G'] with G' = (r + tol) + (sqrt(3) (k + 1) + 1) eps M.
//  (3) The slab parameters.  lo = fl(mn_a - G) with G = fl((r + tol) + m): after these two roundings, lo <= mn_a - G' - (m - (sqrt(3) (k + 1) + 3) eps M).
//      For d_a > 0: p_a >= mn_a - G' and p_a = fl(o_a + fl(d_a T)) <= o_a + d_a T + 2 eps M give d_a T >= (lo - o_a) + (m - (sqrt(3) (k + 1) + 5) eps M), while
//      t1 = fl((lo - o_a) * fl(1 / d_a)) exceeds (lo - o_a) / d_a by at most 3 eps |lo - o_a| / d_a <= 6 eps M / d_a.  So t1 <= T whenever
//      m >= (sqrt(3) (k + 1) + 11) eps M.  The same holds for t2 >= T on the far plane, for d_a < 0 with the roles swapped, and so for
//      tn = max(0, near_a) <= T <= tf = min far_a.
//  (4) The margin.  m = cp_margin_cells(rho_q, rho_0) * cell_max with rho_q = rho_o + r / E: PointMargin's expression for the point o with the radius
//      added to its distance.  As there, C = 279 eps E, so m = 140 eps E (rho_o + r / E + rho_0 + 1) >= 140 eps M with M <= (rho_0 + max(rho_o, 1/2) + r / E) E:
//      (3) holds for k <= 73, where the point walks' own margin is sized for k <= 100 against their smaller need and "a few" is what a triangle that is
//      no needle has.  (m is NOT sized from the far end o + B d of the segment: a contact cannot lie outside the root box grown by r + tol, whatever B is.)
//  The same m is the absolute part of tol (tol = r 2^-16 + m): one length per query, formed once.
// DEEP OVERLAP.  With the answer at T = 0 the cut is 0 and every leaf whose grown box holds o (tn == 0) is still tested, because a smaller id may tie:
// a sphere deep inside a dense mesh pays what TriangleQuery pays for deep penetration.
// A query with a NaN or infinite o or d, r < 0, NaN or infinite, or B < 0 or NaN gets the miss and does not walk (sw_valid).
#include "tirt_internal.h"
#include "tirt_sweep.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"

namespace tirt {

struct SwArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // the scan: kind and record slot of primitive i
    const float *rays; int64_t ray_stride;              // this chunk's first row: o3, d3
    const float *radius; int64_t radius_stride; float radius_all;
    const float *tmax; int64_t tmax_stride; float tmax_all;
    int n;                                              // queries of this chunk
    int stack_size;
    CpEntry *spill;                                     // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    float *out_t; int32_t *out_prim, *out_code; float *out_point; int64_t point_stride; float *out_uv; int64_t uv_stride;
    float *out_normal; int64_t normal_stride; uint8_t *out_blocked; int2 *counts;
    DevCounters *ctr;
};

// m of the query (o, r): PointMargin's expression with r / E added to the point's distance from the grid's centre
TD float sw_margin(const PointMargin &pm, const BvhView &b, const v3 o, const float r)
{
    const float rho_o = maxf(maxf(absf(o.x - b.grid_min[0]), absf(o.y - b.grid_min[1])), absf(o.z - b.grid_min[2])) * pm.inv_ext;
    const float rho_q = rho_o + r * pm.inv_ext;
    return cp_margin_cells(rho_q, pm.rho_0) * pm.cell_max;
}

// the query of row q: false = it gets the miss without a look at any primitive
TD bool sw_load_query(const SwArgs &a, const PointMargin &pm, int q, SwQuery &sq, float &B, float &m)
{
    const float *r = a.rays + (int64_t)q * a.ray_stride;
    const v3 o = V(r[0], r[1], r[2]), d = V(r[3], r[4], r[5]);
    const float rad = a.radius ? a.radius[(int64_t)q * a.radius_stride] : a.radius_all;
    B = a.tmax ? a.tmax[(int64_t)q * a.tmax_stride] : a.tmax_all;
    const bool ok = sw_valid(o, d, rad, B);
    m = ok ? sw_margin(pm, a.bvh, o, rad) : 0.0f;
    sq = sw_query(o, d, ok ? rad : 0.0f, m);
    return ok;
}

TD void sw_store(const SwArgs &a, int q, const SwQuery &sq, const SwHit &h, int prim, unsigned nbox, unsigned nleaf, bool count)
{
    const bool hit = prim >= 0;
    if (a.out_t) a.out_t[q] = h.t;
    if (a.out_prim) a.out_prim[q] = prim;
    if (a.out_code) a.out_code[q] = h.code;
    if (a.out_point) { float *o = a.out_point + (int64_t)q * a.point_stride; o[0] = hit ? h.cp.q.x : 0.0f; o[1] = hit ? h.cp.q.y : 0.0f; o[2] = hit ? h.cp.q.z : 0.0f; }
    if (a.out_uv) { float *o = a.out_uv + (int64_t)q * a.uv_stride; o[0] = hit ? h.cp.u : 0.0f; o[1] = hit ? h.cp.v : 0.0f; }
    if (a.out_normal) { const v3 n = sw_normal(sq, h); float *o = a.out_normal + (int64_t)q * a.normal_stride; o[0] = n.x; o[1] = n.y; o[2] = n.z; }      // (wave-uniform pointer: the ballot inside sees every lane that stores)
    if (a.out_blocked) a.out_blocked[q] = hit ? 1 : 0;
    if (count && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
}

// one record against the query: the kind comes from the caller (the leaf code's shape bit, or the primitive table).  The sphere branch sits behind a
// wave ballot, as cp_record's; a spot or a laser has no surface
TD void sw_test_record(const BvhView &b, int slot, bool is_tri, const SwQuery &sq, float B, float &best_t, int &best_prim, SwHit &best)
{
    const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
    const int prim = __float_as_int(tc.w);
    const v3 pa = V(ta.x, ta.y, ta.z);
    const float cut = __builtin_fminf(best_t, B);
    SwHit h = sw_miss();
    if (is_tri) h = sw_triangle(sq, pa, V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z), cut);
    const bool sph = !is_tri && (int)tb.y == SHAPE_SPHERE;
    if (__builtin_amdgcn_ballot_w64(sph) != 0ull) { if (sph) h = sw_sphere(sq, pa, tb.x, cut); }
    if (sw_accept(h.t, prim, B, best_t, best_prim)) { best_t = h.t; best_prim = prim; best = h; }
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_sw_scan(SwArgs a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    const PointMargin pm(a.bvh);
    SwQuery sq; float B, m;
    const bool ok = sw_load_query(a, pm, q, sq, B, m);
    float best_t = __int_as_float(0x7f800000); int best_prim = -1;
    SwHit best = sw_miss();
    const int np = ok ? a.n_prim : 0;
    for (int i = 0; i < np; i++)
        sw_test_record(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, sq, B, best_t, best_prim, best);
    sw_store(a, q, sq, best, best_prim, 0u, (unsigned)np, COUNT);
}

template <bool COUNT, bool ANY>
__global__ __launch_bounds__(CP_BLOCK) void k_sw_walk(SwArgs a)
{
    __shared__ CpEntry stk[CP_LDS_DEPTH * CP_BLOCK];    // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    const PointMargin pm(b);
    const float inf = __int_as_float(0x7f800000);
    unsigned long long n_over = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        SwQuery sq = sw_query(V(0.0f, 0.0f, 0.0f), V(0.0f, 0.0f, 0.0f), 0.0f, 0.0f); float B = -1.0f, m = 0.0f;
        const bool ok = live && sw_load_query(a, pm, live ? q : 0, sq, B, m);
        float best_t = inf; int best_prim = -1;
        SwHit best = sw_miss();
        // per query: the growth of every box, and per axis 1 / d (0 where the axis has no parameters) and whether the slab then has to hold o
        const float tol = sq.r * SW_TOL_REL + m, G = (sq.r + tol) + m;
        const float ivx = 1.0f / sq.d.x, ivy = 1.0f / sq.d.y, ivz = 1.0f / sq.d.z;
        const bool fx = absf(ivx) < inf, fy = absf(ivy) < inf, fz = absf(ivz) < inf;      // the axis has parameters
        const bool zx = sq.d.x == 0.0f, zy = sq.d.y == 0.0f, zz = sq.d.z == 0.0f;          // the axis has none and the slab must hold o
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        float cut = B;                                   // (best_t starts at +inf)
        int cur = ok ? b.root_qcode : CP_SENT;

        auto pop_live = [&]() {
            while (!st.empty()) { const CpEntry e = st.pop(); if (!(__uint_as_float(e.y) > cut)) return (int)e.x; }
            return CP_SENT;
        };
        while (__builtin_amdgcn_ballot_w64(cur != CP_SENT) != 0ull) {
            // ---- node step: the lanes that are at an inner node
            if (cur >= 0) {
                const uint4 *w = b.cnode + (size_t)cur * 4;
                const uint4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3];
                if (COUNT) nbox += 4;
                constexpr float MISS = 3.0e38f;
                int c0, c1, c2, c3; float l0, l1, l2, l3; bool k0, k1, k2, k3;
                // one axis of one child: the planes decoded as CP_BOX_GAP decodes them, grown by G, and the parameters at which o + t d crosses them
#define SW_AXIS(W, k, ok_, iv_, f_, z_, nr_, fr_)                                                      \
                do {                                                                                \
                    const cp_h2v h__ = __builtin_bit_cast(cp_h2v, (unsigned)(W));                   \
                    const float mn__ = b.grid_min[k] + (float)h__.x * b.cell[k], mx__ = b.grid_min[k] + (float)h__.y * b.cell[k]; \
                    const float lo__ = mn__ - G, hi__ = mx__ + G;                                   \
                    const float t1__ = (lo__ - (ok_)) * (iv_), t2__ = (hi__ - (ok_)) * (iv_);       \
                    const bool out__ = (z_) && !(((ok_) >= lo__) & ((ok_) <= hi__));                \
                    const float n__ = (f_) ? minf(t1__, t2__) : (out__ ? inf : -inf);               \
                    const float x__ = (f_) ? maxf(t1__, t2__) : (out__ ? -inf : inf);               \
                    nr_ = maxf(nr_, n__); fr_ = minf(fr_, x__);                                     \
                } while (0)
                // kept: a child that is there and that the segment can still meet before the cut (never culled on equality; a NaN keeps)
#define SW_BOX(i, X, Y, Z, code_)                                                                     \
                do {                                                                                \
                    float tn__ = 0.0f, tf__ = inf;                                                  \
                    SW_AXIS(X, 0, sq.o.x, ivx, fx, zx, tn__, tf__);                         \
                    SW_AXIS(Y, 1, sq.o.y, ivy, fy, zy, tn__, tf__);                         \
                    SW_AXIS(Z, 2, sq.o.z, ivz, fz, zz, tn__, tf__);                         \
                    c##i = (int)(code_);                                                            \
                    k##i = (c##i != TR_EMPTY) && !(tn__ > tf__) && !(tn__ > cut);                   \
                    l##i = k##i ? tn__ : MISS;                                                      \
                } while (0)
                CP_EACH_CHILD(SW_BOX);
#undef SW_BOX
#undef SW_AXIS
#define SW_CE(la, ca, ka, lb, cb, kb)                                                                 \
                do {                                                                                \
                    const bool s__ = (lb) < (la);                                                   \
                    const float lo__ = s__ ? (lb) : (la), hi__ = s__ ? (la) : (lb);                 \
                    const int clo__ = s__ ? (cb) : (ca), chi__ = s__ ? (ca) : (cb);                 \
                    const bool klo__ = s__ ? (kb) : (ka), khi__ = s__ ? (ka) : (kb);                \
                    la = lo__; lb = hi__; ca = clo__; cb = chi__; ka = klo__; kb = khi__;           \
                } while (0)
                SW_CE(l0, c0, k0, l1, c1, k1); SW_CE(l2, c2, k2, l3, c3, k3); SW_CE(l0, c0, k0, l2, c2, k2); SW_CE(l1, c1, k1, l3, c3, k3); SW_CE(l1, c1, k1, l2, c2, k2);
#undef SW_CE
                if (k3) st.push(CpEntry{(unsigned)c3, __float_as_uint(l3)});
                if (k2) st.push(CpEntry{(unsigned)c2, __float_as_uint(l2)});
                if (k1) st.push(CpEntry{(unsigned)c1, __float_as_uint(l1)});
                cur = k0 ? c0 : pop_live();
            }
            // ---- leaf step: the lanes that are at a leaf
            const bool at_leaf = cur < 0 && cur != CP_SENT;
            if (__builtin_amdgcn_ballot_w64(at_leaf) != 0ull) {
                if (at_leaf) {
                    if (COUNT) nleaf += 1;
                    const int code = ~cur;
                    sw_test_record(b, leaf_slot(code), leaf_is_tri(code), sq, B, best_t, best_prim, best);
                    cut = __builtin_fminf(best_t, B);
                    if (ANY && best_prim >= 0) { st.sp = 0; cur = CP_SENT; }      // blocked: the first accepted contact decides
                    else cur = pop_live();
                }
            }
        }
        if (live) sw_store(a, q, sq, best, best_prim, nbox, nleaf, COUNT);
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

struct SwCall {      // what the two entry points hand to sw_chunks: every pointer is device memory (or null)
    const float *rays; int64_t n, ray_stride;
    const float *radius; int64_t radius_stride; float radius_all;
    const float *tmax; int64_t tmax_stride; float tmax_all;
    int stack_size, flags;
    float *out_t; int32_t *out_prim, *out_code; float *out_point; int64_t point_stride; float *out_uv; int64_t uv_stride;
    float *out_normal; int64_t normal_stride; uint8_t *out_blocked; int2 *counts;
};

// `n` queries in chunks of `chunk` on the context's stream
static int sw_chunks(tirt_ctx *c, const SwCall &p, int chunk)
{
    const bool scan = (p.flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (p.flags & TIRT_COUNT_NODES) != 0;
    const bool any = p.out_blocked && !p.out_t && !p.out_prim && !p.out_code && !p.out_point && !p.out_uv && !p.out_normal;
    SwArgs a = {};
    a.ray_stride = p.ray_stride; a.radius_stride = p.radius_stride; a.radius_all = p.radius_all; a.tmax_stride = p.tmax_stride; a.tmax_all = p.tmax_all;
    a.point_stride = p.point_stride; a.uv_stride = p.uv_stride; a.normal_stride = p.normal_stride;
    return point_walk_chunks(c, a, p.n, chunk, scan, p.stack_size, [&](int64_t base, int m, int, int grid) {
        a.n = m;
        a.rays = p.rays + base * p.ray_stride;
        a.radius = p.radius ? p.radius + base * p.radius_stride : nullptr; a.tmax = p.tmax ? p.tmax + base * p.tmax_stride : nullptr;
        a.out_t = p.out_t ? p.out_t + base : nullptr; a.out_prim = p.out_prim ? p.out_prim + base : nullptr; a.out_code = p.out_code ? p.out_code + base : nullptr;
        a.out_point = p.out_point ? p.out_point + base * p.point_stride : nullptr; a.out_uv = p.out_uv ? p.out_uv + base * p.uv_stride : nullptr;
        a.out_normal = p.out_normal ? p.out_normal + base * p.normal_stride : nullptr; a.out_blocked = p.out_blocked ? p.out_blocked + base : nullptr;
        a.counts = p.counts ? p.counts + base : nullptr;
        with_bool(cnt, [&](auto C) {
            constexpr bool COUNT = decltype(C)::value;
            if (scan) hipLaunchKernelGGL((k_sw_scan<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
            else with_bool(any, [&](auto A) { hipLaunchKernelGGL((k_sw_walk<COUNT, decltype(A)::value>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a); });
        });
    });
}

// one row per thread through sw_kat_row (tirt_sweep.h): the text tirt_kat_sweep_host runs on the host
__global__ void k_kat_sweep(const float *in, int n, int is_sphere, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sw_kat_row(in + (size_t)i * (is_sphere ? SW_KAT_SPH : SW_KAT_TRI), is_sphere, out + (size_t)i * SW_KAT_OUT);
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_sweep(tirt_ctx *c, const float *rays, int64_t n, int64_t ray_stride, const float *radius, int64_t radius_stride, float radius_all,
                     const float *tmax, int64_t tmax_stride, float tmax_all, int stack_size, int flags, float *out_t, int32_t *out_prim, int32_t *out_code,
                     float *out_point, int64_t point_stride, float *out_uv, int64_t uv_stride, float *out_normal, int64_t normal_stride,
                     uint8_t *out_blocked, int32_t *counts, void *stream)
{
    const char *fn = "tirt_query_sweep";
    const std::string f = std::string(fn) + ": ";
    CTX(c);
    if (int rc = point_query_checks(c, fn, n, stack_size, flags, {{true, ray_stride, 6, "ray_stride < 6 (floats per ray)"},
                                    {radius != nullptr, radius_stride, 1, "radius_stride < 1"}, {tmax != nullptr, tmax_stride, 1, "tmax_stride < 1"},
                                    {out_point != nullptr, point_stride, 3, "point_stride < 3 (floats per contact point)"}, {out_uv != nullptr, uv_stride, 2, "uv_stride < 2"},
                                    {out_normal != nullptr, normal_stride, 3, "normal_stride < 3 (floats per normal)"}}, counts, stream)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(rays, f + "null rays");
    const QueryPlan pl = query_plan(c, n, flags, counts);
    if (int rc = require_device_ptrs(c, f, {{rays, "rays"}, {radius, "radius"}, {tmax, "tmax"}, {out_t, "out_t"}, {out_prim, "out_prim"}, {out_code, "out_code"},
                                            {out_point, "out_point"}, {out_uv, "out_uv"}, {out_normal, "out_normal"}, {out_blocked, "out_blocked"},
                                            {pl.counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    const SwCall p = {rays, n, ray_stride, radius, radius_stride, radius_all, tmax, tmax_stride, tmax_all, stack_size, flags, out_t, out_prim, out_code,
                      out_point, point_stride, out_uv, uv_stride, out_normal, normal_stride, out_blocked, pl.counts};
    if (int rc = sw_chunks(c, p, pl.chunk)) return rc;
    return query_end(c, stream);
}

// host arrays staged in device memory (QueryStage), one chunk of all of them, back with a sync.  The walk is handed every output, asked for or not -- but
// `blocked` alone, if the caller asked for nothing else: the ANY walk
int tirt_sweep(tirt_ctx *c, const float *rays, int n, const float *radius, float radius_all, const float *tmax, int stack_size, int flags, float *out_t,
               int32_t *out_prim, int32_t *out_code, float *out_point, float *out_uv, float *out_normal, uint8_t *out_blocked, int32_t *counts)
{
    const char *fn = "tirt_sweep";
    CTX(c);
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(rays, std::string(fn) + ": null rays");
    const size_t N = (size_t)n;
    const bool only_blocked = out_blocked && !out_t && !out_prim && !out_code && !out_point && !out_uv && !out_normal;
    QueryStage s(c);
    const auto k_rays = s.in(rays, 6 * N);
    const auto k_radius = s.in(radius, N);
    const auto k_tmax = s.in(tmax, N);
    const auto k_t = s.out(out_t, N, !only_blocked);
    const auto k_prim = s.out(out_prim, N, !only_blocked);
    const auto k_code = s.out(out_code, N, !only_blocked);
    const auto k_point = s.out(out_point, 3 * N, !only_blocked);
    const auto k_uv = s.out(out_uv, 2 * N, !only_blocked);
    const auto k_normal = s.out(out_normal, 3 * N, !only_blocked);
    const auto k_blocked = s.out(out_blocked, N, out_blocked != nullptr);
    const auto k_counts = s.out_counts(counts, flags, N);
    if (int rc = s.begin()) return rc;
    const SwCall p = {s.ptr(k_rays), n, 6, s.ptr(k_radius), 1, radius_all, s.ptr(k_tmax), 1, __builtin_inff(), stack_size, flags, s.ptr(k_t), s.ptr(k_prim),
                      s.ptr(k_code), s.ptr(k_point), 3, s.ptr(k_uv), 2, s.ptr(k_normal), 3, s.ptr(k_blocked), s.ptr(k_counts)};
    if (int rc = sw_chunks(c, p, n)) return rc;
    return s.finish();
}

int tirt_kat_sweep(tirt_ctx *c, const float *in, int n, int is_sphere, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_sweep: null pointer or negative n");
    TIRT_REQUIRE(is_sphere == 0 || is_sphere == 1, "tirt_kat_sweep: is_sphere is 0 (triangle rows of 18 floats) or 1 (sphere rows of 13)");
    CTX(c);
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_sweep", {{in, kat_row_bytes(n, is_sphere ? SW_KAT_SPH : SW_KAT_TRI)}}, out, kat_row_bytes(n, SW_KAT_OUT), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_sweep, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)din[0], n, is_sphere, (float *)dout);
    });
}

// host only, no context: the same rows through the same text (sw_kat_row), compiled for the host
int tirt_kat_sweep_host(const float *in, int n, int is_sphere, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_sweep_host: null pointer or negative n");
    TIRT_REQUIRE(is_sphere == 0 || is_sphere == 1, "tirt_kat_sweep_host: is_sphere is 0 (triangle rows of 18 floats) or 1 (sphere rows of 13)");
    for (int i = 0; i < n; i++) sw_kat_row(in + (size_t)i * (is_sphere ? SW_KAT_SPH : SW_KAT_TRI), is_sphere, out + (size_t)i * SW_KAT_OUT);
    return TIRT_OK;
}

}  // extern "C"
