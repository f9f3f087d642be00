// tirt_triangle_query.hip -- the closest points between a query TRIANGLE and the scene's triangles (tirt_query_mesh_distance / tirt_mesh_distance /
// tirt_kat_tri_tri / tirt_kat_tri_tri_host, include/tirt.h "Triangle distance").  No reference counterpart: the reference only answers questions that
// start from a ray.
//
//   k_tq_scan   one query triangle per lane against all n primitive records in primitive-id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick on the device
//   k_tq_walk   one query triangle per lane, best-first over the quantised 4-wide nodes `cnode` (BvhView): the hot path
// Both are templates on <COUNT>.  Both call tq_pair (tirt_triangle_query.h) and cp_accept (tirt_closest_point.h) and nothing else decides an answer, and
// the answer is the minimum of a total order on (D2, prim): the walk returns the scan's bits if and only if it never skips a primitive that would have
// been accepted.
//
// THE WALK is point_walk (tirt_point_walk.h), with a box where k_cp_walk has a point: [lo, hi] is the exact box of the query triangle and m the largest of
// PointMargin's margins of its three vertices; lane l of a block holds query base + l and the blocks stride over the chunk.  THE CUT is min(best D2 so
// far, lim2): the leaf tests the record through tq_test_record and returns it.  The stack is PointStack<CpEntry>; an entry beyond stack_size is dropped and
// the query counted in DevCounters::stack_overflow.
// Culling is on lb2 > cut alone, never on equality: with the answer at D2 = 0 every subtree whose grown box meets the query's box (lb2 == 0) is still
// visited, because a primitive of a smaller id may tie at 0.  A deep penetration costs that many leaf tests.
// Analytic spheres, spot and laser leaves are reached and skipped (a NaN D2 is never accepted).  A query with a NaN or infinite coordinate finds nothing
// by the definition (tq_load_query gives it the lim2 of a negative bound): it does not walk, and the scan accepts nothing for it.
// THE LEAF STEP is the register-heavy, divergent part: 21 candidates.  tq_pair keeps each of its five groups in a rolled loop over vertices or edges
// (the operands picked by selects, not by indexed arrays: nothing goes to scratch), so the live state across a candidate is the query (9), the record
// (9), the pair's answer (8) and the walk's own registers; the groups after a d2 of +0 are skipped.
//
// WHY THE CULL IS CONSERVATIVE: the head of tirt_triangle_query.h, which extends the head of tirt_point_walk.h.
#include "tirt_internal.h"
#include "tirt_triangle_query.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"

namespace tirt {

struct TqArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // the scan: kind and record slot of primitive i
    const float *tris; int64_t tri_stride;              // this chunk's first row: p0, p1, p2
    const float *dmax; int64_t dmax_stride; float dmax_all;
    int n;                                              // queries of this chunk
    int stack_size;
    CpEntry *spill;                                     // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    float *out_d2; int32_t *out_prim, *out_code; float *out_points; int64_t points_stride; int2 *counts;
    DevCounters *ctr;
};

struct TqQuery { v3 p0, p1, p2; float lim2; };
struct TqBest { float d2; int prim, code; v3 P, Q; };

// a query with a NaN or infinite coordinate finds nothing by the definition, in the scan as in the walk: its lim2 is that of a negative bound
TD TqQuery tq_load_query(const TqArgs &a, int q)
{
    const float *r = a.tris + (int64_t)q * a.tri_stride;
    TqQuery t;
    t.p0 = V(r[0], r[1], r[2]); t.p1 = V(r[3], r[4], r[5]); t.p2 = V(r[6], r[7], r[8]);
    t.lim2 = cp_limit2(a.dmax ? a.dmax[(int64_t)q * a.dmax_stride] : a.dmax_all);
    if (!(cp_finite3(t.p0) && cp_finite3(t.p1) && cp_finite3(t.p2))) t.lim2 = -1.0f;
    return t;
}

TD TqBest tq_nothing()
{
    TqBest o;
    o.d2 = __int_as_float(0x7f800000); o.prim = -1; o.code = -1; o.P = V(0.0f, 0.0f, 0.0f); o.Q = o.P;
    return o;
}

TD void tq_store(const TqArgs &a, int q, const TqBest &o, unsigned nbox, unsigned nleaf, bool count)
{
    if (a.out_d2) a.out_d2[q] = o.d2;
    if (a.out_prim) a.out_prim[q] = o.prim;
    if (a.out_code) a.out_code[q] = o.code;
    if (a.out_points) { float *w = a.out_points + (int64_t)q * a.points_stride; w[0] = o.P.x; w[1] = o.P.y; w[2] = o.P.z; w[3] = o.Q.x; w[4] = o.Q.y; w[5] = o.Q.z; }
    if (count && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
}

// one record against the query: a triangle through tq_pair; anything else has no part (its D2 would be NaN: never accepted)
TD void tq_test_record(const BvhView &b, int slot, bool is_tri, const TqQuery &t, TqBest &o)
{
    if (is_tri) {
        const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
        const float4 ta = tp[0], tb = tp[1], tc = tp[2];
        const int prim = __float_as_int(tc.w);
        const TqPair r = tq_pair(t.p0, t.p1, t.p2, V(ta.x, ta.y, ta.z), V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
        if (cp_accept(r.d2, prim, t.lim2, o.d2, o.prim)) { o.d2 = r.d2; o.prim = prim; o.code = r.code; o.P = r.P; o.Q = r.Q; }
    }
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_tq_scan(TqArgs a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    const TqQuery t = tq_load_query(a, q);
    TqBest o = tq_nothing();
    for (int i = 0; i < a.n_prim; i++)
        tq_test_record(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, t, o);
    tq_store(a, q, o, 0u, (unsigned)a.n_prim, COUNT);
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_tq_walk(TqArgs a)
{
    __shared__ CpEntry stk[CP_LDS_DEPTH * CP_BLOCK];    // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    const PointMargin pm(b);
    unsigned long long n_over = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        TqQuery t; t.p0 = V(0.0f, 0.0f, 0.0f); t.p1 = t.p0; t.p2 = t.p0; t.lim2 = -1.0f;
        if (live) t = tq_load_query(a, q);
        TqBest o = tq_nothing();
        const v3 lo = V(minf(minf(t.p0.x, t.p1.x), t.p2.x), minf(minf(t.p0.y, t.p1.y), t.p2.y), minf(minf(t.p0.z, t.p1.z), t.p2.z));
        const v3 hi = V(maxf(maxf(t.p0.x, t.p1.x), t.p2.x), maxf(maxf(t.p0.y, t.p1.y), t.p2.y), maxf(maxf(t.p0.z, t.p1.z), t.p2.z));
        const float m = maxf(maxf(pm.margin(b, t.p0), pm.margin(b, t.p1)), pm.margin(b, t.p2));      // rho_p over all three vertices
        const int start = (live && t.lim2 >= 0.0f) ? b.root_qcode : CP_SENT;      // (a negative or NaN bound, a query that is not finite: no walk)
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        point_walk<COUNT>(b, st, m, lo, hi, start, t.lim2, nbox, nleaf, [&](int code) {      // (the first cut is lim2: the best starts at +inf)
            tq_test_record(b, leaf_slot(code), leaf_is_tri(code), t, o);
            return __builtin_fminf(o.d2, t.lim2);
        });
        if (live) tq_store(a, q, o, nbox, nleaf, COUNT);
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

// `n` queries in chunks of `chunk` on the context's stream; every pointer is device memory (or null)
static int tq_chunks(tirt_ctx *c, const float *tris, int64_t n, int64_t tri_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                     int stack_size, int flags, int chunk, float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int64_t points_stride,
                     int2 *counts)
{
    const bool scan = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0;
    TqArgs a = {};
    a.tri_stride = tri_stride; a.dmax_stride = dmax_stride; a.dmax_all = dmax_all;
    a.points_stride = points_stride;
    return point_walk_chunks(c, a, n, chunk, scan, stack_size, [&](int64_t base, int m, int, int grid) {
        a.n = m;
        a.tris = tris + base * tri_stride; a.dmax = dmax ? dmax + base * dmax_stride : nullptr;
        a.out_d2 = out_d2 ? out_d2 + base : nullptr; a.out_prim = out_prim ? out_prim + base : nullptr; a.out_code = out_code ? out_code + base : nullptr;
        a.out_points = out_points ? out_points + base * points_stride : nullptr;
        a.counts = counts ? counts + base : nullptr;
        with_bool(cnt, [&](auto C) {
            constexpr bool COUNT = decltype(C)::value;
            if (scan) hipLaunchKernelGGL((k_tq_scan<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
            else hipLaunchKernelGGL((k_tq_walk<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
        });
    });
}

// one row per thread through tq_kat_row (tirt_triangle_query.h): the text tirt_kat_tri_tri_host runs on the host
__global__ void k_kat_tri_tri(const float *in, int n, int what, int in_stride, int out_stride, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tq_kat_row(in + (size_t)i * in_stride, what, out + (size_t)i * out_stride);
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_mesh_distance(tirt_ctx *c, const float *tris, int64_t n, int64_t tri_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                             int stack_size, int flags, float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int64_t points_stride,
                             int32_t *counts, void *stream)
{
    const char *fn = "tirt_query_mesh_distance";
    const std::string f = std::string(fn) + ": ";
    CTX(c);
    if (int rc = point_query_checks(c, fn, n, stack_size, flags, {{true, tri_stride, 9, "tri_stride < 9 (floats per triangle)"},
                                    {out_points != nullptr, points_stride, 6, "points_stride < 6 (floats per pair of closest points)"},
                                    {dmax != nullptr, dmax_stride, 1, "dmax_stride < 1"}}, counts, stream)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(tris, f + "null tris");
    const QueryPlan pl = query_plan(c, n, flags, counts);
    if (int rc = require_device_ptrs(c, f, {{tris, "tris"}, {dmax, "dmax"}, {out_d2, "out_d2"}, {out_prim, "out_prim"}, {out_code, "out_code"}, {out_points, "out_points"},
                                            {pl.counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = tq_chunks(c, tris, n, tri_stride, dmax, dmax_stride, dmax_all, stack_size, flags, pl.chunk, out_d2, out_prim, out_code, out_points,
                           points_stride, pl.counts)) return rc;
    return query_end(c, stream);
}

// host arrays staged in device memory (QueryStage), one chunk of all of them, back with a sync.  The walk is handed every output, asked for or not
int tirt_mesh_distance(tirt_ctx *c, const float *tris, int n, const float *dmax, int stack_size, int flags, float *out_d2, int32_t *out_prim,
                       int32_t *out_code, float *out_points, int32_t *counts)
{
    const char *fn = "tirt_mesh_distance";
    CTX(c);
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(tris, std::string(fn) + ": null tris");
    const size_t N = (size_t)n;
    QueryStage s(c);
    const auto k_tris = s.in(tris, 9 * N);
    const auto k_dmax = s.in(dmax, N);
    const auto k_d2 = s.out(out_d2, N);
    const auto k_prim = s.out(out_prim, N);
    const auto k_code = s.out(out_code, N);
    const auto k_points = s.out(out_points, 6 * N);
    const auto k_counts = s.out_counts(counts, flags, N);
    if (int rc = s.begin()) return rc;
    if (int rc = tq_chunks(c, s.ptr(k_tris), n, 9, s.ptr(k_dmax), 1, __builtin_inff(), stack_size, flags, n, s.ptr(k_d2), s.ptr(k_prim), s.ptr(k_code),
                           s.ptr(k_points), 6, s.ptr(k_counts))) return rc;
    return s.finish();
}

int tirt_kat_tri_tri(tirt_ctx *c, const float *in, int n, int what, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_tri_tri: null pointer or negative n");
    TIRT_REQUIRE(what >= 0 && what <= 2, "tirt_kat_tri_tri: what is 0 (pair), 1 (segment-segment) or 2 (segment-triangle)");
    CTX(c);
    if (n == 0) return TIRT_OK;
    const int is = TQ_KAT_IN[what], os = TQ_KAT_OUT[what];
    return kat_round_trip(c, "tirt_kat_tri_tri", {{in, kat_row_bytes(n, is)}}, out, kat_row_bytes(n, os), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_tri_tri, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)din[0], n, what, is, os, (float *)dout);
    });
}

// host only, no context: the same rows through the same text (tq_kat_row), compiled for the host
int tirt_kat_tri_tri_host(const float *in, int n, int what, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_tri_tri_host: null pointer or negative n");
    TIRT_REQUIRE(what >= 0 && what <= 2, "tirt_kat_tri_tri_host: what is 0 (pair), 1 (segment-segment) or 2 (segment-triangle)");
    const int is = TQ_KAT_IN[what], os = TQ_KAT_OUT[what];
    for (int i = 0; i < n; i++) tq_kat_row(in + (size_t)i * is, what, out + (size_t)i * os);
    return TIRT_OK;
}

}  // extern "C"
