// tirt_closest_point.hip -- the nearest surface point to a query point (tirt_query_closest_point / tirt_closest_point / tirt_kat_closest_point,
// include/tirt.h "Closest point").  No reference counterpart: the reference only answers questions that start from a ray.
//
//   k_cp_scan   one query per lane against all n primitive records in primitive-id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick on the device
//   k_cp_walk   one query per lane, best-first over the quantised 4-wide nodes `cnode` (BvhView): the hot path
// Both are templates on <COUNT, SIGNED>.  SIGNED (tirt_query_signed_distance / tirt_signed_distance, include/tirt.h "Signed distance") adds an epilogue and
// nothing else: sd_store classifies the answer's (u, v), gathers ONE row of the pseudo-normal table that tirt_signed_distance.hip keeps (a sphere: its
// record again) and stores the signed distance.  The SIGNED = false instantiations hold no trace of it (DESIGN.md has their digests and registers).
//
// Both call cp_triangle / cp_sphere / cp_accept (tirt_closest_point.h) and nothing else decides an answer, and the answer is the minimum of a total
// order on (D2, prim): the walk returns the scan's bits if and only if it never skips a primitive that would have been accepted.
//
// THE WALK is point_walk (tirt_point_walk.h, which has why its cull is conservative) with lo == hi == the query point and the margin of PointMargin; lane l
// of a block holds query base + l and the blocks stride over the chunk.  THE CUT is min(best D2 so far, lim2): the leaf tests the record through
// cp_test_record and returns it.  The stack is PointStack<CpEntry>; DESIGN.md "Closest point" has the sizes and why 16.  An entry beyond stack_size
// is dropped and the query counted in DevCounters::stack_overflow (tirt_stats: TIRT_ERR_STACK), as a ray's.
// The walk starts at root_qcode (a leaf code in a one-primitive scene).  Every analytic sphere is below it: its slot carries its padded box
// (shapes_boxed) or the whole grid, and both contain the sphere, as every ancestor's box does -- the chain nodes at far_qcode exist for rays, whose
// sphere test can answer from outside the padded box; a closest point lies ON the sphere.  Spot and laser leaves are reached and skipped.
// A query with a NaN or infinite coordinate finds nothing by the definition (every D2 is NaN or +inf): it does not walk.
#include "tirt_internal.h"
#include "tirt_closest_point.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"

namespace tirt {

struct CpArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // the scan: kind and record slot of primitive i
    const float *points; int64_t point_stride;          // this chunk's first row
    const float *dmax; int64_t dmax_stride; float dmax_all;
    int n;                                              // queries of this chunk
    int stack_size;
    CpEntry *spill;                                     // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    float *out_d2; int32_t *out_prim; float *out_point; int64_t point_out_stride; float *out_uv; int64_t uv_stride; int2 *counts;
    DevCounters *ctr;
    // signed distance (the SIGNED instantiations alone read these; at the end, so that the others' argument offsets stay what they were)
    const float4 *sd_tab; const int *sd_state; float *out_sd;      // [n_prim][SD_ROWS]; sd_state[0] != 0: the table's build dropped a stack entry
};

TD void cp_store(const CpArgs &a, int q, float best2, int best_prim, const CpPoint &bp, unsigned nbox, unsigned nleaf, bool count)
{
    if (a.out_d2) a.out_d2[q] = best2;
    if (a.out_prim) a.out_prim[q] = best_prim;
    if (a.out_point) { float *o = a.out_point + (int64_t)q * a.point_out_stride; o[0] = bp.q.x; o[1] = bp.q.y; o[2] = bp.q.z; }
    if (a.out_uv) { float *o = a.out_uv + (int64_t)q * a.uv_stride; o[0] = bp.u; o[1] = bp.v; }
    if (count && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
}

// one record against the query: the kind comes from the caller (the leaf code's shape bit, or the primitive table)
TD void cp_test_record(const BvhView &b, int slot, bool is_tri, const v3 p, float lim2, float &best2, int &best_prim, CpPoint &bp)
{
    int prim;
    const CpPoint r = cp_record(b, slot, is_tri, p, prim);
    if (cp_accept(r.d2, prim, lim2, best2, best_prim)) { best2 = r.d2; best_prim = prim; bp = r; }
}

// the SIGNED epilogue: the sign of the answer from the winner's table row (a sphere: from its record, read again); nothing found: +inf.  A table whose
// build ran out of stack is no table: every sd is NaN (and stack_overflow has been counted: tirt_stats says TIRT_ERR_STACK)
TD void sd_store(const CpArgs &a, int q, const v3 p, int best_prim, const CpPoint &bp)
{
    float sd = __int_as_float(0x7f800000);
    if (best_prim >= 0) {
        if (a.primitive[(size_t)best_prim * PRI_VEC] == PRIMITIVE_TRI) {
            const float4 *rows = a.sd_tab + (size_t)best_prim * SD_ROWS;
            int f;
            sd = sd_sign(p, bp, [rows](int k) { const float4 r = rows[k]; return V(r.x, r.y, r.z); }, f);
        } else {
            const float4 *tp = a.bvh.tri + (size_t)a.prim_slot[best_prim] * TRI_STRIDE;
            const float4 ta = tp[0], tb = tp[1];
            sd = sd_sign_sphere(p, bp.d2, V(ta.x, ta.y, ta.z), tb.x);
        }
    }
    if (a.sd_state[0] != 0) sd = __int_as_float(0x7fc00000);
    a.out_sd[q] = sd;
}

template <bool COUNT, bool SIGNED>
__global__ __launch_bounds__(CP_BLOCK) void k_cp_scan(CpArgs a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    v3 p; float lim2;
    cp_load_query(a, q, p, lim2);
    float best2 = __int_as_float(0x7f800000); int best_prim = -1;
    CpPoint bp; bp.d2 = best2; bp.q = V(0.0f, 0.0f, 0.0f); bp.u = 0.0f; bp.v = 0.0f;
    for (int i = 0; i < a.n_prim; i++)
        cp_test_record(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, p, lim2, best2, best_prim, bp);
    cp_store(a, q, best2, best_prim, bp, 0u, (unsigned)a.n_prim, COUNT);
    if constexpr (SIGNED) sd_store(a, q, p, best_prim, bp);
}

template <bool COUNT, bool SIGNED>
__global__ __launch_bounds__(CP_BLOCK) void k_cp_walk(CpArgs a)
{
    __shared__ CpEntry stk[CP_LDS_DEPTH * CP_BLOCK];    // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    const PointMargin pm(b);
    unsigned long long n_over = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        v3 p = V(0.0f, 0.0f, 0.0f); float lim2 = -1.0f;
        if (live) cp_load_query(a, q, p, lim2);
        float best2 = __int_as_float(0x7f800000); int best_prim = -1;
        CpPoint bp; bp.d2 = best2; bp.q = V(0.0f, 0.0f, 0.0f); bp.u = 0.0f; bp.v = 0.0f;
        const float inf = __int_as_float(0x7f800000);
        const bool finite = CP_FINITE3(p, inf);
        const float m = pm.margin(b, p);
        const int start = (live && finite && lim2 >= 0.0f) ? b.root_qcode : CP_SENT;
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        point_walk<COUNT>(b, st, m, p, p, start, lim2, nbox, nleaf, [&](int code) {      // (the first cut is lim2: best2 starts at +inf)
            cp_test_record(b, leaf_slot(code), leaf_is_tri(code), p, lim2, best2, best_prim, bp);
            return __builtin_fminf(best2, lim2);
        });
        if (live) cp_store(a, q, best2, best_prim, bp, nbox, nleaf, COUNT);
        if constexpr (SIGNED) { if (live) sd_store(a, q, p, best_prim, bp); }
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

// `n` queries in chunks of `chunk` on the context's stream; every pointer is device memory (or null)
static int cp_chunks(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                     int stack_size, int flags, int chunk, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                     float *out_uv, int64_t uv_stride, int2 *counts, float *out_sd = nullptr)      // out_sd: the SIGNED kernels (the table stands: sd_table_ensure)
{
    const bool scan = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0, sgn = out_sd != nullptr;
    CpArgs a = {};
    a.point_stride = point_stride; a.dmax_stride = dmax_stride; a.dmax_all = dmax_all;
    a.point_out_stride = point_out_stride; a.uv_stride = uv_stride;
    if (sgn) { a.sd_tab = c->sd_tab.as<float4>(); a.sd_state = c->sd_state.as<int>(); }
    return point_walk_chunks(c, a, n, chunk, scan, stack_size, [&](int64_t base, int m, int, int grid) {
        a.n = m;
        a.points = points + base * point_stride; a.dmax = dmax ? dmax + base * dmax_stride : nullptr;
        a.out_d2 = out_d2 ? out_d2 + base : nullptr; a.out_prim = out_prim ? out_prim + base : nullptr;
        a.out_point = out_point ? out_point + base * point_out_stride : nullptr; a.out_uv = out_uv ? out_uv + base * uv_stride : nullptr;
        a.counts = counts ? counts + base : nullptr;
        a.out_sd = sgn ? out_sd + base : nullptr;
        with_bool(cnt, [&](auto C) { with_bool(sgn, [&](auto S) {
            constexpr bool COUNT = decltype(C)::value, SIGNED = decltype(S)::value;
            if (scan) hipLaunchKernelGGL((k_cp_scan<COUNT, SIGNED>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
            else hipLaunchKernelGGL((k_cp_walk<COUNT, SIGNED>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
        }); });
    });
}

// tirt_query_closest_point, and with `sgn` tirt_query_signed_distance (the same checks, out_sd beside the other outputs, the table made first)
static int query_closest_point(tirt_ctx *c, const char *fn, bool sgn, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride,
                               float dmax_all, int stack_size, int flags, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                               float *out_uv, int64_t uv_stride, int32_t *counts, float *out_sd, void *stream)
{
    const std::string f = std::string(fn) + ": ";
    if (int rc = point_query_checks(c, fn, n, stack_size, flags, {{true, point_stride, 3, "point_stride < 3 (floats per point)"},
                                    {out_point != nullptr, point_out_stride, 3, "point_out_stride < 3 (floats per closest point)"},
                                    {out_uv != nullptr, uv_stride, 2, "uv_stride < 2"}, {dmax != nullptr, dmax_stride, 1, "dmax_stride < 1"}}, counts, stream)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, f + "null points");
    TIRT_REQUIRE(!sgn || out_sd, f + "null out_sd");
    const QueryPlan pl = query_plan(c, n, flags, counts);
    if (int rc = require_device_ptrs(c, f, {{points, "points"}, {dmax, "dmax"}, {out_d2, "out_d2"}, {out_prim, "out_prim"}, {out_point, "out_point"}, {out_uv, "out_uv"},
                                            {sgn ? out_sd : nullptr, "out_sd"}, {pl.counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (sgn) if (int rc = sd_table_ensure(c, stack_size)) return rc;      // (on the context's stream, after the caller's work: no host sync)
    if (int rc = cp_chunks(c, points, n, point_stride, dmax, dmax_stride, dmax_all, stack_size, flags, pl.chunk, out_d2, out_prim, out_point,
                           point_out_stride, out_uv, uv_stride, pl.counts, sgn ? out_sd : nullptr)) return rc;
    return query_end(c, stream);
}

// host arrays staged in device memory (QueryStage), one chunk of all of them, back with a sync.  The walk is handed every output, asked for or not.
// `sgn`: tirt_signed_distance -- the table is made first and, the stream being waited for anyway, its build's verdict read: TIRT_ERR_STACK, no answers
static int closest_point_host(tirt_ctx *c, const char *fn, bool sgn, const float *points, int n, const float *dmax, int stack_size, int flags, float *out_d2,
                              int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts, float *out_sd)
{
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, std::string(fn) + ": null points");
    TIRT_REQUIRE(!sgn || out_sd, std::string(fn) + ": null out_sd");
    const size_t N = (size_t)n;
    QueryStage s(c);
    const auto k_points = s.in(points, 3 * N);
    const auto k_dmax = s.in(dmax, N);
    const auto k_d2 = s.out(out_d2, N);
    const auto k_prim = s.out(out_prim, N);
    const auto k_point = s.out(out_point, 3 * N);
    const auto k_uv = s.out(out_uv, 2 * N);
    const auto k_counts = s.out_counts(counts, flags, N);
    const auto k_sd = s.out(out_sd, N, sgn);
    if (int rc = s.begin()) return rc;
    if (sgn) if (int rc = sd_table_ensure(c, stack_size)) return rc;
    if (int rc = cp_chunks(c, s.ptr(k_points), n, 3, s.ptr(k_dmax), 1, __builtin_inff(), stack_size, flags, n, s.ptr(k_d2), s.ptr(k_prim), s.ptr(k_point), 3,
                           s.ptr(k_uv), 2, s.ptr(k_counts), s.ptr(k_sd))) return rc;
    if (sgn) if (int rc = sd_table_verdict(c, fn)) return rc;      // (waits for the stream)
    return s.finish();
}

// rows of (p3, a3, b3, c3) or (p3, c3, r) -> d2, q3, u, v
__global__ void k_kat_closest_point(const float *in, int n, int is_sphere, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = in + (size_t)i * (is_sphere ? 7 : 12);
    const v3 p = V(r[0], r[1], r[2]);
    const CpPoint a = is_sphere ? cp_sphere(p, V(r[3], r[4], r[5]), r[6])
                                : cp_triangle(p, V(r[3], r[4], r[5]), V(r[6], r[7], r[8]), V(r[9], r[10], r[11]));
    float *o = out + (size_t)i * 6;
    o[0] = a.d2; o[1] = a.q.x; o[2] = a.q.y; o[3] = a.q.z; o[4] = a.u; o[5] = a.v;
}

// rows of (p3, a3, b3, c3, N[7][3]) -> sd, feature: cp_triangle, then sd_sign on the row's own pseudo-normals
__global__ void k_kat_signed_distance(const float *in, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = in + (size_t)i * 33;
    const v3 p = V(r[0], r[1], r[2]);
    const CpPoint a = cp_triangle(p, V(r[3], r[4], r[5]), V(r[6], r[7], r[8]), V(r[9], r[10], r[11]));
    const float *N = r + 12;
    int f;
    const float sd = sd_sign(p, a, [N](int k) { return V(N[3 * k], N[3 * k + 1], N[3 * k + 2]); }, f);
    out[(size_t)i * 2] = sd; out[(size_t)i * 2 + 1] = (float)f;
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_closest_point(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                             int stack_size, int flags, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                             float *out_uv, int64_t uv_stride, int32_t *counts, void *stream)
{
    CTX(c);
    return query_closest_point(c, "tirt_query_closest_point", false, points, n, point_stride, dmax, dmax_stride, dmax_all, stack_size, flags, out_d2, out_prim,
                               out_point, point_out_stride, out_uv, uv_stride, counts, nullptr, stream);
}

int tirt_query_signed_distance(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                               int stack_size, int flags, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                               float *out_uv, int64_t uv_stride, int32_t *counts, void *stream, float *out_sd)
{
    CTX(c);
    return query_closest_point(c, "tirt_query_signed_distance", true, points, n, point_stride, dmax, dmax_stride, dmax_all, stack_size, flags, out_d2, out_prim,
                               out_point, point_out_stride, out_uv, uv_stride, counts, out_sd, stream);
}

int tirt_signed_distance(tirt_ctx *c, const float *points, int n, const float *dmax, int stack_size, int flags, float *out_d2, int32_t *out_prim,
                         float *out_point, float *out_uv, int32_t *counts, float *out_sd)
{
    CTX(c);
    return closest_point_host(c, "tirt_signed_distance", true, points, n, dmax, stack_size, flags, out_d2, out_prim, out_point, out_uv, counts, out_sd);
}

int tirt_kat_signed_distance(tirt_ctx *c, const float *in, int n, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_signed_distance: null pointer or negative n");
    CTX(c);
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_signed_distance", {{in, kat_row_bytes(n, 33)}}, out, kat_row_bytes(n, 2), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_signed_distance, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)din[0], n, (float *)dout);
    });
}

int tirt_closest_point(tirt_ctx *c, const float *points, int n, const float *dmax, int stack_size, int flags, float *out_d2, int32_t *out_prim,
                       float *out_point, float *out_uv, int32_t *counts)
{
    CTX(c);
    return closest_point_host(c, "tirt_closest_point", false, points, n, dmax, stack_size, flags, out_d2, out_prim, out_point, out_uv, counts, nullptr);
}

int tirt_kat_closest_point(tirt_ctx *c, const float *in, int n, int is_sphere, float *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_closest_point: null pointer or negative n");
    CTX(c);
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_closest_point", {{in, kat_row_bytes(n, is_sphere ? 7 : 12)}}, out, kat_row_bytes(n, 6), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_closest_point, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)din[0], n, is_sphere, (float *)dout);
    });
}

}  // extern "C"
