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
// THE WALK.  A wave is a block (no barrier anywhere); lane l holds query base + l and the blocks stride over the chunk.  A node visit decodes the four
// children's planes (grid_min + h * cell, h the fp16 halves of the record), forms lb2 = sum over the axes of max(mn - p - m, p - mx - m, 0)^2 with the
// margin m of PointMargin (tirt_point_walk.h), drops empty slots and children with lb2 > cut (cut = min(best D2 so far, lim2)), sorts the rest (five compare-exchanges, as k_trace),
// descends into the nearest and pushes the others far to near WITH their lb2; a popped entry is tested against the cut of that moment again (the best
// distance of a nearest-neighbour walk shrinks fast: most entries are dead when they surface).  Leaves gather the three quads of the record; the
// sphere branch (a square root and a division) sits behind a wave ballot, as in trace_leaf_step.  Node steps and leaf steps alternate, each for the
// lanes that are at one.  The stack is PointStack (tirt_point_walk.h) with entries of 8 bytes (child code, lb2): the first CP_LDS_DEPTH of a lane live in LDS
// ([entry][lane]), the rest of its stack_size in the context's spill buffer ([entry][global thread]) -- DESIGN.md "Closest point" has the sizes and why 16.  An entry beyond stack_size
// is dropped and the query counted in DevCounters::stack_overflow (tirt_stats: TIRT_ERR_STACK), as a ray's.
// The walk starts at root_qcode (a leaf code in a one-primitive scene).  Every analytic sphere is below it: its slot carries its padded box
// (shapes_boxed) or the whole grid, and both contain the sphere, as every ancestor's box does -- the chain nodes at far_qcode exist for rays, whose
// sphere test can answer from outside the padded box; a closest point lies ON the sphere.  Spot and laser leaves are reached and skipped.
// A query with a NaN or infinite coordinate finds nothing by the definition (every D2 is NaN or +inf): it does not walk.
//
// WHY THE CULL IS CONSERVATIVE: the head of tirt_point_walk.h, beside the margin it is about (PointMargin, which k_sd_build shares, as it does the stack).
#include "tirt_internal.h"
#include "tirt_closest_point.h"
#include "tirt_point_walk.h"

namespace tirt {

constexpr int CP_WAVES_PER_CU = 20;          // persistent blocks per CU at most: what 8 KiB of LDS each admits (62 VGPRs would admit 32)

typedef unsigned CpEntry __attribute__((ext_vector_type(2)));      // a stack entry: (child code, bits of lb2)

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

TD void cp_load_query(const CpArgs &a, int q, v3 &p, float &lim2)
{
    const float *r = a.points + (int64_t)q * a.point_stride;
    p = V(r[0], r[1], r[2]);
    lim2 = cp_limit2(a.dmax ? a.dmax[(int64_t)q * a.dmax_stride] : a.dmax_all);
}

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
    const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
    const int prim = __float_as_int(tc.w);
    const v3 pa = V(ta.x, ta.y, ta.z);
    CpPoint r; r.d2 = __int_as_float(0x7fc00000); r.q = V(0.0f, 0.0f, 0.0f); r.u = 0.0f; r.v = 0.0f;      // spot / laser: no surface, a NaN D2 is never accepted
    if (is_tri) r = cp_triangle(p, pa, V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
    const bool sph = !is_tri && (int)tb.y == SHAPE_SPHERE;
    if (__builtin_amdgcn_ballot_w64(sph) != 0ull) { if (sph) r = cp_sphere(p, pa, tb.x); }
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
        const bool finite = absf(p.x) < best2 && absf(p.y) < best2 && absf(p.z) < best2;      // false for NaN and +-inf
        const float m = pm.margin(b, p);
        float cut = lim2;                       // min(best2, lim2): best2 starts at +inf
        int cur = (live && finite && lim2 >= 0.0f) ? b.root_qcode : CP_SENT;
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        // the next entry that can still win, or CP_SENT; most are dead by the time they surface
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
                // kept: a child that is there and can still win (never culled on equality).  The flag travels with the child through the sort, so
                // a kept child whose lb2 overflowed to +inf (a query ~1e19 away, cut = +inf) sorts behind the dropped ones and is still pushed
#define CP_BOX(i, X, Y, Z, code_)                                                                   \
                do {                                                                                \
                    const float ex__ = CP_AXIS_GAP(b, m, X, 0, p.x), ey__ = CP_AXIS_GAP(b, m, Y, 1, p.y), ez__ = CP_AXIS_GAP(b, m, Z, 2, p.z); \
                    const float s__ = (ex__ * ex__ + ey__ * ey__) + ez__ * ez__;                    \
                    c##i = (int)(code_);                                                            \
                    k##i = (c##i != TR_EMPTY) && !(s__ > cut);                                      \
                    l##i = k##i ? s__ : MISS;                                                       \
                } while (0)
                CP_EACH_CHILD(CP_BOX);
#define CP_CE(la, ca, ka, lb, cb, kb)                                                               \
                do {                                                                                \
                    const bool s__ = (lb) < (la);                                                   \
                    const float lo__ = s__ ? (lb) : (la), hi__ = s__ ? (la) : (lb);                 \
                    const int clo__ = s__ ? (cb) : (ca), chi__ = s__ ? (ca) : (cb);                 \
                    const bool klo__ = s__ ? (kb) : (ka), khi__ = s__ ? (ka) : (kb);                \
                    la = lo__; lb = hi__; ca = clo__; cb = chi__; ka = klo__; kb = khi__;           \
                } while (0)
                CP_CE(l0, c0, k0, l1, c1, k1); CP_CE(l2, c2, k2, l3, c3, k3); CP_CE(l0, c0, k0, l2, c2, k2); CP_CE(l1, c1, k1, l3, c3, k3); CP_CE(l1, c1, k1, l2, c2, k2);
                if (k3) st.push(CpEntry{(unsigned)c3, __float_as_uint(l3)});
                if (k2) st.push(CpEntry{(unsigned)c2, __float_as_uint(l2)});
                if (k1) st.push(CpEntry{(unsigned)c1, __float_as_uint(l1)});
                cur = k0 ? c0 : pop_live();
            }
            // ---- leaf step: the lanes that are at a leaf
            const bool at_leaf = cur < 0 && cur != CP_SENT;
            if (__builtin_amdgcn_ballot_w64(at_leaf) != 0ull) {
                if (at_leaf) {
                    const int code = ~cur;
                    if (COUNT) nleaf += 1;
                    cp_test_record(b, leaf_slot(code), leaf_is_tri(code), p, lim2, best2, best_prim, bp);
                    cut = __builtin_fminf(best2, lim2);
                    cur = pop_live();
                }
            }
        }
        if (live) cp_store(a, q, best2, best_prim, bp, nbox, nleaf, COUNT);
        if constexpr (SIGNED) { if (live) sd_store(a, q, p, best_prim, bp); }
        if (st.overflow) n_over++;
    }
    n_over = wave_sum(n_over);
    if (lane == 0 && n_over && a.ctr) atomicAdd(&a.ctr->stack_overflow, n_over);
}

// `n` queries in chunks of `chunk` on the context's stream; every pointer is device memory (or null)
static int cp_chunks(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all,
                     int stack_size, int flags, int chunk, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                     float *out_uv, int64_t uv_stride, int2 *counts, float *out_sd = nullptr)      // out_sd: the SIGNED kernels (the table stands: sd_table_ensure)
{
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    const bool scan = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0;
    CpArgs a = {};
    a.bvh = bvh_view(c);
    a.primitive = c->primitive.as<int>(); a.prim_slot = c->prim_slot.as<int>(); a.n_prim = c->n;
    a.point_stride = point_stride; a.dmax_stride = dmax_stride; a.dmax_all = dmax_all;
    a.stack_size = stack_size; a.point_out_stride = point_out_stride; a.uv_stride = uv_stride;
    a.ctr = c->dev_counters.as<DevCounters>();
    const bool sgn = out_sd != nullptr;
    if (sgn) { a.sd_tab = c->sd_tab.as<float4>(); a.sd_state = c->sd_state.as<int>(); }
    // the walk's grid: a lane for every query of a chunk, as far as the stacks allow (the scan has no stack)
    int grid_max = 0;
    if (!scan) if (int rc = point_walk_launch_shape(c, stack_size, CP_WAVES_PER_CU, ((int64_t)(n < chunk ? n : chunk) + CP_BLOCK - 1) / CP_BLOCK, grid_max, a.spill)) return rc;
    for (int64_t base = 0; base < n; base += chunk) {
        const int m = (int)(n - base < chunk ? n - base : chunk);
        a.n = m;
        a.points = points + base * point_stride; a.dmax = dmax ? dmax + base * dmax_stride : nullptr;
        a.out_d2 = out_d2 ? out_d2 + base : nullptr; a.out_prim = out_prim ? out_prim + base : nullptr;
        a.out_point = out_point ? out_point + base * point_out_stride : nullptr; a.out_uv = out_uv ? out_uv + base * uv_stride : nullptr;
        a.counts = counts ? counts + base : nullptr;
        a.out_sd = sgn ? out_sd + base : nullptr;
        const int blocks = (m + CP_BLOCK - 1) / CP_BLOCK;
#define CP_LAUNCH(K, G)                                                                             \
        do {                                                                                        \
            if (sgn) { if (cnt) hipLaunchKernelGGL((K<true, true>), dim3(G), dim3(CP_BLOCK), 0, c->stream, a);      \
                       else hipLaunchKernelGGL((K<false, true>), dim3(G), dim3(CP_BLOCK), 0, c->stream, a); }       \
            else { if (cnt) hipLaunchKernelGGL((K<true, false>), dim3(G), dim3(CP_BLOCK), 0, c->stream, a);         \
                   else hipLaunchKernelGGL((K<false, false>), dim3(G), dim3(CP_BLOCK), 0, c->stream, a); }          \
        } while (0)
        if (scan) CP_LAUNCH(k_cp_scan, blocks);
        else { const int g = blocks < grid_max ? blocks : grid_max; CP_LAUNCH(k_cp_walk, g); }
#undef CP_LAUNCH
    }
    return TIRT_OK;
}

// tirt_query_closest_point, and with `sgn` tirt_query_signed_distance (the same checks, out_sd beside the other outputs, the table made first)
static int query_closest_point(tirt_ctx *c, const char *fn, bool sgn, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride,
                               float dmax_all, int stack_size, int flags, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                               float *out_uv, int64_t uv_stride, int32_t *counts, float *out_sd, void *stream)
{
    const std::string f = std::string(fn) + ": ";
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    TIRT_REQUIRE(point_stride >= 3, f + "point_stride < 3 (floats per point)");
    TIRT_REQUIRE(!out_point || point_out_stride >= 3, f + "point_out_stride < 3 (floats per closest point)");
    TIRT_REQUIRE(!out_uv || uv_stride >= 2, f + "uv_stride < 2");
    TIRT_REQUIRE(!dmax || dmax_stride >= 1, f + "dmax_stride < 1");
    TIRT_REQUIRE(!counts || ((uintptr_t)counts & 7) == 0, f + "counts must be 8-byte aligned");
    if (int rc = require_caller_stream(c, fn, stream, "queries")) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, f + "null points");
    TIRT_REQUIRE(!sgn || out_sd, f + "null out_sd");
    if (int rc = require_device_ptr(c, points, (f + "points").c_str())) return rc;
    if (dmax) if (int rc = require_device_ptr(c, dmax, (f + "dmax").c_str())) return rc;
    if (out_d2) if (int rc = require_device_ptr(c, out_d2, (f + "out_d2").c_str())) return rc;
    if (out_prim) if (int rc = require_device_ptr(c, out_prim, (f + "out_prim").c_str())) return rc;
    if (out_point) if (int rc = require_device_ptr(c, out_point, (f + "out_point").c_str())) return rc;
    if (out_uv) if (int rc = require_device_ptr(c, out_uv, (f + "out_uv").c_str())) return rc;
    if (sgn) if (int rc = require_device_ptr(c, out_sd, (f + "out_sd").c_str())) return rc;
    const bool want_counts = counts && (flags & TIRT_COUNT_NODES);
    if (want_counts) if (int rc = require_device_ptr(c, counts, (f + "counts").c_str())) return rc;
    const int chunk = (int)(n < (int64_t)c->query_chunk ? n : (int64_t)c->query_chunk);
    if (int rc = query_begin(c, stream)) return rc;
    if (sgn) if (int rc = sd_table_ensure(c, stack_size)) return rc;      // (on the context's stream, after the caller's work: no host sync)
    if (int rc = cp_chunks(c, points, n, point_stride, dmax, dmax_stride, dmax_all, stack_size, flags, chunk, out_d2, out_prim, out_point,
                           point_out_stride, out_uv, uv_stride, want_counts ? (int2 *)counts : nullptr, sgn ? out_sd : nullptr)) return rc;
    return query_end(c, stream);
}

// host arrays staged in the context's query scratch (query_mem: 52 bytes per query, 56 with out_sd), one chunk of all of them, back with a sync.
// `sgn`: tirt_signed_distance -- the table is made first and, the stream being waited for anyway, its build's verdict read: TIRT_ERR_STACK, no answers
static int closest_point_host(tirt_ctx *c, const char *fn, bool sgn, const float *points, int n, const float *dmax, int stack_size, int flags, float *out_d2,
                              int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts, float *out_sd)
{
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, std::string(fn) + ": null points");
    TIRT_REQUIRE(!sgn || out_sd, std::string(fn) + ": null out_sd");
    const size_t N = (size_t)n, bytes = N * (sgn ? 56 : 52);
    hipStream_t st = c->stream;
    if (bytes > c->query_mem.bytes) {
        TIRT_HIP(hipStreamSynchronize(st));
        if (c->query_mem.ensure(bytes)) return TIRT_ERR_HIP;
    }
    // counts [n][2] first (8-byte aligned), then points [n][3], dmax [n], d2 [n], prim [n], point [n][3], uv [n][2], sd [n]
    int2 *d_counts = c->query_mem.as<int2>();
    float *d_points = (float *)(d_counts + N), *d_dmax = d_points + 3 * N, *d_d2 = d_dmax + N;
    int32_t *d_prim = (int32_t *)(d_d2 + N);
    float *d_point = (float *)(d_prim + N), *d_uv = d_point + 3 * N, *d_sd = d_uv + 2 * N;
    const bool want_counts = counts && (flags & TIRT_COUNT_NODES);
    TIRT_HIP(hipMemcpyAsync(d_points, points, sizeof(float) * 3 * N, hipMemcpyHostToDevice, st));
    if (dmax) TIRT_HIP(hipMemcpyAsync(d_dmax, dmax, sizeof(float) * N, hipMemcpyHostToDevice, st));
    if (sgn) if (int rc = sd_table_ensure(c, stack_size)) return rc;
    if (int rc = cp_chunks(c, d_points, n, 3, dmax ? d_dmax : nullptr, 1, __builtin_inff(), stack_size, flags, n, d_d2, d_prim, d_point, 3, d_uv, 2,
                           want_counts ? d_counts : nullptr, sgn ? d_sd : nullptr)) return rc;
    if (sgn) if (int rc = sd_table_verdict(c, fn)) return rc;      // (waits for the stream)
    if (out_d2) TIRT_HIP(hipMemcpyAsync(out_d2, d_d2, sizeof(float) * N, hipMemcpyDeviceToHost, st));
    if (out_prim) TIRT_HIP(hipMemcpyAsync(out_prim, d_prim, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    if (out_point) TIRT_HIP(hipMemcpyAsync(out_point, d_point, sizeof(float) * 3 * N, hipMemcpyDeviceToHost, st));
    if (out_uv) TIRT_HIP(hipMemcpyAsync(out_uv, d_uv, sizeof(float) * 2 * N, hipMemcpyDeviceToHost, st));
    if (want_counts) TIRT_HIP(hipMemcpyAsync(counts, d_counts, sizeof(int2) * N, hipMemcpyDeviceToHost, st));
    if (sgn) TIRT_HIP(hipMemcpyAsync(out_sd, d_sd, sizeof(float) * N, hipMemcpyDeviceToHost, st));
    TIRT_HIP(hipStreamSynchronize(st));
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
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
