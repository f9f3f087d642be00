// tirt_winding.hip -- the generalized winding number of query points (tirt_query_winding_number / tirt_winding_number / tirt_winding_prepare /
// tirt_winding_table_download / tirt_kat_winding / tirt_kat_winding_host, include/tirt.h "Winding number").  No reference counterpart.
//
//   k_wn_level      the integer moments of every 4-wide node, bottom-up, one launch per level of the tree: a lane per node adds the sums of its inner
//                   children (made by the launch before) and the terms of its triangle leaves (wn_moment_add)
//   k_wn_convert    a lane per (node, child slot): the fp32 row of the slot's inner child from that child's sums and the slot's decoded box (wn_moment_row)
//   k_wn_scan       one query per lane over all n primitive records in primitive-id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick on the device
//   k_wn_walk       one query per lane over the quantised 4-wide nodes `cnode` (BvhView): the hot path
// The last two are templates on <COUNT>.  Both add wn_quant(wn_triangle) / wn_quant(wn_sphere) (tirt_winding.h) per primitive in 64-bit integers, and the walk
// replaces the primitives beneath an inner child by the two far-field terms of its moment row iff d2 > beta^2 r2: a sum of integers, so neither the order
// of the visits nor the numbering of the nodes changes a bit, and with beta = +inf (no child is ever approximated) the walk's sum IS the scan's.
//
// THE WALK.  Lane l of a block holds query base + l and the blocks stride over the chunk; node steps and leaf steps alternate behind wave ballots, each for
// the lanes that are at one (a wave is a block: no barrier).  A node step reads the four child codes (the planes are not needed: r2 of the table row stands
// for the box), and per slot: empty -- skipped; a leaf -- waits for a leaf step; an inner child -- the first quad of its row (p~, r2), then either the
// other three quads and the two terms, or the child waits for a node step.  Nothing is sorted and nothing is culled (k_sd_build's kind of loop).  The stack
// is PointStack<int> (tirt_point_walk.h): CP_LDS_DEPTH entries per lane in LDS, the rest of stack_size in the context's spill buffer.  An entry that does
// not fit is a subtree the sum misses: the query answers NaN and counts in DevCounters::stack_overflow (tirt_stats: TIRT_ERR_STACK).
// The walk starts at root_qcode (a leaf code in a one-primitive scene); every primitive has one leaf below it (the chain nodes at far_qcode are not entered).
// An analytic sphere beneath an approximated child contributes nothing to the moments and nothing is owed: d2 > r2 puts q outside the ball about p~
// that holds the child's box, the box holds the sphere, and the sphere's term outside itself is 0.
// A query with a NaN or infinite coordinate answers NaN and does not walk.
#include "tirt_internal.h"
#include "tirt_winding.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"

namespace tirt {

constexpr int WN_BUILD_BLOCK = 128;

struct WnBuildArgs {
    const uint4 *cnode; const float4 *tri; int n_nodes;
    float grid_min[3], cell[3];
    WnScale scale;
    long long *sums; float4 *tab;
};

// the sums of the nodes first .. first + count - 1 (one level of the tree; the levels below it stand)
__global__ __launch_bounds__(WN_BUILD_BLOCK) void k_wn_level(WnBuildArgs a, int first, int count)
{
    const int t = blockIdx.x * WN_BUILD_BLOCK + threadIdx.x;
    if (t >= count) return;
    const int node = first + t;
    const uint4 q3 = a.cnode[(size_t)node * 4 + 3];
    const int code[4] = {(int)q3.x, (int)q3.y, (int)q3.z, (int)q3.w};
    const v3 gm = V(a.grid_min[0], a.grid_min[1], a.grid_min[2]);
    long long m[WN_MOMENTS];
#pragma unroll
    for (int k = 0; k < WN_MOMENTS; k++) m[k] = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (code[c] == TR_EMPTY) continue;
        if (code[c] >= 0) {
            if (code[c] > node && code[c] < a.n_nodes) {      // (a child lies on the next level: always; a record that says otherwise is not followed)
                const long long *s = a.sums + (size_t)code[c] * WN_MOMENTS;
#pragma unroll
                for (int k = 0; k < WN_MOMENTS; k++) m[k] += s[k];
            }
        } else if (leaf_is_tri(~code[c])) {
            const float4 *tp = a.tri + (size_t)leaf_slot(~code[c]) * TRI_STRIDE;
            const float4 ta = tp[0], tb = tp[1], tc = tp[2];
            wn_moment_add(m, V(ta.x, ta.y, ta.z), V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z), gm, a.scale);
        }
    }
    long long *o = a.sums + (size_t)node * WN_MOMENTS;
#pragma unroll
    for (int k = 0; k < WN_MOMENTS; k++) o[k] = m[k];
}

// the rows: t = 4 * node + slot.  A slot that names no inner node gets a row of zeros
__global__ __launch_bounds__(WN_BUILD_BLOCK) void k_wn_convert(WnBuildArgs a)
{
    const int t = blockIdx.x * WN_BUILD_BLOCK + threadIdx.x;
    if (t >= 4 * a.n_nodes) return;
    const int node = t >> 2, c = t & 3;
    const unsigned *w = (const unsigned *)(a.cnode + (size_t)node * 4);
    const int code = (int)w[12 + c];
    float row[4 * WN_ROW_QUADS];
#pragma unroll
    for (int k = 0; k < 4 * WN_ROW_QUADS; k++) row[k] = 0.0f;
    if (code > node && code < a.n_nodes) {
        float mn[3], mx[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {      // the decode of CP_BOX_GAP
            const cp_h2v h = __builtin_bit_cast(cp_h2v, w[3 * c + k]);
            mn[k] = a.grid_min[k] + (float)h.x * a.cell[k]; mx[k] = a.grid_min[k] + (float)h.y * a.cell[k];
        }
        long long m[WN_MOMENTS];
        const long long *s = a.sums + (size_t)code * WN_MOMENTS;
#pragma unroll
        for (int k = 0; k < WN_MOMENTS; k++) m[k] = s[k];
        wn_moment_row(m, V(a.grid_min[0], a.grid_min[1], a.grid_min[2]), V(mn[0], mn[1], mn[2]), V(mx[0], mx[1], mx[2]), a.scale, row);
    }
    float4 *o = a.tab + (size_t)t * WN_ROW_QUADS;
#pragma unroll
    for (int k = 0; k < WN_ROW_QUADS; k++) o[k] = make_float4(row[4 * k], row[4 * k + 1], row[4 * k + 2], row[4 * k + 3]);
}

struct WnArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // the scan: kind and record slot of primitive i
    const float *points; int64_t point_stride;          // this chunk's first row
    int n;                                              // queries of this chunk
    int stack_size;
    int *spill;                                         // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    float beta2;                                        // beta * beta, formed once on the host (+inf: nothing is approximated)
    const float4 *tab;                                  // [wide_nodes * 4][WN_ROW_QUADS]
    float *out_w; int2 *counts;
    DevCounters *ctr;
};

// the quantised term of the record in `slot`: the kind comes from the caller (the leaf code's shape bit, or the primitive table); spot / laser: 0
TD long long wn_record(const BvhView &b, int slot, bool is_tri, const v3 p)
{
    const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
    float om = 0.0f;
    if (is_tri) om = wn_triangle(p, V(ta.x, ta.y, ta.z), V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
    else if ((int)tb.y == SHAPE_SPHERE) om = wn_sphere(p, V(ta.x, ta.y, ta.z), tb.x);
    return wn_quant(om);
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_wn_scan(WnArgs a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    const float *r = a.points + (int64_t)q * a.point_stride;
    const v3 p = V(r[0], r[1], r[2]);
    long long S = 0;
    const bool finite = cp_finite3(p);
    if (finite) for (int i = 0; i < a.n_prim; i++) S += wn_record(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, p);
    a.out_w[q] = finite ? wn_result(S) : __int_as_float(0x7fc00000);
    if (COUNT && a.counts) a.counts[q] = make_int2(0, finite ? a.n_prim : 0);
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_wn_walk(WnArgs a)
{
    __shared__ int stk[CP_LDS_DEPTH * CP_BLOCK];      // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    unsigned long long n_over = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        v3 p = V(0.0f, 0.0f, 0.0f);
        if (live) { const float *r = a.points + (int64_t)q * a.point_stride; p = V(r[0], r[1], r[2]); }
        const float inf = __int_as_float(0x7f800000);
        const bool finite = CP_FINITE3(p, inf);
        int cur = (live && finite) ? b.root_qcode : CP_SENT;
        long long S = 0;
        unsigned nbox = 0, nleaf = 0;
        PointStack<int> st(stk, a.spill, a.stack_size, lane);
        // a child that is there: an inner one far enough away adds its two terms, every other one waits -- the first as the next step, the others on the stack
#define WN_CHILD(i, X, Y, Z, code_)                                                                 \
        do {                                                                                        \
            const int c__ = (int)(code_);                                                           \
            if (c__ != TR_EMPTY) {                                                                  \
                bool wait__ = true;                                                                 \
                if (c__ >= 0) {                                                                     \
                    const float4 r0 = rows[WN_ROW_QUADS * i];                                       \
                    const v3 d__ = V(r0.x - p.x, r0.y - p.y, r0.z - p.z);                           \
                    const float d2__ = dot(d__, d__);                                               \
                    if (d2__ > a.beta2 * r0.w) {                                                    \
                        const float4 r1 = rows[WN_ROW_QUADS * i + 1], r2 = rows[WN_ROW_QUADS * i + 2], r3 = rows[WN_ROW_QUADS * i + 3]; \
                        const float C__[9] = {r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w}; \
                        float t0__, t1__;                                                           \
                        wn_far_terms(d__, d2__, V(r1.x, r1.y, r1.z), C__, t0__, t1__);              \
                        S += wn_quant(t0__) + wn_quant(t1__);                                       \
                        wait__ = false;                                                             \
                    }                                                                               \
                }                                                                                   \
                if (wait__) { if (nxt == CP_SENT) nxt = c__; else st.push(c__); }                   \
            }                                                                                       \
        } while (0)

        while (__builtin_amdgcn_ballot_w64(cur != CP_SENT) != 0ull) {
            // ---- node step: the lanes that are at an inner node
            if (cur >= 0) {
                const uint4 q3 = b.cnode[(size_t)cur * 4 + 3];
                const float4 *rows = a.tab + (size_t)cur * (4 * WN_ROW_QUADS);
                if (COUNT) nbox += 4;
                int nxt = CP_SENT;
                WN_CHILD(0, 0, 0, 0, q3.x); WN_CHILD(1, 0, 0, 0, q3.y); WN_CHILD(2, 0, 0, 0, q3.z); WN_CHILD(3, 0, 0, 0, q3.w);
                cur = nxt;
                if (cur == CP_SENT && !st.empty()) cur = st.pop();
            }
            // ---- leaf step: the lanes that are at a leaf
            const bool at_leaf = cur < 0 && cur != CP_SENT;
            if (__builtin_amdgcn_ballot_w64(at_leaf) != 0ull) {
                if (at_leaf) {
                    if (COUNT) nleaf += 1;
                    const int code = ~cur;
                    S += wn_record(b, leaf_slot(code), leaf_is_tri(code), p);
                    cur = st.empty() ? CP_SENT : st.pop();
                }
            }
        }
#undef WN_CHILD
        if (live) {
            a.out_w[q] = (finite && !st.overflow) ? wn_result(S) : __int_as_float(0x7fc00000);
            if (COUNT && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
        }
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

// the table's build, queued on the context's stream
static int wn_table_build(tirt_ctx *c)
{
    const size_t nodes = (size_t)c->wide_nodes;
    const size_t sums_bytes = sizeof(long long) * WN_MOMENTS * nodes, tab_bytes = sizeof(float4) * WN_ROW_QUADS * 4 * nodes;
    if (sums_bytes > c->wn_sums.bytes || tab_bytes > c->wn_tab.bytes || !c->wn_tab.p || !c->wn_sums.p) {      // growing frees the old buffers, which queued work may still use
        TIRT_HIP(hipStreamSynchronize(c->stream));
        if (c->wn_sums.ensure(sums_bytes) || c->wn_tab.ensure(tab_bytes)) return TIRT_ERR_HIP;
    }
    c->wn_tab_valid = false;
    if (nodes) {
        TIRT_REQUIRE(c->wide_level_off.size() >= 2 && c->wide_level_off.back() == c->wide_nodes, "winding number: the levels of the 4-wide tree are not known");
        WnBuildArgs a = {};
        a.cnode = c->cnode.as<uint4>(); a.tri = c->tri.as<float4>(); a.n_nodes = c->wide_nodes;
        float cell_max = c->grid_cell[0];
        for (int k = 0; k < 3; k++) { a.grid_min[k] = c->grid_min[k]; a.cell[k] = c->grid_cell[k]; if (c->grid_cell[k] > cell_max) cell_max = c->grid_cell[k]; }
        a.scale = WnScale::of(cell_max * (2.0f * TR_GRID_HALF));
        a.sums = c->wn_sums.as<long long>(); a.tab = c->wn_tab.as<float4>();
        for (int L = (int)c->wide_level_off.size() - 2; L >= 0; L--) {
            const int first = c->wide_level_off[L], count = c->wide_level_off[L + 1] - first;
            if (count <= 0) continue;
            hipLaunchKernelGGL(k_wn_level, dim3((count + WN_BUILD_BLOCK - 1) / WN_BUILD_BLOCK), dim3(WN_BUILD_BLOCK), 0, c->stream, a, first, count);
        }
        hipLaunchKernelGGL(k_wn_convert, dim3((unsigned)((4 * nodes + WN_BUILD_BLOCK - 1) / WN_BUILD_BLOCK)), dim3(WN_BUILD_BLOCK), 0, c->stream, a);
        TIRT_HIP(hipGetLastError());
    }
    c->wn_tab_valid = true;
    return TIRT_OK;
}

int wn_table_ensure(tirt_ctx *c)
{
    if (c->wn_tab_valid) return TIRT_OK;
    return wn_table_build(c);
}

// `n` queries in chunks of `chunk` on the context's stream; every pointer is device memory (or null); the table stands (wn_table_ensure)
static int wn_chunks(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, float beta, int stack_size, int flags, int chunk, float *out_w, int2 *counts)
{
    const bool scan = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0;
    WnArgs a = {};
    a.point_stride = point_stride; a.beta2 = beta * beta; a.tab = c->wn_tab.as<float4>();
    return point_walk_chunks(c, a, n, chunk, scan, stack_size, [&](int64_t base, int m, int, int grid) {
        a.n = m;
        a.points = points + base * point_stride;
        a.out_w = out_w + base; a.counts = counts ? counts + base : nullptr;
        with_bool(cnt, [&](auto C) {
            constexpr bool COUNT = decltype(C)::value;
            if (scan) hipLaunchKernelGGL((k_wn_scan<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
            else hipLaunchKernelGGL((k_wn_walk<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
        });
    });
}

static int wn_check_beta(const char *fn, float beta)
{
    TIRT_REQUIRE(beta >= 1.0f, std::string(fn) + ": beta must be >= 1 or +inf");
    return TIRT_OK;
}

// one row per thread through wn_kat_row (tirt_winding.h): the text tirt_kat_winding_host runs on the host
__global__ void k_kat_winding(const float *in, int n, int is_sphere, uint32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    wn_kat_row(in + (size_t)i * (is_sphere ? WN_KAT_SPH : WN_KAT_TRI), is_sphere, out + (size_t)i * WN_KAT_OUT);
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_winding_number(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, float beta, int stack_size, int flags, float *out_w,
                              int32_t *counts, void *stream)
{
    CTX(c);
    const char *fn = "tirt_query_winding_number";
    const std::string f = std::string(fn) + ": ";
    if (int rc = point_query_checks(c, fn, n, stack_size, flags, {{true, point_stride, 3, "point_stride < 3 (floats per point)"}}, counts, stream)) return rc;
    if (int rc = wn_check_beta(fn, beta)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, f + "null points");
    TIRT_REQUIRE(out_w, f + "null out_w");
    const QueryPlan pl = query_plan(c, n, flags, counts);
    if (int rc = require_device_ptrs(c, f, {{points, "points"}, {out_w, "out_w"}, {pl.counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = wn_table_ensure(c)) return rc;      // (on the context's stream, after the caller's work: no host sync)
    if (int rc = wn_chunks(c, points, n, point_stride, beta, stack_size, flags, pl.chunk, out_w, pl.counts)) return rc;
    return query_end(c, stream);
}

int tirt_winding_number(tirt_ctx *c, const float *points, int n, float beta, int stack_size, int flags, float *out_w, int32_t *counts)
{
    CTX(c);
    const char *fn = "tirt_winding_number";
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (int rc = wn_check_beta(fn, beta)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, std::string(fn) + ": null points");
    TIRT_REQUIRE(out_w, std::string(fn) + ": null out_w");
    const size_t N = (size_t)n;
    QueryStage s(c);
    const auto k_points = s.in(points, 3 * N);
    const auto k_w = s.out(out_w, N);
    const auto k_counts = s.out_counts(counts, flags, N);
    if (int rc = s.begin()) return rc;
    if (int rc = wn_table_ensure(c)) return rc;
    if (int rc = wn_chunks(c, s.ptr(k_points), n, 3, beta, stack_size, flags, n, s.ptr(k_w), s.ptr(k_counts))) return rc;
    return s.finish();
}

int tirt_winding_prepare(tirt_ctx *c)
{
    CTX(c);
    TIRT_REQUIRE(c->built, "tirt_winding_prepare: LBVH not built");
    if (int rc = wn_table_ensure(c)) return rc;
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int tirt_winding_table_download(tirt_ctx *c, float *table, int64_t *sums, int32_t info[2])
{
    CTX(c);
    TIRT_REQUIRE(c->built && info, "tirt_winding_table_download: LBVH not built / null pointer");
    if (int rc = wn_table_ensure(c)) return rc;
    const size_t nodes = (size_t)c->wide_nodes;
    if (table && nodes) TIRT_HIP(hipMemcpyAsync(table, c->wn_tab.p, sizeof(float4) * WN_ROW_QUADS * 4 * nodes, hipMemcpyDeviceToHost, c->stream));
    if (sums && nodes) TIRT_HIP(hipMemcpyAsync(sums, c->wn_sums.p, sizeof(long long) * WN_MOMENTS * nodes, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    float cell_max = c->grid_cell[0];
    for (int k = 1; k < 3; k++) if (c->grid_cell[k] > cell_max) cell_max = c->grid_cell[k];
    info[0] = c->wide_nodes; info[1] = WnScale::of(cell_max * (2.0f * TR_GRID_HALF)).e;
    return TIRT_OK;
}

int tirt_kat_winding(tirt_ctx *c, const float *in, int n, int is_sphere, uint32_t *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_winding: null pointer or negative n");
    TIRT_REQUIRE(is_sphere == 0 || is_sphere == 1, "tirt_kat_winding: is_sphere is 0 (triangle rows of 12 floats) or 1 (sphere rows of 7)");
    CTX(c);
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_winding", {{in, kat_row_bytes(n, is_sphere ? WN_KAT_SPH : WN_KAT_TRI)}}, out, kat_row_bytes(n, WN_KAT_OUT), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_winding, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)din[0], n, is_sphere, (uint32_t *)dout);
    });
}

// host only, no context: the same rows through the same text (wn_kat_row), compiled for the host
int tirt_kat_winding_host(const float *in, int n, int is_sphere, uint32_t *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_winding_host: null pointer or negative n");
    TIRT_REQUIRE(is_sphere == 0 || is_sphere == 1, "tirt_kat_winding_host: is_sphere is 0 (triangle rows of 12 floats) or 1 (sphere rows of 7)");
    for (int i = 0; i < n; i++) wn_kat_row(in + (size_t)i * (is_sphere ? WN_KAT_SPH : WN_KAT_TRI), is_sphere, out + (size_t)i * WN_KAT_OUT);
    return TIRT_OK;
}

}  // extern "C"
