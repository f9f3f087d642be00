// tirt_nearest.hip -- the k nearest primitives of a query point, in order, and the count of all within the bound (tirt_query_nearest / tirt_nearest /
// tirt_kat_nearest_list, include/tirt.h "K nearest primitives").  No reference counterpart: the reference only answers questions that start from a ray.
//
//   k_nn_walk<COUNT, COUNT_ALL>   one query per lane, best-first over the quantised 4-wide nodes `cnode` (BvhView): the hot path
//   k_nn_scan<COUNT>              one query per lane against all n primitive records in primitive-id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick
//   k_nn_resolve                  the lists in the caller's [N, k] layout with the padding, the counts, and Q, u, v formed again from the records
//
// Nothing but cp_triangle / cp_sphere (tirt_closest_point.h) decides a primitive's D2, and nothing but NnList (tirt_nearest.h) whether and where it goes in
// the list.  N is a set and the list the first k of a total order on (D2, prim): neither depends on the order of the visits, so the walk returns the
// scan's bits if and only if it never skips a primitive that would have been accepted.
//
// THE WALK is point_walk (tirt_point_walk.h), as k_cp_walk's: lo == hi == the query point, the margin of PointMargin, PointStack<CpEntry>.  THE CUT is the list's:
//     cut = lim2                                   while the list has room (its threshold is "nothing", D2 = +inf)
//     cut = min(lim2, D2 of the worst entry)       once the list holds k
//     cut = lim2                                   always under COUNT_ALL (the caller wants |N|: every element of N has to be met)
// The leaf offers the record to the set and the list (nn_offer) and returns that.  The argument of tirt_point_walk.h holds with it: a skipped subtree holds
// only primitives with D2 > cut, and such a primitive is no element of N (cut <= lim2), or sorts behind the worst entry of a full list whatever its id
// (cut = that entry's D2, and the threshold only ever moves forward).  A primitive whose D2 EQUALS the threshold's is below no skipped node; it joins if
// its id is smaller (cp_accept).
// The walk starts at root_qcode, as k_cp_walk does (every analytic sphere is below it), and never enters the chain nodes at far_qcode: a leaf is met at
// most once, so no primitive appears twice in a list or in the count.  Spot and laser leaves are reached and skipped (a NaN D2).  A query with a NaN or
// infinite coordinate, or a negative or NaN bound, has N = {}: it does not walk.
// THE LIST lives in the context's chunk scratch as [entry][query] (8 bytes per entry: a wave's access to entry e is contiguous) with its threshold in
// registers; per query the scratch holds 8 k bytes of list and 8 bytes of (entries held, |N|).  Chunks are max(256, query_chunk_rays / max(k, 1)) queries.
// An entry beyond stack_size is dropped and the query counted in DevCounters::stack_overflow (tirt_stats: TIRT_ERR_STACK).
#include <string.h>
#include "tirt_internal.h"
#include "tirt_closest_point.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"
#include "tirt_nearest.h"

namespace tirt {

struct NnArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // kind and record slot of primitive i (the scan and the resolve)
    const float *points; int64_t point_stride;          // this chunk's first row
    const float *dmax; int64_t dmax_stride; float dmax_all;
    int n, k;                                           // queries of this chunk; entries of a list at most
    int stack_size;
    CpEntry *spill;                                     // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    uint2 *list; int2 *meta;                            // [k][stride] entries (bits D2, prim); per query (entries held, |N|)
    size_t stride;                                      // queries of a full chunk: the distance between two entries of one query
    int2 *counts;                                       // TIRT_COUNT_NODES: N_box, N_leaf per query of the chunk (or nullptr)
    DevCounters *ctr;
};

// one query's list in the chunk scratch: entry e of query i at list[e * stride + i], so a wave's access to entry e is one run of 512 bytes
struct NnStore {
    uint2 *p; size_t stride;
    TD NnEntry get(int e) const { const uint2 v = p[(size_t)e * stride]; NnEntry r; r.d2 = __uint_as_float(v.x); r.prim = (int)v.y; return r; }
    TD void set(int e, const NnEntry c) const { p[(size_t)e * stride] = make_uint2(__float_as_uint(c.d2), (unsigned)c.prim); }
};

// a candidate against the set and the list: counts it if it is an element of N, inserts it if it sorts before the threshold
TD void nn_offer(NnList &L, const NnStore &store, float d2, int prim, float lim2, int &count)
{
    if (NnList::member(d2, prim, lim2)) count++;
    if (L.wants(d2, prim, lim2)) { NnEntry e; e.d2 = d2; e.prim = prim; L.insert(store, e); }
}

template <bool COUNT>
__global__ __launch_bounds__(CP_BLOCK) void k_nn_scan(NnArgs a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    v3 p; float lim2;
    cp_load_query(a, q, p, lim2);
    NnList L(a.k);
    const NnStore store = {a.list + q, a.stride};
    int count = 0;
    for (int i = 0; i < a.n_prim; i++) {
        int prim;
        const CpPoint r = cp_record(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, p, prim);
        nn_offer(L, store, r.d2, prim, lim2, count);
    }
    a.meta[q] = make_int2(L.n, count);
    if (COUNT && a.counts) a.counts[q] = make_int2(0, a.n_prim);
}

template <bool COUNT, bool COUNT_ALL>
__global__ __launch_bounds__(CP_BLOCK) void k_nn_walk(NnArgs a)
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
        NnList L(a.k);
        const NnStore store = {a.list + q, a.stride};
        int count = 0;
        const float inf = __int_as_float(0x7f800000);
        const bool finite = CP_FINITE3(p, inf);
        const float m = pm.margin(b, p);
        const int start = (live && finite && lim2 >= 0.0f) ? b.root_qcode : CP_SENT;
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        point_walk<COUNT>(b, st, m, p, p, start, lim2, nbox, nleaf, [&](int code) {      // (the first cut is lim2: the threshold starts at +inf)
            int prim;
            const CpPoint r = cp_record(b, leaf_slot(code), leaf_is_tri(code), p, prim);
            nn_offer(L, store, r.d2, prim, lim2, count);
            return COUNT_ALL ? lim2 : __builtin_fminf(L.thr_d2, lim2);
        });
        if (live) {
            a.meta[q] = make_int2(L.n, count);
            if (COUNT && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
        }
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

// thread (i, j): entry j of query i of the chunk into the caller's arrays (at query `base` + i); j == 0 also writes the count.  Q, u, v: cp_triangle /
// cp_sphere on the query and the primitive's record once more -- the function and the operands the walk had, hence its bits.  Padding: (+inf, -1, 0, 0).
__global__ void k_nn_resolve(NnArgs a, int64_t base, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride, float *out_uv,
                             int64_t uv_stride, int32_t *out_count)
{
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int kk = a.k > 0 ? a.k : 1;
    if (id >= (int64_t)a.n * kk) return;
    const int i = (int)(id % a.n), j = (int)(id / a.n);
    const int64_t g = base + i;
    const int2 m = a.meta[i];
    if (j == 0 && out_count) out_count[g] = m.y;
    if (j >= a.k) return;
    float d2 = __int_as_float(0x7f800000); int prim = -1;
    CpPoint r; r.d2 = d2; r.q = V(0.0f, 0.0f, 0.0f); r.u = 0.0f; r.v = 0.0f;
    if (j < m.x) {
        const uint2 e = a.list[(size_t)j * a.stride + i];
        d2 = __uint_as_float(e.x); prim = (int)e.y;
        if (out_point || out_uv) {
            const float *row = a.points + (int64_t)i * a.point_stride;
            const v3 p = V(row[0], row[1], row[2]);
            int id;      // (prim again; an entry of a list has a surface: a shape in it is a sphere)
            r = cp_record(a.bvh, a.prim_slot[prim], a.primitive[(size_t)prim * PRI_VEC] == PRIMITIVE_TRI, p, id);
        }
    }
    const int64_t at = g * a.k + j;
    if (out_d2) out_d2[at] = d2;
    if (out_prim) out_prim[at] = prim;
    if (out_point) { float *o = out_point + at * point_out_stride; o[0] = r.q.x; o[1] = r.q.y; o[2] = r.q.z; }
    if (out_uv) { float *o = out_uv + at * uv_stride; o[0] = r.u; o[1] = r.v; }
}

// Queries per chunk: max(256, query_chunk_rays / max(k, 1)), as tirt_query_hits, so that the scratch -- 8 B x k of list and 8 B of (entries, |N|) per
// query -- stays of the order the other queries' is.
static int nn_chunk_of(const tirt_ctx *c, int64_t n, int k)
{
    int64_t chunk = (int64_t)c->query_chunk / (k > 0 ? k : 1);
    if (chunk < 256) chunk = 256;
    return (int)(n < chunk ? n : chunk);
}

// `n` queries in chunks of `chunk` on the context's stream: walk (or scan), then resolve; every pointer is device memory (or null)
static int nn_chunks(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all, int k,
                     int stack_size, int flags, int chunk, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride, float *out_uv,
                     int64_t uv_stride, int32_t *out_count, int2 *counts)
{
    // the scratch of one chunk: (entries, |N|) per query first (8-byte aligned), then the lists
    if (int rc = query_scratch(c, (size_t)chunk * (8 + 8 * (size_t)k))) return rc;
    const bool scan = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0, count_all = out_count != nullptr;
    NnArgs a = {};
    a.point_stride = point_stride; a.dmax_stride = dmax_stride; a.dmax_all = dmax_all;
    a.k = k;
    a.meta = c->query_mem.as<int2>(); a.list = (uint2 *)(a.meta + chunk); a.stride = (size_t)chunk;
    return point_walk_chunks(c, a, n, chunk, scan, stack_size, [&](int64_t base, int m, int, int grid) {
        a.n = m;
        a.points = points + base * point_stride; a.dmax = dmax ? dmax + base * dmax_stride : nullptr;
        a.counts = counts ? counts + base : nullptr;
        with_bool(cnt, [&](auto C) {
            constexpr bool COUNT = decltype(C)::value;
            if (scan) hipLaunchKernelGGL((k_nn_scan<COUNT>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
            else with_bool(count_all, [&](auto A) { hipLaunchKernelGGL((k_nn_walk<COUNT, decltype(A)::value>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a); });
        });
        const int64_t threads = (int64_t)m * (k > 0 ? k : 1);
        hipLaunchKernelGGL(k_nn_resolve, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, a, base, out_d2, out_prim, out_point,
                           point_out_stride, out_uv, uv_stride, out_count);
    });
}

// (the checks of k and of the outputs need no context: they come first)
#define NN_K_CHECKS(fn)                                                                                                         \
    TIRT_REQUIRE(k >= 0 && k <= TIRT_NEAREST_MAX, fn ": k outside 0..TIRT_NEAREST_MAX (64)");                                   \
    TIRT_REQUIRE(k > 0 || out_count, fn ": k == 0 without out_count (nothing to return)");                                      \
    TIRT_REQUIRE(k == 0 || out_d2 || out_prim || out_point || out_uv || out_count, fn ": no output at all (nothing to return)")

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_nearest(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all, int k,
                       int stack_size, int flags, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride, float *out_uv,
                       int64_t uv_stride, int32_t *out_count, int32_t *counts, void *stream)
{
    const char *fn = "tirt_query_nearest";
    const std::string f = std::string(fn) + ": ";
    NN_K_CHECKS("tirt_query_nearest");
    CTX(c);
    if (int rc = point_query_checks(c, fn, n, stack_size, flags, {{true, point_stride, 3, "point_stride < 3 (floats per point)"},
                                    {out_point != nullptr, point_out_stride, 3, "point_out_stride < 3 (floats per closest point)"},
                                    {out_uv != nullptr, uv_stride, 2, "uv_stride < 2"}, {dmax != nullptr, dmax_stride, 1, "dmax_stride < 1"}}, counts, stream)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, f + "null points");
    int2 *const want_counts = query_plan(c, n, flags, counts).counts;
    if (int rc = require_device_ptrs(c, f, {{points, "points"}, {dmax, "dmax"}, {out_d2, "out_d2"}, {out_prim, "out_prim"}, {out_point, "out_point"}, {out_uv, "out_uv"},
                                            {out_count, "out_count"}, {want_counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = nn_chunks(c, points, n, point_stride, dmax, dmax_stride, dmax_all, k, stack_size, flags, nn_chunk_of(c, n, k), out_d2, out_prim, out_point,
                           point_out_stride, out_uv, uv_stride, out_count, want_counts)) return rc;
    return query_end(c, stream);
}

// host arrays staged in device memory (QueryStage), through the chunks above, back to the host with a sync.  The walk is handed the outputs the caller
// asked for, and no others
int tirt_nearest(tirt_ctx *c, const float *points, int n, const float *dmax, int k, int stack_size, int flags, float *out_d2, int32_t *out_prim,
                 float *out_point, float *out_uv, int32_t *out_count, int32_t *counts)
{
    const char *fn = "tirt_nearest";
    NN_K_CHECKS("tirt_nearest");
    CTX(c);
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    if (n == 0) return TIRT_OK;
    TIRT_REQUIRE(points, std::string(fn) + ": null points");
    const size_t N = (size_t)n, K = (size_t)k;
    QueryStage s(c);
    const auto k_points = s.in(points, 3 * N);
    const auto k_dmax = s.in(dmax, N);
    const auto k_count = s.out(out_count, N, out_count != nullptr);
    const auto k_d2 = s.out(out_d2, K * N, out_d2 != nullptr);
    const auto k_prim = s.out(out_prim, K * N, out_prim != nullptr);
    const auto k_point = s.out(out_point, 3 * K * N, out_point != nullptr);
    const auto k_uv = s.out(out_uv, 2 * K * N, out_uv != nullptr);
    const auto k_counts = s.out_counts(counts, flags, N);
    if (int rc = s.begin()) return rc;
    if (int rc = nn_chunks(c, s.ptr(k_points), n, 3, s.ptr(k_dmax), 1, __builtin_inff(), k, stack_size, flags, nn_chunk_of(c, n, k), s.ptr(k_d2), s.ptr(k_prim),
                           s.ptr(k_point), 3, s.ptr(k_uv), 2, s.ptr(k_count), s.ptr(k_counts))) return rc;
    return s.finish();
}

// host only, no context: candidates (d2[i], prim[i]) in the order given through NnList (tirt_nearest.h), the text k_nn_walk and k_nn_scan run
int tirt_kat_nearest_list(const float *d2, const int32_t *prim, int n, int k, float lim2, float *out_d2, int32_t *out_prim, int32_t *out_info)
{
    TIRT_REQUIRE(out_info && n >= 0 && (n == 0 || (d2 && prim)), "tirt_kat_nearest_list: null pointer or negative n");
    TIRT_REQUIRE(k >= 0 && k <= TIRT_NEAREST_MAX && (k == 0 || (out_d2 && out_prim)), "tirt_kat_nearest_list: k outside 0..TIRT_NEAREST_MAX (64), or no out_d2 / out_prim");
    struct HostList {
        float *d2; int32_t *prim;
        NnEntry get(int e) const { NnEntry r; r.d2 = d2[e]; r.prim = prim[e]; return r; }
        void set(int e, const NnEntry c) const { d2[e] = c.d2; prim[e] = c.prim; }
    } list = {out_d2, out_prim};
    NnList L(k);
    int members = 0;
    for (int i = 0; i < n; i++) {
        TIRT_REQUIRE(prim[i] >= 0, "tirt_kat_nearest_list: a candidate's primitive id is negative");
        if (NnList::member(d2[i], prim[i], lim2)) members++;
        if (L.wants(d2[i], prim[i], lim2)) { NnEntry e; e.d2 = d2[i]; e.prim = prim[i]; L.insert(list, e); }
    }
    for (int j = L.n; j < k; j++) { out_d2[j] = __builtin_inff(); out_prim[j] = -1; }      // the padding of the definition
    out_info[0] = L.n; out_info[1] = members; memcpy(&out_info[2], &L.thr_d2, 4); out_info[3] = L.thr_prim;
    return TIRT_OK;
}

}  // extern "C"
