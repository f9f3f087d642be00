// tirt_pairs.hip -- pair lists: EVERY primitive within a distance of a query point (the fixed-radius neighbour list) and every scene triangle within a distance
// of a query triangle (the contact pair list), as rows of a CSR layout (tirt_query_point_pairs / tirt_query_mesh_pairs / tirt_point_pairs / tirt_mesh_pairs /
// tirt_kat_pairs_host; include/tirt.h "Point pairs" and "Triangle pairs").  No reference counterpart: the reference only answers questions that start from a ray.
//
//   k_pp_walk<COUNT, FILL>, k_tqp_walk<COUNT, FILL>    one query per lane, best-first over the quantised 4-wide nodes `cnode` (BvhView): the hot path
//   k_pp_scan<FILL>, k_tqp_scan<FILL>                  one query per lane against all n primitive records in id order (TIRT_TRAVERSE_EXHAUSTIVE): the yardstick
//   k_pairs_block_sum, k_pairs_scan_sums, k_pairs_scan_add      the row lengths to row_start, in place (tirt_pairs.h "SCAN")
//   k_pairs_order<CODE>                                one wave per row: the row into the definition's order, in place (tirt_pairs.h "ORDER")
//   k_pp_resolve, k_tqp_resolve                        one wave per row: Q, u, v / P, Q of every pair formed again from the records
//
// Nothing but cp_record (points; tirt_point_walk.h) and tq_pair (triangles; tirt_triangle_query.h) decides a pair's D2, nothing but NnList::member
// (tirt_nearest.h) whether it is an element of the row, and nothing but the key (tirt_pairs.h) where it stands in it.  The row is a SET in a total order:
// neither depends on the order of the visits, so the walk returns the scan's bits if and only if it never skips an element.
//
// THE WALK is point_walk (tirt_point_walk.h) with k_nn_walk's set-up for a point and k_tq_walk's for a triangle (the box of T, the largest of the three
// margins).  THE CUT is lim2, always -- k_nn_walk<., COUNT_ALL>'s: every element has to be met.  A skipped subtree holds only primitives with D2 > lim2,
// which are no elements (the heads of tirt_point_walk.h and tirt_triangle_query.h: lb2 <= D2 as computed numbers).  The walk never enters the chain nodes at
// far_qcode: a leaf is met at most once, so no primitive appears twice in a row.
// TWO WALKS.  The counting walk (FILL = false) leaves the number of elements of row q in row_start[q + 1]; the scan turns the lengths into offsets; the
// filling walk (FILL = true) meets the same elements in the same order (the same tree, the same cut) and its lane writes member number idx to
// row_start[q] + idx, guarded by idx < the row's length: whatever a walk does -- a stack overflow drops subtrees --, it never writes outside its row.  A row
// that does not fit the capacity entirely (pairs_row_fits) is not walked a second time.  Neither walk needs scratch: counts and rows live in the caller's arrays.
// THE ORDER PASS sorts each row by its key in place: rows of up to PAIRS_LDS_ROW pairs in LDS (8 KiB of keys, and a byte per pair for the triangles' code),
// longer rows by the same network on the caller's arrays in global memory -- correct for any length, in place, and NOT TUNED: O(len log^2 len) exchanges of
// 64 lanes with a barrier per step, each a global round trip.  Short rows are not tuned either: a row of five pairs still has a wave to itself.
// An entry beyond stack_size is dropped and the query counted in DevCounters::stack_overflow (tirt_stats: TIRT_ERR_STACK), once per walk that dropped one.
#include <string.h>
#include <vector>
#include "tirt_internal.h"
#include "tirt_closest_point.h"
#include "tirt_triangle_query.h"
#include "tirt_point_walk.h"
#include "tirt_query_stage.h"
#include "tirt_nearest.h"
#include "tirt_pairs.h"

namespace tirt {

struct PairArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;      // kind and record slot of primitive i (the scan and the resolve)
    const float *query; int64_t query_stride;           // this launch's first row: a point (3 floats) or a triangle (9: p0, p1, p2)
    const float *dmax; int64_t dmax_stride; float dmax_all;
    int n;                                              // queries of this launch (a chunk)
    int stack_size;
    CpEntry *spill;                                     // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    int64_t *row_start;                                 // of this launch's first query: [q] and [q + 1] are row q's
    int64_t capacity;                                   // pairs the out arrays hold
    float *out_d2; int32_t *out_prim, *out_code;        // the whole arrays: a row's offset is global
    int2 *counts;                                       // TIRT_COUNT_NODES: N_box, N_leaf per query of this launch (or nullptr)
    DevCounters *ctr;
};

// ---- the two kinds of query: what a lane holds, whether it walks, its box and margin, and one record against it
struct PpKind {
    struct Query { v3 p; float lim2; };
    static TD Query idle() { Query t; t.p = V(0.0f, 0.0f, 0.0f); t.lim2 = -1.0f; return t; }
    static TD Query load(const PairArgs &a, int q)
    {
        const float *r = a.query + (int64_t)q * a.query_stride;
        Query t; t.p = V(r[0], r[1], r[2]);
        t.lim2 = cp_limit2(a.dmax ? a.dmax[(int64_t)q * a.dmax_stride] : a.dmax_all);
        return t;
    }
    static TD bool walks(const Query &t) { return cp_finite3(t.p) && t.lim2 >= 0.0f; }      // (a query that is not finite has no element: every D2 is NaN or +inf)
    static TD void box(const BvhView &b, const PointMargin &pm, const Query &t, v3 &lo, v3 &hi, float &m) { lo = t.p; hi = t.p; m = pm.margin(b, t.p); }
    static TD bool test(const BvhView &b, int slot, bool is_tri, const Query &t, float &d2, int &prim, int &code)
    {
        const CpPoint r = cp_record(b, slot, is_tri, t.p, prim);
        d2 = r.d2; code = 0;
        return NnList::member(r.d2, prim, t.lim2);
    }
};
struct TqpKind {
    struct Query { v3 p0, p1, p2; float lim2; };
    static TD Query idle() { Query t; t.p0 = V(0.0f, 0.0f, 0.0f); t.p1 = t.p0; t.p2 = t.p0; t.lim2 = -1.0f; return t; }
    static TD Query load(const PairArgs &a, int q)      // (tq_load_query's rule: a T that is not finite gets the lim2 of a negative bound)
    {
        const float *r = a.query + (int64_t)q * a.query_stride;
        Query t;
        t.p0 = V(r[0], r[1], r[2]); t.p1 = V(r[3], r[4], r[5]); t.p2 = V(r[6], r[7], r[8]);
        t.lim2 = cp_limit2(a.dmax ? a.dmax[(int64_t)q * a.dmax_stride] : a.dmax_all);
        if (!(cp_finite3(t.p0) && cp_finite3(t.p1) && cp_finite3(t.p2))) t.lim2 = -1.0f;
        return t;
    }
    static TD bool walks(const Query &t) { return t.lim2 >= 0.0f; }
    static TD void box(const BvhView &b, const PointMargin &pm, const Query &t, v3 &lo, v3 &hi, float &m)
    {
        lo = V(minf(minf(t.p0.x, t.p1.x), t.p2.x), minf(minf(t.p0.y, t.p1.y), t.p2.y), minf(minf(t.p0.z, t.p1.z), t.p2.z));
        hi = V(maxf(maxf(t.p0.x, t.p1.x), t.p2.x), maxf(maxf(t.p0.y, t.p1.y), t.p2.y), maxf(maxf(t.p0.z, t.p1.z), t.p2.z));
        m = maxf(maxf(pm.margin(b, t.p0), pm.margin(b, t.p1)), pm.margin(b, t.p2));
    }
    // a triangle through tq_pair; anything else has no part
    static TD bool test(const BvhView &b, int slot, bool is_tri, const Query &t, float &d2, int &prim, int &code)
    {
        if (!is_tri) return false;
        const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
        const float4 ta = tp[0], tb = tp[1], tc = tp[2];
        prim = __float_as_int(tc.w);
        const TqPair r = tq_pair(t.p0, t.p1, t.p2, V(ta.x, ta.y, ta.z), V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
        d2 = r.d2; code = r.code;
        return NnList::member(r.d2, prim, t.lim2);
    }
};

// a row's range for the filling pass: its first slot and its length, 0 for a row that does not fit
TD int pairs_row_of(const PairArgs &a, int q, int64_t &r0)
{
    r0 = a.row_start[q];
    return pairs_row_len(r0, a.row_start[q + 1], a.capacity);
}
// member number idx of a row of `len` pairs that starts at r0
template <bool TRI>
TD void pairs_store(const PairArgs &a, int64_t r0, int len, int idx, float d2, int prim, int code)
{
    if (idx < len) {
        const int64_t at = r0 + idx;
        if (a.out_d2) a.out_d2[at] = d2;
        if (a.out_prim) a.out_prim[at] = prim;
        if (TRI && a.out_code) a.out_code[at] = code;
    }
}

template <class K, bool TRI, bool FILL>
TD void pairs_scan_body(const PairArgs &a)
{
    const int q = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (q >= a.n) return;
    const typename K::Query t = K::load(a, q);
    int64_t r0 = 0;
    const int len = FILL ? pairs_row_of(a, q, r0) : 0;
    int idx = 0;
    if (!FILL || len > 0) {
        for (int i = 0; i < a.n_prim; i++) {
            float d2 = 0.0f; int prim = -1, code = 0;
            if (K::test(a.bvh, a.prim_slot[i], a.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI, t, d2, prim, code)) {
                if (FILL) pairs_store<TRI>(a, r0, len, idx, d2, prim, code);
                idx++;
            }
        }
    }
    if (!FILL) a.row_start[q + 1] = idx;
    if (a.counts) a.counts[q] = make_int2(0, a.n_prim);
}

template <class K, bool TRI, bool COUNT, bool FILL>
TD void pairs_walk_body(const PairArgs &a, CpEntry *stk)
{
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    const PointMargin pm(b);
    unsigned long long n_over = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        typename K::Query t = K::idle();
        if (live) t = K::load(a, q);
        int64_t r0 = 0;
        int len = 0;
        if (FILL && live) len = pairs_row_of(a, q, r0);
        v3 lo, hi; float m;
        K::box(b, pm, t, lo, hi, m);
        const int start = (live && K::walks(t) && (!FILL || len > 0)) ? b.root_qcode : CP_SENT;      // (an empty row, or one that does not fit: no second walk)
        PointStack<CpEntry> st(stk, a.spill, a.stack_size, lane);
        unsigned nbox = 0, nleaf = 0;
        int idx = 0;
        point_walk<COUNT>(b, st, m, lo, hi, start, t.lim2, nbox, nleaf, [&](int code) {
            float d2 = 0.0f; int prim = -1, pc = 0;
            if (K::test(b, leaf_slot(code), leaf_is_tri(code), t, d2, prim, pc)) {
                if (FILL) pairs_store<TRI>(a, r0, len, idx, d2, prim, pc);
                idx++;
            }
            return t.lim2;
        });
        if (live) {
            if (!FILL) a.row_start[q + 1] = idx;
            if (COUNT && a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
        }
        if (st.overflow) n_over++;
    }
    point_walk_count_overflow(n_over, lane, a.ctr);
}

template <bool FILL> __global__ __launch_bounds__(CP_BLOCK) void k_pp_scan(PairArgs a) { pairs_scan_body<PpKind, false, FILL>(a); }
template <bool FILL> __global__ __launch_bounds__(CP_BLOCK) void k_tqp_scan(PairArgs a) { pairs_scan_body<TqpKind, true, FILL>(a); }
template <bool COUNT, bool FILL>
__global__ __launch_bounds__(CP_BLOCK) void k_pp_walk(PairArgs a)
{
    __shared__ CpEntry stk[CP_LDS_DEPTH * CP_BLOCK];    // [entry][lane]
    pairs_walk_body<PpKind, false, COUNT, FILL>(a, stk);
}
template <bool COUNT, bool FILL>
__global__ __launch_bounds__(CP_BLOCK) void k_tqp_walk(PairArgs a)
{
    __shared__ CpEntry stk[CP_LDS_DEPTH * CP_BLOCK];    // [entry][lane]
    pairs_walk_body<TqpKind, true, COUNT, FILL>(a, stk);
}

// ---- the scan: rs = row_start + 1 holds n lengths, then n inclusive sums (tirt_pairs.h "SCAN"; pairs_scan_host is the same three passes)
// (1) sums[b] = the sum of block b's lengths
__global__ __launch_bounds__(PAIRS_SCAN_BLOCK) void k_pairs_block_sum(const int64_t *rs, int64_t n, int64_t *sums)
{
    __shared__ unsigned long long s_w[PAIRS_SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * PAIRS_SCAN_BLOCK + threadIdx.x;
    const unsigned long long w = wave_sum(i < n ? (unsigned long long)rs[i] : 0ull);
    if (lane == 0) s_w[wid] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < PAIRS_SCAN_BLOCK / 64; k++) s += s_w[k];
        sums[blockIdx.x] = (int64_t)s;
    }
}
// an inclusive scan of one value per thread over a block of PAIRS_SCAN_BLOCK threads: a shuffle scan inside each wave, the wave totals through LDS
// (k_pixel_scan's, on 64-bit sums).  Every thread of the block calls it; s_w is the block's, free to reuse after the barrier the caller places
TD long long pairs_block_inclusive(long long v, long long *s_w, long long &block_total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PAIRS_SCAN_BLOCK / 64; w++) { const long long s = s_w[w]; if (w < wid) before += s; total += s; }
    block_total = total;
    return before + inc;
}
// (2) one block: sums[0 .. nb) -> their exclusive prefix sums in place, PAIRS_SCAN_BLOCK per trip with the carry of the earlier trips
__global__ __launch_bounds__(PAIRS_SCAN_BLOCK) void k_pairs_scan_sums(int64_t *sums, int64_t nb)
{
    __shared__ long long s_w[PAIRS_SCAN_BLOCK / 64];
    long long carry = 0;                                         // (every thread holds the same carry)
    for (int64_t base = 0; base < nb; base += PAIRS_SCAN_BLOCK) {      // (the same trips for every thread)
        const int64_t i = base + threadIdx.x;
        const long long v = i < nb ? (long long)sums[i] : 0;
        long long total;
        const long long inc = pairs_block_inclusive(v, s_w, total);
        if (i < nb) sums[i] = (int64_t)(carry + inc - v);
        carry += total;
        __syncthreads();                                         // s_w has been read by all
    }
}
// (3) block b: the inclusive sums of its own lengths plus its offset; row_start[0] = 0
__global__ __launch_bounds__(PAIRS_SCAN_BLOCK) void k_pairs_scan_add(int64_t *row_start, int64_t n, const int64_t *sums)
{
    __shared__ long long s_w[PAIRS_SCAN_BLOCK / 64];
    int64_t *rs = row_start + 1;
    const int64_t i = (int64_t)blockIdx.x * PAIRS_SCAN_BLOCK + threadIdx.x;
    const long long v = i < n ? (long long)rs[i] : 0;
    long long total;
    const long long inc = pairs_block_inclusive(v, s_w, total);
    if (i < n) rs[i] = (int64_t)((long long)sums[blockIdx.x] + inc);
    if (i == 0) row_start[0] = 0;
}

// ---- the order pass: a row's storage for the network of tirt_pairs.h -- in LDS (the address space stays in the member's type: ds_* instructions, never
// flat_* ones through the aperture), or the caller's arrays themselves
template <bool CODE>
struct PairsLdsRow {
    typedef __attribute__((address_space(3))) uint64_t LdsKey;
    typedef __attribute__((address_space(3))) unsigned char LdsCode;
    LdsKey *k; LdsCode *c;
    TD uint64_t key(int64_t i) const { return k[i]; }
    TD void swap(int64_t i, int64_t j) const
    {
        const uint64_t a = k[i], b = k[j]; k[i] = b; k[j] = a;
        if (CODE) { const unsigned char x = c[i], y = c[j]; c[i] = y; c[j] = x; }
    }
};
template <bool CODE>
struct PairsGlobalRow {
    float *d2; int32_t *prim, *code;
    TD uint64_t key(int64_t i) const { return pairs_key(__float_as_uint(d2[i]), prim[i]); }
    TD void swap(int64_t i, int64_t j) const
    {
        const float a = d2[i], b = d2[j]; d2[i] = b; d2[j] = a;
        const int32_t p = prim[i], r = prim[j]; prim[i] = r; prim[j] = p;
        if (CODE) { const int32_t x = code[i], y = code[j]; code[i] = y; code[j] = x; }
    }
};
// the steps of the network on the row M by this wave (a block is a wave): a step's exchanges side by side, a barrier -- with its workgroup fence, which orders
// the global path's stores before the next step's loads -- between steps
template <class M>
TD void pairs_order_row(const M &m, int len)
{
    const int64_t cnt = pairs_step_count(len);
    pairs_sort_steps(len, [&](int k, int j) {
        for (int64_t t = threadIdx.x; t < cnt; t += CP_BLOCK) pairs_exchange(m, k, j, t, (int64_t)len);
        __syncthreads();
    });
}
template <bool CODE>
__global__ __launch_bounds__(CP_BLOCK) void k_pairs_order(const int64_t *row_start, int64_t n, int64_t capacity, float *out_d2, int32_t *out_prim, int32_t *out_code)
{
    __shared__ uint64_t s_key[PAIRS_LDS_ROW];
    __shared__ unsigned char s_code[CODE ? PAIRS_LDS_ROW : 4];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {      // block-uniform, and so is everything that decides a branch below
        const int64_t r0 = row_start[row];
        const int len = pairs_row_len(r0, row_start[row + 1], capacity);
        if (len < 2) continue;
        if (len <= PAIRS_LDS_ROW) {
            for (int i = lane; i < len; i += CP_BLOCK) {
                s_key[i] = pairs_key(__float_as_uint(out_d2[r0 + i]), out_prim[r0 + i]);
                if (CODE) s_code[i] = (unsigned char)out_code[r0 + i];
            }
            __syncthreads();
            const PairsLdsRow<CODE> m = {(typename PairsLdsRow<CODE>::LdsKey *)s_key, (typename PairsLdsRow<CODE>::LdsCode *)s_code};
            pairs_order_row(m, len);
            for (int i = lane; i < len; i += CP_BLOCK) {
                const uint64_t key = s_key[i];
                out_d2[r0 + i] = __uint_as_float((unsigned)(key >> 32));
                out_prim[r0 + i] = (int32_t)(unsigned)key;
                if (CODE) out_code[r0 + i] = (int32_t)(signed char)s_code[i];
            }
            __syncthreads();                                         // the next row's loads overwrite s_key
        } else {
            const PairsGlobalRow<CODE> m = {out_d2 + r0, out_prim + r0, CODE ? out_code + r0 : nullptr};
            pairs_order_row(m, len);
        }
    }
}

// ---- the per-pair attributes, after the order: one wave per row, lane i takes pairs i, i + 64, ...  The functions and the operands the walk had, hence the
// bits closest() gives for that pair.  A slot whose id is no primitive's (a FILL call on a row_start that is not of these queries) gets zeros.
__global__ __launch_bounds__(CP_BLOCK) void k_pp_resolve(PairArgs a, int64_t n, float *out_point, int64_t point_out_stride, float *out_uv, int64_t uv_stride)
{
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const int64_t r0 = a.row_start[row];
        const int len = pairs_row_len(r0, a.row_start[row + 1], a.capacity);
        if (len == 0) continue;
        const float *qr = a.query + row * a.query_stride;
        const v3 p = V(qr[0], qr[1], qr[2]);
        for (int i = threadIdx.x; i < len; i += CP_BLOCK) {
            const int64_t at = r0 + i;
            const int prim = a.out_prim[at];
            CpPoint r; r.d2 = 0.0f; r.q = V(0.0f, 0.0f, 0.0f); r.u = 0.0f; r.v = 0.0f;
            if ((unsigned)prim < (unsigned)a.n_prim) {
                int id;
                r = cp_record(a.bvh, a.prim_slot[prim], a.primitive[(size_t)prim * PRI_VEC] == PRIMITIVE_TRI, p, id);
            }
            if (out_point) { float *o = out_point + at * point_out_stride; o[0] = r.q.x; o[1] = r.q.y; o[2] = r.q.z; }
            if (out_uv) { float *o = out_uv + at * uv_stride; o[0] = r.u; o[1] = r.v; }
        }
    }
}
__global__ __launch_bounds__(CP_BLOCK) void k_tqp_resolve(PairArgs a, int64_t n, float *out_points, int64_t points_stride)
{
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const int64_t r0 = a.row_start[row];
        const int len = pairs_row_len(r0, a.row_start[row + 1], a.capacity);
        if (len == 0) continue;
        const float *qr = a.query + row * a.query_stride;
        const v3 p0 = V(qr[0], qr[1], qr[2]), p1 = V(qr[3], qr[4], qr[5]), p2 = V(qr[6], qr[7], qr[8]);
        for (int i = threadIdx.x; i < len; i += CP_BLOCK) {
            const int64_t at = r0 + i;
            const int prim = a.out_prim[at];
            v3 P = V(0.0f, 0.0f, 0.0f), Q = P;
            if ((unsigned)prim < (unsigned)a.n_prim && a.primitive[(size_t)prim * PRI_VEC] == PRIMITIVE_TRI) {
                const float4 *tp = a.bvh.tri + (size_t)a.prim_slot[prim] * TRI_STRIDE;
                const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                const TqPair r = tq_pair(p0, p1, p2, V(ta.x, ta.y, ta.z), V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
                P = r.P; Q = r.Q;
            }
            float *o = out_points + at * points_stride;
            o[0] = P.x; o[1] = P.y; o[2] = P.z; o[3] = Q.x; o[4] = Q.y; o[5] = Q.z;
        }
    }
}

// ---- the host's side
struct PairsCall {
    bool tri;
    const float *query; int64_t n, query_stride;
    const float *dmax; int64_t dmax_stride; float dmax_all;
    int mode; int64_t capacity; int stack_size, flags;
    int64_t *row_start; float *out_d2; int32_t *out_prim, *out_code;
    float *attr0; int64_t attr0_stride; float *attr1; int64_t attr1_stride;      // points: Q and (u, v); triangles: P then Q (attr0 alone)
    int2 *counts;
};

// what a call is refused for before a context is looked at: the mode, the outputs, the capacity, the alignment
static int pairs_arg_checks(const std::string &f, const PairsCall &p)
{
    TIRT_REQUIRE(p.mode == TIRT_PAIRS_COUNT || p.mode == TIRT_PAIRS_FILL || p.mode == TIRT_PAIRS_BOTH, f + "unknown mode (TIRT_PAIRS_COUNT, TIRT_PAIRS_FILL or TIRT_PAIRS_BOTH)");
    TIRT_REQUIRE(p.row_start, f + "null row_start");
    TIRT_REQUIRE(((uintptr_t)p.row_start & 7) == 0, f + "row_start must be 8-byte aligned");
    if (p.mode != TIRT_PAIRS_COUNT) TIRT_REQUIRE(p.capacity >= 0, f + "capacity < 0");
    if (p.mode != TIRT_PAIRS_COUNT && p.capacity > 0) {      // (arrays of 0 pairs hold no row that has a pair: they are not looked at)
        TIRT_REQUIRE(p.out_prim || p.out_d2, f + "FILL / BOTH without out_prim and without out_d2 (nothing to return)");
        TIRT_REQUIRE((p.flags & TIRT_PAIRS_UNORDERED) || (p.out_prim && p.out_d2), f + "the order of a row is by (out_d2, out_prim): both are needed without TIRT_PAIRS_UNORDERED");
        TIRT_REQUIRE(p.out_prim || !(p.attr0 || p.attr1), f + "the per-pair points need out_prim");
    }
    return TIRT_OK;
}

// the launches of a call on the context's stream; every pointer is device memory (or null)
static int pairs_run(tirt_ctx *c, const PairsCall &p)
{
    const bool scan = (p.flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (p.flags & TIRT_COUNT_NODES) != 0, ordered = (p.flags & TIRT_PAIRS_UNORDERED) == 0;
    const bool count = p.mode != TIRT_PAIRS_FILL, fill = p.mode != TIRT_PAIRS_COUNT && p.capacity > 0;      // (no row that has a pair fits arrays of 0 pairs)
    const int64_t n = p.n;
    // the scan's block sums: the only scratch (8 bytes per PAIRS_SCAN_BLOCK queries)
    const int64_t nb = pairs_scan_blocks(n);
    if (count) if (int rc = query_scratch(c, (size_t)nb * 8)) return rc;
    PairArgs a = {};
    a.query_stride = p.query_stride; a.dmax_stride = p.dmax_stride; a.dmax_all = p.dmax_all;
    a.capacity = p.capacity;
    a.out_d2 = p.out_d2; a.out_prim = p.out_prim; a.out_code = p.out_code;
    // one walk (or scan) per chunk; FILL = false leaves the lengths, FILL = true writes the rows.  N_box / N_leaf come from the counting walk, or from the
    // filling walk of a FILL call
    auto walks = [&](bool filling, bool with_counts) {
        return point_walk_chunks(c, a, n, query_plan(c, n, p.flags, nullptr).chunk, scan, p.stack_size, [&](int64_t base, int m, int, int grid) {
            a.n = m;
            a.query = p.query + base * p.query_stride; a.dmax = p.dmax ? p.dmax + base * p.dmax_stride : nullptr;
            a.row_start = p.row_start + base;
            a.counts = with_counts && p.counts ? p.counts + base : nullptr;
            with_bool(filling, [&](auto F) { with_bool(cnt && with_counts, [&](auto C) {
                constexpr bool FILL = decltype(F)::value, COUNT = decltype(C)::value;
                if (scan) { if (p.tri) hipLaunchKernelGGL((k_tqp_scan<FILL>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
                            else hipLaunchKernelGGL((k_pp_scan<FILL>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a); }
                else { if (p.tri) hipLaunchKernelGGL((k_tqp_walk<COUNT, FILL>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
                       else hipLaunchKernelGGL((k_pp_walk<COUNT, FILL>), dim3(grid), dim3(CP_BLOCK), 0, c->stream, a); }
            }); });
        });
    };
    if (count) {
        if (int rc = walks(false, true)) return rc;
        int64_t *sums = c->query_mem.as<int64_t>();
        hipLaunchKernelGGL(k_pairs_block_sum, dim3((unsigned)nb), dim3(PAIRS_SCAN_BLOCK), 0, c->stream, (const int64_t *)(p.row_start + 1), n, sums);
        hipLaunchKernelGGL(k_pairs_scan_sums, dim3(1), dim3(PAIRS_SCAN_BLOCK), 0, c->stream, sums, nb);
        hipLaunchKernelGGL(k_pairs_scan_add, dim3((unsigned)nb), dim3(PAIRS_SCAN_BLOCK), 0, c->stream, p.row_start, n, (const int64_t *)sums);
    }
    if (fill) {
        if (int rc = walks(true, !count)) return rc;
        // a wave per row, as many as keep the device busy
        const int64_t rows_grid = (int64_t)c->cu_count * 32;
        const unsigned g = (unsigned)(n < rows_grid ? n : rows_grid);
        if (ordered) {
            if (p.tri && p.out_code) hipLaunchKernelGGL((k_pairs_order<true>), dim3(g), dim3(CP_BLOCK), 0, c->stream, (const int64_t *)p.row_start, n, p.capacity, p.out_d2, p.out_prim, p.out_code);
            else hipLaunchKernelGGL((k_pairs_order<false>), dim3(g), dim3(CP_BLOCK), 0, c->stream, (const int64_t *)p.row_start, n, p.capacity, p.out_d2, p.out_prim, (int32_t *)nullptr);
        }
        if (p.attr0 || p.attr1) {
            a.query = p.query; a.row_start = p.row_start; a.n = 0; a.counts = nullptr;
            if (p.tri) hipLaunchKernelGGL(k_tqp_resolve, dim3(g), dim3(CP_BLOCK), 0, c->stream, a, n, p.attr0, p.attr0_stride);
            else hipLaunchKernelGGL(k_pp_resolve, dim3(g), dim3(CP_BLOCK), 0, c->stream, a, n, p.attr0, p.attr0_stride, p.attr1, p.attr1_stride);
        }
    }
    return TIRT_OK;
}

// the device entry of both kinds: the checks, the two events around the launches
static int pairs_query(tirt_ctx *c, const char *fn, PairsCall p, int32_t *counts, void *stream)
{
    const std::string f = std::string(fn) + ": ";
    if (int rc = pairs_arg_checks(f, p)) return rc;
    CTX(c);
    const StrideCheck q_stride = p.tri ? StrideCheck{true, p.query_stride, 9, "tri_stride < 9 (floats per triangle)"} : StrideCheck{true, p.query_stride, 3, "point_stride < 3 (floats per point)"};
    const StrideCheck a0_stride = p.tri ? StrideCheck{p.attr0 != nullptr, p.attr0_stride, 6, "points_stride < 6 (floats per pair of closest points)"}
                                        : StrideCheck{p.attr0 != nullptr, p.attr0_stride, 3, "point_out_stride < 3 (floats per closest point)"};
    if (int rc = point_query_checks(c, fn, p.n, p.stack_size, p.flags & ~TIRT_PAIRS_UNORDERED, {q_stride, a0_stride, {!p.tri && p.attr1, p.attr1_stride, 2, "uv_stride < 2"},
                                    {p.dmax != nullptr, p.dmax_stride, 1, "dmax_stride < 1"}}, counts, stream)) return rc;
    const bool fill = p.mode != TIRT_PAIRS_COUNT && p.capacity > 0;
    if (!fill) { p.out_d2 = nullptr; p.out_prim = nullptr; p.out_code = nullptr; p.attr0 = nullptr; p.attr1 = nullptr; }      // COUNT writes row_start and nothing else
    if (int rc = require_device_ptrs(c, f, {{p.row_start, "row_start"}})) return rc;
    if (p.n == 0) {
        if (p.mode == TIRT_PAIRS_FILL) return TIRT_OK;
        if (int rc = query_begin(c, stream)) return rc;
        TIRT_HIP(hipMemsetAsync(p.row_start, 0, sizeof(int64_t), c->stream));
        return query_end(c, stream);
    }
    TIRT_REQUIRE(p.query, f + (p.tri ? "null tris" : "null points"));
    p.counts = query_plan(c, p.n, p.flags, counts).counts;
    if (int rc = require_device_ptrs(c, f, {{p.query, p.tri ? "tris" : "points"}, {p.dmax, "dmax"}, {p.out_d2, "out_d2"}, {p.out_prim, "out_prim"}, {p.out_code, "out_code"},
                                            {p.attr0, p.tri ? "out_points" : "out_point"}, {p.attr1, "out_uv"}, {p.counts, "counts"}})) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = pairs_run(c, p)) return rc;
    return query_end(c, stream);
}

// the host entry of both kinds: host arrays staged in device memory (QueryStage; the per-pair columns hold `capacity` pairs), through pairs_run, back to
// the host with a sync.  Only the rows that were written come back: what lies behind them in the caller's arrays stays as it was
static int pairs_host(tirt_ctx *c, const char *fn, PairsCall p, int32_t *counts)
{
    const std::string f = std::string(fn) + ": ";
    if (int rc = pairs_arg_checks(f, p)) return rc;
    CTX(c);
    if (int rc = query_common_checks(c, fn, "n", p.n, p.stack_size, p.flags & ~TIRT_PAIRS_UNORDERED)) return rc;
    const bool fill = p.mode != TIRT_PAIRS_COUNT && p.capacity > 0;
    if (p.n == 0) { if (p.mode != TIRT_PAIRS_FILL) p.row_start[0] = 0; return TIRT_OK; }
    TIRT_REQUIRE(p.query, f + (p.tri ? "null tris" : "null points"));
    const size_t N = (size_t)p.n, QW = p.tri ? 9 : 3, CAP = fill ? (size_t)p.capacity : 0, A0 = p.tri ? 6 : 3;      // A0: floats of attr0 per pair (P, Q or Q)
    const int64_t *h_row = p.row_start;
    QueryStage s(c);
    const auto k_row = p.mode == TIRT_PAIRS_FILL ? s.in(p.row_start, N + 1) : s.out(p.row_start, N + 1);
    const auto k_query = s.in(p.query, QW * N);
    const auto k_dmax = s.in(p.dmax, N);
    // (the key of the order needs d2 and prim on the device whichever of them the caller wants back)
    const auto k_d2 = s.out(p.out_d2, CAP, fill);
    const auto k_prim = s.out(p.out_prim, CAP, fill);
    const auto k_code = s.out(p.out_code, CAP, fill && p.tri && p.out_code);
    const auto k_a0 = s.out(p.attr0, A0 * CAP, fill && p.attr0);
    const auto k_a1 = s.out(p.attr1, 2 * CAP, fill && p.attr1);
    const auto k_counts = s.out_counts(counts, p.flags, N);
    if (int rc = s.begin()) return rc;
    p.query = s.ptr(k_query); p.query_stride = (int64_t)QW; p.dmax = s.ptr(k_dmax); p.dmax_stride = 1; p.dmax_all = __builtin_inff();
    p.row_start = s.ptr(k_row);
    p.out_d2 = s.ptr(k_d2); p.out_prim = s.ptr(k_prim); p.out_code = s.ptr(k_code);
    p.attr0 = s.ptr(k_a0); p.attr0_stride = (int64_t)A0;
    p.attr1 = s.ptr(k_a1); p.attr1_stride = 2;
    p.counts = s.ptr(k_counts);
    if (int rc = pairs_run(c, p)) return rc;
    if (int rc = s.fetch(k_row)) return rc;
    if (int rc = s.fetch(k_counts)) return rc;
    if (int rc = s.sync()) return rc;
    size_t written = 0;      // the rows that fit are a prefix of the rows
    for (size_t i = 0; fill && i < N && pairs_row_fits(h_row[i], h_row[i + 1], p.capacity); i++) written = (size_t)h_row[i + 1];
    if (int rc = s.fetch(k_d2, written)) return rc;
    if (int rc = s.fetch(k_prim, written)) return rc;
    if (int rc = s.fetch(k_code, written)) return rc;
    if (int rc = s.fetch(k_a0, A0 * written)) return rc;
    if (int rc = s.fetch(k_a1, 2 * written)) return rc;
    return s.finish();
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_query_point_pairs(tirt_ctx *c, const float *points, int64_t n, int64_t point_stride, const float *dmax, int64_t dmax_stride, float dmax_all, int mode,
                           int64_t capacity, int stack_size, int flags, int64_t *row_start, float *out_d2, int32_t *out_prim, float *out_point,
                           int64_t point_out_stride, float *out_uv, int64_t uv_stride, int32_t *counts, void *stream)
{
    PairsCall p = {false, points, n, point_stride, dmax, dmax_stride, dmax_all, mode, capacity, stack_size, flags, row_start, out_d2, out_prim, nullptr,
                   out_point, point_out_stride, out_uv, uv_stride, nullptr};
    return pairs_query(c, "tirt_query_point_pairs", p, counts, stream);
}

int tirt_query_mesh_pairs(tirt_ctx *c, const float *tris, int64_t n, int64_t tri_stride, const float *dmax, int64_t dmax_stride, float dmax_all, int mode,
                          int64_t capacity, int stack_size, int flags, int64_t *row_start, float *out_d2, int32_t *out_prim, int32_t *out_code,
                          float *out_points, int64_t points_stride, int32_t *counts, void *stream)
{
    PairsCall p = {true, tris, n, tri_stride, dmax, dmax_stride, dmax_all, mode, capacity, stack_size, flags, row_start, out_d2, out_prim, out_code,
                   out_points, points_stride, nullptr, 0, nullptr};
    return pairs_query(c, "tirt_query_mesh_pairs", p, counts, stream);
}

int tirt_point_pairs(tirt_ctx *c, const float *points, int n, const float *dmax, int mode, int64_t capacity, int stack_size, int flags, int64_t *row_start,
                     float *out_d2, int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts)
{
    PairsCall p = {false, points, n, 3, dmax, 1, __builtin_inff(), mode, capacity, stack_size, flags, row_start, out_d2, out_prim, nullptr, out_point, 3,
                   out_uv, 2, nullptr};
    return pairs_host(c, "tirt_point_pairs", p, counts);
}

int tirt_mesh_pairs(tirt_ctx *c, const float *tris, int n, const float *dmax, int mode, int64_t capacity, int stack_size, int flags, int64_t *row_start,
                    float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int32_t *counts)
{
    PairsCall p = {true, tris, n, 9, dmax, 1, __builtin_inff(), mode, capacity, stack_size, flags, row_start, out_d2, out_prim, out_code, out_points, 6,
                   nullptr, 0, nullptr};
    return pairs_host(c, "tirt_mesh_pairs", p, counts);
}

// host only, no context: rows of members (d2, prim) in the order given -- row i is the next row_len[i] entries -- through the scan, the capacity rule and
// the network of tirt_pairs.h, the text the kernels run
int tirt_kat_pairs_host(const float *d2, const int32_t *prim, const int32_t *row_len, int n_rows, int64_t capacity, int64_t *row_start, float *out_d2,
                        int32_t *out_prim)
{
    TIRT_REQUIRE(row_start && n_rows >= 0 && (n_rows == 0 || row_len), "tirt_kat_pairs_host: null pointer or negative n_rows");
    TIRT_REQUIRE(capacity >= 0 && (capacity == 0 || (out_d2 && out_prim)), "tirt_kat_pairs_host: capacity < 0, or no out_d2 / out_prim");
    int64_t total = 0;
    for (int i = 0; i < n_rows; i++) {
        TIRT_REQUIRE(row_len[i] >= 0, "tirt_kat_pairs_host: a row's length is negative");
        row_start[i + 1] = row_len[i];
        total += row_len[i];
    }
    TIRT_REQUIRE(total == 0 || (d2 && prim), "tirt_kat_pairs_host: null d2 / prim");
    for (int64_t i = 0; i < total; i++)
        TIRT_REQUIRE(prim[i] >= 0 && d2[i] >= 0.0f && d2[i] < __builtin_inff(), "tirt_kat_pairs_host: an entry is no member (prim < 0, or D2 negative, NaN or +inf)");
    std::vector<int64_t> sums((size_t)pairs_scan_blocks(n_rows) + 1);
    pairs_scan_host(row_start, n_rows, sums.data());
    struct HostRow {
        float *d2; int32_t *prim;
        uint64_t key(int64_t i) const { uint32_t b; memcpy(&b, &d2[i], 4); return pairs_key(b, prim[i]); }
        void swap(int64_t i, int64_t j) const { const float a = d2[i]; d2[i] = d2[j]; d2[j] = a; const int32_t p = prim[i]; prim[i] = prim[j]; prim[j] = p; }
    };
    for (int i = 0; i < n_rows; i++) {
        const int64_t r0 = row_start[i];
        const int len = pairs_row_len(r0, row_start[i + 1], capacity);      // 0: the row does not fit (or is empty): nothing of it is written
        for (int j = 0; j < len; j++) { out_d2[r0 + j] = d2[r0 + j]; out_prim[r0 + j] = prim[r0 + j]; }
        HostRow m = {out_d2 + r0, out_prim + r0};
        const int64_t cnt = pairs_step_count(len);
        pairs_sort_steps(len, [&](int k, int j) { for (int64_t t = 0; t < cnt; t++) pairs_exchange(m, k, j, t, (int64_t)len); });
    }
    return TIRT_OK;
}

}  // extern "C"
