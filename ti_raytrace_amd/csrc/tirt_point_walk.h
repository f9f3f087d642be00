// tirt_point_walk.h -- the walk of a POINT, or of a small box, over the quantised 4-wide nodes `cnode` (BvhView), once.  Its users:
//   k_cp_walk   (tirt_closest_point.hip)    point_walk with lo == hi == the query point; the cut is min(best D2, lim2)
//   k_nn_walk   (tirt_nearest.hip)          point_walk with lo == hi == the query point; the cut is the list's threshold (lim2 alone under COUNT_ALL)
//   k_tq_walk   (tirt_triangle_query.hip)   point_walk with [lo, hi] the query triangle's box; the cut is min(best D2, lim2)
//   k_sd_build  (tirt_signed_distance.hip)  its own loop (it descends where the gap is 0, culls nothing and sorts nothing) over the same margin, gap and stack
//   k_multi_hit (tirt_multi_hit.hip)        PointStack<int> and the grid sizing alone (a ray's walk)
// Here: the margin by which a child's decoded box is grown and the distance of an interval to it (PointMargin, CP_BOX_GAP; CP_AXIS_GAP for a point), the
// stack of one lane (PointStack), THE WALK (point_walk) with the end of its kernels (point_walk_count_overflow), what its kernels and their scans read
// (cp_load_query, cp_finite3, cp_record), and on the host the grid whose stacks fit (point_walk_grid, point_walk_launch_shape) and the launches of a call in
// chunks (point_walk_chunks, with point_walk_args and with_bool).
// A wave is a block (CP_BLOCK lanes, no barrier anywhere): a lane holds one query and the blocks stride over the work.
//
// WHY THE CULL IS CONSERVATIVE.  point_walk skips a subtree on lb2 > cut only, never on equality -- at a node (`kept`) and at a pop (pop_live) -- and the
// cut a leaf returns only ever shrinks and is never below the D2 of a primitive that could still be accepted (each kernel's head says why for its cut).
// So it suffices that lb2 <= D2 holds, as computed fp32
// numbers, for every primitive t below the node.  (k_sd_build descends where lb2 == 0 and needs the same for D2 = 0: a triangle with a corner AT the
// point.  k_tq_walk's box in place of p: the head of tirt_triangle_query.h.)  Write eps = 2^-24, E = the largest extent of the padded root box, C = E / 60000 = the largest cell,
// M = the largest coordinate magnitude among p and the scene, d = the distance from p to t.
//  (1) The computed D2.  cp_triangle's Q is a vertex, or a + ab u with u in [0, 1] (AB, AC, BC: the region tests make numerator and denominator
//      non-negative with numerator <= denominator, and a correctly rounded quotient keeps that), or (a + ab u) + ac v with u = vb den, v = vc den.
//      On an edge the exact a + ab u lies on the segment, hence in the leaf's exact box, and the evaluated one differs from it by the roundings of
//      b - a, the product and the sum: <= 2 eps M per coordinate.  In the interior u, v, 1 - u - v carry the error of va, vb, vc (differences of
//      products of dot products whose terms reach |ab| |ap|): a relative error of order eps (|p - a| / |ab|) in (u, v), i.e. a shift of Q IN THE
//      TRIANGLE'S PLANE of order eps (d + |ab|), a few eps M again.  So Q is within k eps M of the box with k "a few"; p - Q adds eps M / 2 per
//      coordinate and the dot product 3 eps relative.  sqrt(D2) >= (d_box - sqrt(3) (k + 1) eps M) (1 - 2 eps), d_box = the exact distance from p to
//      the exact box.  The sphere: |len - r| is off by <= 3 eps max(len, r) <= 3 eps (M + d) from a distance to a surface inside its box.
//      [A needle whose area is so small against its edges that va + vb + vc is rounding noise can put the interior's Q further out than that; such a
//      triangle has no trustworthy interior answer in the scan either.  The margin below is sized for k <= 100, not for "a few".]
//  (2) The computed lb2.  A decoded plane is off by eps E / 4 (the product) + eps M / 2 (the sum), the differences mn - p, p - mx by eps M each at
//      most, the squares and sums by 3 eps relative: sqrt(lb2) <= (|e| + 3 sqrt(3) eps M) (1 + 2 eps), e the exact per-axis distances to the
//      quantised box moved outward by m.
//  (3) The slack.  A quantised plane is >= 0.9 of ITS axis' cell outside the exact box (tirt_internal.h: rounded outward by at least one cell); that
//      cell can be tiny on a flat scene's thin axis, so it is not relied on beyond the rounding of the planes themselves.  The margin m is the SAME
//      length on all axes, m = mc * C.  With x the exact per-axis distances to the exact box (|x| = d_box) and e_a <= max(x_a - m, 0):
//      |x|^2 = |e|^2 + 2 e.(x - e) + |x - e|^2 >= (|e| + m)^2 whenever e != 0, because x_a - e_a = m on every axis with e_a > 0.  So |e| <= d_box - m.
//  Together: lb2 <= D2 if m >= sqrt(3) (k + 4) eps M + 4 eps d.  With rho_p = max_a |p_a - grid_min_a| / E and rho_0 = max_a |grid_min_a| / E,
//  M <= (rho_0 + max(rho_p, 1/2)) E and d <= sqrt(3) (rho_p + 1/2) E; eps E = 0.00358 C.  mc = 0.5 + 0.5 (rho_p + rho_0) (cp_margin_cells) gives
//  m >= 0.5 C (rho_p + rho_0 + 1) >= 140 eps M and leaves >= 100 eps M for k after the 4 sqrt(3) eps M and 4 eps d terms (<= 14 + 14 eps M-equivalents).
//  Unlike trace_margin_cells it grows with the SCENE's distance from the origin too (rho_0): a mesh 10^4 extents from the origin has vertices that are
//  36 cells apart in fp32.  Half a cell is 8e-6 of the extent: it costs no visit worth counting near the scene; a query many extents away
//  gets a margin that swallows the boxes and its walk degenerates towards the scan, which is acceptable (no cut-off).
#pragma once
#include "tirt_internal.h"
#include "tirt_closest_point.h"

namespace tirt {

constexpr int CP_BLOCK = 64;                 // one wave per block
#ifndef CP_LDS_DEPTH_N
#define CP_LDS_DEPTH_N 16
#endif
constexpr int CP_LDS_DEPTH = CP_LDS_DEPTH_N;  // stack entries per lane in LDS: 16 x 8 B x 64 lanes = 8 KiB per block (24: the same rate, 32 / 48: 15 % / 36 % slower, profiles/closest_point_rate.txt)
constexpr size_t CP_SPILL_BYTES_MAX = (size_t)256 << 20;      // the grid shrinks until the stacks' global tails fit this
constexpr int CP_SENT = (int)0x80000000;     // "nothing to do": never a node index nor a leaf code (k_trace's TR_SENT)

// ---- the margin (the argument above is about exactly these expressions, in this order) ----
TD float cp_margin_cells(float rho_p, float rho_0) { return 0.5f + 0.5f * (rho_p + rho_0); }
struct PointMargin {
    float cell_max, inv_ext, rho_0;          // wave-uniform: formed once per kernel
    TD explicit PointMargin(const BvhView &b)
        : cell_max(maxf(maxf(b.cell[0], b.cell[1]), b.cell[2])),
          inv_ext(1.0f / (cell_max * (2.0f * TR_GRID_HALF))),
          rho_0(maxf(maxf(absf(b.grid_min[0]), absf(b.grid_min[1])), absf(b.grid_min[2])) * inv_ext) {}
    TD float margin(const BvhView &b, const v3 p) const      // m of the point p: a length, the same on all axes
    {
        const float rho_p = maxf(maxf(absf(p.x - b.grid_min[0]), absf(p.y - b.grid_min[1])), absf(p.z - b.grid_min[2])) * inv_ext;
        return cp_margin_cells(rho_p, rho_0) * cell_max;
    }
};
typedef _Float16 cp_h2v __attribute__((ext_vector_type(2)));
// the distance between the interval [lo_, hi_] and the decoded planes of axis k of one child (dword W of its node), less the margin m_, never negative:
// 0 = the interval meets the grown box on this axis.  THE gap expression: a point is the interval lo_ == hi_ == pk (CP_AXIS_GAP, k_sd_build's)
#define CP_BOX_GAP(b_, m_, W, k, lo_, hi_)                                                          \
                ({  const cp_h2v h__ = __builtin_bit_cast(cp_h2v, (unsigned)(W));                   \
                    const float mn__ = (b_).grid_min[k] + (float)h__.x * (b_).cell[k], mx__ = (b_).grid_min[k] + (float)h__.y * (b_).cell[k]; \
                    maxf(maxf(mn__ - (hi_), (lo_) - mx__) - (m_), 0.0f); })
#define CP_AXIS_GAP(b_, m_, W, k, pk) CP_BOX_GAP(b_, m_, W, k, pk, pk)
// the four children of a node record q0 .. q3 (tirt_internal.h: dword 3c + a = the planes of child c on axis a, dwords 12 .. 15 = the codes): F(c, X, Y, Z, code) each
#define CP_EACH_CHILD(F) F(0, q0.x, q0.y, q0.z, q3.x); F(1, q0.w, q1.x, q1.y, q3.y); F(2, q1.z, q1.w, q2.x, q3.z); F(3, q2.y, q2.z, q2.w, q3.w)

// ---- the stack of one lane: entries of type E, the first CP_LDS_DEPTH in the block's LDS array ([entry][lane]), the rest of stack_size in `spill`
// ([entry][global thread], gridDim.x * CP_BLOCK threads: what point_walk_launch_shape sized).  An entry beyond stack_size is dropped and `overflow` stays set.
// The LDS array keeps its address space in the member's type: every access is a ds_* or a global_* instruction, never a flat_* one through the aperture.
template <class E>
struct PointStack {
    typedef __attribute__((address_space(3))) E LdsE;
    LdsE *lds; E *spill;
    size_t gthreads, gtid; int lane;         // threads of the grid, this one among them, and in its block
    int cap, sp = 0;                         // stack_size; entries on the stack
    bool overflow = false;
    TD PointStack(E *lds_array, E *spill_, int stack_size, int lane_)
        : lds((LdsE *)lds_array), spill(spill_), gthreads((size_t)gridDim.x * CP_BLOCK), gtid((size_t)blockIdx.x * CP_BLOCK + lane_), lane(lane_), cap(stack_size) {}
    TD bool empty() const { return sp == 0; }
    TD void push(const E e)
    {
        if (sp < cap) {
            if (sp < CP_LDS_DEPTH) lds[sp * CP_BLOCK + lane] = e;
            else spill[(size_t)(sp - CP_LDS_DEPTH) * gthreads + gtid] = e;
            sp++;
        } else overflow = true;              // out of room: the entry is lost
    }
    TD E pop() { sp--; return sp < CP_LDS_DEPTH ? lds[sp * CP_BLOCK + lane] : spill[(size_t)(sp - CP_LDS_DEPTH) * gthreads + gtid]; }      // (not of an empty stack)
};

// ---- THE WALK of k_cp_walk, k_nn_walk and k_tq_walk: best-first over `cnode` for the lane's query, whose exact box is [lo, hi] (a point: lo == hi) and
// whose margin is m.  Node steps and leaf steps alternate behind wave ballots, each for the lanes that are at one (a wave is a block: no barrier).
// A node visit decodes the four children's planes, forms lb2 = the sum over the axes of CP_BOX_GAP^2, drops empty slots and children with lb2 > cut,
// sorts the rest (five compare-exchanges, as k_trace), descends into the nearest and pushes the others far to near WITH their lb2; a popped entry is
// tested against the cut of that moment again (the cut shrinks fast: most entries are dead when they surface).  `leaf(code)` tests the record of a
// leaf code and returns the cut that holds after it; the cut never grows.  `cur` is the start: root_qcode, or CP_SENT for a lane that does not walk.
typedef unsigned CpEntry __attribute__((ext_vector_type(2)));      // a stack entry: (child code, bits of lb2)
constexpr int CP_WAVES_PER_CU = 20;          // persistent blocks per CU at most, for all three: what 8 KiB of LDS each admits (k_cp_walk / k_nn_walk: their 59 .. 66 VGPRs would admit 32; k_tq_walk: its 102 .. 105 VGPRs run 16 at a time, the rest wait their turn)

template <bool COUNT, class Leaf>
TD void point_walk(const BvhView &b, PointStack<CpEntry> &st, const float m, const v3 lo, const v3 hi, int cur, float cut, unsigned &nbox, unsigned &nleaf, Leaf leaf)
{
    // the next entry that can still win, or CP_SENT
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
#define WALK_BOX(i, X, Y, Z, code_)                                                                   \
            do {                                                                                    \
                const float ex__ = CP_BOX_GAP(b, m, X, 0, lo.x, hi.x), ey__ = CP_BOX_GAP(b, m, Y, 1, lo.y, hi.y), ez__ = CP_BOX_GAP(b, m, Z, 2, lo.z, hi.z); \
                const float s__ = (ex__ * ex__ + ey__ * ey__) + ez__ * ez__;                        \
                c##i = (int)(code_);                                                                \
                k##i = (c##i != TR_EMPTY) && !(s__ > cut);                                          \
                l##i = k##i ? s__ : MISS;                                                           \
            } while (0)
            CP_EACH_CHILD(WALK_BOX);
#undef WALK_BOX
#define WALK_CE(la, ca, ka, lb, cb, kb)                                                               \
            do {                                                                                    \
                const bool s__ = (lb) < (la);                                                       \
                const float lo__ = s__ ? (lb) : (la), hi__ = s__ ? (la) : (lb);                     \
                const int clo__ = s__ ? (cb) : (ca), chi__ = s__ ? (ca) : (cb);                     \
                const bool klo__ = s__ ? (kb) : (ka), khi__ = s__ ? (ka) : (kb);                    \
                la = lo__; lb = hi__; ca = clo__; cb = chi__; ka = klo__; kb = khi__;               \
            } while (0)
            WALK_CE(l0, c0, k0, l1, c1, k1); WALK_CE(l2, c2, k2, l3, c3, k3); WALK_CE(l0, c0, k0, l2, c2, k2); WALK_CE(l1, c1, k1, l3, c3, k3); WALK_CE(l1, c1, k1, l2, c2, k2);
#undef WALK_CE
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
                cut = leaf(~cur);
                cur = pop_live();
            }
        }
    }
}

// the end of a walk kernel: the queries of this wave that lost a stack entry, in one atomic (tirt_stats: TIRT_ERR_STACK)
TD void point_walk_count_overflow(unsigned long long n_over, int lane, DevCounters *ctr)
{
    n_over = wave_sum(n_over);
    if (lane == 0 && n_over && ctr) atomicAdd(&ctr->stack_overflow, n_over);
}

// ---- what the walks and their scans read: the query (CpArgs, NnArgs: the same fields), the test of its coordinates, and a primitive's record
template <class Args>
TD void cp_load_query(const Args &a, int q, v3 &p, float &lim2)
{
    const float *r = a.points + (int64_t)q * a.point_stride;
    p = V(r[0], r[1], r[2]);
    lim2 = cp_limit2(a.dmax ? a.dmax[(int64_t)q * a.dmax_stride] : a.dmax_all);
}
// false for NaN and +-inf: such a query finds nothing by the definition (every D2 is NaN or +inf) and does not walk.  One text in two forms, each where the
// compiler keeps what it made of the copies this replaces (profiles/shared_walk_isa.txt): in place in k_cp_walk / k_nn_walk, a call in tq_load_query
#define CP_FINITE3(p_, inf_) (absf((p_).x) < (inf_) && absf((p_).y) < (inf_) && absf((p_).z) < (inf_))
TD bool cp_finite3(const v3 p) { const float inf = __int_as_float(0x7f800000); return CP_FINITE3(p, inf); }
// D2, Q, u, v of the record in `slot` against p, and its primitive id: the kind comes from the caller (the leaf code's shape bit, or the primitive table).
// The sphere branch (a square root and a division) sits behind a wave ballot, as in trace_leaf_step
TD CpPoint cp_record(const BvhView &b, int slot, bool is_tri, const v3 p, int &prim)
{
    const float4 *tp = b.tri + (size_t)slot * TRI_STRIDE;
    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
    prim = __float_as_int(tc.w);
    const v3 pa = V(ta.x, ta.y, ta.z);
    CpPoint r; r.d2 = __int_as_float(0x7fc00000); r.q = V(0.0f, 0.0f, 0.0f); r.u = 0.0f; r.v = 0.0f;      // spot / laser: no surface, a NaN D2 is never accepted
    if (is_tri) r = cp_triangle(p, pa, V(tb.x, tb.y, tb.z), V(tc.x, tc.y, tc.z));
    const bool sph = !is_tri && (int)tb.y == SHAPE_SPHERE;
    if (__builtin_amdgcn_ballot_w64(sph) != 0ull) { if (sph) r = cp_sphere(p, pa, tb.x); }
    return r;
}

// ---- the host's side of the same stack: how many blocks, and the tails they need.  THE invariant between this and PointStack: `spill` holds
// (stack_size - CP_LDS_DEPTH) * grid * CP_BLOCK entries, and the kernel is launched with at most `grid` blocks of CP_BLOCK threads.
// The arithmetic alone: at most waves_per_cu persistent blocks per CU, fewer while the tails would not fit CP_SPILL_BYTES_MAX, no more than the work has blocks.
inline int point_walk_grid(int cu_count, int stack_size, size_t entry_bytes, int waves_per_cu, int64_t work_blocks, size_t &tail_bytes)
{
    int64_t grid = (int64_t)cu_count * waves_per_cu;
    tail_bytes = stack_size > CP_LDS_DEPTH ? (size_t)(stack_size - CP_LDS_DEPTH) * entry_bytes : 0;      // per thread
    if (tail_bytes) { const int64_t fit = (int64_t)(CP_SPILL_BYTES_MAX / (tail_bytes * CP_BLOCK)); if (grid > fit) grid = fit > 0 ? fit : 1; }
    return (int)(grid < work_blocks ? grid : work_blocks);
}
// ... and the context's spill buffer grown to it (only when there is a tail; growing frees the old buffer, which queued work may still use)
template <class E>
inline int point_walk_launch_shape(tirt_ctx *c, int stack_size, int waves_per_cu, int64_t work_blocks, int &grid, E *&spill)
{
    size_t tail;
    grid = point_walk_grid(c->cu_count, stack_size, sizeof(E), waves_per_cu, work_blocks, tail);
    spill = nullptr;
    const size_t want = tail * CP_BLOCK * (size_t)grid;
    if (want > c->spill.bytes) {
        TIRT_HIP(hipStreamSynchronize(c->stream));
        if (c->spill.ensure(want)) return TIRT_ERR_HIP;
    }
    if (tail) spill = c->spill.as<E>();
    return TIRT_OK;
}

// ---- the launches of a call, shared by cp_chunks, nn_chunks, tq_chunks, sw_chunks and pairs_run
// the fields every walk's Args has (CpArgs, NnArgs, TqArgs, SwArgs, PairArgs: the same names); after ensure_counters
template <class Args>
inline void point_walk_args(tirt_ctx *c, int stack_size, Args &a)
{
    a.bvh = bvh_view(c);
    a.primitive = c->primitive.as<int>(); a.prim_slot = c->prim_slot.as<int>(); a.n_prim = c->n;
    a.stack_size = stack_size;
    a.ctr = c->dev_counters.as<DevCounters>();
}
// a runtime bool as a template argument: f(std::true_type()) or f(std::false_type())
template <class F> inline void with_bool(bool b, F f) { if (b) f(std::true_type()); else f(std::false_type()); }
// `n` queries in chunks of `chunk`: the counters, the shared fields of `a`, the walk's grid -- a lane for every query of a chunk, as far as the stacks allow
// (the scan has no stack: a block per CP_BLOCK queries) -- and f(base, m, blocks, grid) per chunk of m queries in `blocks` blocks, to launch on `grid` of them
template <class Args, class F>
inline int point_walk_chunks(tirt_ctx *c, Args &a, int64_t n, int chunk, bool scan, int stack_size, F f)
{
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    point_walk_args(c, stack_size, a);
    int grid_max = 0;
    if (!scan) if (int rc = point_walk_launch_shape(c, stack_size, CP_WAVES_PER_CU, ((int64_t)(n < chunk ? n : chunk) + CP_BLOCK - 1) / CP_BLOCK, grid_max, a.spill)) return rc;
    for (int64_t base = 0; base < n; base += chunk) {
        const int m = (int)(n - base < chunk ? n - base : chunk);
        const int blocks = (m + CP_BLOCK - 1) / CP_BLOCK;
        f(base, m, blocks, scan || blocks < grid_max ? blocks : grid_max);
    }
    return TIRT_OK;
}

}  // namespace tirt
