// tirt_point_walk.h -- what a walk of a POINT over the quantised 4-wide nodes `cnode` (BvhView) is made of, once, for k_cp_walk (tirt_closest_point.hip)
// and k_sd_build (tirt_signed_distance.hip): the margin by which a child's decoded box is grown and the distance of a coordinate to it (PointMargin,
// CP_AXIS_GAP), the stack of one lane (PointStack), and on the host the grid whose stacks fit (point_walk_grid, point_walk_launch_shape).
// A wave is a block (CP_BLOCK lanes, no barrier anywhere): a lane holds one point and the blocks stride over the work.
//
// WHY THE CULL IS CONSERVATIVE.  k_cp_walk skips a subtree on lb2 > cut only, never on equality, so it suffices that lb2 <= D2 holds, as computed fp32
// numbers, for every primitive t below the node.  (k_sd_build descends where lb2 == 0 and needs the same for D2 = 0: a triangle with a corner AT the
// point.)  Write eps = 2^-24, E = the largest extent of the padded root box, C = E / 60000 = the largest cell,
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
// the distance of coordinate pk to the decoded planes of axis k of one child (dword W of its node), less the margin m_, never negative: 0 = inside the grown box
#define CP_AXIS_GAP(b_, m_, W, k, pk)                                                               \
                ({  const cp_h2v h__ = __builtin_bit_cast(cp_h2v, (unsigned)(W));                   \
                    const float mn__ = (b_).grid_min[k] + (float)h__.x * (b_).cell[k], mx__ = (b_).grid_min[k] + (float)h__.y * (b_).cell[k]; \
                    maxf(maxf(mn__ - (pk), (pk) - mx__) - (m_), 0.0f); })
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

}  // namespace tirt
