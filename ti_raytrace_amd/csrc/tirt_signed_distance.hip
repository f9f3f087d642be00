// tirt_signed_distance.hip -- the table behind the signed queries (tirt_query_signed_distance / tirt_signed_distance, include/tirt.h "Signed distance"):
// per primitive id seven float4 -- the unit face normal and the angle-weighted pseudo-normals of the three corners and the three edges (Baerentzen & Aanaes
// 2005) -- and the three edge classes.  The sign of a query is the side of the pseudo-normal of the FEATURE its closest point lies on (sd_sign,
// tirt_closest_point.h); the face normal alone is wrong at every sharp or concave vertex and edge, where several triangles tie.
//
// The scene has no connectivity: its vertex rows are a triangle soup.  k_sd_build finds it on the device, without welding anything: one lane per triangle
// CORNER walks the quantised 4-wide nodes `cnode` from root_qcode and descends into every child whose decoded box, grown by k_cp_walk's margin
// (PointMargin: the head of tirt_point_walk.h has why it covers the decode's rounding), contains the corner's position v.  A triangle with a
// corner AT v has v in its exact box, which the quantised boxes of its leaf slot and of every ancestor contain: every such triangle is reached, once
// (a primitive has one leaf; the chain nodes at far_qcode hold analytic spheres only and are not entered).  At a triangle leaf t' that is valid
// (0 < |g|^2 < inf) and has a corner == v (three fp32 ==), the lane adds I(alpha' n') to the vertex sum, and, if the corner before or after that one
// == v1 (the end of the edge that LEAVES this lane's corner: AB for A, BC for B, CA for C), I(n') to the edge sum and t' to the edge's counts.
// I(x) = (int64) rintf(x * 2^30): the sums are integers, so they do not depend on the order of the visits, and neither does the table.
// The lane then writes its two rows; the class bits go into row 0's last word with an atomic OR (the table is zeroed first, which is also what the
// rows of spheres, spots and lasers are).  tests/signed_distance_expected.py restates all of it in numpy with brute-force matching.
//
// The stack is k_cp_walk's (PointStack, tirt_point_walk.h) with 4-byte entries (a child code; nothing is culled, so there is no lb2): CP_LDS_DEPTH per lane
// in LDS, the rest of stack_size in the context's spill buffer.  An entry that does not fit is a triangle the sums may miss: the lane raises SdState::overflow and counts in
// DevCounters::stack_overflow.  The SIGNED kernels answer NaN from such a table, tirt_stats reports TIRT_ERR_STACK, and every entry that waits for the
// stream anyway (tirt_signed_distance, _prepare, _table_download) reads the verdict and returns TIRT_ERR_STACK itself (sd_table_verdict).
#include "tirt_internal.h"
#include "tirt_closest_point.h"
#include "tirt_point_walk.h"

namespace tirt {

constexpr int SD_WAVES_PER_CU = 16;          // persistent blocks per CU at most (4 KiB of LDS each)
constexpr int SD_PREPARE_STACK = 4096;       // tirt_signed_distance_prepare / _table_download: the largest stack there is (the grid shrinks to fit its tails)

struct SdState { int overflow, pad; unsigned long long boundary, nonmanifold, flipped, invalid; };

struct SdArgs {
    BvhView bvh;
    const int *primitive, *prim_slot; int n_prim;
    int stack_size;
    int *spill;                              // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    float4 *tab; SdState *state; DevCounters *ctr;
};

TD bool sd_same(const v3 a, const v3 b) { return (a.x == b.x) & (a.y == b.y) & (a.z == b.z); }

__global__ __launch_bounds__(CP_BLOCK) void k_sd_build(SdArgs a)
{
    __shared__ int stk[CP_LDS_DEPTH * CP_BLOCK];      // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    const PointMargin pm(b);
    const int total = 3 * a.n_prim;
    unsigned long long n_over = 0, n_boundary = 0, n_nonmanifold = 0, n_flipped = 0, n_invalid = 0;

    for (int base = blockIdx.x * CP_BLOCK; base < total; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int t = base + lane;
        const int prim = t < total ? t / 3 : 0, k = t - 3 * prim;
        const bool is_tri = t < total && a.primitive[(size_t)prim * PRI_VEC] == PRIMITIVE_TRI;
        v3 v = V(0.0f, 0.0f, 0.0f), v1 = v, own_n = v; bool own_valid = true;
        if (is_tri) {
            const float4 *tp = b.tri + (size_t)a.prim_slot[prim] * TRI_STRIDE;
            const float4 ta = tp[0], tb = tp[1], tc = tp[2];
            const v3 pa = V(ta.x, ta.y, ta.z), pb = V(tb.x, tb.y, tb.z), pc = V(tc.x, tc.y, tc.z);
            v = k == 0 ? pa : (k == 1 ? pb : pc);
            v1 = k == 0 ? pb : (k == 1 ? pc : pa);
            own_valid = sd_triangle_normal(pa, pb, pc, own_n);
        }
        const float m = pm.margin(b, v);
        long long sx = 0, sy = 0, sz = 0, ex = 0, ey = 0, ez = 0;
        int others = 0, same_way = 0;
        int cur = is_tri ? b.root_qcode : CP_SENT;
        PointStack<int> st(stk, a.spill, a.stack_size, lane);
        // a child that is there and whose grown box holds v: the first becomes the next node, the others wait on the stack
#define SD_CHILD(i, X, Y, Z, code_)                                                                 \
        do {                                                                                        \
            const float gx__ = CP_AXIS_GAP(b, m, X, 0, v.x), gy__ = CP_AXIS_GAP(b, m, Y, 1, v.y), gz__ = CP_AXIS_GAP(b, m, Z, 2, v.z); \
            if (((int)(code_) != TR_EMPTY) & (gx__ == 0.0f) & (gy__ == 0.0f) & (gz__ == 0.0f)) {    \
                if (nxt == CP_SENT) nxt = (int)(code_); else st.push((int)(code_));                 \
            }                                                                                       \
        } while (0)

        while (cur != CP_SENT) {
            if (cur >= 0) {
                const uint4 *w = b.cnode + (size_t)cur * 4;
                const uint4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3];
                int nxt = CP_SENT;
                CP_EACH_CHILD(SD_CHILD);
                cur = nxt;
                if (cur == CP_SENT && !st.empty()) cur = st.pop();
            } else {
                const int code = ~cur;
                if (leaf_is_tri(code)) {
                    const float4 *tp = b.tri + (size_t)leaf_slot(code) * TRI_STRIDE;
                    const float4 ta = tp[0], tb = tp[1], tc = tp[2];
                    const int other = __float_as_int(tc.w);
                    const v3 pa = V(ta.x, ta.y, ta.z), pb = V(tb.x, tb.y, tb.z), pc = V(tc.x, tc.y, tc.z);
                    const bool e0 = sd_same(pa, v), e1 = sd_same(pb, v), e2 = sd_same(pc, v);
                    if (e0 | e1 | e2) {
                        v3 nh;
                        if (sd_triangle_normal(pa, pb, pc, nh)) {
                            // the corner at v (a valid triangle has one at most), the one after it and the one before it
                            const v3 cj = e0 ? pa : (e1 ? pb : pc), cn = e0 ? pb : (e1 ? pc : pa), cp = e0 ? pc : (e1 ? pa : pb);
                            const float alpha = sd_corner_angle(cn - cj, cp - cj);
                            sx += sd_quant(alpha * nh.x); sy += sd_quant(alpha * nh.y); sz += sd_quant(alpha * nh.z);
                            const bool at_next = sd_same(cn, v1), at_prev = sd_same(cp, v1);
                            if (at_next | at_prev) {
                                ex += sd_quant(nh.x); ey += sd_quant(nh.y); ez += sd_quant(nh.z);
                                if (other != prim) { others++; if (at_next) same_way++; }
                            }
                        }
                    }
                }
                cur = st.empty() ? CP_SENT : st.pop();
            }
        }
#undef SD_CHILD

        if (is_tri) {
            float4 *rows = a.tab + (size_t)prim * SD_ROWS;
            const int cls = others == 0 ? 1 : (others >= 2 ? 2 : (same_way ? 3 : 0));
            rows[1 + k] = make_float4((float)sx, (float)sy, (float)sz, 0.0f);
            rows[k == 0 ? 4 : (k == 1 ? 6 : 5)] = make_float4((float)ex, (float)ey, (float)ez, 0.0f);
            int bits = cls << (2 * k);
            if (k == 0) {
                float *r0 = (float *)rows;
                r0[0] = own_n.x; r0[1] = own_n.y; r0[2] = own_n.z;
                if (!own_valid) { bits |= 64; n_invalid++; }
            }
            if (bits) atomicOr((int *)rows + 3, bits);
            n_boundary += cls == 1; n_nonmanifold += cls == 2; n_flipped += cls == 3;
        }
        if (st.overflow) { a.state->overflow = 1; n_over++; }      // (the entry is lost, and the table with it)
    }
    n_over = wave_sum(n_over); n_boundary = wave_sum(n_boundary); n_nonmanifold = wave_sum(n_nonmanifold);
    n_flipped = wave_sum(n_flipped); n_invalid = wave_sum(n_invalid);
    if (lane == 0) {
        if (n_over && a.ctr) atomicAdd(&a.ctr->stack_overflow, n_over);
        if (n_boundary) atomicAdd(&a.state->boundary, n_boundary);
        if (n_nonmanifold) atomicAdd(&a.state->nonmanifold, n_nonmanifold);
        if (n_flipped) atomicAdd(&a.state->flipped, n_flipped);
        if (n_invalid) atomicAdd(&a.state->invalid, n_invalid);
    }
}

// the build, queued on the context's stream
static int sd_table_build(tirt_ctx *c, int stack_size)
{
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    const size_t tab_bytes = sizeof(float4) * SD_ROWS * (size_t)c->n;
    if (tab_bytes > c->sd_tab.bytes || !c->sd_state.p) {      // growing frees the old buffer, which queued work may still use
        TIRT_HIP(hipStreamSynchronize(c->stream));
        if (c->sd_tab.ensure(tab_bytes) || c->sd_state.ensure(sizeof(SdState))) return TIRT_ERR_HIP;
    }
    c->sd_tab_valid = false;
    SdArgs a = {};
    a.bvh = bvh_view(c);
    a.primitive = c->primitive.as<int>(); a.prim_slot = c->prim_slot.as<int>(); a.n_prim = c->n;
    a.stack_size = stack_size;
    a.tab = c->sd_tab.as<float4>(); a.state = c->sd_state.as<SdState>(); a.ctr = c->dev_counters.as<DevCounters>();
    int grid;
    if (int rc = point_walk_launch_shape(c, stack_size, SD_WAVES_PER_CU, ((int64_t)3 * c->n + CP_BLOCK - 1) / CP_BLOCK, grid, a.spill)) return rc;
    TIRT_HIP(hipMemsetAsync(c->sd_tab.p, 0, tab_bytes, c->stream));
    TIRT_HIP(hipMemsetAsync(c->sd_state.p, 0, sizeof(SdState), c->stream));
    hipLaunchKernelGGL(k_sd_build, dim3(grid), dim3(CP_BLOCK), 0, c->stream, a);
    TIRT_HIP(hipGetLastError());
    c->sd_tab_valid = true; c->sd_tab_checked = false; c->sd_tab_stack = stack_size;
    return TIRT_OK;
}

// A table that stands is kept; one whose verdict nobody has read is made again only by a call that brings a larger stack than it was built with
int sd_table_ensure(tirt_ctx *c, int stack_size)
{
    if (c->sd_tab_valid && (c->sd_tab_checked || stack_size <= c->sd_tab_stack)) return TIRT_OK;
    return sd_table_build(c, stack_size);
}

static int sd_table_state(tirt_ctx *c, const char *fn, SdState &h)
{
    TIRT_HIP(hipMemcpyAsync(&h, c->sd_state.p, sizeof(SdState), hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    if (h.overflow) {
        c->sd_tab_valid = false;
        set_error(std::string(fn) + ": the build of the signed-distance table ran out of traversal stack (stack_size " + std::to_string(c->sd_tab_stack) +
                  "): there is no table, raise stack_size");
        return TIRT_ERR_STACK;
    }
    c->sd_tab_checked = true;
    return TIRT_OK;
}

int sd_table_verdict(tirt_ctx *c, const char *fn)
{
    if (!c->sd_tab_valid || c->sd_tab_checked) return TIRT_OK;
    SdState h;
    return sd_table_state(c, fn, h);
}

// the table made now, with the largest stack unless one stands already, and waited for
static int sd_table_now(tirt_ctx *c, const char *fn, SdState &h)
{
    TIRT_REQUIRE(c->built, std::string(fn) + ": LBVH not built");
    if (!c->sd_tab_valid || (!c->sd_tab_checked && c->sd_tab_stack < SD_PREPARE_STACK))
        if (int rc = sd_table_build(c, SD_PREPARE_STACK)) return rc;
    return sd_table_state(c, fn, h);
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_signed_distance_prepare(tirt_ctx *c, int64_t report[5])
{
    CTX(c);
    SdState h;
    if (int rc = sd_table_now(c, "tirt_signed_distance_prepare", h)) return rc;
    if (report) {
        report[0] = (int64_t)h.boundary; report[1] = (int64_t)h.nonmanifold; report[2] = (int64_t)h.flipped; report[3] = (int64_t)h.invalid;
        report[4] = c->n;
    }
    return TIRT_OK;
}

int tirt_signed_distance_table_download(tirt_ctx *c, float *out)
{
    TIRT_REQUIRE(out, "tirt_signed_distance_table_download: null pointer");
    CTX(c);
    SdState h;
    if (int rc = sd_table_now(c, "tirt_signed_distance_table_download", h)) return rc;
    TIRT_HIP(hipMemcpyAsync(out, c->sd_tab.p, sizeof(float4) * SD_ROWS * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

}  // extern "C"
