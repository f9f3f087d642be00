// tirt_multi_hit.hip -- the first k hits along each ray, in order, and the count of all hits (tirt_query_hits / tirt_trace_hits, include/tirt.h "First K hits").
// No reference counterpart as an entry point: the hit set H is what the reference's exhaustive traversal (Scene.py:702-744) would MEET -- every
// primitive whose leaf it reaches and whose test gives 0 < t < B -- where Scene.closet_hit keeps only the nearest of them.
//
//   k_multi_hit<EXHAUSTIVE, CUTOUT, COUNT_ALL>   the walk: one lane per ray, a wave is a block (no barrier), the blocks stride over the chunk (as k_cp_walk)
//   k_multi_hit_resolve                          the lists in the caller's [N, k] layout with padding, the 13-float records, the counts
//
// Nothing but trace_leaf_step (tirt_internal.h) decides whether a candidate is a hit, and nothing but MhList (tirt_multi_hit.h) where it goes in the list.
// H is a set and the list the minimum of a total order on (t, -leaf): neither depends on the order of the visits, so the ordered walk returns the
// exhaustive walk's bits if and only if it never skips a leaf whose candidate would have been accepted.
//
// THE ORDERED WALK runs on the quantised 4-wide nodes `cnode` with plain 16-byte global loads: no LDS tree top, no re-fetch, no stash.  The per-ray
// set-up and the box test are k_trace's, text and all (TR_GRID_AXIS / TR_CBOX, tirt_trace_box.h); the children are sorted near to far, the misses
// dropped, the rest pushed.  The stack is PointStack<int> (tirt_point_walk.h): 16 child codes per lane in LDS (4 KiB per block), the rest of
// stack_size in the context's spill buffer (point_walk_launch_shape).
// DISTANCE CULL, k_trace's rule with k_trace's constants: a child whose entry distance exceeds
//     lim = min(TR_CULL_SLACK * thr_t, TR_BOUND_SLACK * tmax, INF_VALUE)
// is skipped.  thr_t is the list's threshold distance (tirt_multi_hit.h): the bound B while the list has room, its worst entry's t once it is full --
// a hit beyond it cannot join, and a hit AT it joins only with a larger leaf, which the slack covers as it covers k_trace's equal-distance rule.
// With COUNT_ALL (the caller wants |H|) every element of H has to be met: the threshold term is left out and the bound alone culls, with the slack the
// occlusion query uses on its bound.  A ray whose origin is more than TR_FAR_RHO extents from the grid gets no distance cull at all, for k_trace's
// reason (from there the reference's own distances are rounding noise), and starts at far_qcode.
// THE SPHERE RULE.  The chain nodes at far_qcode hold the analytic spheres with whole-grid boxes BESIDE the root, and the tree below the root holds
// the same spheres with their padded boxes: a far-origin ray can be shown a sphere's leaf twice.  For a closest hit that is harmless (equal t, and
// leaf > hit_leaf is false); here it would enter the list twice and count twice.  The rule: A RAY THAT ENTERS THROUGH THE CHAIN NODES SKIPS EVERY SHAPE
// LEAF BELOW THE ROOT (a child of a node with index < far_qcode whose code has the shape bit).  The chain has already shown it every sphere, whatever
// the padded boxes say; spot and laser shapes have no surface.  So a leaf is met at most once by every ray, in both walks (the two-child tree of
// the exhaustive walk holds each leaf once).
// THE EXHAUSTIVE WALK (TIRT_TRAVERSE_EXHAUSTIVE) is the yardstick: the two-child `wnode` records by the reference's rule -- the root box first, then
// both children of every box that passes `slabs`, leaves untested -- with no distance cull and no VERIFY: k_trace's exhaustive branch with a list.
// A ray with a NaN component passes every `slabs` and fails every primitive test: H = {} without a walk, in both modes.  tmax <= 0 or NaN: likewise.
#include "tirt_internal.h"
#include "tirt_trace_box.h"
#include "tirt_point_walk.h"
#include "tirt_multi_hit.h"

namespace tirt {

constexpr int MH_WAVES_PER_CU = 32;          // persistent blocks per CU at most (4 KiB of LDS each)

struct MhArgs {
    BvhView bvh;
    const float4 *rec;                        // the chunk's rays: (o.xyz, d.x), (d.y, d.z, -, tmax) -- k_query_pack's records
    float4 *list; int2 *meta;                 // [k][stride] entries (t, u, v, bits leaf); per ray (entries held, |H|)
    size_t stride;                            // rays of a full chunk: the distance between two entries of one ray
    int n, k, stack_size;
    int *spill;                               // the stacks' tails (point_walk_launch_shape), or nullptr when stack_size <= CP_LDS_DEPTH
    int2 *counts;                             // TIRT_COUNT_NODES: N_box, N_leaf per ray of the chunk (or nullptr)
    DevCounters *ctr;
    CutView cut;                              // the CUTOUT instantiations alone read it (MhCutSource)
};
// (MhCutSource reads the kernel-argument segment as an MhArgs: the struct must stay k_multi_hit's first and only explicit argument)
struct MhCutSource {
    static TD void load(const float4 *&uv, const int *&tex)
    {
        const __attribute__((address_space(4))) MhArgs *ca = (const __attribute__((address_space(4))) MhArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        uv = ca->cut.uv; tex = ca->cut.tex;
    }
};

// one ray's list in the chunk scratch: entry e of ray i at list[e * stride + i], so a wave's access to entry e is one line
struct MhStore {
    float4 *p; size_t stride;
    TD MhEntry get(int e) const { const float4 v = p[(size_t)e * stride]; MhEntry r; r.t = v.x; r.u = v.y; r.v = v.z; r.leaf = __float_as_int(v.w); return r; }
    TD void set(int e, const MhEntry c) const { p[(size_t)e * stride] = make_float4(c.t, c.u, c.v, __int_as_float(c.leaf)); }
};

// one compare-exchange of the child sort: (distance, code) pairs, nearer first
TD void mh_ce(float &da, int &ca, float &db, int &cb)
{
    const bool s = db < da;
    const float lo = s ? db : da, hi = s ? da : db;
    const int clo = s ? cb : ca, chi = s ? ca : cb;
    da = lo; db = hi; ca = clo; cb = chi;
}
TD bool mh_shape_leaf(int c) { return c < 0 && !leaf_is_tri(~c); }

template <bool EXHAUSTIVE, bool CUTOUT, bool COUNT_ALL>
__global__ __launch_bounds__(CP_BLOCK) void k_multi_hit(MhArgs a)
{
    __shared__ int stk[CP_LDS_DEPTH * CP_BLOCK];       // [entry][lane]
    const BvhView &b = a.bvh;
    const int lane = threadIdx.x;
    unsigned long long n_over = 0;
    // (the names TR_GRID_AXIS reads)
    const float c_ic0 = b.inv_cell[0], c_ic1 = b.inv_cell[1], c_ic2 = b.inv_cell[2];
    const float c_ce0 = b.cell[0], c_ce1 = b.cell[1], c_ce2 = b.cell[2];
    const bool chain = b.far_qcode != b.root_qcode;     // the spheres stand beside the root for far-origin rays

    for (int base = blockIdx.x * CP_BLOCK; base < a.n; base += gridDim.x * CP_BLOCK) {      // wave-uniform
        const int q = base + lane;
        const bool live = q < a.n;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (live) { r0 = a.rec[2 * (size_t)q]; r1 = a.rec[2 * (size_t)q + 1]; }
        const v3 o = V(r0.x, r0.y, r0.z), d = V(r0.w, r1.x, r1.y);
        const float tmax = r1.w;
        const RayCtx r = make_ray(o, d);
        const bool par = ray_has_parallel_axis(r);
        const float B = tmax < INF_VALUE ? tmax : INF_VALUE;
        const bool walks = live && tmax > 0.0f && ((o.x == o.x) & (o.y == o.y) & (o.z == o.z) & (d.x == d.x) & (d.y == d.y) & (d.z == d.z));
        MhList L(a.k, B);
        const MhStore store = {a.list + q, a.stride};
        int count = 0;
        unsigned nbox = 1, nleaf = 0;

        float gAx = 0.0f, gAy = 0.0f, gAz = 0.0f, gBnx = 0.0f, gBny = 0.0f, gBnz = 0.0f, gBfx = 0.0f, gBfy = 0.0f, gBfz = 0.0f;
        int grotx = 0, groty = 0, grotz = 0;
        bool far = false;
        float cap = INF_VALUE;                  // the part of lim that does not move: min(TR_BOUND_SLACK * tmax, INF_VALUE), or no cull at all
        if (!EXHAUSTIVE) {
            // margin in cells, the same on all axes (trace_margin_cells, tirt_internal.h); rho = trace_origin_rho's expression
            const float relx__ = b.grid_min[0] - o.x, rely__ = b.grid_min[1] - o.y, relz__ = b.grid_min[2] - o.z;
            const float rho__ = maxf(maxf(absf(relx__) * b.inv_extent[0], absf(rely__) * b.inv_extent[1]), absf(relz__) * b.inv_extent[2]);
            const float mc__ = trace_margin_cells(rho__);
            far = rho__ > TR_FAR_RHO;
            TR_GRID_AXIS(relx__, d.x, r.idx, 0, gAx, gBnx, gBfx, grotx);
            TR_GRID_AXIS(rely__, d.y, r.idy, 1, gAy, gBny, gBfy, groty);
            TR_GRID_AXIS(relz__, d.z, r.idz, 2, gAz, gBnz, gBfz, grotz);
            if (!far) cap = __builtin_fminf(tmax * TR_BOUND_SLACK, INF_VALUE);
        }
        // lim of the moment: the threshold term is there for a near ray that is not counting
        auto limit = [&]() { return __builtin_fminf((COUNT_ALL || far) ? INF_VALUE : L.thr_t * TR_CULL_SLACK, cap); };
        float lim = limit();
        const bool skip_shapes = !EXHAUSTIVE && far && chain;

        int cur = CP_SENT;
        if (walks) cur = EXHAUSTIVE ? b.root_code : (far ? b.far_qcode : b.root_qcode);
        if (EXHAUSTIVE && cur >= 0) {            // the reference's first step: the root box
            float tn;
            if (!slabs(r, b.root_min[0], b.root_min[1], b.root_min[2], b.root_max[0], b.root_max[1], b.root_max[2], tn)) cur = CP_SENT;
        }
        PointStack<int> st(stk, a.spill, a.stack_size, lane);
        auto pop = [&]() { return st.empty() ? CP_SENT : st.pop(); };

        while (__builtin_amdgcn_ballot_w64(cur != CP_SENT) != 0ull) {
            // ---- node step: the lanes that are at an inner node
            if (cur >= 0) {
                if (EXHAUSTIVE) {
                    // reference order on the two-child nodes: both children of every box that passes `slabs`, leaves without a box test, right child pushed
                    const float4 *w = (const float4 *)((const char *)b.wnode + ((size_t)(unsigned)cur << 6));
                    const float4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3];
                    const int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
                    nbox += 2;
                    float tl, tr;
                    const int pl = slabs(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tl);
                    const int pr = slabs(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tr);
                    const bool hl = (pl != 0) || (cl < 0), hr = (pr != 0) || (cr < 0);
                    if (hl && hr) st.push(cr);
                    cur = hl ? cl : (hr ? cr : pop());
                } else {
                    const uint4 *w = b.cnode + (size_t)cur * 4;
                    const uint4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3];
                    int c0 = (int)q3.x, c1 = (int)q3.y, c2 = (int)q3.z, c3 = (int)q3.w;
                    nbox += 4;
                    constexpr float MISS = 3.0e38f;
                    const int lim_i = __float_as_int(lim);      // > 0: a ray that walks has tmax > 0 and hits have t > 0
                    float d0, d1, d2, d3;                        // entry distance of a hit box, MISS otherwise
                    TR_CBOX(q0.x, q0.y, q0.z, d0);
                    TR_CBOX(q0.w, q1.x, q1.y, d1);
                    TR_CBOX(q1.z, q1.w, q2.x, d2);
                    TR_CBOX(q2.y, q2.z, q2.w, d3);
                    if (skip_shapes && cur < b.far_qcode) {     // the sphere rule (head of this file)
                        if (mh_shape_leaf(c0)) d0 = MISS;
                        if (mh_shape_leaf(c1)) d1 = MISS;
                        if (mh_shape_leaf(c2)) d2 = MISS;
                        if (mh_shape_leaf(c3)) d3 = MISS;
                    }
                    mh_ce(d0, c0, d1, c1); mh_ce(d2, c2, d3, c3); mh_ce(d0, c0, d2, c2); mh_ce(d1, c1, d3, c3); mh_ce(d1, c1, d2, c2);
                    if (d3 < MISS) st.push(c3);
                    if (d2 < MISS) st.push(c2);
                    if (d1 < MISS) st.push(c1);
                    cur = (d0 < MISS) ? c0 : pop();
                }
            }
            // ---- leaf step: the lanes that are at a leaf (trace_leaf_step ballots for spheres and cut-outs)
            const bool at_leaf = cur < 0 && cur != CP_SENT;
            if (__builtin_amdgcn_ballot_w64(at_leaf) != 0ull) {
                if (at_leaf) {
                    const int code = ~cur;
                    nleaf += 1;
                    // copies of the threshold: the function overwrites them on acceptance.  Counting: against (B, -1), which is membership of H
                    float ht = COUNT_ALL ? B : L.thr_t, hu = 0.0f, hv = 0.0f;
                    int hl = COUNT_ALL ? -1 : L.thr_leaf, hp = -1;      // (hp: the record's primitive id is not kept, the resolve reads the leaf's row)
                    bool accepted;
                    if constexpr (CUTOUT) accepted = trace_leaf_step<!EXHAUSTIVE, true, MhCutSource>(b, r, par, code, ht, hu, hv, hp, hl);
                    else accepted = trace_leaf_step<!EXHAUSTIVE>(b, r, par, code, ht, hu, hv, hp, hl);
                    if (accepted) {
                        count++;
                        if (L.wants(ht, hl)) {
                            MhEntry e; e.t = ht; e.u = hu; e.v = hv; e.leaf = hl;
                            L.insert(store, e);
                            lim = limit();
                        }
                    }
                    cur = pop();
                }
            }
        }
        if (live) {
            a.meta[q] = make_int2(L.n, count);
            if (a.counts) a.counts[q] = make_int2((int)nbox, (int)nleaf);
        }
        if (st.overflow) n_over++;
    }
    n_over = wave_sum(n_over);
    if (lane == 0 && a.ctr) {
        if (n_over) atomicAdd(&a.ctr->stack_overflow, n_over);
        if (blockIdx.x == 0) atomicAdd(&a.ctr->rays_closest, (unsigned long long)a.n);
    }
}

// thread (i, j): entry j of ray i of the chunk into the caller's arrays; j == 0 also writes the count.  A record is tirt_trace_closest's: t, then
// hit_attributes (pos, gnormal, normal, tex); padding is a miss as k_query_resolve_closest writes it (the reference normalises (0, 0, 0) on a miss)
__global__ void k_multi_hit_resolve(SceneView s, const float *compact, const float4 *rec, const float4 *list, const int2 *meta, size_t stride, int64_t base,
                                    int n, int k, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *out_count)
{
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int kk = k > 0 ? k : 1;
    if (id >= (int64_t)n * kk) return;
    const int i = (int)(id % n), j = (int)(id / n);
    const int64_t g = base + i;
    const int2 m = meta[i];
    if (j == 0 && out_count) out_count[g] = m.y;
    if (j >= k) return;
    float t = INF_VALUE, u = 0.0f, v = 0.0f; int prim = -1;
    if (j < m.x) {
        const float4 e = list[(size_t)j * stride + i];
        t = e.x; u = e.y; v = e.z;
        prim = (int)compact[(size_t)__float_as_int(e.w) * CPN_VEC + 1];      // the leaf's reference row (UtilsFunc.py:get_compact_node_prim), as trace_leaf_step reads it
    }
    const int64_t at = g * k + j;
    if (out_t) out_t[at] = t;
    if (out_prim) out_prim[at] = prim;
    if (!out_hit) return;
    const float4 r0 = rec[2 * (size_t)i], r1 = rec[2 * (size_t)i + 1];
    HitAttr h; h.pos = h.gnor = h.nor = h.tex = V(0.0f, 0.0f, 0.0f);
    if (prim >= 0) h = hit_attributes(s, V(r0.x, r0.y, r0.z), V(r0.w, r1.x, r1.y), prim, t, u, v);
    else { h.gnor = normalized(h.gnor); h.nor = normalized(h.nor); }
    float *o = out_hit + at * hit_stride;
    o[0] = t;
    o[1] = h.pos.x; o[2] = h.pos.y; o[3] = h.pos.z;
    o[4] = h.gnor.x; o[5] = h.gnor.y; o[6] = h.gnor.z;
    o[7] = h.nor.x; o[8] = h.nor.y; o[9] = h.nor.z;
    o[10] = h.tex.x; o[11] = h.tex.y; o[12] = h.tex.z;
}

template <bool EXHAUSTIVE, bool CUTOUT>
static void mh_launch_as(hipStream_t st, int grid, const MhArgs &a, bool count_all)
{
    if (count_all) hipLaunchKernelGGL((k_multi_hit<EXHAUSTIVE, CUTOUT, true>), dim3(grid), dim3(CP_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_multi_hit<EXHAUSTIVE, CUTOUT, false>), dim3(grid), dim3(CP_BLOCK), 0, st, a);
}

// How many blocks walk a chunk of up to `chunk_rays` rays, with the spill buffer grown to their stacks' tails: once per call, before the chunks
int multi_hit_shape(tirt_ctx *c, int stack_size, int64_t chunk_rays, MultiHitShape &shape)
{
    int *spill = nullptr;
    if (int rc = point_walk_launch_shape(c, stack_size, MH_WAVES_PER_CU, (chunk_rays + CP_BLOCK - 1) / CP_BLOCK, shape.grid, spill)) return rc;
    shape.spill = spill;
    return TIRT_OK;
}

// one chunk on the context's stream: the walk over `n` packed rays at `rec` into list / meta, then the resolve into the caller's arrays at ray `base`
int multi_hit_chunk(tirt_ctx *c, const MultiHitShape &shape, const float4 *rec, float4 *list, int2 *meta, size_t stride, int64_t base, int n, int k,
                    int stack_size, int flags, bool count_all, int2 *counts, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride,
                    int32_t *out_count)
{
    if (int rc = ensure_cutout_records(c)) return rc;
    MhArgs a = {};
    a.bvh = bvh_view(c);
    a.rec = rec; a.list = list; a.meta = meta; a.stride = stride; a.n = n; a.k = k; a.stack_size = stack_size;
    a.spill = (int *)shape.spill; a.counts = counts; a.ctr = c->dev_counters.as<DevCounters>();
    const bool exh = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0;
    const int blocks = (n + CP_BLOCK - 1) / CP_BLOCK, grid = blocks < shape.grid ? blocks : shape.grid;
    if (c->has_cutout) {
        a.cut.uv = c->cut_uv.as<float4>(); a.cut.tex = c->tex.as<int>();
        TIRT_REQUIRE(c->cut_rec_valid && a.cut.uv && a.cut.tex, "k_multi_hit: the cut-out records are stale (internal: ensure_cutout_records was not run)");
        if (exh) mh_launch_as<true, true>(c->stream, grid, a, count_all); else mh_launch_as<false, true>(c->stream, grid, a, count_all);
    } else {
        if (exh) mh_launch_as<true, false>(c->stream, grid, a, count_all); else mh_launch_as<false, false>(c->stream, grid, a, count_all);
    }
    const int64_t threads = (int64_t)n * (k > 0 ? k : 1);
    hipLaunchKernelGGL(k_multi_hit_resolve, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, scene_view(c), c->compact.as<float>(), rec,
                       (const float4 *)list, (const int2 *)meta, stride, base, n, k, out_t, out_prim, out_hit, hit_stride, out_count);
    return TIRT_OK;
}

}  // namespace tirt
