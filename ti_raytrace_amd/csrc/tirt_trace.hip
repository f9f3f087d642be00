// tirt_trace.hip -- BVH traversal: k_trace, its launchers and trace_rays.
//
// Reference path: Scene.closet_hit (Scene.py:702-744, traversal stack in GLOBAL memory, exhaustive visit order, no t-culling) and
// Scene.closet_hit_shadow (:671-699), inlined per pixel by the reference's integrators; here one kernel over dense ray queues, launched per
// bounce by the wavefront pipeline (tirt_render.hip) and per batch of rays by everything else (trace_rays).
//
// Traversal: persistent waves, one ray per lane with re-fetch, traversal stack in LDS ([entry][lane]
// layout: conflict-free) with a paged global-memory spill buffer.  Two visiting rules, same closest hit:
//   EXHAUSTIVE  the reference's, on the 64-byte two-child nodes: every internal node whose box
//               passes `slabs` has both children visited, leaves are intersected unconditionally.
//               Used for the N_box / N_leaf "algorithmic bytes" counts and as a parity cross-check.
//   ORDERED     on the 64-byte quantised 4-wide nodes (tirt_internal.h `cnode`; top five levels in LDS):
//               children near to far, children whose entry distance exceeds the current hit (with a
//               1e-4 relative margin) are skipped, leaf children are pre-tested against their (slightly
//               inflated) box.  The quantised boxes contain the reference's; a candidate hit is accepted
//               only if the reference would have reached that leaf (`slabs` on the exact boxes, see
//               BvhView), so the closest hit is the reference's.  Product default.
// Exact-t ties are resolved as the reference's visit order does (it pops the right child
// first and keeps the first-found candidate on `t < hit_t`): the candidate with the larger
// compact-node index wins.
#include "tirt_trace.h"
#include "tirt_trace_box.h"

namespace tirt {

// The bound ladder (TR_PAD / TR_PADG) is compiled only with -DTIRT_EXPERIMENTS (`make experiments` -> libtirt_exp.so).  What rounds 3-5 built, measured and did not adopt
// left this file in round 6 and can be put back from tools/exp/patches/: the settled A/B switches (stash, drained-slices count, node-loop threshold, quad-cooperative fetch,
// non-temporal streams, asm record fetch, drain diagnostics, no-verify: r06_settled_ab_switches_of_k_trace.patch) and the persistent tail kernel (KIND_TAIL: the rest of a
// batch in one launch, a lane keeping a PATH through shade / shadow ray / next ray; bit-identical, slower at every switch point: r06_persistent_tail_kernel.patch).
#if !defined(TIRT_EXPERIMENTS) && (defined(TR_PAD) || defined(TR_PADG))
#error "the bound ladder (TR_PAD / TR_PADG) needs an experiments build: add -DTIRT_EXPERIMENTS"
#endif

// Persistent waves with ray re-fetch ("while-while" traversal): every wave keeps pulling rays
// from the queue through one wave-aggregated atomic whenever at least TR_REFILL_MIN of its 64
// lanes are idle, so that a few long rays do not leave the other lanes of the wave parked
// (a one-ray-per-lane loop measured 15 % VALU lane utilisation on this workload).  Inner-node
// steps and triangle tests run in separate loops so that lanes doing the same thing run together.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) int lds_int;
constexpr int TR_PAGE = 8;                    // stack entries moved per page-out / page-in
constexpr int TR_SENT = (int)0x80000000;      // "stack empty": never a node index nor a leaf code

constexpr int TR_MIN_WAVES = 6;        // 80 VGPRs: five 256-thread blocks per CU and room for a shading wave per SIMD (tirt_internal.h, TR_TOP_CAP)
// The arguments a ray only needs when it is fetched, written back or paged (40 pointers, the grid constants) are NOT read from the by-value
// argument: held in SGPRs across the whole walk they overflow the scalar register file, and the compiler parks them in VGPR lanes --
// v_writelane / v_readlane, VALU instructions, ~245 of them per refill of a kernel that is bound by VALU issue.  They are read from the
// kernel-argument segment where they are needed instead (scalar loads: no VALU), through a pointer the optimiser cannot see through, so
// that it can neither hoist the loads out of the persistent loop nor keep their results alive across it.
typedef const __attribute__((address_space(4))) TraceArgs *cold_args_t;
#define TR_COLD(ca) cold_args_t ca = (cold_args_t)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(ca))

// ---- bound ladder (tools/ladder.sh, profiles/r05_bound_ladder.txt; experiments only, nothing of it in the product build) ----
// What limits k_trace is asked of the kernel itself: -DTR_PAD=k adds k VALU instructions to every node visit that change nothing (v_fma_f32 x, x, 1.0, 0
// on the nine grid registers of the ray: independent chains, no extra register, films stay bit-identical) -- a kernel bound by VALU issue slows down
// from k = 0 on by k / (instructions of a visit), one with slack does not until the slack is used; -DTR_PAD_LATE puts them behind the sort (in the
// dependent chain of the visit) instead of behind the loads (in the shadow of their latency).  -DTR_PADG=k adds k dummy gathers -- one dword from
// k other 64-byte node records, landed in a scratch kilobyte of LDS by global_load_lds, so that no register and no wait is spent on them: load on
// the texture-address / L1 / L2 path only (+ 3 VALU each for the address).
#if defined(TR_PAD) || defined(TR_PADG)
#ifndef TR_PAD
#define TR_PAD 0
#endif
#ifndef TR_PADG
#define TR_PADG 0
#endif
#ifdef TR_PAD_LATE
#define TR_PAD_WHERE 1
#else
#define TR_PAD_WHERE 0
#endif
#ifdef TR_PAD_MAX          // the pad as an instruction of the node step's own class (v_max / v_min / v_cmp / v_cndmask / v_alignbit / v_fma_mix issue at half the rate of v_fma / v_add: tools/micro/valu_issue.hip)
#define TR_PAD1(reg) asm volatile("v_max_f32 %0, %0, %0" : "+v"(reg))
#else
#define TR_PAD1(reg) asm volatile("v_fma_f32 %0, %0, 1.0, 0" : "+v"(reg))
#endif
#define TR_LADDER_PADS(where)                                                                        \
    do {                                                                                             \
        if ((where) == TR_PAD_WHERE) {                                                               \
            _Pragma("unroll") for (int p__ = 0; p__ < TR_PAD; p__++) {                               \
                switch (p__ % 9) {                                                                   \
                case 0: TR_PAD1(gAx); break; case 1: TR_PAD1(gAy); break; case 2: TR_PAD1(gAz); break;      \
                case 3: TR_PAD1(gBnx); break; case 4: TR_PAD1(gBny); break; case 5: TR_PAD1(gBnz); break;   \
                case 6: TR_PAD1(gBfx); break; case 7: TR_PAD1(gBfy); break; default: TR_PAD1(gBfz); break;  \
                }                                                                                    \
            }                                                                                        \
        }                                                                                            \
        if ((where) == 0) {                                                                          \
            _Pragma("unroll") for (int g__ = 0; g__ < TR_PADG; g__++) {                              \
                const unsigned dn__ = ((unsigned)cur + 977u * (unsigned)(g__ + 1)) & 32767u;         \
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const char *)b.cnode + (dn__ << 6)), \
                    (__attribute__((address_space(3))) void *)(size_t)(top_base + (unsigned)TR_TOP_SLOTS * 64u + (unsigned)(tid & ~63) * 4u), 4, 0, 0); \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#else
#define TR_LADDER_PADS(where) do { } while (0)
#endif

// (CutSource reads the kernel-argument segment as a TraceArgsCut: the struct must stay k_trace's first and only explicit argument, TraceArgs its base at offset 0)
static_assert(std::is_base_of<TraceArgs, TraceArgsCut>::value && sizeof(TraceArgsCut) >= sizeof(TraceArgs) + sizeof(CutView) && sizeof(TraceArgsCut) <= sizeof(TraceArgs) + 2 * sizeof(CutView),
              "TraceArgsCut is TraceArgs with the CutView behind it");
struct CutSource {
    static TD void load(const float4 *&uv, const int *&tex)
    {
        const __attribute__((address_space(4))) TraceArgsCut *ca = (const __attribute__((address_space(4))) TraceArgsCut *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ca));
        uv = ca->cut.uv; tex = ca->cut.tex;
    }
};
template <int MODE, bool COUNT, int KIND, bool CUTOUT = false>
__global__ __launch_bounds__(TR_BLOCK, TR_MIN_WAVES) void k_trace(typename trace_args_of<CUTOUT>::type a)
{
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];      // [lds_depth][TR_BLOCK]
    const int TR_LDS_DEPTH = a.lds_depth;
    constexpr bool MAY_SHADOW = (KIND != KIND_CLOSEST);
    constexpr bool STASH = (MODE != TIRT_TRAVERSE_EXHAUSTIVE);
    constexpr bool BOUNDED = MAY_SHADOW && (MODE != TIRT_TRAVERSE_EXHAUSTIVE);
    const int count_c = (KIND == KIND_SHADOW_ACC || KIND == KIND_QUERY) ? 0 : (a.count_ptr ? *a.count_ptr : a.count_fixed);
    const int count_s = (KIND == KIND_CLOSEST) ? 0 : (KIND == KIND_MIXED ? *a.scount_ptr : (a.count_ptr ? *a.count_ptr : a.count_fixed));
    const int count = count_c + count_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t gstride = (size_t)gridDim.x * TR_BLOCK, gtid = (size_t)blockIdx.x * TR_BLOCK + tid;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const BvhView &b = a.bvh;

    // per-lane ray state
    bool have = false, par = false, is_sh = (KIND == KIND_SHADOW_ACC || KIND == KIND_QUERY);
    int q = 0, cur = TR_SENT, hit_prim = -1, hit_leaf = -1, expect = -3;
    int pend = 0;                               // ordered mode: one stashed leaf code (0 = none; leaf codes are negative)
    unsigned n_overflow = 0;
    float hit_t = INF_VALUE, hit_u = 0.0f, hit_v = 0.0f, cull_far = 3.0e38f, settle = -1.0f;
    float lim = INF_VALUE;                      // ordered mode: min(hit_t * 1.0001, cull_far, INF_VALUE), entry distances beyond it are skipped
    // (ordered mode: a NEGATIVE cull_far marks a ray whose origin is more than TR_FAR_RHO root-box extents away -- no distance culling for it, see the set-up code)
    unsigned nbox = 0, nleaf = 0;
    RayCtx r = {};
    // ordered mode: the ray in the grid of the quantised nodes.  Plane h (fp16, in cells) of axis a is crossed at
    // t = h * gA + gB (gA = cell / d, gB = (grid_min - o) / d); gBn / gBf are gB moved outward by a margin of
    // 0.25 cells + 0.25 cells per root-box extent of distance between the origin and the grid (see the set-up code
    // for what it covers); grot = 16 where gA < 0 rotates a (min | max << 16) plane
    // pair so that the low half is always the near plane.  Axis-parallel components (|d| < 1e-6, where the
    // reference tests the origin against the slab instead, UtilsFunc.py:500-503) do the same in grid units through
    // the same two FMAs: gA = 1e30, gBn / gBf = (-(origin cell) -+ margin) * 1e30, so that the "near distance" is hugely
    // negative or positive and the "far distance" hugely positive or negative according to the side of the planes
    // the origin lies on.  (Ignoring such an axis would be conservative too, but a ray that ignores an axis walks a
    // whole slice of the scene: a few of them per million rays set the duration of every launch.)
    float gAx = 0.0f, gAy = 0.0f, gAz = 0.0f, gBnx = 0.0f, gBny = 0.0f, gBnz = 0.0f, gBfx = 0.0f, gBfy = 0.0f, gBfz = 0.0f;
    int grotx = 0, groty = 0, grotz = 0;
    bool exhausted = false;
    unsigned long long tk_start = 0, tk_exh = 0;
    if (COUNT) tk_start = wall_clock64();
    const int S_LOG = a.slice_log2, S_MASK = (1 << S_LOG) - 1;
    int home = (int)((blockIdx.x * (TR_BLOCK / 64) + (tid >> 6)) & S_MASK), tried = 0;      // wave-uniform
    const int full_chunks = count >> 6;
    unsigned long long sum_box = 0, sum_leaf = 0, sum_box_s = 0, sum_leaf_s = 0, n_over = 0;
    unsigned long long d_it_node = 0, d_lanes_node = 0, d_it_leaf = 0, d_lanes_leaf = 0, d_refills = 0, d_outer = 0;

    // Traversal stack.  `sa` is the LDS address of the TOP entry; entry e of a lane lives at
    // lds_stack + e * TR_BLOCK * 4 + tid * 4.  Entry 0 is a sentinel (TR_SENT, written once), so a pop
    // needs no emptiness test; entries 1 .. TR_LDS_DEPTH-1 hold the stack.  A lane whose LDS part is
    // full pages its oldest TR_PAGE entries out to the global spill buffer ([entry][global thread])
    // and pages them back in when it pops the sentinel -- both on wave-uniform cold paths outside the
    // inner-node loop (which leaves as soon as some lane's LDS part is full), so the hot loop only
    // ever touches LDS.  Addresses are compared as signed ints: after popping the sentinel `sa` is one
    // entry below the bottom.
    constexpr unsigned ENTRY = TR_BLOCK * 4u;
    const unsigned sa_bottom = (unsigned)(size_t)(lds_int *)lds_stack + (unsigned)tid * 4u;
    const unsigned sa_hi = (unsigned)(TR_LDS_DEPTH - 3) * ENTRY + sa_bottom;     // a step pushes up to three entries: page out at this fill level
    unsigned sa = sa_bottom;
    int paged = 0;                              // pages of this lane's stack that live in the spill buffer
#define LDS_AT(addr) (*(lds_int *)(size_t)(addr))
    LDS_AT(sa_bottom) = TR_SENT;
    // the top TR_TOP_LEVELS levels of the 4-wide tree (7 x 16 bytes per record) sit behind the stacks: a
    // visit there costs LDS bandwidth instead of the texture-address path this kernel is bound by
    const unsigned top_base = (unsigned)(size_t)(lds_int *)lds_stack + (unsigned)TR_LDS_DEPTH * ENTRY;
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) u4v lds_u4;
    if (MODE != TIRT_TRAVERSE_EXHAUSTIVE) {
        for (int k = tid; k < b.top_count * 4; k += TR_BLOCK)
        { const uint4 g = b.cnode[k]; *(lds_u4 *)(size_t)(top_base + (unsigned)k * 16u) = u4v{g.x, g.y, g.z, g.w}; }
        __syncthreads();
    }
#define TR_PAGE_OUT()                                                                                \
    do {                                                                                             \
        TR_COLD(ca);                                                                                 \
        if ((paged + 1) * TR_PAGE <= ca->spill_depth) {                                                \
            for (int k__ = 0; k__ < TR_PAGE; k__++)                                                  \
                ca->spill[(size_t)(paged * TR_PAGE + k__) * gstride + gtid] = LDS_AT(sa_bottom + (unsigned)(k__ + 1) * ENTRY); \
            for (unsigned e__ = sa_bottom + (TR_PAGE + 1) * ENTRY; e__ <= sa; e__ += ENTRY)          \
                LDS_AT(e__ - TR_PAGE * ENTRY) = LDS_AT(e__);                                         \
            sa -= TR_PAGE * ENTRY; paged++;                                                          \
        } else { n_overflow++; sa -= ENTRY; }      /* out of room: the entry on top is lost (counted) */ \
    } while (0)
#define TR_PAGE_IN()                                                                                 \
    do {                                                                                             \
        TR_COLD(ca);                                                                                 \
        paged--;                                                                                     \
        for (int k__ = 0; k__ < TR_PAGE; k__++)                                                      \
            LDS_AT(sa_bottom + (unsigned)(k__ + 1) * ENTRY) = ca->spill[(size_t)(paged * TR_PAGE + k__) * gstride + gtid]; \
        sa = sa_bottom + TR_PAGE * ENTRY;                                                            \
    } while (0)
#define TR_POP(dst) do { dst = LDS_AT(sa); sa -= ENTRY; } while (0)

    for (;;) {
        // ---- refill idle lanes -------------------------------------------------------------
        const unsigned long long idle = ballot64(!have);
        if (idle != 0ull && !exhausted && (__popcll(idle) >= a.refill_min || idle == ~0ull)) {
            TR_COLD(ca);
            // (all of them read here, in one batch of scalar loads with one wait: left to itself the compiler loads each where it is used,
            // a chain of a dozen dependent round trips per refill)
            int *const c_fetch = ca->fetch;
            const float *const c_ox = ca->ox, *const c_oy = ca->oy, *const c_oz = ca->oz, *const c_dx = ca->dx, *const c_dy = ca->dy, *const c_dz = ca->dz;
            const float *const c_sox = MAY_SHADOW ? ca->sox : nullptr, *const c_soy = MAY_SHADOW ? ca->soy : nullptr, *const c_soz = MAY_SHADOW ? ca->soz : nullptr;
            const float *const c_sdx = MAY_SHADOW ? ca->sdx : nullptr, *const c_sdy = MAY_SHADOW ? ca->sdy : nullptr, *const c_sdz = MAY_SHADOW ? ca->sdz : nullptr;
            const int *const c_sprim = MAY_SHADOW ? ca->sprim : nullptr; const float *const c_sdist = MAY_SHADOW ? ca->sdist : nullptr;
            const float4 *const c_ray4 = (KIND == KIND_CLOSEST || KIND == KIND_QUERY) ? ca->ray4 : nullptr;
            const int *const c_rindex = (KIND == KIND_QUERY) ? ca->ray_index : nullptr;
            const float c_gm0 = ca->bvh.grid_min[0], c_gm1 = ca->bvh.grid_min[1], c_gm2 = ca->bvh.grid_min[2];
            const float c_ie0 = ca->bvh.inv_extent[0], c_ie1 = ca->bvh.inv_extent[1], c_ie2 = ca->bvh.inv_extent[2];
            const float c_ic0 = ca->bvh.inv_cell[0], c_ic1 = ca->bvh.inv_cell[1], c_ic2 = ca->bvh.inv_cell[2];
            const float c_ce0 = ca->bvh.cell[0], c_ce1 = ca->bvh.cell[1], c_ce2 = ca->bvh.cell[2];
            const float c_rn0 = ca->bvh.root_min[0], c_rn1 = ca->bvh.root_min[1], c_rn2 = ca->bvh.root_min[2];
            const float c_rx0 = ca->bvh.root_max[0], c_rx1 = ca->bvh.root_max[1], c_rx2 = ca->bvh.root_max[2];
            const int c_root = ca->bvh.root_code, c_rootq = ca->bvh.root_qcode, c_farq = ca->bvh.far_qcode;
            asm volatile("" :: "s"(c_fetch), "s"(c_ox), "s"(c_oy), "s"(c_oz), "s"(c_dx), "s"(c_dy), "s"(c_dz), "s"(c_gm0), "s"(c_gm1), "s"(c_gm2), "s"(c_ie0), "s"(c_ie1), "s"(c_ie2),
                         "s"(c_ic0), "s"(c_ic1), "s"(c_ic2), "s"(c_ce0), "s"(c_ce1), "s"(c_ce2), "s"(c_rn0), "s"(c_rn1), "s"(c_rn2), "s"(c_rx0), "s"(c_rx1), "s"(c_rx2));
            if (MAY_SHADOW) asm volatile("" :: "s"(c_sox), "s"(c_soy), "s"(c_soz), "s"(c_sdx), "s"(c_sdy), "s"(c_sdz), "s"(c_sprim), "s"(c_sdist));
            if (KIND == KIND_CLOSEST || KIND == KIND_QUERY) asm volatile("" :: "s"(c_ray4), "s"(c_rindex));
            const unsigned long long fm = idle;
            int my = count;
            if (fm != 0ull && !exhausted) {
            const int n_idle = __popcll(fm);
            if (COUNT) d_refills++;
            const int leader = __ffsll((long long)fm) - 1;
            // rays of slice `home`: its 64-ray chunks are the global chunks home, home + S, home + 2S, ... (interleaved), or the home-th contiguous
            // stretch of the closest-hit rays followed by the home-th stretch of the shadow rays (slices_contig)
            const bool contig = ca->slices_contig != 0;
            const int Lc__ = ((((count_c + 63) >> 6) + S_MASK) >> S_LOG) << 6, Ls__ = ((((count_s + 63) >> 6) + S_MASK) >> S_LOG) << 6;
            int lenc__ = count_c - home * Lc__; lenc__ = lenc__ < 0 ? 0 : (lenc__ > Lc__ ? Lc__ : lenc__);
            int lens__ = count_s - home * Ls__; lens__ = lens__ < 0 ? 0 : (lens__ > Ls__ ? Ls__ : lens__);
            const int len = contig ? lenc__ + lens__
                                   : (((full_chunks >> S_LOG) + (home < (full_chunks & S_MASK) ? 1 : 0)) << 6) + (home == (full_chunks & S_MASK) ? (count & 63) : 0);
            int base = 0;
            if (lane == leader) base = atomicAdd(c_fetch + home * TR_FETCH_STRIDE, n_idle);
            base = __shfl(base, leader, 64);
            const int v = base + __popcll(fm & lt_mask);                  // index within the slice
            if (contig) my = v < lenc__ ? home * Lc__ + v : (v < len ? count_c + home * Ls__ + (v - lenc__) : count);
            else my = v < len ? (((((v >> 6) << S_LOG) + home) << 6) | (v & 63)) : count;
            if (base + n_idle >= len) {                                    // slice drained: move on
                // The wave whose fetch reached the end of a slice counts the slice as drained, and a wave that moves on looks at that count: once it
                // says "all of them" there is nothing to look for.  Without it every wave of a launch learns that by one atomic round trip per
                // slice, 32 in a row on 32 lines that 5 120 waves are hammering: ~0.15 ms, the better part of what a launch of few rays takes.
                int *const c_drained = c_fetch + TR_SLICES_MAX * TR_FETCH_STRIDE;
                if (lane == leader && base < (len > 0 ? len : 1)) atomicAdd(c_drained, 1);
                if (__hip_atomic_load(c_drained, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > S_MASK) tried = S_MASK;
                home = (home + 1) & S_MASK;
                if (++tried > S_MASK) { exhausted = true; if (COUNT) tk_exh = wall_clock64(); }
            }
            }
            const bool setup_now = !have && my < count;
            if (setup_now) {
                q = my;
                if (KIND == KIND_MIXED) { is_sh = my >= count_c; if (is_sh) q = my - count_c; }
                const bool mixed_sh = (KIND == KIND_MIXED) && is_sh;
                v3 o, d; int rec_expect = -3; float rec_bound = -1.0f;
                const bool from_rec = (KIND == KIND_CLOSEST || KIND == KIND_QUERY) && c_ray4 != nullptr;          // wave-uniform
                if (from_rec) {
                    const size_t ri = (KIND == KIND_QUERY && c_rindex) ? (size_t)c_rindex[q] : (size_t)q;
                    const float4 r0 = c_ray4[2 * ri], r1 = c_ray4[2 * ri + 1];
                    o = V(r0.x, r0.y, r0.z); d = V(r0.w, r1.x, r1.y); rec_expect = __float_as_int(r1.z); rec_bound = r1.w;
                } else {
#define TR_LDS_(p) __builtin_nontemporal_load(&(p))
                    o = mixed_sh ? V(TR_LDS_(c_sox[q]), TR_LDS_(c_soy[q]), TR_LDS_(c_soz[q]))
                                 : ((KIND == KIND_CLOSEST && c_ox == nullptr) ? V(ca->eye[0], ca->eye[1], ca->eye[2]) : V(TR_LDS_(c_ox[q]), TR_LDS_(c_oy[q]), TR_LDS_(c_oz[q])));
                    d = mixed_sh ? V(TR_LDS_(c_sdx[q]), TR_LDS_(c_sdy[q]), TR_LDS_(c_sdz[q])) : V(TR_LDS_(c_dx[q]), TR_LDS_(c_dy[q]), TR_LDS_(c_dz[q]));
                }
                r = make_ray(o, d);
                par = ray_has_parallel_axis(r);
                hit_t = INF_VALUE; hit_u = 0.0f; hit_v = 0.0f; hit_prim = -1; hit_leaf = -1;
                nbox = 1; nleaf = 0; sa = sa_bottom; paged = 0; n_overflow = 0; pend = 0;
                cull_far = 3.0e38f; settle = -1.0f; expect = -3;
                float t_bound = -1.0f;
                if (MAY_SHADOW && is_sh) {
                    expect = from_rec ? rec_expect : TR_LDS_(c_sprim[q]);
                    if (BOUNDED) t_bound = from_rec ? rec_bound : TR_LDS_(c_sdist[q]);
                }
                if (MODE != TIRT_TRAVERSE_EXHAUSTIVE) {
                    // margin in cells, the same on all axes (trace_margin_cells, tirt_internal.h: what it has to cover); rho = trace_origin_rho's expression on the cold arguments
                    const float relx__ = c_gm0 - o.x, rely__ = c_gm1 - o.y, relz__ = c_gm2 - o.z;
                    const float rho__ = maxf(maxf(absf(relx__) * c_ie0, absf(rely__) * c_ie1), absf(relz__) * c_ie2);
                    const float mc__ = trace_margin_cells(rho__);
                    // From far away the reference's Moller-Trumbore returns distances that are rounding noise (its o - v0 carries
                    // |o - v0| * 2^-24, divided by a determinant of the order of the triangle's area): a small or edge-on triangle
                    // seen from hundreds of extents away can "hit" tens of units in FRONT of the surface the ray really meets first,
                    // and the reference, which never culls by distance, takes it.  A ray that starts more than TR_FAR_RHO extents
                    // from the grid therefore does not cull by distance either (no hit-distance cull, no target-distance bound):
                    // it visits every leaf whose boxes it passes, as the reference does, and so finds the same candidates.
                    if (rho__ > TR_FAR_RHO) cull_far = -3.0e38f;
                    // (TR_GRID_AXIS, and TR_CBOX of the node step: tirt_trace_box.h, one text for this kernel and k_multi_hit)
                    TR_GRID_AXIS(relx__, d.x, r.idx, 0, gAx, gBnx, gBfx, grotx);
                    TR_GRID_AXIS(rely__, d.y, r.idy, 1, gAy, gBny, gBfy, groty);
                    TR_GRID_AXIS(relz__, d.z, r.idz, 2, gAz, gBnz, gBfz, grotz);
                }
                if (BOUNDED && t_bound > 0.0f && cull_far > 0.0f) { cull_far = t_bound * TR_BOUND_SLACK; settle = t_bound * 0.99f; }
                lim = __builtin_fminf(__builtin_fminf(hit_t * TR_CULL_SLACK, __builtin_fabsf(cull_far)), INF_VALUE);      // (v_min: a canonical value, so the node loop does not re-canonicalise it every step)
                // (a far-origin ray cannot trust the padded boxes of the analytic spheres: it starts at a chain node that holds the root and
                // those spheres with whole-grid boxes, BvhView::far_qcode, and so tests them whatever their boxes say -- as the reference does)
                cur = (MODE == TIRT_TRAVERSE_EXHAUSTIVE) ? c_root : (cull_far < 0.0f ? c_farq : c_rootq);
                // The reference's first step: the root box.  The ordered walk only needs it as a shortcut -- a candidate is accepted after the boxes
                // of ALL its ancestors, the root's included, have been seen to pass `slabs` (leaf phase) --, and it is a shortcut for rays that
                // start outside the scene (camera rays: KIND_CLOSEST).  Bounce and shadow rays start on a surface inside the root box and pass it:
                // for them the test (~30 instructions per refill, at a fifth of the lanes) is skipped and the rare outsider spends one node step instead.
                if ((MODE == TIRT_TRAVERSE_EXHAUSTIVE || KIND == KIND_CLOSEST) && cur >= 0) {
                    float tn;
                    if (!slabs(r, c_rn0, c_rn1, c_rn2, c_rx0, c_rx1, c_rx2, tn)) cur = TR_SENT;
                }
                // A ray with a NaN component passes every `slabs` test (all comparisons are false)
                // and fails every primitive test, in the reference as well: it walks the whole tree
                // and misses.  Same result, without the walk (ordered mode; the exhaustive mode keeps the walk).  (NaN shading normals come from
                // process_normal's acos of a dot product just above 1, Scene.py:377.)
                if (MODE != TIRT_TRAVERSE_EXHAUSTIVE &&
                    !((o.x == o.x) & (o.y == o.y) & (o.z == o.z) & (d.x == d.x) & (d.y == d.y) & (d.z == d.z))) cur = TR_SENT;
                have = true;
            }
        }
        if (ballot64(have) == 0ull) { if (exhausted) break; continue; }

        // ---- inner nodes.  Lanes that reached a leaf (or finished) wait here; the loop goes on
        // while at least node_min lanes still have inner-node work, or nobody is waiting at all.
        // (idle lanes keep cur == TR_SENT, so `cur >= 0` alone means "has inner-node work".)
        // Written to keep the VALU and SALU instruction counts down (59 VALU per step, was 82): the
        // t-cull folded into the far distance, selects on lane masks, stack push/pop without index
        // arithmetic or emptiness tests, no cold code inside the loop.
        // A lane that reaches a leaf does not stop there: the leaf goes into a one-entry stash (`pend`) and the walk
        // goes on with the next stack entry; only a second leaf makes the lane wait.  The primitive tests then run for
        // all stashed leaves of the wave together (lane utilisation of the node loop 0.61 -> 0.73, of the leaf phase 0.38 -> 0.45), at the
        // price of a few node visits the earlier hit would have culled (+2 %).
        if (STASH) { if (have && cur < 0 && cur != TR_SENT && pend == 0) { pend = cur; TR_POP(cur); } }
        const int lim_i = __float_as_int(lim);                  // > 0 always
        // The node loop is left once fewer than node_min lanes have node work and some lane waits at a leaf -- at most: a wave that holds few
        // rays (the end of a launch, no refill any more) would leave it for every single leaf, so the threshold is also bounded by 3/4 of
        // the lanes that hold a ray at all (1/2 and 5/8: no gain, 7/8: half of it; a lone batch -- one rank's share of an 8-GPU job --
        // 3.13 -> 3.06 ms per step, four overlapped batches unchanged: profiles/r04g_node_threshold_ab.log)
        constexpr int TR_NODE_FRAC = 6;
        int node_min_w = (__popcll(ballot64(have)) * TR_NODE_FRAC) >> 3; node_min_w = node_min_w < a.node_min ? node_min_w : a.node_min;
        for (;;) {
            const bool act = cur >= 0;
            const unsigned long long am = ballot64(act);
            if (am == 0ull) break;
            const int n_act = __popcll(am);
            if (n_act < node_min_w && ballot64(have && cur < 0) != 0ull) break;
            if (wave_any((int)sa >= (int)sa_hi)) break;        // a lane's LDS stack is full: page out below (cold)
            if (COUNT) { d_it_node++; d_lanes_node += (unsigned long long)n_act; }
            if (act) {
                if (MODE == TIRT_TRAVERSE_EXHAUSTIVE) {
                    // reference order on the two-child nodes: both children of every box that passes
                    // `slabs`, leaves without a box test, right child first (left is pushed)
                    const float4 *w = (const float4 *)((const char *)b.wnode + ((unsigned)cur << 6));
                    const float4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3];
                    const int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
                    if (COUNT) nbox += 2;
                    float tl, tr;
                    int pl, pr;
                    if (!par) {
                        pl = slabs_fast(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tl);
                        pr = slabs_fast(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tr);
                    } else {
                        pl = slabs(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tl);
                        pr = slabs(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tr);
                    }
                    const bool hl = (pl != 0) || (cl < 0), hr = (pr != 0) || (cr < 0);
                    if (hl && hr) { sa += ENTRY; LDS_AT(sa) = cr; }
                    int next = hl ? cl : cr;
                    if (!(hl || hr)) TR_POP(next);
                    cur = next;
                } else {
                    // ordered mode on the quantised 4-wide nodes: four box tests, children visited near to far
                    uint4 q0, q1, q2, q3;
#define TR_U4(v) make_uint4((v).x, (v).y, (v).z, (v).w)
                    const unsigned top_addr = top_base + ((unsigned)cur << 6);
                    // The record comes from LDS for some lanes and from global memory for the others, into the SAME sixteen registers.  Written in C++ the
                    // compiler orders the two (a write-after-write on a register, as it sees it): s_waitcnt vmcnt(0) before the first ds_read, i.e. a wave with
                    // lanes on both sides -- nearly every step -- pays the two latencies in a row.  The lanes are disjoint (complementary exec masks) and a
                    // returning load writes only the lanes it was issued for, so nothing has to be ordered: both sets of loads are issued back to back here, one
                    // wait.  +2 % on the headline (profiles/r05e: 4 525 -> 4 620 Mrays/s), films and hit records unchanged (same loads, same bits).
                    {
                        u4v r0__, r1__, r2__, r3__;
                        unsigned long long sv__;
                        const unsigned long long topm__ = ballot64(cur < TR_TOP_SLOTS);
                        const unsigned goff__ = (unsigned)cur << 6;
                        asm volatile(
                            "s_mov_b64 %4, exec\n\t"
                            "s_and_b64 exec, %4, %8\n\t"
                            "s_cbranch_execz .Ltr_fetch_g%=\n\t"
                            "ds_read_b128 %0, %5\n\t"
                            "ds_read_b128 %1, %5 offset:16\n\t"
                            "ds_read_b128 %2, %5 offset:32\n\t"
                            "ds_read_b128 %3, %5 offset:48\n"
                            ".Ltr_fetch_g%=:\n\t"
                            "s_andn2_b64 exec, %4, %8\n\t"
                            "s_cbranch_execz .Ltr_fetch_e%=\n\t"
                            "global_load_dwordx4 %0, %6, %7\n\t"
                            "global_load_dwordx4 %1, %6, %7 offset:16\n\t"
                            "global_load_dwordx4 %2, %6, %7 offset:32\n\t"
                            "global_load_dwordx4 %3, %6, %7 offset:48\n"
                            ".Ltr_fetch_e%=:\n\t"
                            "s_mov_b64 exec, %4\n\t"
                            "s_waitcnt vmcnt(0) lgkmcnt(0)"
                            : "=&v"(r0__), "=&v"(r1__), "=&v"(r2__), "=&v"(r3__), "=&s"(sv__)
                            : "v"(top_addr), "v"(goff__), "s"(b.cnode), "s"(topm__)
                            : "memory");
                        q0 = TR_U4(r0__); q1 = TR_U4(r1__); q2 = TR_U4(r2__); q3 = TR_U4(r3__);
                        if (COUNT) { if (cur < TR_TOP_SLOTS) d_outer++; }
                    }
                    TR_LADDER_PADS(0);
                    int c0 = (int)q3.x, c1 = (int)q3.y, c2 = (int)q3.z, c3 = (int)q3.w;
                    if (COUNT) nbox += 4;
                    constexpr float MISS = 3.0e38f;
                    float d0, d1, d2, d3;                // entry distance of a hit box, MISS otherwise
                    // near/far crossing of each axis: one rotate, two v_fma_mix_f32 (fp16 plane x f32 + f32); then
                    // box hit and entry not beyond the cull distance: tn <= min(tf, lim)
                    TR_CBOX(q0.x, q0.y, q0.z, d0);
                    TR_CBOX(q0.w, q1.x, q1.y, d1);
                    TR_CBOX(q1.z, q1.w, q2.x, d2);
                    TR_CBOX(q2.y, q2.z, q2.w, d3);
                    // sort the four (distance, child) pairs: misses end up last
#define TR_CE(da, ca, db, cb)                                                                        \
                    do {                                                                             \
                        const bool s__ = (db) < (da);                                                \
                        const float lo__ = s__ ? (db) : (da), hi__ = s__ ? (da) : (db);              \
                        const int clo__ = s__ ? (cb) : (ca), chi__ = s__ ? (ca) : (cb);              \
                        da = lo__; db = hi__; ca = clo__; cb = chi__;                                \
                    } while (0)
                    // (nearest-only selection, 3 exchanges instead of 5, measured 5 % slower: more nodes visited)
                    TR_CE(d0, c0, d1, c1); TR_CE(d2, c2, d3, c3); TR_CE(d0, c0, d2, c2); TR_CE(d1, c1, d3, c3); TR_CE(d1, c1, d2, c2);
                    TR_LADDER_PADS(1);
                    if (d3 < MISS) { sa += ENTRY; LDS_AT(sa) = c3; }
                    if (d2 < MISS) { sa += ENTRY; LDS_AT(sa) = c2; }
                    if (d1 < MISS) { sa += ENTRY; LDS_AT(sa) = c1; }
                    int next = c0;
                    if (!(d0 < MISS)) TR_POP(next);
                    if (STASH) { if ((next < 0) & (next != TR_SENT) & (pend == 0)) { pend = next; TR_POP(next); } }
                    cur = next;
                }
            }
        }

        // ---- cold: lanes whose LDS stack is full move their oldest entries to the spill buffer ------
        if (wave_any(have && (int)sa >= (int)sa_hi)) {
            if (have && (int)sa >= (int)sa_hi) TR_PAGE_OUT();
        }

        // ---- leaf: one primitive test ---------------------------------------------------------
        const bool from_pend = STASH && pend != 0;
        const bool leaf_now = have && (from_pend || (cur < 0 && cur != TR_SENT));
        if (COUNT) {
            const int n_l = __popcll(ballot64(leaf_now));
            if (n_l) { d_it_leaf++; d_lanes_leaf += (unsigned long long)n_l; }
        }
        if (leaf_now) {
            // trace_leaf_step (tirt_internal.h): the reference's primitive test, its acceptance rule with the equal-distance rule, and -- ordered walk -- the proof
            // that the reference would have visited this leaf (`slabs` on its exact box, else on every ancestor); shared with k_pvb_cand
            const int code = ~(from_pend ? pend : cur);
            if (COUNT) nleaf += 1;
            bool accepted;
            if constexpr (CUTOUT) accepted = trace_leaf_step<MODE != TIRT_TRAVERSE_EXHAUSTIVE, true, CutSource>(b, r, par, code, hit_t, hit_u, hit_v, hit_prim, hit_leaf);
            else accepted = trace_leaf_step<MODE != TIRT_TRAVERSE_EXHAUSTIVE>(b, r, par, code, hit_t, hit_u, hit_v, hit_prim, hit_leaf);
            if (from_pend) pend = 0; else TR_POP(cur);
            if (accepted) {
                lim = __builtin_fminf(__builtin_fminf(cull_far < 0.0f ? INF_VALUE : hit_t * TR_CULL_SLACK, __builtin_fabsf(cull_far)), INF_VALUE);      // (v_min: a canonical value, so the node loop does not re-canonicalise it every step)
                if (BOUNDED && hit_prim != expect && hit_t < settle) { cur = TR_SENT; paged = 0; pend = 0; }      // answer settled: "occluded"
            }
        }

        // ---- a lane that popped the sentinel but has paged-out entries gets them back (cold) ---------
        if (ballot64(have && cur == TR_SENT && paged > 0) != 0ull) {
            if (have && cur == TR_SENT && paged > 0) { TR_PAGE_IN(); TR_POP(cur); }
        }

        // ---- finished rays write back and free their lane ---------------------------------------
        if (have && cur == TR_SENT && pend == 0) {
            TR_COLD(ca);
            float4 *const c_hit = ca->hit;
            const int *const c_sdst = MAY_SHADOW ? ca->sdst : nullptr;
            float *const c_rr = MAY_SHADOW ? ca->rr : nullptr, *const c_rg = MAY_SHADOW ? ca->rg : nullptr, *const c_rb = MAY_SHADOW ? ca->rb : nullptr;
            float *const c_fr = MAY_SHADOW ? ca->fr : nullptr, *const c_fg = MAY_SHADOW ? ca->fg : nullptr, *const c_fb = MAY_SHADOW ? ca->fb : nullptr;
            const float *const c_scr = MAY_SHADOW ? ca->scr : nullptr, *const c_scg = MAY_SHADOW ? ca->scg : nullptr, *const c_scb = MAY_SHADOW ? ca->scb : nullptr;
            const float *const c_scw = MAY_SHADOW ? ca->scw : nullptr;
            if (MAY_SHADOW) asm volatile("" :: "s"(c_hit), "s"(c_sdst), "s"(c_rr), "s"(c_rg), "s"(c_rb), "s"(c_fr), "s"(c_fg), "s"(c_fb), "s"(c_scr), "s"(c_scg), "s"(c_scb), "s"(c_scw));      // one batch of scalar loads (as in the refill)
            if (!(MAY_SHADOW && is_sh) || KIND == KIND_QUERY) {
                { typedef float f4n __attribute__((ext_vector_type(4))); f4n hv__ = {hit_t, hit_u, hit_v, __int_as_float(hit_prim)}; __builtin_nontemporal_store(hv__, (f4n *)&c_hit[q]); }
            } else if (hit_prim == expect) {                 // integrator/PT_RGB.py:105-109
                const int dst = TR_LDS_(c_sdst[q]);
                float *pr = dst >= 0 ? c_rr + dst : c_fr + ~dst;
                float *pg = dst >= 0 ? c_rg + dst : c_fg + ~dst;
                float *pb = dst >= 0 ? c_rb + dst : c_fb + ~dst;
                *pr = *pr + TR_LDS_(c_scr[q]); *pg = *pg + TR_LDS_(c_scg[q]); *pb = *pb + TR_LDS_(c_scb[q]);
                if (c_scw) { float *pw = dst >= 0 ? ca->rw + dst : ca->fw + ~dst; *pw = *pw + c_scw[q]; }
            }
            if (COUNT) {
                if (MAY_SHADOW && is_sh) { sum_box_s += nbox; sum_leaf_s += nleaf; }
                else { sum_box += nbox; sum_leaf += nleaf; }
                if (ca->per_ray_counts) ca->per_ray_counts[q] = make_int2((int)nbox, (int)nleaf);
            }
            if (n_overflow) n_over++;
            have = false; sa = sa_bottom;
        }
    }
    TR_COLD(ca);
    if (ca->ctr) {
        if (COUNT) {
            sum_box = wave_sum(sum_box); sum_leaf = wave_sum(sum_leaf);
            sum_box_s = wave_sum(sum_box_s); sum_leaf_s = wave_sum(sum_leaf_s);
            if (lane == 0 && (sum_box | sum_leaf)) { atomicAdd(&ca->ctr->box_closest, sum_box); atomicAdd(&ca->ctr->leaf_closest, sum_leaf); }
            if (lane == 0 && (sum_box_s | sum_leaf_s)) { atomicAdd(&ca->ctr->box_shadow, sum_box_s); atomicAdd(&ca->ctr->leaf_shadow, sum_leaf_s); }
        }
        if (COUNT) { d_outer = wave_sum(d_outer); if (lane == 0) atomicAdd(&ca->ctr->it_outer, d_outer); }   // lane-visits of LDS-resident (top) nodes
        if (COUNT && lane == 0) {
            atomicAdd(&ca->ctr->it_node, d_it_node); atomicAdd(&ca->ctr->lanes_node, d_lanes_node);
            atomicAdd(&ca->ctr->it_leaf, d_it_leaf); atomicAdd(&ca->ctr->lanes_leaf, d_lanes_leaf);
            atomicAdd(&ca->ctr->refills, d_refills);
            const unsigned long long tk_end = wall_clock64();
            atomicAdd(&ca->ctr->wave_ticks, tk_end - tk_start); atomicAdd(&ca->ctr->drain_ticks, tk_end - (tk_exh ? tk_exh : tk_end)); atomicAdd(&ca->ctr->waves, 1ull);
            if (ca->timeline) {
                // HW_ID (wave, SIMD, CU, shader array, shader engine) and XCC_ID of the CU this wave ran on
                const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
                unsigned long long *rec = ca->timeline + (size_t)(gtid >> 6) * 4;
                rec[0] = tk_start; rec[1] = tk_exh; rec[2] = tk_end; rec[3] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
            }
        }
        if (n_over) atomicAdd(&ca->ctr->stack_overflow, n_over);
        if (gtid == 0 && !ca->no_ray_count) {
            if (count_c) atomicAdd(&ca->ctr->rays_closest, (unsigned long long)count_c);
            if (count_s) atomicAdd(&ca->ctr->rays_shadow, (unsigned long long)count_s);
        }
    }
}

// diagnostics: option "trace_timeline" = k >= 0 arms the k-th counting launch from now on; it writes [start, queue empty, end, hw id] per wave
unsigned long long *timeline_for(tirt_ctx *c, int flags, int grid)
{
    if (c->timeline_arm < 0 || !(flags & TIRT_COUNT_NODES)) return nullptr;
    if (c->timeline_arm-- != 0) return nullptr;
    c->timeline_waves = grid * (TR_BLOCK / 64);
    if (c->timeline.ensure(sizeof(unsigned long long) * 4 * (size_t)c->timeline_waves)) { c->timeline_waves = 0; return nullptr; }
    if (hipMemsetAsync(c->timeline.p, 0, sizeof(unsigned long long) * 4 * (size_t)c->timeline_waves, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); c->timeline_waves = 0; return nullptr; }      // no timeline rather than a half-cleared one
    return c->timeline.as<unsigned long long>();
}

template <int MODE, bool COUNT, int KIND, bool CUTOUT = false>
static int launch_trace_as(tirt_ctx *c, hipStream_t stream, const typename trace_args_of<CUTOUT>::type &a, dim3 g, dim3 b, size_t lds)
{
    // more than 64 KB of dynamic LDS per block (stacks + tree top): the opt-in is per kernel AND per device
    static size_t allowed[TIRT_MAX_DEVICES] = {};
    TIRT_REQUIRE(lds <= c->lds_optin, "k_trace: trace_lds_depth needs more LDS than the device has per block");
    const int dev = (c->device >= 0 && c->device < TIRT_MAX_DEVICES) ? c->device : 0;
    if (lds > allowed[dev] || c->device >= TIRT_MAX_DEVICES) {
        TIRT_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_trace<MODE, COUNT, KIND, CUTOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        allowed[dev] = lds;
    }
    hipLaunchKernelGGL((k_trace<MODE, COUNT, KIND, CUTOUT>), g, b, lds, stream, a);
    return TIRT_OK;
}
// the visiting rule and the counting twin, by `flags`
template <int KIND, bool CUTOUT>
static int launch_trace_flags(tirt_ctx *c, hipStream_t stream, const typename trace_args_of<CUTOUT>::type &a, int flags, int grid)
{
    const bool exh = (flags & TIRT_TRAVERSE_EXHAUSTIVE) != 0, cnt = (flags & TIRT_COUNT_NODES) != 0;
    dim3 g(grid), b(TR_BLOCK);
    const size_t lds = trace_lds_bytes(a.lds_depth);
    if (exh && cnt) return launch_trace_as<TIRT_TRAVERSE_EXHAUSTIVE, true, KIND, CUTOUT>(c, stream, a, g, b, lds);
    if (exh) return launch_trace_as<TIRT_TRAVERSE_EXHAUSTIVE, false, KIND, CUTOUT>(c, stream, a, g, b, lds);
    if (cnt) return launch_trace_as<TIRT_TRAVERSE_ORDERED, true, KIND, CUTOUT>(c, stream, a, g, b, lds);
    return launch_trace_as<TIRT_TRAVERSE_ORDERED, false, KIND, CUTOUT>(c, stream, a, g, b, lds);
}
template <int KIND>
static int launch_trace_kind(tirt_ctx *c, hipStream_t stream, const TraceArgs &a, int flags, int grid)
{
    // a scene with a cut-out triangle (tirt_ctx::has_cutout, the feature word's SF_CUTOUT) gets the CUTOUT twin of whatever it would launch; every other scene what it always got
    if (!c->has_cutout) return launch_trace_flags<KIND, false>(c, stream, a, flags, grid);
    TraceArgsCut ac; static_cast<TraceArgs &>(ac) = a;
    ac.cut.uv = c->cut_uv.as<float4>(); ac.cut.tex = c->tex.as<int>();
    TIRT_REQUIRE(c->cut_rec_valid && ac.cut.uv && ac.cut.tex, "k_trace: the cut-out records are stale (internal: ensure_cutout_records was not run)");
    return launch_trace_flags<KIND, true>(c, stream, ac, flags, grid);
}
int launch_trace(tirt_ctx *c, hipStream_t stream, int kind, const TraceArgs &a, int flags, int grid)
{
    switch (kind) {
    case KIND_CLOSEST: return launch_trace_kind<KIND_CLOSEST>(c, stream, a, flags, grid);
    case KIND_SHADOW_ACC: return launch_trace_kind<KIND_SHADOW_ACC>(c, stream, a, flags, grid);
    case KIND_MIXED: return launch_trace_kind<KIND_MIXED>(c, stream, a, flags, grid);
    default: return launch_trace_kind<KIND_QUERY>(c, stream, a, flags, grid);
    }
}

int ensure_spill(tirt_ctx *c, DevBuf &spill, int stack_size, int &spill_depth)
{
    int cap = stack_size > 64 ? stack_size : 64;
    spill_depth = cap - (c->tr_lds_depth - 1);      // entry 0 of the LDS part is the sentinel
    if (spill_depth < 0) spill_depth = 0;
    spill_depth = (spill_depth + TR_PAGE - 1) / TR_PAGE * TR_PAGE;
    return spill.ensure(sizeof(int) * (size_t)(spill_depth > 0 ? spill_depth : 1) * TR_GRID_MAX * TR_BLOCK);
}
void fill_tunables(const tirt_ctx *c, TraceArgs &a)
{ a.lds_depth = c->tr_lds_depth; a.refill_min = c->tr_refill_min; a.node_min = c->tr_node_min; a.slice_log2 = c->tr_slice_log2; a.slices_contig = c->slices_contiguous; }

// The paged tail of the traversal stacks (sized by the integrator's stack size: 2 GB per lane at bdpt_stack_size 1024) and the ray-fetch cursors
// of a lane (lane < 0: the main stream), into `a`.  (The lanes' counter buffers hold the per-bounce cursors of the path tracer as well: ensure()
// keeps a larger one.)
static int trace_buffers(tirt_ctx *c, int lane, int stack_size, TraceArgs &a)
{
    DevBuf &spill = lane < 0 ? c->spill : c->lanes[lane].spill;
    DevBuf &fetch = lane < 0 ? c->counters_mem : c->lanes[lane].counters_mem;
    if (ensure_spill(c, spill, stack_size, a.spill_depth)) return TIRT_ERR_HIP;
    if (fetch.ensure(sizeof(int) * TR_FETCH_STRIDE * TR_FETCH_LINES)) return TIRT_ERR_HIP;
    a.spill = spill.as<int>(); a.fetch = fetch.as<int>();
    return TIRT_OK;
}

// The buffers of BDPT's rays allocated up front: a caller that sizes its batches to the free memory (bdpt_render) calls this BEFORE it
// measures, and a failed allocation ends the call before anything has been blended into the film.
int trace_rays_prepare(tirt_ctx *c, int lane)
{
    TraceArgs a = {};
    return trace_buffers(c, lane, c->bdpt_stack, a);
}

int trace_rays(tirt_ctx *c, const TraceJob &j)
{
    if (j.count <= 0) return TIRT_OK;
    if (int rc = ensure_cutout_records(c)) return rc;
    hipStream_t st = j.lane < 0 ? c->stream : c->lanes[j.lane].stream;
    TraceArgs a = {};
    if (int rc = trace_buffers(c, j.lane, j.stack_size, a)) return rc;
    TIRT_HIP(hipMemsetAsync(a.fetch, 0, sizeof(int) * TR_FETCH_STRIDE * TR_FETCH_LINES, st));
    a.bvh = bvh_view(c);
    a.ray4 = j.ray4; a.ray_index = j.ray_index;
    if (!j.ray4) { a.dx = j.dx; a.dy = j.dy; a.dz = j.dz; for (int k = 0; k < 3; k++) a.eye[k] = c->cam.eye[k]; }      // camera rays (ox == nullptr): from the eye
    a.count_ptr = j.count_ptr; a.count_fixed = j.count; a.hit = j.hit;
    a.ctr = c->dev_counters.as<DevCounters>(); a.no_ray_count = j.count_rays ? 0 : 1;
    a.per_ray_counts = (j.flags & TIRT_COUNT_NODES) ? j.per_ray_counts : nullptr;
    fill_tunables(c, a);
    int grid = (j.count + TR_BLOCK - 1) / TR_BLOCK; if (grid > j.grid_cap) grid = j.grid_cap;
    a.timeline = timeline_for(c, j.flags, grid);
    return launch_trace(c, st, j.query ? KIND_QUERY : KIND_CLOSEST, a, j.flags, grid);
}
}  // namespace tirt
