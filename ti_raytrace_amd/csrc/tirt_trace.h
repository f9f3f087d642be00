// tirt_trace.h -- what the traversal (tirt_trace.hip: k_trace and its launchers) and its callers share: the argument struct of a launch, the
// launch entry of the path tracer's scheduler (tirt_render.hip) and the one-call service of everybody else (trace_rays).
#pragma once
#include "tirt_internal.h"

namespace tirt {

constexpr int TR_GRID_MAX = 2048;      // upper bound on persistent blocks (sizes the spill buffer)

// MIXED: closest rays of bounce b + shadow rays of bounce b-1 in one launch.  QUERY: connection rays of BDPT -- "is sprim[q] the closest
// hit, about sdist[q] away?" walked like a shadow ray (bounded), answered with the hit record (t, u, v, prim) instead of an accumulation.
enum { KIND_CLOSEST = 0, KIND_SHADOW_ACC = 1, KIND_MIXED = 2, KIND_QUERY = 3 };
struct TraceArgs {
    BvhView bvh;
    const float *ox, *oy, *oz, *dx, *dy, *dz;    // rays, dense: ray q at index q
    float eye[3];                                // KIND_CLOSEST with ox == nullptr (camera rays): the common origin
    const int *count_ptr; int count_fixed;       // number of rays: *count_ptr if non-null
    float4 *hit;                                 // KIND_CLOSEST output, index q: (t, u, v, bits prim)
    // KIND_SHADOW_ACC: contribution of ray q goes to (rr,rg,rb)[sdst[q]] or (fr,fg,fb)[~sdst[q]]
    const int *sprim, *sdst; const float *sdist, *scr, *scg, *scb; float *rr, *rg, *rb, *fr, *fg, *fb;
    const float *scw; float *rw, *fw;            // PT_Spec: the fourth hero wavelength's contribution / radiance (nullptr for the RGB integrators)
    int *spill; int spill_depth;                 // global stack tail: [entry][global thread]
    // KIND_MIXED: the shadow rays live in their own arrays; indices [count, count + scount) are shadow rays
    const float *sox, *soy, *soz, *sdx, *sdy, *sdz; const int *scount_ptr;
    // ray-fetch cursors of this launch (zero on entry).  Same-address device atomics retire at one per
    // ~11 ns on MI355X (tools/micro/atomic_rate.hip), which would cap a single cursor at ~3 Grays/s, so
    // the queue is cut into 2^slice_log2 interleaved slices (64-ray chunks, chunk c belongs to slice
    // c mod S), each with its own cursor in its own 128-byte line; a wave drains its home slice and
    // then moves on to the next one.
    int *fetch; int slice_log2;
    // slices_contig: slice h is the h-th CONTIGUOUS 1/S of the queue (of the closest-hit rays and of the shadow rays each) instead of every S-th chunk.
    // The home slice of a wave is (4 x block + wave) mod 32 and blocks go round-robin over the eight XCDs, so slices 4x .. 4x+3 are served by XCD x
    // first: with paths numbered pixel-block major (TileMap::F) that is one region of the film -- one part of the scene -- per L2.
    int slices_contig;
    int lds_depth;                               // stack entries per lane kept in LDS
    int refill_min;                              // re-fetch rays when this many lanes of a wave are idle
    int node_min;                                // leave the inner-node loop below this many busy lanes
    DevCounters *ctr; int2 *per_ray_counts;
    unsigned long long *timeline;        // diagnostics (option "trace_timeline"): per wave [start, queue found empty, end, hardware id] of this launch
    int no_ray_count;                            // the caller counts its rays itself (queues with dead entries)
    // KIND_CLOSEST / KIND_QUERY: the rays as 32-byte records instead of six arrays -- (o.xyz, d.x), (d.y, d.z, bits expect, bound): two 16-byte
    // loads per ray where the arrays take six to eight (the BDPT ray lists: their kernels are bound by the number of memory instructions)
    const float4 *ray4;
    const int *ray_index;                        // KIND_QUERY: ray q is record ray_index[q] of ray4 (BDPT: the connection rays stay where they were staged; the queue is a list of places)
};
// the argument of the CUTOUT twins (scenes with a cut-out triangle): TraceArgs, and behind it the vertex uvs in the records' order and the texture buffer
// (trace_leaf_step), read from the kernel-argument segment where a tagged candidate needs them (CutSource).  The opaque instantiations keep TraceArgs itself:
// not an offset of their argument block moves, the hidden arguments behind it included.
struct TraceArgsCut : TraceArgs { CutView cut; };
template <bool CUTOUT> struct trace_args_of { typedef TraceArgs type; };
template <> struct trace_args_of<true> { typedef TraceArgsCut type; };

constexpr int TR_FETCH_STRIDE = 32;           // ints between two slice cursors (one 128-byte line each)
constexpr int TR_SLICES_MAX = 64;
constexpr int TR_FETCH_LINES = TR_SLICES_MAX + 1;   // one cursor per slice, each in a line of its own, + the line of the drained-slices count

// ---- what the path tracer's scheduler (pt_render) launches through; every function is in tirt_trace.hip ----
// One launch of k_trace<KIND_*> on `stream`: the instantiation by `flags` (TIRT_TRAVERSE_EXHAUSTIVE | TIRT_COUNT_NODES) and by the scene (its CUTOUT twin)
int launch_trace(tirt_ctx *c, hipStream_t stream, int kind, const TraceArgs &a, int flags, int grid);
int ensure_spill(tirt_ctx *c, DevBuf &spill, int stack_size, int &spill_depth);      // the paged tail of the traversal stacks, sized by the integrator's stack size
void fill_tunables(const tirt_ctx *c, TraceArgs &a);                                 // lds_depth, refill_min, node_min and the slicing, from the context's options
unsigned long long *timeline_for(tirt_ctx *c, int flags, int grid);                  // TraceArgs::timeline of the next launch: non-null for the one that "trace_timeline" armed

// One k_trace launch outside the path tracer (trace_rays, tirt_trace.hip): the traversal service of BDPT, the primary beams, Debug and the
// ray queries.  The rays are 32-byte records (TraceArgs::ray4) or, without them, camera rays from the eye with their directions in dx / dy / dz.
struct TraceJob {
    int lane = -1;                               // < 0: the main stream, c->spill and c->counters_mem; else that render lane's stream and buffers
    int stack_size = 64;                         // sizes the spill (the integrator's stack_size)
    int flags = 0;                               // TIRT_TRAVERSE_EXHAUSTIVE | TIRT_COUNT_NODES: the instantiation, timeline arming
    bool query = false;                          // KIND_QUERY (bounded queries whose expect / bound ride in the records) instead of KIND_CLOSEST
    const float4 *ray4 = nullptr;
    const int *ray_index = nullptr;              // KIND_QUERY: ray q is record ray_index[q]
    const float *dx = nullptr, *dy = nullptr, *dz = nullptr;
    int count = 0; const int *count_ptr = nullptr;      // the rays: *count_ptr if given, `count` then being its capacity (sizes the grid)
    float4 *hit = nullptr;
    int2 *per_ray_counts = nullptr;              // N_box / N_leaf per ray, under TIRT_COUNT_NODES only
    bool count_rays = true;                      // false: the caller counts its rays itself (TraceArgs::no_ray_count)
    int grid_cap = 0;                            // persistent blocks at most: c->tr_grid_alone or c->tr_grid
};
int trace_rays(tirt_ctx *c, const TraceJob &j);
int trace_rays_prepare(tirt_ctx *c, int lane);      // allocates what trace_rays needs on that lane at bdpt_stack_size (stack spill, fetch cursors)

}  // namespace tirt
