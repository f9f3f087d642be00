// tirt_query.hip -- closest-hit and occlusion queries on rays that live in device memory (tirt_query_closest / tirt_query_occluded), and
// the host route (tirt_trace_closest / tirt_trace_shadow) through the same closest-hit path.  At the end of the file: the same plumbing around the
// first-K-hits walk of tirt_multi_hit.hip (tirt_query_hits / tirt_trace_hits).
//
// No reference counterpart as an entry point: the traversal is Scene.closet_hit / closet_hit_shadow (Scene.py:702-744, 671-699), run by
// the existing k_trace instantiations.  What is new is the plumbing around it, in chunks of option "query_chunk_rays" rays, all on the
// context's main stream, ordered after and before the caller's stream by two events (no host sync):
//
//   k_query_pack               caller rays (f32, any row stride >= 6) -> 32-byte records TraceArgs::ray4: (o.xyz, d.x), (d.y, d.z, bits expect, bound)
//   k_trace<closest | query>   closest hit, or the bounded query with bound = tmax                 (trace_rays, tirt_trace.hip)
//   k_query_resolve_closest    t, prim and optionally the 13-float record of tirt_trace_closest
//   k_query_resolve_occluded   one byte per ray: t < INF_VALUE && t < tmax
//
// Why the occlusion answer is exact: with bound = tmax > 0 an ordered walk stops early ("settled") only on an accepted hit with
// hit_t < 0.99 tmax, which is a hit the reference finds too, so its closest is closer still and below tmax; a walk that does not settle
// culls nothing nearer than 1.01 tmax and so ends with the reference's closest hit whenever that is below tmax, and with a hit at or beyond
// tmax (or a miss) otherwise.  Rays from far away (no culling), the exhaustive walk and tmax <= 0 / NaN (no bound) end with the full closest
// hit.  A miss leaves t = INF_VALUE (1e6, the reference's value), which is why the test is not a bare t < tmax.
#include "tirt_trace.h"
#include "tirt_query_stage.h"

namespace tirt {

constexpr int QUERY_EXPECT = -2;          // the `expect` of an occlusion query: equals no primitive id, and k_trace gives it no meaning of its own

__global__ void k_query_pack(const float *rays, int64_t base, int n, int64_t ray_stride, int occluded, const float *tmax, int64_t tmax_stride,
                             float tmax_all, float4 *rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = base + i;
    const float *r = rays + g * ray_stride;
    const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5];
    int expect = -3; float bound = -1.0f;                 // closest: the "no query" encoding of the BDPT ray lists
    if (occluded) { expect = QUERY_EXPECT; bound = tmax ? tmax[g * tmax_stride] : tmax_all; }
    rec[2 * (size_t)i] = make_float4(ox, oy, oz, dx);
    rec[2 * (size_t)i + 1] = make_float4(dy, dz, __int_as_float(expect), bound);
}

// the record of tirt_trace_closest: t, then hit_attributes (pos, gnormal, normal, tex); a miss normalises (0, 0, 0) as the reference does
__global__ void k_query_resolve_closest(SceneView s, const float4 *rec, const float4 *hit, int64_t base, int n, float *out_t, int32_t *out_prim,
                                        float *out_hit, int64_t hit_stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = base + i;
    const float4 hr = hit[i];
    if (out_t) out_t[g] = hr.x;
    if (out_prim) out_prim[g] = __float_as_int(hr.w);
    if (!out_hit) return;
    const float4 r0 = rec[2 * (size_t)i], r1 = rec[2 * (size_t)i + 1];
    HitAttr h; h.pos = h.gnor = h.nor = h.tex = V(0.0f, 0.0f, 0.0f);
    if (hr.x < INF_VALUE) h = hit_attributes(s, V(r0.x, r0.y, r0.z), V(r0.w, r1.x, r1.y), __float_as_int(hr.w), hr.x, hr.y, hr.z);
    else { h.gnor = normalized(h.gnor); h.nor = normalized(h.nor); }     // reference normalises (0,0,0) on a miss
    float *o = out_hit + g * hit_stride;
    o[0] = hr.x;
    o[1] = h.pos.x; o[2] = h.pos.y; o[3] = h.pos.z;
    o[4] = h.gnor.x; o[5] = h.gnor.y; o[6] = h.gnor.z;
    o[7] = h.nor.x; o[8] = h.nor.y; o[9] = h.nor.z;
    o[10] = h.tex.x; o[11] = h.tex.y; o[12] = h.tex.z;
}

// the bound the record carries is the caller's tmax, bit for bit (NaN and -1 compare false: 0)
__global__ void k_query_resolve_occluded(const float4 *rec, const float4 *hit, int64_t base, int n, uint8_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float t = hit[i].x, tmax = rec[2 * (size_t)i + 1].w;
    out[base + i] = (t < INF_VALUE && t < tmax) ? 1 : 0;
}

// Device memory of this context's device, as the HIP runtime libtirt.so runs on sees it.  A pointer of another runtime (a second
// libamdhip64 in the process, _native._check_one_hip_runtime) or of the host is refused here, before anything is queued.
int require_device_ptr(tirt_ctx *c, const void *p, const char *what)
{
    hipPointerAttribute_t at = {};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();                               // an unknown pointer leaves a sticky error behind
    if (e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.device == c->device) return TIRT_OK;
    set_error(std::string(what) + ": not device memory of this context's device " + std::to_string(c->device) +
              " (a host pointer, another device's memory, or memory of a second HIP runtime in the process -- libtirt.so and the "
              "caller's framework must share one libamdhip64)");
    return TIRT_ERR_ARG;
}

// The caller's stream must be one of this process's HIP runtime and not capturing a graph (`what` cannot be captured): refused before anything is queued.
int require_caller_stream(tirt_ctx *c, const std::string &fn, void *stream, const char *what)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        set_error(fn + ": the caller's stream is not a stream of this process's HIP runtime");
        return TIRT_ERR_ARG;
    }
    TIRT_REQUIRE(cs == hipStreamCaptureStatusNone, fn + ": the caller's stream is capturing a graph (" + what + " cannot be captured)");
    return TIRT_OK;
}

// what every query entry checks first, on rays (`count` = "nr") and on points ("n") alike
int query_common_checks(tirt_ctx *c, const char *fn, const char *count, int64_t n, int stack_size, int flags)
{
    TIRT_REQUIRE(c->built, std::string(fn) + ": LBVH not built");
    TIRT_REQUIRE(n >= 0, std::string(fn) + ": " + count + " < 0");
    TIRT_REQUIRE(stack_size >= 1 && stack_size <= 4096, std::string(fn) + ": stack_size 1..4096");
    TIRT_REQUIRE((flags & ~(TIRT_TRAVERSE_EXHAUSTIVE | TIRT_COUNT_NODES)) == 0, std::string(fn) + ": unknown flags");
    return TIRT_OK;
}
int point_query_checks(tirt_ctx *c, const char *fn, int64_t n, int stack_size, int flags, std::initializer_list<StrideCheck> strides, const int32_t *counts, void *stream)
{
    if (int rc = query_common_checks(c, fn, "n", n, stack_size, flags)) return rc;
    for (const StrideCheck &s : strides) TIRT_REQUIRE(!s.present || s.stride >= s.minimum, std::string(fn) + ": " + s.text);
    TIRT_REQUIRE(!counts || ((uintptr_t)counts & 7) == 0, std::string(fn) + ": counts must be 8-byte aligned");
    return require_caller_stream(c, fn, stream, "queries");
}
static int ray_query_checks(tirt_ctx *c, const char *fn, int64_t nr, int64_t ray_stride, int stack_size, int flags, void *stream)
{
    if (int rc = query_common_checks(c, fn, "nr", nr, stack_size, flags)) return rc;
    TIRT_REQUIRE(ray_stride >= 6, std::string(fn) + ": ray_stride < 6 (floats per ray: origin, direction)");
    return require_caller_stream(c, fn, stream, "queries");
}

// The kernels' scratch (query_mem) of at least `bytes`.  Growing the buffer waits for the work queued on the context's stream, which may still
// read the old one.
int query_scratch(tirt_ctx *c, size_t bytes)
{
    if (bytes > c->query_mem.bytes) {
        TIRT_HIP(hipStreamSynchronize(c->stream));
        if (c->query_mem.ensure(bytes)) return TIRT_ERR_HIP;
    }
    return TIRT_OK;
}

// Scratch of one chunk of `chunk` rays (ray records, then hit records).
static int query_prepare(tirt_ctx *c, int chunk, float4 *&rec, float4 *&hit)
{
    if (int rc = query_scratch(c, (size_t)chunk * 48)) return rc;
    rec = c->query_mem.as<float4>();
    hit = rec + 2 * (size_t)chunk;
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    return TIRT_OK;
}

// the two ordering events are made on first use
int query_begin(tirt_ctx *c, void *stream)
{
    if (!c->query_ev_in) TIRT_HIP(hipEventCreateWithFlags(&c->query_ev_in, hipEventDisableTiming));
    if (!c->query_ev_out) TIRT_HIP(hipEventCreateWithFlags(&c->query_ev_out, hipEventDisableTiming));
    TIRT_HIP(hipEventRecord(c->query_ev_in, (hipStream_t)stream));
    TIRT_HIP(hipStreamWaitEvent(c->stream, c->query_ev_in, 0));
    return TIRT_OK;
}

int query_end(tirt_ctx *c, void *stream)
{
    TIRT_HIP(hipGetLastError());
    TIRT_HIP(hipEventRecord(c->query_ev_out, c->stream));
    TIRT_HIP(hipStreamWaitEvent((hipStream_t)stream, c->query_ev_out, 0));
    return TIRT_OK;
}

// pack, trace, resolve: `nr` rays in chunks of `chunk` through the records at `rec` / `hit` (query_prepare) on the context's stream.
// `job` holds the traversal settings; counts: N_box / N_leaf per ray under TIRT_COUNT_NODES (or nullptr).
static int closest_chunks(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, int chunk, float4 *rec, float4 *hit, TraceJob job,
                          bool count_launches, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int2 *counts)
{
    const SceneView sv = scene_view(c);
    const int B = 256;
    job.ray4 = rec; job.hit = hit;
    for (int64_t base = 0; base < nr; base += chunk) {
        const int n = (int)(nr - base < chunk ? nr - base : chunk);
        const dim3 g((unsigned)((n + B - 1) / B));
        hipLaunchKernelGGL(k_query_pack, g, dim3(B), 0, c->stream, rays, base, n, ray_stride, 0, (const float *)nullptr, (int64_t)0, 0.0f, rec);
        job.count = n; job.per_ray_counts = counts ? counts + base : nullptr;
        if (count_launches) c->launches_trace_closest++;
        if (int rc = trace_rays(c, job)) return rc;
        hipLaunchKernelGGL(k_query_resolve_closest, g, dim3(B), 0, c->stream, sv, (const float4 *)rec, (const float4 *)hit, base, n, out_t, out_prim,
                           out_hit, hit_stride);
    }
    return TIRT_OK;
}

int query_closest(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, int stack_size, int flags, float *out_t, int32_t *out_prim,
                  float *out_hit, int64_t hit_stride, int32_t *counts, void *stream)
{
    const char *fn = "tirt_query_closest";
    if (int rc = ray_query_checks(c, fn, nr, ray_stride, stack_size, flags, stream)) return rc;
    TIRT_REQUIRE(!out_hit || hit_stride >= 13, "tirt_query_closest: hit_stride < 13 (floats per hit record)");
    TIRT_REQUIRE(!counts || ((uintptr_t)counts & 7) == 0, "tirt_query_closest: counts must be 8-byte aligned");
    if (nr == 0) return TIRT_OK;
    TIRT_REQUIRE(rays, "tirt_query_closest: null rays");
    const QueryPlan pl = query_plan(c, nr, flags, counts);
    if (int rc = require_device_ptrs(c, "tirt_query_closest: ", {{rays, "rays"}, {out_t, "out_t"}, {out_prim, "out_prim"}, {out_hit, "out_hit"}, {pl.counts, "counts"}})) return rc;
    float4 *rec, *hit;
    if (int rc = query_prepare(c, pl.chunk, rec, hit)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    TraceJob job; job.stack_size = stack_size; job.flags = flags; job.grid_cap = c->tr_grid_alone;
    if (int rc = closest_chunks(c, rays, nr, ray_stride, pl.chunk, rec, hit, job, true, out_t, out_prim, out_hit, hit_stride, pl.counts)) return rc;
    return query_end(c, stream);
}

// tirt_trace_closest / tirt_trace_shadow: host rays (6 floats each) staged in device memory, one chunk of all of them through the
// closest-hit path above with the grid of a busy GPU (trace_grid), shadow: t, else the 13-float record, back to the host with a sync.
int trace_host(tirt_ctx *c, const float *rays, int nr, int stack_size, int flags, bool shadow, float *out_f, int32_t *out_prim, int32_t *counts)
{
    TIRT_REQUIRE(c->built, "trace: LBVH not built");
    TIRT_REQUIRE(nr >= 0, "trace: nr < 0");
    if (nr == 0) return TIRT_OK;
    float4 *rec, *hit;
    if (int rc = query_prepare(c, nr, rec, hit)) return rc;
    const size_t N = (size_t)nr;
    QueryStage s(c);
    const auto k_rays = s.in(rays, 6 * N);
    const auto k_out = s.out(out_f, (shadow ? 1 : 13) * N);      // t, or the records
    const auto k_prim = s.out(out_prim, N);
    const auto k_counts = s.out_counts(counts, flags, N);
    if (int rc = s.begin()) return rc;
    float *d_out = s.ptr(k_out);
    TraceJob job; job.stack_size = stack_size; job.flags = flags; job.grid_cap = c->tr_grid;
    if (int rc = closest_chunks(c, s.ptr(k_rays), nr, 6, nr, rec, hit, job, false, shadow ? d_out : nullptr, s.ptr(k_prim), shadow ? nullptr : d_out, 13,
                                s.ptr(k_counts))) return rc;
    return s.finish();
}

int query_occluded(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, const float *tmax, int64_t tmax_stride, float tmax_all,
                   int stack_size, int flags, uint8_t *out_occluded, void *stream)
{
    const char *fn = "tirt_query_occluded";
    if (int rc = ray_query_checks(c, fn, nr, ray_stride, stack_size, flags, stream)) return rc;
    TIRT_REQUIRE(!tmax || tmax_stride >= 1, "tirt_query_occluded: tmax_stride < 1");
    if (nr == 0) return TIRT_OK;
    TIRT_REQUIRE(rays && out_occluded, "tirt_query_occluded: null rays / out_occluded");
    if (int rc = require_device_ptrs(c, "tirt_query_occluded: ", {{rays, "rays"}, {tmax, "tmax"}, {out_occluded, "out_occluded"}})) return rc;
    const int chunk = query_plan(c, nr, flags, nullptr).chunk;
    float4 *rec, *hit;
    if (int rc = query_prepare(c, chunk, rec, hit)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    TraceJob job; job.stack_size = stack_size; job.flags = flags; job.query = true; job.ray4 = rec; job.hit = hit; job.grid_cap = c->tr_grid_alone;
    const int B = 256;
    for (int64_t base = 0; base < nr; base += chunk) {
        const int n = (int)(nr - base < chunk ? nr - base : chunk);
        const dim3 g((unsigned)((n + B - 1) / B));
        hipLaunchKernelGGL(k_query_pack, g, dim3(B), 0, c->stream, rays, base, n, ray_stride, 1, tmax, tmax_stride, tmax_all, rec);
        job.count = n;
        c->launches_trace_shadow++;
        if (int rc = trace_rays(c, job)) return rc;
        hipLaunchKernelGGL(k_query_resolve_occluded, g, dim3(B), 0, c->stream, (const float4 *)rec, (const float4 *)hit, base, n, out_occluded);
    }
    return query_end(c, stream);
}

// ---- the first k hits and the count of all (include/tirt.h "First K hits"; the walk is tirt_multi_hit.hip's) ----
// Rays per chunk: max(256, query_chunk_rays / max(k, 1)), so that the scratch -- 32 B of ray record, 16 B x k of list and 8 B of (entries, count) per ray --
// stays of the order the other queries' is.
static int hits_chunk_of(const tirt_ctx *c, int64_t nr, int k)
{
    int64_t chunk = (int64_t)c->query_chunk / (k > 0 ? k : 1);
    if (chunk < 256) chunk = 256;
    return (int)(nr < chunk ? nr : chunk);
}
struct HitsScratch { float4 *rec, *list; int2 *meta; MultiHitShape shape; };
static int hits_prepare(tirt_ctx *c, int chunk, int k, int stack_size, HitsScratch &s)
{
    if (int rc = query_scratch(c, (size_t)chunk * (40 + 16 * (size_t)k))) return rc;
    s.rec = c->query_mem.as<float4>();
    s.list = s.rec + 2 * (size_t)chunk;
    s.meta = (int2 *)(s.list + (size_t)k * chunk);
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    return multi_hit_shape(c, stack_size, chunk, s.shape);
}
// pack, walk, resolve: `nr` rays in chunks of `chunk` on the context's stream; every pointer is device memory (or null)
static int hits_chunks(tirt_ctx *c, const HitsScratch &s, const float *rays, int64_t nr, int64_t ray_stride, const float *tmax, int64_t tmax_stride,
                       float tmax_all, int k, int stack_size, int flags, int chunk, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride,
                       int32_t *out_count, int2 *counts)
{
    const int B = 256;
    for (int64_t base = 0; base < nr; base += chunk) {
        const int n = (int)(nr - base < chunk ? nr - base : chunk);
        hipLaunchKernelGGL(k_query_pack, dim3((unsigned)((n + B - 1) / B)), dim3(B), 0, c->stream, rays, base, n, ray_stride, 1, tmax, tmax_stride, tmax_all, s.rec);
        if (int rc = multi_hit_chunk(c, s.shape, s.rec, s.list, s.meta, (size_t)chunk, base, n, k, stack_size, flags, out_count != nullptr,
                                     counts ? counts + base : nullptr, out_t, out_prim, out_hit, hit_stride, out_count)) return rc;
    }
    return TIRT_OK;
}

int query_hits(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, const float *tmax, int64_t tmax_stride, float tmax_all, int k, int stack_size,
               int flags, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *out_count, int32_t *counts, void *stream)
{
    const char *fn = "tirt_query_hits";
    if (int rc = ray_query_checks(c, fn, nr, ray_stride, stack_size, flags, stream)) return rc;
    TIRT_REQUIRE(!out_hit || hit_stride >= 13, "tirt_query_hits: hit_stride < 13 (floats per hit record)");
    TIRT_REQUIRE(!tmax || tmax_stride >= 1, "tirt_query_hits: tmax_stride < 1");
    TIRT_REQUIRE(!counts || ((uintptr_t)counts & 7) == 0, "tirt_query_hits: counts must be 8-byte aligned");
    if (nr == 0) return TIRT_OK;
    TIRT_REQUIRE(rays, "tirt_query_hits: null rays");
    int2 *const want_counts = query_plan(c, nr, flags, counts).counts;
    if (int rc = require_device_ptrs(c, "tirt_query_hits: ", {{rays, "rays"}, {tmax, "tmax"}, {out_t, "out_t"}, {out_prim, "out_prim"}, {out_hit, "out_hit"},
                                                             {out_count, "out_count"}, {want_counts, "counts"}})) return rc;
    const int chunk = hits_chunk_of(c, nr, k);
    HitsScratch s;
    if (int rc = hits_prepare(c, chunk, k, stack_size, s)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = hits_chunks(c, s, rays, nr, ray_stride, tmax, tmax_stride, tmax_all, k, stack_size, flags, chunk, out_t, out_prim, out_hit, hit_stride,
                             out_count, want_counts)) return rc;
    return query_end(c, stream);
}

// tirt_trace_hits: host arrays staged in device memory (QueryStage), through the chunks above, back to the host with a sync
int trace_hits_host(tirt_ctx *c, const float *rays, int nr, const float *tmax, int k, int stack_size, int flags, float *out_t, int32_t *out_prim,
                    float *out_hit, int32_t *out_count, int32_t *counts)
{
    if (int rc = query_common_checks(c, "tirt_trace_hits", "nr", nr, stack_size, flags)) return rc;
    if (nr == 0) return TIRT_OK;
    TIRT_REQUIRE(rays, "tirt_trace_hits: null rays");
    const size_t N = (size_t)nr, K = (size_t)k;
    const int chunk = hits_chunk_of(c, nr, k);
    HitsScratch s;
    if (int rc = hits_prepare(c, chunk, k, stack_size, s)) return rc;
    QueryStage q(c);      // (the walk is handed the outputs the caller asked for, and no others)
    const auto k_rays = q.in(rays, 6 * N);
    const auto k_tmax = q.in(tmax, N);
    const auto k_t = q.out(out_t, K * N, out_t != nullptr);
    const auto k_prim = q.out(out_prim, K * N, out_prim != nullptr);
    const auto k_hit = q.out(out_hit, 13 * K * N, out_hit != nullptr);
    const auto k_count = q.out(out_count, N, out_count != nullptr);
    const auto k_counts = q.out_counts(counts, flags, N);
    if (int rc = q.begin()) return rc;
    if (int rc = hits_chunks(c, s, q.ptr(k_rays), nr, 6, q.ptr(k_tmax), 1, __builtin_inff(), k, stack_size, flags, chunk, q.ptr(k_t), q.ptr(k_prim), q.ptr(k_hit), 13,
                             q.ptr(k_count), q.ptr(k_counts))) return rc;
    return q.finish();
}

}  // namespace tirt
