// tirt_dynamic.hip -- moving the triangles of an uploaded scene in place (tirt_vertex_update / tirt_vertex_update_device, tirt_scene_box).
//
// No reference counterpart as an entry point: the reference sets its vertex field once (Scene.setup_data_gpu, Scene.py:299-308).  What the host
// half of a fresh Scene derives from the positions is done here on the device, so that a moved scene followed by tirt_lbvh_build holds the bits
// of a scene built from the moved positions:
//
//   k_dyn_validate     the incoming positions are finite (nothing is written before this has said so)
//   k_dyn_scatter      positions -> columns 0..2, normals -> columns 3..5 of the vertex rows; without normals Scene.cal_normal's face normal
//                      (Scene.py:169-179): normalize((v1-v0) x (v2-v0)) in DOUBLE from the f32 positions, in numpy's operation order, rounded to
//                      f32 once (this file is compiled with -ffp-contract=off like the rest: no fused multiply-add; f64 sqrt and division are the
//                      compiler's correctly rounded expansions -- tests/test_gpu_dynamic.py compares them with numpy bit for bit)
//   k_dyn_box_partial  Scene._add_block's box over ALL vertex rows, starting from (+INF_VALUE, -INF_VALUE) as Scene.__init__ does: wave reduce, block
//   k_dyn_box_final    partials, one small second launch (min / max are exact: any order gives the host's bits).  Shapes do not extend it (quirk B8).
//
// Everything runs on the context's stream after sync_all (no batch in flight sees half-moved geometry), the device variant after the work
// queued on the caller's stream (one event, as tirt_query_*); the calls wait on the host, as the build that has to follow does anyway.
#include "tirt_internal.h"

namespace tirt {

constexpr int DYN_BLOCK = 256, DYN_BOX_BLOCKS_MAX = 1024;

// rows [count] of 3 floats at pos + i * stride: flag[0] = 1 if any of them is not finite (every writer stores the same value)
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_validate(const float *pos, int64_t stride, int64_t count, int *flag)
{
    const int64_t i = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i >= count) return;
    const float *p = pos + i * stride;
    const float x = p[0], y = p[1], z = p[2];
    const bool finite = ((int)(absf(x) <= 3.402823466e+38f) & (int)(absf(y) <= 3.402823466e+38f) & (int)(absf(z) <= 3.402823466e+38f)) != 0;      // false for NaN and +-inf
    if (!finite) flag[0] = 1;
}

// Where cal_normal normalises a zero vector (0.0 * inf) numpy leaves the host FPU's default NaN: on x86 (SSE) the sign bit is set, and that
// is what is written here.  On a host whose default NaN has it clear (AArch64) a fresh scene's NaN normals differ from these in that one bit:
// NaN in the same places, but not the same payload (tests/test_gpu_dynamic.py, test_face_normals_equal_cal_normal, would show it).
TD float dyn_round_normal(double v)
{
    const float f = (float)v;
    return f != f ? __int_as_float((int)0xffc00000u) : f;
}

// one thread per triangle t of the update: vertex rows first + 3t .. first + 3t + 2
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_scatter(float *vertex, int64_t first, int64_t ntri, const float *pos, int64_t pos_stride,
                                                           const float *nrm, int64_t nrm_stride)
{
    const int64_t t = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (t >= ntri) return;
    float p[3][3];
    for (int k = 0; k < 3; k++) {
        const float *s = pos + (3 * t + k) * pos_stride;
        p[k][0] = s[0]; p[k][1] = s[1]; p[k][2] = s[2];
    }
    float n[3][3];
    if (nrm) {
        for (int k = 0; k < 3; k++) {
            const float *s = nrm + (3 * t + k) * nrm_stride;
            n[k][0] = s[0]; n[k][1] = s[1]; n[k][2] = s[2];
        }
    } else {
        // Scene.cal_normal: a = v1 - v0, b = v2 - v0, n = a x b, inv = 1.0 / sqrt(n0 n0 + n1 n1 + n2 n2), n * inv -- every step rounded to double
        const double a0 = (double)p[1][0] - (double)p[0][0], a1 = (double)p[1][1] - (double)p[0][1], a2 = (double)p[1][2] - (double)p[0][2];
        const double b0 = (double)p[2][0] - (double)p[0][0], b1 = (double)p[2][1] - (double)p[0][1], b2 = (double)p[2][2] - (double)p[0][2];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        const double inv = 1.0 / sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        const float f0 = dyn_round_normal(c0 * inv), f1 = dyn_round_normal(c1 * inv), f2 = dyn_round_normal(c2 * inv);
        for (int k = 0; k < 3; k++) { n[k][0] = f0; n[k][1] = f1; n[k][2] = f2; }
    }
    for (int k = 0; k < 3; k++) {
        float *d = vertex + (size_t)(first + 3 * t + k) * VER_VEC;
        d[0] = p[k][0]; d[1] = p[k][1]; d[2] = p[k][2];
        d[3] = n[k][0]; d[4] = n[k][1]; d[5] = n[k][2];
    }
}

struct DynBox { float lo[3], hi[3]; };
TD void dyn_box_add(DynBox &b, float x, float y, float z)
{
    b.lo[0] = __builtin_fminf(b.lo[0], x); b.lo[1] = __builtin_fminf(b.lo[1], y); b.lo[2] = __builtin_fminf(b.lo[2], z);
    b.hi[0] = __builtin_fmaxf(b.hi[0], x); b.hi[1] = __builtin_fmaxf(b.hi[1], y); b.hi[2] = __builtin_fmaxf(b.hi[2], z);
}
// (an empty box must stay empty: its corners are not points of it)
TD void dyn_box_merge(DynBox &b, const float *lo, const float *hi)
{
    for (int k = 0; k < 3; k++) { b.lo[k] = __builtin_fminf(b.lo[k], lo[k]); b.hi[k] = __builtin_fmaxf(b.hi[k], hi[k]); }
}
// the box of the whole block in thread 0: xor-shuffles inside each wave, the four waves' boxes through LDS
TD void dyn_box_block_reduce(DynBox &b)
{
    __shared__ float part[DYN_BLOCK / 64][6];
    for (int off = 32; off >= 1; off >>= 1)
        for (int k = 0; k < 3; k++) {
            b.lo[k] = __builtin_fminf(b.lo[k], __shfl_xor(b.lo[k], off, 64));
            b.hi[k] = __builtin_fmaxf(b.hi[k], __shfl_xor(b.hi[k], off, 64));
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; k++) { part[wave][k] = b.lo[k]; part[wave][3 + k] = b.hi[k]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < DYN_BLOCK / 64; w++) dyn_box_merge(b, &part[w][0], &part[w][3]);
}
TD DynBox dyn_box_empty()
{
    DynBox b;
    for (int k = 0; k < 3; k++) { b.lo[k] = INF_VALUE; b.hi[k] = -INF_VALUE; }
    return b;
}
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_box_partial(const float *vertex, int nv, float *partial)
{
    DynBox b = dyn_box_empty();
    for (int64_t i = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x; i < nv; i += (int64_t)gridDim.x * DYN_BLOCK) {
        const float *p = vertex + (size_t)i * VER_VEC;
        dyn_box_add(b, p[0], p[1], p[2]);
    }
    dyn_box_block_reduce(b);
    if (threadIdx.x == 0) for (int k = 0; k < 3; k++) { partial[6 * blockIdx.x + k] = b.lo[k]; partial[6 * blockIdx.x + 3 + k] = b.hi[k]; }
}
__global__ __launch_bounds__(DYN_BLOCK) void k_dyn_box_final(const float *partial, int nparts, float *box)
{
    DynBox b = dyn_box_empty();
    for (int i = threadIdx.x; i < nparts; i += DYN_BLOCK) {
        const float *p = partial + 6 * (size_t)i;
        dyn_box_merge(b, p, p + 3);
    }
    dyn_box_block_reduce(b);
    if (threadIdx.x == 0) for (int k = 0; k < 3; k++) { box[k] = b.lo[k]; box[3 + k] = b.hi[k]; }
}

// what the runtime libtirt.so runs on knows about p: 1 = device (or managed) memory of this context's device, 0 = not known to it or
// host memory, -1 = another device's memory
static int dyn_pointer_kind(const tirt_ctx *c, const void *p)
{
    hipPointerAttribute_t at = {};
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();                               // an unknown pointer leaves a sticky error behind
    if (e != hipSuccess) return 0;
    if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return at.device == c->device ? 1 : -1;
    return 0;
}

// scratch: [0] the validation flag, [16 floats on] the box, then the block partials of the box, then the staged rows of the host variant
constexpr size_t DYN_OFF_BOX = 64, DYN_OFF_PARTIAL = 128, DYN_OFF_STAGE = DYN_OFF_PARTIAL + sizeof(float) * 6 * DYN_BOX_BLOCKS_MAX;

static int dyn_common_checks(tirt_ctx *c, const char *fn, int64_t first, int64_t count, const float *pos, int64_t pos_stride, const float *nrm,
                             int64_t nrm_stride)
{
    const std::string f(fn);
    TIRT_REQUIRE(c->n >= 1, f + ": no scene uploaded");
    TIRT_REQUIRE(first >= 0 && count >= 0 && first <= (int64_t)c->nv && count <= (int64_t)c->nv - first,
                 f + ": vertices first .. first + count - 1 are not all within the uploaded scene's " + std::to_string(c->nv));
    TIRT_REQUIRE(first % 3 == 0 && count % 3 == 0, f + ": first and count are in vertices and must be multiples of 3 (whole triangles)");
    if (count == 0) return TIRT_OK;
    TIRT_REQUIRE(pos, f + ": null pos");
    TIRT_REQUIRE(pos_stride >= 3, f + ": pos_stride < 3 (floats per row)");
    TIRT_REQUIRE(!nrm || nrm_stride >= 3, f + ": nrm_stride < 3 (floats per row)");
    return TIRT_OK;
}

// validate, scatter, box -- `pos` / `nrm` are device memory by now (the caller's own in the device variant, read twice: by the validation and,
// after a host wait, by the scatter -- the rows must not change during the call, include/tirt.h); the context is idle (sync_all) and c->stream ordered after the caller's work
static int dyn_apply(tirt_ctx *c, const char *fn, int64_t first, int64_t count, const float *pos, int64_t pos_stride, const float *nrm,
                     int64_t nrm_stride)
{
    hipStream_t st = c->stream;
    char *base = c->dyn_mem.as<char>();
    int *flag = (int *)base;
    float *box = (float *)(base + DYN_OFF_BOX), *partial = (float *)(base + DYN_OFF_PARTIAL);
    TIRT_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_dyn_validate, dim3((unsigned)((count + DYN_BLOCK - 1) / DYN_BLOCK)), dim3(DYN_BLOCK), 0, st, pos, pos_stride, count, flag);
    int bad = 0;
    TIRT_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    TIRT_HIP(hipStreamSynchronize(st));
    TIRT_HIP(hipGetLastError());
    TIRT_REQUIRE(!bad, std::string(fn) + ": a position is NaN or infinite (nothing was changed)");

    // With motion records on and a history to carry (tirt_temporal.hip) the first update since the last accumulate keeps the rows that view saw.
    // The history stays, marked as moved, only once everything below has succeeded: a call that fails half way leaves it empty
    const bool keep_history = c->mv_rec.p && c->tp_valid;
    if (keep_history && !c->mv_moved) {
        const size_t bytes = sizeof(float) * VER_VEC * (size_t)c->nv;
        if (c->mv_snap.ensure(bytes)) return TIRT_ERR_HIP;
        TIRT_HIP(hipMemcpyAsync(c->mv_snap.p, c->vertex.p, bytes, hipMemcpyDeviceToDevice, st));
    }
    c->tp_valid = false;                       // the rows change from here on: without motion records the history assumes the world stood still
    const int64_t ntri = count / 3;
    hipLaunchKernelGGL(k_dyn_scatter, dim3((unsigned)((ntri + DYN_BLOCK - 1) / DYN_BLOCK)), dim3(DYN_BLOCK), 0, st, c->vertex.as<float>(), first, ntri,
                       pos, pos_stride, nrm, nrm_stride);
    int nb = (c->nv + DYN_BLOCK - 1) / DYN_BLOCK;
    if (nb > DYN_BOX_BLOCKS_MAX) nb = DYN_BOX_BLOCKS_MAX;
    hipLaunchKernelGGL(k_dyn_box_partial, dim3(nb), dim3(DYN_BLOCK), 0, st, (const float *)c->vertex.as<float>(), c->nv, partial);
    hipLaunchKernelGGL(k_dyn_box_final, dim3(1), dim3(DYN_BLOCK), 0, st, (const float *)partial, nb, box);
    float hb[6];
    TIRT_HIP(hipMemcpyAsync(hb, box, sizeof(hb), hipMemcpyDeviceToHost, st));
    // from here on the old build describes geometry that is gone, whatever the copy and the sync below return
    c->built = false; c->built_sah = 0; c->shade_rec_valid = false; c->light_rec_valid = false; c->pvb_valid = false; c->sd_tab_valid = false; c->wn_tab_valid = false;
    refresh_shade_features(c);                 // (with the tables it selects kernels for; moving vertices changes no bit of it)
    TIRT_HIP(hipStreamSynchronize(st));
    TIRT_HIP(hipGetLastError());
    for (int k = 0; k < 3; k++) { c->bmin[k] = hb[k]; c->bmax[k] = hb[3 + k]; }
    if (keep_history) { c->tp_valid = true; c->mv_moved = true; }      // the snapshot holds the rows of the last accumulated view
    return TIRT_OK;
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_vertex_update(tirt_ctx *c, int64_t first, int64_t count, const float *pos, int64_t pos_stride, const float *nrm, int64_t nrm_stride)
{
    const char *fn = "tirt_vertex_update";
    TIRT_REQUIRE(c, "null context");
    TIRT_HIP(hipSetDevice(c->device));
    if (int rc = dyn_common_checks(c, fn, first, count, pos, pos_stride, nrm, nrm_stride)) return rc;
    if (count == 0) return TIRT_OK;
    TIRT_REQUIRE(dyn_pointer_kind(c, pos) == 0, "tirt_vertex_update: pos is device memory (tirt_vertex_update_device takes device pointers)");
    TIRT_REQUIRE(!nrm || dyn_pointer_kind(c, nrm) == 0, "tirt_vertex_update: nrm is device memory while pos is host memory (both host here, both device in tirt_vertex_update_device)");
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    const size_t rows = (size_t)count, stage_floats = 3 * rows * (nrm ? 2 : 1);
    if (c->dyn_mem.ensure(DYN_OFF_STAGE + sizeof(float) * stage_floats)) return TIRT_ERR_HIP;
    float *d_pos = (float *)(c->dyn_mem.as<char>() + DYN_OFF_STAGE), *d_nrm = nrm ? d_pos + 3 * rows : nullptr;
    // rows of stride 3 go as they are; others are packed first (the vector outlives the copy: dyn_apply ends with a sync)
    std::vector<float> packed;
    const float *src_pos = pos, *src_nrm = nrm;
    if (pos_stride != 3 || (nrm && nrm_stride != 3)) {
        packed.resize(stage_floats);
        for (size_t i = 0; i < rows; i++) for (int k = 0; k < 3; k++) packed[3 * i + k] = pos[i * (size_t)pos_stride + k];
        if (nrm) for (size_t i = 0; i < rows; i++) for (int k = 0; k < 3; k++) packed[3 * (rows + i) + k] = nrm[i * (size_t)nrm_stride + k];
        src_pos = packed.data(); src_nrm = nrm ? packed.data() + 3 * rows : nullptr;
    }
    TIRT_HIP(hipMemcpyAsync(d_pos, src_pos, sizeof(float) * 3 * rows, hipMemcpyHostToDevice, c->stream));
    if (nrm) TIRT_HIP(hipMemcpyAsync(d_nrm, src_nrm, sizeof(float) * 3 * rows, hipMemcpyHostToDevice, c->stream));
    const int rc = dyn_apply(c, fn, first, count, d_pos, 3, d_nrm, 3);
    if (rc == TIRT_ERR_HIP) (void)hipStreamSynchronize(c->stream);      // `packed` must not go while a copy may still read it
    return rc;
}

int tirt_vertex_update_device(tirt_ctx *c, int64_t first, int64_t count, const float *pos, int64_t pos_stride, const float *nrm, int64_t nrm_stride,
                              void *stream)
{
    const char *fn = "tirt_vertex_update_device";
    TIRT_REQUIRE(c, "null context");
    TIRT_HIP(hipSetDevice(c->device));
    if (int rc = dyn_common_checks(c, fn, first, count, pos, pos_stride, nrm, nrm_stride)) return rc;
    if (int rc = require_caller_stream(c, fn, stream, "a geometry update")) return rc;
    if (count == 0) return TIRT_OK;
    const char *why = " is not device memory of this context's device (a host pointer -- both pointers host: tirt_vertex_update --, another device's "
                      "memory, or memory of a second HIP runtime in the process)";
    TIRT_REQUIRE(dyn_pointer_kind(c, pos) == 1, std::string("tirt_vertex_update_device: pos") + why);
    TIRT_REQUIRE(!nrm || dyn_pointer_kind(c, nrm) == 1, std::string("tirt_vertex_update_device: nrm") + why);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    if (c->dyn_mem.ensure(DYN_OFF_STAGE)) return TIRT_ERR_HIP;
    if (!c->query_ev_in) TIRT_HIP(hipEventCreateWithFlags(&c->query_ev_in, hipEventDisableTiming));
    TIRT_HIP(hipEventRecord(c->query_ev_in, (hipStream_t)stream));
    TIRT_HIP(hipStreamWaitEvent(c->stream, c->query_ev_in, 0));
    return dyn_apply(c, fn, first, count, pos, pos_stride, nrm, nrm_stride);
}

int tirt_scene_box(tirt_ctx *c, float bmin[3], float bmax[3])
{
    TIRT_REQUIRE(c, "null context");
    TIRT_REQUIRE(bmin && bmax, "tirt_scene_box: null pointer");
    TIRT_REQUIRE(c->n >= 1, "tirt_scene_box: no scene uploaded");
    for (int k = 0; k < 3; k++) { bmin[k] = c->bmin[k]; bmax[k] = c->bmax[k]; }
    return TIRT_OK;
}

}  // extern "C"
