// tirt_aov.hip -- feature buffers of the path tracer: first-hit albedo, shading normal, depth and coverage of the film's own camera rays.
//
// No reference counterpart (integrator/Debug.py writes one such view per call over hdr).  After the bounce-0 traversal of a wavefront batch
// PathState::hit[0 .. S) holds the closest hit of every camera ray and PathSoA st[0].dx / dy / dz its direction, on both routes (k_trace alone,
// or the candidate lists + leftover k_trace + scatter); both stay as they are until bounce 1.  k_aov is one more reader of them: per local pixel
// it folds the F samples of the batch, in frame order, into the pixel's TIRT_AOV_WORDS running means with k_film's recurrence
// (integrator/PT_RGB.py:134-136).  The values are k_debug_resolve's (tirt_debug.hip): the same material row (or albedo texture), the same hit_attributes call.
//
// Batches run on different lanes and the recurrence is order dependent, so the k_aov launches are chained through events of their own
// (Lane::aov_done, tirt_ctx::last_aov) -- not through last_film, which is recorded at the END of a batch and would serialise the lanes.
#include "tirt_internal.h"

namespace tirt {

typedef float f4s__ __attribute__((ext_vector_type(4)));

// One thread per local pixel k.  The slot's hit record (one 16-byte load) and direction words are streams, read once: non-temporal.  The loads of
// frame f + 1 are issued before the dependent gathers of frame f (primitive row -> vertex rows / material row) are waited for.
// LIST: the batch's local pixels are a pixel set's list (mapped_pixel, tirt_internal.h).
template <bool LIST>
__global__ __launch_bounds__(256) void k_aov(SceneView sc, v3 eye, TileMap tm, int P, int F, uint32_t frame_begin, const float4 *hit,
                                             const float *dx, const float *dy, const float *dz, float *aov)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = mapped_pixel<LIST>(tm, k);
    float4 *const px = (float4 *)(aov + (size_t)p * TIRT_AOV_WORDS);
    const float4 lo = px[0], hi = px[1];
    float a0 = lo.x, a1 = lo.y, a2 = lo.z, a3 = lo.w, a4 = hi.x, a5 = hi.y, a6 = hi.z, a7 = hi.w;
    int s = frame_pixel_to_slot(tm, P, 0, k);
    f4s__ h = __builtin_nontemporal_load((const f4s__ *)&hit[s]);
    v3 d = V(__builtin_nontemporal_load(&dx[s]), __builtin_nontemporal_load(&dy[s]), __builtin_nontemporal_load(&dz[s]));
    for (int f = 0; f < F; f++) {
        f4s__ hn = h; v3 dn = d;
        if (f + 1 < F) {
            s = frame_pixel_to_slot(tm, P, f + 1, k);
            hn = __builtin_nontemporal_load((const f4s__ *)&hit[s]);
            dn = V(__builtin_nontemporal_load(&dx[s]), __builtin_nontemporal_load(&dy[s]), __builtin_nontemporal_load(&dz[s]));
        }
        v3 alb = V(0.0f, 0.0f, 0.0f), nor = alb;
        float depth = 0.0f, alpha = 0.0f;
        if (h.x < INF_VALUE) {
            const int prim = __float_as_int(h.w);
            const float *m = sc.material + (size_t)sc.primitive[(size_t)prim * PRI_VEC + 2] * MAT_VEC;
            alb = V(m[2], m[3], m[4]);
            const HitAttr a = hit_attributes(sc, eye, d, prim, h.x, h.y, h.z);
            nor = a.nor;
            // a textured material: the texture's colour at the hit's uv (tirt_device.h, tex_albedo), as k_shade's reflectance before srgb_to_lrgb
            if (sc.tex) {
                const int ti = material_texture(m); if (ti >= 0) alb = tex_albedo(sc.tex, ti, a.tex.x, a.tex.y);
                nor = shading_normal_rows(sc, m, prim, a.tex, nor);      // a normal-mapped material: the mapped normal, as k_shade's `normal`
            }
            depth = h.x; alpha = 1.0f;
        }
        const float frame = (float)(int)(frame_begin + (uint32_t)f);
        const float coff = 1.0f / (frame + 1.0f);
        a0 = alb.x * coff + a0 * (1.0f - coff);
        a1 = alb.y * coff + a1 * (1.0f - coff);
        a2 = alb.z * coff + a2 * (1.0f - coff);
        a3 = nor.x * coff + a3 * (1.0f - coff);
        a4 = nor.y * coff + a4 * (1.0f - coff);
        a5 = nor.z * coff + a5 * (1.0f - coff);
        a6 = depth * coff + a6 * (1.0f - coff);
        a7 = alpha * coff + a7 * (1.0f - coff);
        h = hn; d = dn;
    }
    px[0] = make_float4(a0, a1, a2, a3);
    px[1] = make_float4(a4, a5, a6, a7);
}

// Queued on the lane's stream once the bounce-0 closest hits of its batch are complete, and before anything of bounce 1 (pt_render).
int aov_launch(tirt_ctx *c, Lane &L, const TileMap &tm, int P, int F, uint32_t frame_begin)
{
    // the running mean is order dependent: this batch's records follow the previous batch's
    if (c->last_aov) TIRT_HIP(hipStreamWaitEvent(L.stream, c->last_aov, 0));
    v3 eye; eye.x = c->cam.eye[0]; eye.y = c->cam.eye[1]; eye.z = c->cam.eye[2];
    const int B = 256;
    hipLaunchKernelGGL(tm.pixels ? k_aov<true> : k_aov<false>, dim3((P + B - 1) / B), dim3(B), 0, L.stream, scene_view(c), eye, tm, P, F, frame_begin, L.ps.hit,
                       L.ps.st[0].dx, L.ps.st[0].dy, L.ps.st[0].dz, c->aov.as<float>());
    TIRT_HIP(hipEventRecord(L.aov_done, L.stream));
    c->last_aov = L.aov_done;
    return TIRT_OK;
}

}  // namespace tirt
