// tirt_debug.hip -- the Debug integrator: one primary-hit view per pixel.
//
// Reference: integrator/Debug.py:44-67 is one per-pixel kernel -- camera ray (Camera.py:122-142), Scene.closet_hit, and an
// AOV written over hdr[i, j]: the hit's material colour (:65) or one of its normals mapped to [0, 1] (:62-64, commented
// out there).  No bounce loop, no shading, no running mean.  Here it is three launches on the context's main stream:
//
//   k_debug_generate   camera direction of every local pixel            Camera.py:131-142
//   k_trace<closest>   closest hit, origin = the eye (TraceArgs::eye)    Scene.py:702-744 (trace_rays, tirt_trace.hip)
//   k_debug_resolve    the view of the chosen mode, written to hdr       integrator/Debug.py:55-67
//
// Queue index k is local pixel k of this context's tile (local_to_pixel): a wave holds an 8 x 8 pixel bundle, as in k_generate.
// Pixels of other tiles are not touched.
#include "tirt_trace.h"

namespace tirt {

__global__ void k_debug_generate(CameraView cam, TileMap tm, int P, uint32_t frame, uint32_t seed, float *dx, float *dy, float *dz)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = local_to_pixel(tm, k);
    const int i = p / tm.H, j = p - i * tm.H;
    float jx = 0.0f, jy = 0.0f;
    if (frame != 0) {                                    // Camera.py:135-137, the same draws as k_generate
        jx = tm_rand(seed, (uint32_t)p, frame, TM_DIM_JX) - 0.5f;
        jy = tm_rand(seed, (uint32_t)p, frame, TM_DIM_JY) - 0.5f;
    }
    const v3 d = camera_ray_direction(cam, i, j, jx, jy);
    dx[k] = d.x; dy[k] = d.y; dz[k] = d.z;
}

// integrator/Debug.py:55-67.  A miss writes (0, 0, 0).  On a hit:
//   albedo   get_material_color(material, get_prim_mindex(primitive, prim_id))      (:65, UtilsFunc.py:132-133); a textured material: tex_albedo at the hit's uv
//   fnormal  (faceforward(normal, -direction, gnormal) + 1) * 0.5                   (:62; UtilsFunc.py:466-467: sign(dot(i, nref)) * n)
//   normal   (normal + 1) * 0.5                                                     (:63); a normal-mapped material: the mapped normal, here and in fnormal
//   gnormal  (gnormal + 1) * 0.5                                                    (:64)
__global__ void k_debug_resolve(SceneView sc, v3 eye, TileMap tm, int P, int mode, const float *dx, const float *dy, const float *dz,
                                const float4 *hit, float *hdr)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = local_to_pixel(tm, k);
    const float4 h = hit[k];
    v3 rad = V(0.0f, 0.0f, 0.0f);
    if (h.x < INF_VALUE) {
        const int prim = __float_as_int(h.w);
        if (mode == TIRT_DEBUG_ALBEDO) {
            const float *m = sc.material + (size_t)sc.primitive[(size_t)prim * PRI_VEC + 2] * MAT_VEC;
            rad = V(m[2], m[3], m[4]);
            if (sc.tex) {                                // a textured material: the texture's colour at the hit's uv (tirt_device.h, tex_albedo)
                const int ti = material_texture(m);
                if (ti >= 0) { const HitAttr a = hit_attributes(sc, eye, V(dx[k], dy[k], dz[k]), prim, h.x, h.y, h.z); rad = tex_albedo(sc.tex, ti, a.tex.x, a.tex.y); }
            }
        } else {
            const v3 d = V(dx[k], dy[k], dz[k]);
            const HitAttr a = hit_attributes(sc, eye, d, prim, h.x, h.y, h.z);
            v3 nor = a.nor;                              // a normal-mapped material: the mapped normal (tirt_device.h, tex_normal), in the normal and fnormal views
            if (sc.tex && mode != TIRT_DEBUG_GNORMAL) nor = shading_normal_rows(sc, sc.material + (size_t)sc.primitive[(size_t)prim * PRI_VEC + 2] * MAT_VEC, prim, a.tex, nor);
            v3 n = (mode == TIRT_DEBUG_GNORMAL) ? a.gnor : nor;
            if (mode == TIRT_DEBUG_FNORMAL) { const float s = signf(dot(-d, a.gnor)); n = V(s * n.x, s * n.y, s * n.z); }
            rad = V((n.x + 1.0f) * 0.5f, (n.y + 1.0f) * 0.5f, (n.z + 1.0f) * 0.5f);
        }
    }
    float *o = hdr + (size_t)p * 3;
    o[0] = rad.x; o[1] = rad.y; o[2] = rad.z;
}

// The first two launches: the camera rays of this context's local pixels at `frame` (0: through the pixel centres, no jitter) and their closest
// hits, both in c->debug_mem, indexed by local pixel.  The callers have checked the build, the camera and the film.
int debug_trace(tirt_ctx *c, uint32_t frame, uint32_t seed, int stack_size, int flags, DebugRays &r)
{
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    const int P = (int)c->npix_local;
    // scratch: one hit record (16 B) and three direction words per local pixel
    const size_t hit_bytes = sizeof(float4) * (size_t)P, dir_bytes = sizeof(float) * (((size_t)P + 3) & ~(size_t)3);
    if (c->debug_mem.ensure(hit_bytes + 3 * dir_bytes)) return TIRT_ERR_HIP;
    r.hit = c->debug_mem.as<float4>();
    r.dx = (float *)((char *)c->debug_mem.p + hit_bytes); r.dy = (float *)((char *)r.dx + dir_bytes); r.dz = (float *)((char *)r.dy + dir_bytes);
    r.tm = TileMap{c->tile_rank, c->tile_count, c->tile_size, c->H, c->tile_blocked, 0};
    const int B = 256, G = (P + B - 1) / B;
    hipLaunchKernelGGL(k_debug_generate, dim3(G), dim3(B), 0, c->stream, c->cam, r.tm, P, frame, seed, r.dx, r.dy, r.dz);
    TraceJob job; job.stack_size = stack_size; job.flags = flags; job.dx = r.dx; job.dy = r.dy; job.dz = r.dz; job.count = P; job.hit = r.hit; job.grid_cap = c->tr_grid_alone;
    c->launches_trace_closest++;
    return trace_rays(c, job);
}

int debug_render(tirt_ctx *c, uint32_t frame, uint32_t seed, int mode, int stack_size, int flags)
{
    TIRT_REQUIRE(c->built, "tirt_debug_render: LBVH not built");
    TIRT_REQUIRE(c->cam_set, "tirt_debug_render: camera not set");
    TIRT_REQUIRE(c->hdr.p && c->npix_local >= 0, "tirt_debug_render: film not created");
    TIRT_REQUIRE(mode >= TIRT_DEBUG_ALBEDO && mode <= TIRT_DEBUG_GNORMAL, "tirt_debug_render: mode is one of TIRT_DEBUG_*");
    TIRT_REQUIRE(stack_size >= 1 && stack_size <= 4096, "tirt_debug_render: stack_size 1..4096");
    TIRT_REQUIRE((flags & ~(TIRT_TRAVERSE_EXHAUSTIVE | TIRT_COUNT_NODES)) == 0, "tirt_debug_render: unknown flags");
    if (c->npix_local == 0) return TIRT_OK;
    DebugRays r;
    if (int rc = debug_trace(c, frame, seed, stack_size, flags, r)) return rc;
    const int P = (int)c->npix_local, B = 256, G = (P + B - 1) / B;
    v3 eye; eye.x = c->cam.eye[0]; eye.y = c->cam.eye[1]; eye.z = c->cam.eye[2];
    hipLaunchKernelGGL(k_debug_resolve, dim3(G), dim3(B), 0, c->stream, scene_view(c), eye, r.tm, P, mode, r.dx, r.dy, r.dz, r.hit, c->hdr.as<float>());
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

}  // namespace tirt
