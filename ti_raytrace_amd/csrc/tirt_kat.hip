// tirt_kat.hip -- the known-answer entry points of include/tirt.h (tirt_kat_*): device functions evaluated row by row, one thread per row, for the tests
// that hold them to the oracle bit for bit.  Every entry checks its own arguments and then makes one kat_round_trip (tirt_internal.h).  The kernels of
// tirt_kat_env_*, tirt_kat_shade_step, tirt_kat_shade_spec_step and tirt_kat_spec live beside the code they evaluate (tirt_envsample.hip, tirt_render.hip, tirt_spectral.hip).
#include "tirt_internal.h"
#include "tirt_spectral.h"
#include "tirt_pvb.h"

namespace tirt {

// ---- known-answer-test kernels ------------------------------------------------------------------------
__global__ void k_kat_math(int fn, const float *x, const float *y, float *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.0f;
    switch (fn) {
        case 0: r = tm_sin(x[i]); break;
        case 1: r = tm_cos(x[i]); break;
        case 2: r = tm_exp(x[i]); break;
        case 3: r = tm_log(x[i]); break;
        case 4: r = tm_pow(x[i], y[i]); break;
        case 5: r = tm_atan2(x[i], y[i]); break;
        case 6: r = tm_acos(x[i]); break;
        case 7: r = tm_sqrt(x[i]); break;
        case 8: r = x[i] / y[i]; break;
        case 9: r = tm_rand(tm_f2u(x[i]), tm_f2u(y[i]), 3u, 5u); break;
        case 10: { float sn, cs; tm_sincos(x[i], &sn, &cs); r = sn; } break;
        case 11: { float sn, cs; tm_sincos(x[i], &sn, &cs); r = cs; } break;
    }
    out[i] = r;
}
__global__ void k_kat_brdf(int which, const float *in, int in_stride, float *out, int out_stride, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * in_stride;
    float *o = out + (size_t)i * out_stride;
    if (which == 0) {
        float pdf; float f = disney_evaluate_pdf(a, V(a[10], a[11], a[12]), V(a[13], a[14], a[15]), V(a[16], a[17], a[18]), pdf);
        o[0] = f; o[1] = pdf;
    } else if (which == 1) {
        v3 r = disney_sample(a, V(a[10], a[11], a[12]), V(a[13], a[14], a[15]), a[16], a[17], a[18]);
        o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 2) {
        float fb; v3 r = glass_sample(a, V(a[10], a[11], a[12]), V(a[13], a[14], a[15]), a[16], fb);
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = fb;
    } else if (which == 3) {
        v3 r = offset_ray(V(a[0], a[1], a[2]), V(a[3], a[4], a[5]));
        o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 4) {
        v3 r = cosine_sample_hemisphere(a[0], a[1]); o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 5) {
        map_to_disk(a[0], a[1], o[0], o[1]);
    } else if (which == 6) {
        o[0] = power_heuristic(a[0], a[1]);
    } else if (which == 7) {
        v3 r = inverse_transform(V(a[0], a[1], a[2]), V(a[3], a[4], a[5])); o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 8) {
        v3 r = srgb_to_lrgb(V(a[0], a[1], a[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 9) {
        o[0] = lrgb_to_srgb1(a[0]); o[1] = lrgb_to_srgb1(a[1]); o[2] = lrgb_to_srgb1(a[2]);
    } else if (which == 10) {
        o[0] = tone_aces1(a[0]); o[1] = tone_aces1(a[1]); o[2] = tone_aces1(a[2]);
    } else if (which == 11) {
        float suc; v3 r = refract_(V(a[0], a[1], a[2]), V(a[3], a[4], a[5]), a[6], suc); o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = suc;
    } else if (which == 12) {
        o[0] = schlick(a[0], a[1]);
    } else if (which == 13) {
        o[0] = gtr2(a[0], a[1]);
    } else if (which == 14) {
        o[0] = smithg_ggx(a[0], a[1]);
    } else if (which == 15) {
        o[0] = schlick_fresnel(a[0]);
    } else if (which == 16) {
        float fb; v3 r = glass_sample_lambda(V(a[0], a[1], a[2]), V(a[3], a[4], a[5]), a[6], a[7], fb); o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = fb;
    } else if (which == 17) {
        CameraView cv; for (int k = 0; k < 12; k++) cv.view_inv[k] = a[k];
        cv.eye[0] = cv.eye[1] = cv.eye[2] = 0.0f; cv.fx = a[16]; cv.fy = a[17]; cv.cx = a[18]; cv.cy = a[19];
        v3 r = camera_ray_direction(cv, (int)a[20], (int)a[21], a[22], a[23]); o[0] = r.x; o[1] = r.y; o[2] = r.z;
    } else if (which == 18) {
        const RayCtx r = make_ray(V(a[0], a[1], a[2]), V(a[3], a[4], a[5])); float tn;
        const int full = slabs(r, a[6], a[7], a[8], a[9], a[10], a[11], tn);
        o[0] = (float)full;
        o[1] = ray_has_parallel_axis(r) ? (float)full : (float)slabs_fast(r, a[6], a[7], a[8], a[9], a[10], a[11], tn);     // the branch-free form k_trace uses where it may
    }
}

// ---- known-answer kernels of the shading tables (tests/test_gpu_shade_tables.py): the un-hoisted device functions, per primitive / light / sample ----
// which 0, per primitive i: hit_attributes' gnor (zero for a shape: a sphere's normal depends on the hit), get_prim_area   -> gnor3, area
// which 1, per light list entry i: get_prim_area, the choice pdf of sample_li (after light_shape_visible), the material colour  -> area, pdf, rgb
__global__ void k_kat_shade_tables(SceneView s, int which, float *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (which == 0) {
        float *o = out + (size_t)i * 4;
        v3 g = V(0.0f, 0.0f, 0.0f);
        if (s.primitive[(size_t)i * PRI_VEC] == PRIMITIVE_TRI) g = hit_attributes(s, g, V(0.0f, 0.0f, 1.0f), i, 1.0f, 0.25f, 0.25f).gnor;
        o[0] = g.x; o[1] = g.y; o[2] = g.z; o[3] = get_prim_area(s, i);
    } else {
        float *o = out + (size_t)i * 5;
        const int light_prim = s.light[i];
        const float *lm = s.material + (size_t)s.primitive[(size_t)light_prim * PRI_VEC + 2] * MAT_VEC;
        const float light_area = get_prim_area(s, light_prim);
        float light_choice_pdf = 1.0f / ((float)s.light_count * light_area);
        (void)light_shape_visible(s, light_prim, V(0.0f, 0.0f, 1.0f), V(0.0f, 0.0f, 1.0f), 1.0f, light_choice_pdf);
        o[0] = light_area; o[1] = light_choice_pdf; o[2] = lm[2]; o[3] = lm[3]; o[4] = lm[4];
    }
}
// One NEE set-up of Scene.sample_li for (random number of the light choice, a, b, shaded point): first by the un-hoisted functions, then from the
// light records.  in: u, a, b, p3 -> out: 2 x (pos3, normal3 after its three normalisations, emission3 x visible, area, choice pdf, light_dist)
TD void kat_nee_store(float *o, v3 pos, v3 nor, v3 em, float area, float pdf, float dist)
{ o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = nor.x; o[4] = nor.y; o[5] = nor.z; o[6] = em.x; o[7] = em.y; o[8] = em.z; o[9] = area; o[10] = pdf; o[11] = dist; }
__global__ void k_kat_light_sample(SceneView s, const float *in, float *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * 6;
    float *o = out + (size_t)i * 24;
    int lidx = (int)(a[0] * (float)s.light_count);
    if (lidx >= s.light_count) lidx = s.light_count - 1;
    if (lidx < 0) lidx = 0;                                  // (a test input outside [0, 1]: stay inside the tables)
    const v3 p = V(a[3], a[4], a[5]);
    {
        const int light_prim = s.light[lidx];
        v3 light_pos, light_normal;
        get_prim_random_point_normal(s, light_prim, a[1], a[2], light_pos, light_normal);
        const float *lm = s.material + (size_t)s.primitive[(size_t)light_prim * PRI_VEC + 2] * MAT_VEC;
        const float light_area = get_prim_area(s, light_prim);
        float light_choice_pdf = 1.0f / ((float)s.light_count * light_area);
        light_normal = normalized(light_normal);
        v3 light_dir = p - light_pos;
        const float light_dist = norm(light_dir);
        light_dir = light_dir / light_dist;
        const v3 em = V(lm[2], lm[3], lm[4]) * light_shape_visible(s, light_prim, light_dir, light_normal, light_dist, light_choice_pdf);
        kat_nee_store(o, light_pos, light_normal, em, light_area, light_choice_pdf, light_dist);
    }
    {
        v3 light_pos, light_normal;
        const LightRec lr = light_sample_rec(s.light_rec, lidx, a[1], a[2], light_pos, light_normal);
        light_normal = normalized(light_normal);
        v3 light_dir = p - light_pos;
        const float light_dist = norm(light_dir);
        light_dir = light_dir / light_dist;
        const v3 em = lr.emission * light_shape_visible_rec(lr, light_dir, light_normal, light_dist);
        kat_nee_store(o + 12, light_pos, light_normal, em, lr.area, lr.choice_pdf, light_dist);
    }
}

// ---- known-answer evaluation of tex_alpha and the cut-out decision (tirt_kat_texture_alpha): row i on thread i ----
__global__ void k_kat_texture_alpha(const int *tex, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * in_stride;
    const float al = tex_alpha(tex, __float_as_int(a[0]), a[1], a[2]);
    float *o = out + (size_t)i * out_stride;
    o[0] = al; o[1] = al >= 0.5f ? 1.0f : 0.0f;
}
// ---- known-answer evaluation of tex_albedo (tirt_kat_texture): row i on thread i ----
__global__ void k_kat_texture(const int *tex, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * in_stride;
    float *o = out + (size_t)i * out_stride;
    const v3 c = tex_albedo(tex, __float_as_int(a[0]), a[1], a[2]);
    const v3 l = srgb_to_lrgb(c);
    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = l.x; o[4] = l.y; o[5] = l.z;
}

// ---- known-answer evaluation of the material maps (tirt_kat_material_maps): row i on thread i, from the vertex rows as k_aov and Debug read them ----
__global__ void k_kat_material_maps(SceneView sc, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * in_stride;
    float *o = out + (size_t)i * out_stride;
    const int prim = __float_as_int(a[0]);
    const int *pr = sc.primitive + (size_t)prim * PRI_VEC;
    const float *m = sc.material + (size_t)pr[2] * MAT_VEC;
    v3 uv = V(0.0f, 0.0f, 0.0f), N = uv;
    // hit_attributes' expressions for uv and normal, restated here because that function needs a ray (for shapes) and these rows have none: a change to its
    // interpolation must be made here too -- tests/test_gpu_material_maps.py holds k_aov and Debug, which call hit_attributes, and this entry to one restatement.
    // A shape has uv 0 and, without a ray, no normal here: (0, 0, 0)
    if (pr[0] == PRIMITIVE_TRI) {
        const int vi = pr[1];
        const float u = a[1], v = a[2], ba = 1.0f - u - v;
        uv = (vtx_uv(sc, vi) * ba + vtx_uv(sc, vi + 1) * u) + vtx_uv(sc, vi + 2) * v;
        N = normalized((vtx_nor(sc, vi) * ba + vtx_nor(sc, vi + 1) * u) + vtx_nor(sc, vi + 2) * v);
    }
    float rough = m[6], metal = m[5];
    const int ri = material_map(m, 7), mi = material_map(m, 8);
    if (ri >= 0) rough = tex_roughness(sc.tex, ri, uv.x, uv.y);
    if (mi >= 0) metal = tex_metallic(sc.tex, mi, uv.x, uv.y);
    const v3 Np = shading_normal_rows(sc, m, prim, uv, N);
    o[0] = uv.x; o[1] = uv.y; o[2] = rough; o[3] = metal; o[4] = Np.x; o[5] = Np.y; o[6] = Np.z; o[7] = 0.0f;
}

// ---- one camera ray against its pixel's candidate list (tirt_kat_primary_list_walk): pvb_walk_list itself -- the function k_pvb_cand and k_pvb_cand_shade call --
// on the context's lists.  Blocks of one wave, row r on lane r & 63 of wave r >> 6: the caller's order decides which rays share a wave and its ballots.  The
// padding lanes of the last wave make the call with live = false, as the padding threads of a batch do.
__global__ __launch_bounds__(64) void k_kat_pvb_walk(BvhView b, PvbView pv, CameraView cam, TileMap tm, int P, const int *local_pixel, const float *jx, const float *jy,
                                                     float *out, int out_stride, int n)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    const bool live = r < n;
    const int k = live ? local_pixel[r] : 0;
    const int p = local_to_pixel(tm, k), i = p / tm.H, j = p - i * tm.H;
    const v3 d = live ? camera_ray_direction(cam, i, j, jx[r], jy[r]) : V(0.0f, 0.0f, 1.0f);
    const v3 eye = V(cam.eye[0], cam.eye[1], cam.eye[2]);
    float hit_t, hit_u, hit_v; int hit_prim;
    int steps = 0, trips = 0;
    const bool resolved = pvb_walk_list(b, pv, P, k, live, eye, d, hit_t, hit_u, hit_v, hit_prim, steps, trips);
    if (!live) return;
    float *o = out + (size_t)r * out_stride;
    o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = resolved ? 1.0f : 0.0f;
    o[4] = hit_t; o[5] = hit_u; o[6] = hit_v; o[7] = __int_as_float(hit_prim); o[8] = (float)steps;
}

}  // namespace tirt

using namespace tirt;

extern "C" {

int tirt_kat_primary_list_walk(tirt_ctx *c, int n, const int32_t *local_pixel, const float *jx, const float *jy, float *out, int out_stride)
{
    const char *fn = "tirt_kat_primary_list_walk";
    TIRT_REQUIRE(local_pixel && jx && jy && out && n >= 0, std::string(fn) + ": null pointer or negative n");
    TIRT_REQUIRE(out_stride >= 9, std::string(fn) + ": stride too small (9 words out)");
    CTX(c);
    bool have = false;
    if (int rc = pvb_lists_for_tests(c, fn, have)) return rc;
    TIRT_REQUIRE(have, std::string(fn) + ": the context has no candidate lists (option \"primary_beams\" off, a scene with cut-outs, an empty film or no list memory)");
    const int P = (int)c->npix_local;
    for (int i = 0; i < n; i++)
        TIRT_REQUIRE(local_pixel[i] >= 0 && local_pixel[i] < P, std::string(fn) + ": row " + std::to_string(i) + ": local pixel outside [0, P)");
    if (n == 0) return TIRT_OK;
    const TileMap tm = {c->tile_rank, c->tile_count, c->tile_size, c->H, c->tile_blocked, 0};
    return kat_round_trip(c, fn, {{local_pixel, kat_row_bytes(n, 1)}, {jx, kat_row_bytes(n, 1)}, {jy, kat_row_bytes(n, 1)}}, out, kat_row_bytes(n, out_stride),
                          [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_pvb_walk, dim3((n + 63) / 64), dim3(64), 0, c->stream, bvh_view(c), pvb_current_view(c), c->cam, tm, P, (const int *)din[0],
                           (const float *)din[1], (const float *)din[2], (float *)dout, out_stride, n);
    });
}

// host only, no context: pvb_beam_triangle_off (tirt_pvb.h) -- the text k_pvb_beam calls -- compiled for the host, on operands formed as k_pvb_beam forms them.
// Row of 31 floats: eye (3), cell (3), the pyramid's four corner directions in k_pvb_beam's order (12), eps (4), the triangle's corners (9).  The face normals
// are turned inward by the sum of the four directions (k_pvb_beam uses the pixel's centre direction: the same side for any pyramid that is not flat).
int tirt_kat_beam_triangle_host(const float *in, int n, int edges, int32_t *out)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_beam_triangle_host: null pointer or negative n");
    TIRT_REQUIRE(edges == 0 || edges == 1, "tirt_kat_beam_triangle_host: edges is 0 (the four faces) or 1 (and the triangle's edge planes)");
    for (int i = 0; i < n; i++) {
        const float *a = in + (size_t)i * 31;
        const v3 eye = V(a[0], a[1], a[2]), cell = V(a[3], a[4], a[5]);
        v3 dg[4], nrm[4], g[3];
        for (int q = 0; q < 4; q++) dg[q] = V(a[6 + 3 * q] / cell.x, a[7 + 3 * q] / cell.y, a[8 + 3 * q] / cell.z);
        const v3 dcg = (dg[0] + dg[1]) + (dg[2] + dg[3]);
        for (int q = 0; q < 4; q++) {
            v3 nn = cross(dg[q], dg[(q + 1) & 3]);
            if (dot(nn, dcg) < 0.0f) nn = -nn;
            nrm[q] = nn;
        }
        for (int j = 0; j < 3; j++) { const float *w = a + 22 + 3 * j; g[j] = V((w[0] - eye.x) / cell.x, (w[1] - eye.y) / cell.y, (w[2] - eye.z) / cell.z); }
        out[i] = pvb_beam_triangle_off(nrm, a + 18, dg, g[0], g[1], g[2], edges != 0) ? 1 : 0;
    }
    return TIRT_OK;
}

int tirt_kat_env_sample(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_env_sample: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 2 && out_stride >= 10, "tirt_kat_env_sample: stride too small (2 words in, 10 out)");
    CTX(c);
    return kat_env(c, 0, in, in_stride, out, out_stride, n);
}

int tirt_kat_env_pdf(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_env_pdf: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 3 && out_stride >= 5, "tirt_kat_env_pdf: stride too small (3 words in, 5 out)");
    CTX(c);
    return kat_env(c, 1, in, in_stride, out, out_stride, n);
}

int tirt_kat_env_lookup(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_env_lookup: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 2 && out_stride >= 3, "tirt_kat_env_lookup: stride too small (2 words in, 3 out)");
    CTX(c);
    return kat_env_lookup(c, in, in_stride, out, out_stride, n);
}

int tirt_kat_texture_alpha(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_texture_alpha: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 3 && out_stride >= 2, "tirt_kat_texture_alpha: stride too small (3 words in, 2 out)");
    CTX(c);
    TIRT_REQUIRE(c->tex_count > 0, "tirt_kat_texture_alpha: no textures uploaded (tirt_texture_upload)");
    for (int i = 0; i < n; i++) {
        const int32_t id = ((const int32_t *)in)[(size_t)i * in_stride];
        TIRT_REQUIRE(id >= 0 && id < c->tex_count, "tirt_kat_texture_alpha: row " + std::to_string(i) + ": texture number outside [0, count)");
    }
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_texture_alpha", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_texture_alpha, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->tex.as<int>(), (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

int tirt_kat_texture(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_texture: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 3 && out_stride >= 6, "tirt_kat_texture: stride too small (3 words in, 6 out)");
    CTX(c);
    TIRT_REQUIRE(c->tex_count > 0, "tirt_kat_texture: no textures uploaded (tirt_texture_upload)");
    for (int i = 0; i < n; i++) {
        const int32_t id = ((const int32_t *)in)[(size_t)i * in_stride];
        TIRT_REQUIRE(id >= 0 && id < c->tex_count, "tirt_kat_texture: row " + std::to_string(i) + ": texture number outside [0, count)");
    }
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_texture", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_texture, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->tex.as<int>(), (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

int tirt_kat_material_maps(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_material_maps: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 3 && out_stride >= 8, "tirt_kat_material_maps: stride too small (3 words in, 8 out)");
    CTX(c);
    TIRT_REQUIRE(c->n >= 1, "tirt_kat_material_maps: no scene");
    TIRT_REQUIRE(c->tex_count > 0, "tirt_kat_material_maps: no textures uploaded (tirt_texture_upload)");
    for (int i = 0; i < n; i++) {
        const int32_t prim = ((const int32_t *)in)[(size_t)i * in_stride];
        TIRT_REQUIRE(prim >= 0 && prim < c->n, "tirt_kat_material_maps: row " + std::to_string(i) + ": prim outside [0, n_prims)");
    }
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    return kat_round_trip(c, "tirt_kat_material_maps", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_material_maps, dim3((n + 255) / 256), dim3(256), 0, c->stream, scene_view(c), (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

int tirt_kat_math(tirt_ctx *c, int fn, const float *x, const float *y, float *out, int n)
{
    CTX(c);
    TIRT_REQUIRE(x && y && out && n >= 0, "tirt_kat_math: null");
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_math", {{x, kat_row_bytes(n, 1)}, {y, kat_row_bytes(n, 1)}}, out, kat_row_bytes(n, 1), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_math, dim3((n + 255) / 256), dim3(256), 0, c->stream, fn, (const float *)din[0], (const float *)din[1], (float *)dout, n);
    });
}

int tirt_kat_brdf(tirt_ctx *c, int which, const float *in, int in_stride, float *out, int out_stride, int n)
{
    CTX(c);
    TIRT_REQUIRE(in && out && n >= 0 && which >= 0 && which <= 18, "tirt_kat_brdf: bad args");
    const int need_in[19] = {19, 19, 17, 6, 2, 2, 2, 6, 3, 3, 3, 7, 2, 2, 2, 1, 8, 24, 12}, need_out[19] = {2, 3, 4, 3, 3, 2, 1, 3, 3, 3, 3, 4, 1, 1, 1, 1, 4, 3, 2};
    TIRT_REQUIRE(in_stride >= need_in[which] && out_stride >= need_out[which], "tirt_kat_brdf: stride too small");
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_brdf", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_brdf, dim3((n + 255) / 256), dim3(256), 0, c->stream, which, (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

int tirt_kat_shade_step(tirt_ctx *c, uint32_t feat, const float *in, int in_stride, float *out, int out_stride, int n)
{
    // what needs no context first (and no device: these refusals hold for a null context too)
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_shade_step: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 23 && out_stride >= 28, "tirt_kat_shade_step: stride too small (23 words in, 28 out)");
    TIRT_REQUIRE(kat_shade_step_has_inst(feat), "tirt_kat_shade_step: feat is not an instantiation of k_shade (the words tirt_shade_instantiation returns: include/tirt.h, tirt_kat_shade_step)");
    CTX(c);
    return kat_shade_step(c, feat, in, in_stride, out, out_stride, n);
}

int tirt_kat_shade_spec_step(tirt_ctx *c, uint32_t feat, const float *in, int in_stride, float *out, int out_stride, int n)
{
    // what needs no context first (and no device: these refusals hold for a null context too)
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_shade_spec_step: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 23 && out_stride >= 29, "tirt_kat_shade_spec_step: stride too small (23 words in, 29 out)");
    TIRT_REQUIRE(kat_shade_spec_step_has_inst(feat), "tirt_kat_shade_spec_step: feat is not an instantiation of k_shade_spec (32, 4 or 127: include/tirt.h, tirt_kat_shade_spec_step)");
    CTX(c);
    return kat_shade_spec_step(c, feat, in, in_stride, out, out_stride, n);
}

int tirt_kat_shade_tables(tirt_ctx *c, int which, const float *in, float *out, int n)
{
    CTX(c);
    TIRT_REQUIRE(out && n >= 0 && which >= 0 && which <= 2, "tirt_kat_shade_tables: bad args");
    TIRT_REQUIRE(c->n >= 1, "tirt_kat_shade_tables: no scene");
    TIRT_REQUIRE(which == 2 ? (in && c->light_count > 0) : n == (which == 0 ? c->n : c->light_count), "tirt_kat_shade_tables: n is the primitive / light count; which 2 needs input and a light");
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (ensure_shade_records(c)) return TIRT_ERR_HIP;
    // (only which 2 reads input rows)
    return kat_round_trip(c, "tirt_kat_shade_tables", {{in, which == 2 ? kat_row_bytes(n, 6) : 0}}, out, kat_row_bytes(n, which == 0 ? 4 : which == 1 ? 5 : 24), [&](const void *const *din, void *dout) {
        if (which == 2) hipLaunchKernelGGL(k_kat_light_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, scene_view(c), (const float *)din[0], (float *)dout, n);
        else hipLaunchKernelGGL(k_kat_shade_tables, dim3((n + 255) / 256), dim3(256), 0, c->stream, scene_view(c), which, (float *)dout, n);
    });
}

}  // extern "C"
