// tirt_device.h -- device-side restatement (HIP, gfx950) of the reference's @ti.func helpers:
// UtilsFunc.py (slabs, sampling, ONB, GTR/Smith/Schlick, refract, offset_ray, colour),
// Scene.py (intersect_tri/prim, areas, light sampling), brdf/Disney.py, brdf/Glass.py,
// texture/Texture.py.  fp32 operation order follows the reference expression by
// expression (this whole library is compiled with -ffp-contract=off); transcendental
// functions come from tirt_math.h so that results are bit-reproducible against the CPU
// oracle.  Each function cites the reference lines it follows.
#pragma once
#include <hip/hip_runtime.h>
#include "tirt_math.h"

#define TD __device__ __forceinline__

namespace tirt {

// ---- reference constants ---------------------------------------------------------------
constexpr int MAT_VEC = 10, VER_VEC = 9, PRI_VEC = 3, SHA_VEC = 10, NOD_VEC = 11, CPN_VEC = 9;  // SceneData.py:33-38
constexpr int SHAPE_SPHERE = 1, SHAPE_SPOT = 3, SHAPE_LASER = 4;                                 // SceneData.py:40-44
constexpr int PRIMITIVE_TRI = 1;                                                                // SceneData.py:47
constexpr int MAT_DISNEY = 0, MAT_GLASS = 1, MAT_LIGHT = 2;                                      // SceneData.py:50-52
constexpr float INF_VALUE = 1000000.0f;             // UtilsFunc.py:38
constexpr float PI_UF = (float)3.1415956;           // UtilsFunc.py:37 (sic, quirk B1)
constexpr float PI_SCENE = (float)3.1415926;        // Scene.py:319,343; integrator/PT_RGB.py:129-130

struct v3 { float x, y, z; };
__host__ TD v3 V(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
__host__ TD v3 operator+(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
__host__ TD v3 operator-(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ TD v3 operator*(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
__host__ TD v3 operator*(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
__host__ TD v3 operator/(v3 a, float s) { return V(a.x / s, a.y / s, a.z / s); }
__host__ TD v3 operator-(v3 a) { return V(-a.x, -a.y, -a.z); }
__host__ TD float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ TD v3 cross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
TD float norm(v3 a) { return tm_sqrt(dot(a, a)); }
// taichi Vector.normalized(): invlen = 1 / norm; invlen * self
TD v3 normalized(v3 a) { float inv = 1.0f / norm(a); return a * inv; }
__host__ TD float absf(float x) { return x < 0.0f ? -x : x; }
TD float minf(float a, float b) { return a < b ? a : b; }
TD float maxf(float a, float b) { return a > b ? a : b; }
TD float clampf(float x, float lo, float hi) { return minf(hi, maxf(lo, x)); }
TD float signf(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
TD float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
TD v3 mix3(v3 a, v3 b, float t) { return V(mixf(a.x, b.x, t), mixf(a.y, b.y, t), mixf(a.z, b.z, t)); }

// ---- votes and sums over a wave of 64 (k_trace, k_shade, k_shade_spec) ------------------------
TD unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
TD bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
TD unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- scene view passed to kernels by value ---------------------------------------------------
struct SceneView {
    const float *vertex;     // [nv*9]
    const int *primitive;    // [n*3]
    const float *material;   // [nm*10]
    const float *shape;      // [ns*10]
    const int *light;        // [nl]
    const int *env;          // [w*h]
    const float *mat_lrgb;   // [nm*3] srgb_to_lrgb(material colour), filled on device at upload
    const float4 *shade_rec; // [n*8] one 128-byte line per primitive: what k_shade needs to shade a hit on it (k_shade_records)
    const float4 *light_rec; // [light_count*8] one 128-byte line per entry of `light`: what sample_li needs of that emitter (k_light_records)
    const int *tex;          // albedo textures (tirt_texture_upload): T quads (offset, w, h, wrap), then the packed texels; offset counts ints from `tex`.  nullptr: none
    int n, light_count, env_w, env_h;
    float env_power;
};
struct CameraView { float view_inv[12]; float eye[3]; float fx, fy, cx, cy; };

// ---- scene feature word (tirt_api.hip, shade_features_core): what of the shading code a scene can reach at all, from the material rows, the
// kinds of the emitters on the light list and the environment.  k_shade / k_shade_spec are compiled per feature set (tirt_render.hip): a
// branch whose bit is clear in the instantiation's mask is not compiled, one whose bit is the only emitter kind left is taken without a test ----
enum : unsigned {
    SF_GLASS = 1u,            // a material row of type MAT_GLASS
    SF_ENV = 2u,              // env_power != 0 or a texel of the environment image that is not black
    SF_LIGHT_TRI = 4u,        // a triangle on the light list
    SF_LIGHT_SPOT_LASER = 8u, // a spot or a laser on the light list
    SF_NO_LIGHT = 16u,        // light_count == 0
    SF_LIGHT_SPHERE = 32u,    // a sphere on the light list
    SF_LIGHT_OTHER = 64u,     // an emitter of no kind sample_li knows (it samples the origin): generic kernel only
    SF_ALL = 127u,
    SF_TEXTURE = 128u,        // a material row that is not an emitter's names an uploaded albedo texture (not part of SF_ALL: untextured scenes keep their kernels)
    SF_CUTOUT = 512u,         // a triangle's material row that is not an emitter's names, in word 1, an uploaded texture flagged as a cut-out mask (tirt_texture_cutout): k_trace's
                              // CUTOUT twins.  Reported by tirt_shade_features; no instantiation of k_shade depends on it (pick_shade masks it out)
    SF_TEXTURE_PARAM = 256u,  // a material row that is not an emitter's names an uploaded roughness, metallic or normal texture (words 7..9; implies uvs in the shading records as 128 does)
    SF_ENV_SAMPLE = 1024u,    // environment importance sampling is switched on (tirt_env_sampling), the environment is lit and its sampling table exists: k_shade's ENV twins.
                              // Kept beside tirt_ctx::shade_features as 512 is (k_shade_spec and BDPT never see it); reported by tirt_shade_features
    SF_ENV_HDR = 2048u,       // the uploaded environment is RGBE8 (tirt_env_upload_hdr) and lit (bit 2): k_shade's HDR twins decode its texels.  Derived (env_hdr_active), never stored in
                              // the context's word, reported by tirt_shade_features; the 8-bit kernels are compiled without it and keep their code
    SF_LIGHT_POWER = 4096u,   // emitters are chosen by power (tirt_light_sampling mode 1), the list holds triangles and spheres only and its table has total > 0: k_shade's POWER twins.
                              // Derived (light_power_active), never stored in the context's word (k_shade_spec and BDPT never see it); reported by tirt_shade_features
    SF_LIGHT_KINDS = SF_LIGHT_TRI | SF_LIGHT_SPOT_LASER | SF_LIGHT_SPHERE | SF_LIGHT_OTHER
};

TD v3 vtx_pos(const SceneView &s, int i) { const float *p = s.vertex + (size_t)i * VER_VEC; return V(p[0], p[1], p[2]); }
TD v3 vtx_nor(const SceneView &s, int i) { const float *p = s.vertex + (size_t)i * VER_VEC; return V(p[3], p[4], p[5]); }
TD v3 vtx_uv(const SceneView &s, int i)  { const float *p = s.vertex + (size_t)i * VER_VEC; return V(p[6], p[7], p[8]); }

// ---- UtilsFunc.py:494-523 slabs, with 1/d hoisted out (same quotient, computed once per ray) ----
struct RayCtx { float ox, oy, oz, dx, dy, dz, idx, idy, idz; };
TD RayCtx make_ray(v3 o, v3 d)
{
    RayCtx r; r.ox = o.x; r.oy = o.y; r.oz = o.z; r.dx = d.x; r.dy = d.y; r.dz = d.z;
    r.idx = 1.0f / d.x; r.idy = 1.0f / d.y; r.idz = 1.0f / d.z;
    return r;
}
TD void slab_axis(float o, float d, float ood, float mn, float mx, float &tmin, float &tmax, int &ret)
{
    if (absf(d) < 0.000001f) {
        if ((o < mn) | (o > mx)) ret = 0;
    } else {
        float t1 = (mn - o) * ood;
        float t2 = (mx - o) * ood;
        if (t1 > t2) { float tmp = t1; t1 = t2; t2 = tmp; }
        if (t1 > tmin) tmin = t1;
        if (t2 < tmax) tmax = t2;
        if (tmin > tmax) ret = 0;
    }
}
// returns the reference's 0/1 and, through tnear, the entry distance it computed
TD int slabs(const RayCtx &r, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float &tnear)
{
    int ret = 1; float tmin = 0.0f, tmax = INF_VALUE;
    slab_axis(r.ox, r.dx, r.idx, mnx, mxx, tmin, tmax, ret);
    slab_axis(r.oy, r.dy, r.idy, mny, mxy, tmin, tmax, ret);
    slab_axis(r.oz, r.dz, r.idz, mnz, mxz, tmin, tmax, ret);
    tnear = tmin;
    return ret;
}
// Branch-free form for rays with |d| >= 1e-6 on every axis (all but axis-parallel rays).
// Same products and the same min/max selections as slab_axis, so tmin/tmax are the same
// floats; tmin only grows and tmax only shrinks across the axes, so the reference's
// per-axis `tmin > tmax` checks are equivalent to the single check at the end (no NaN can
// arise: 1/d is finite).
TD bool ray_has_parallel_axis(const RayCtx &r)
{ return (absf(r.dx) < 0.000001f) || (absf(r.dy) < 0.000001f) || (absf(r.dz) < 0.000001f); }
TD int slabs_fast(const RayCtx &r, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float &tnear)
{
    const float ax = (mnx - r.ox) * r.idx, bx = (mxx - r.ox) * r.idx;
    const float ay = (mny - r.oy) * r.idy, by = (mxy - r.oy) * r.idy;
    const float az = (mnz - r.oz) * r.idz, bz = (mxz - r.oz) * r.idz;
    const float tmin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)),
                                       __builtin_fmaxf(__builtin_fminf(az, bz), 0.0f));
    const float tmax = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)),
                                       __builtin_fminf(__builtin_fmaxf(az, bz), INF_VALUE));
    tnear = tmin;
    return (tmin > tmax) ? 0 : 1;
}

// ---- Scene.py:603-638 intersect_tri on a packed (v0, E1 = v1-v0, E2 = v2-v0) triangle ------------
TD float intersect_tri_packed(v3 origin, v3 direction, v3 v0, v3 E1, v3 E2, float &u, float &v)
{
    float t = INF_VALUE; u = 0.0f; v = 0.0f;
    v3 P = cross(direction, E2);
    float det = dot(E1, P);
    v3 T;
    if (det > 0.0f) T = origin - v0;
    else { T = v0 - origin; det = -det; }
    if (det > 0.0f) {
        u = dot(T, P);
        if ((u >= 0.0f) & (u <= det)) {
            v3 Q = cross(T, E1);
            v = dot(direction, Q);
            if ((v >= 0.0f) & (u + v <= det)) {
                t = dot(E2, Q);
                float fInvDet = 1.0f / det;
                t *= fInvDet; u *= fInvDet; v *= fInvDet;
            }
        }
    }
    return t;
}

// ---- Scene.py:565-596 / 653-665 sphere branch of intersect_prim(_any) ----------------------------
TD float intersect_sphere(v3 origin, v3 direction, v3 centre, float r, float &c_out)
{
    float hit_t = INF_VALUE;
    v3 oc = centre - origin;
    float dis_oc_square = dot(oc, oc);
    float dis_op = dot(direction, oc);
    float dis_cp = tm_sqrt(dis_oc_square - dis_op * dis_op);
    c_out = 0.0f;
    if (dis_cp < r) {
        float a = dot(direction, direction);
        float b = -2.0f * dis_op;
        float c = dis_oc_square - r * r;
        hit_t = (-b - tm_sqrt(b * b - 4.0f * a * c)) / 2.0f / a;
        c_out = c;
    }
    return hit_t;
}

// ---- hit attributes of the winning candidate (Scene.py:537-561, 565-596) -----------------------
struct HitAttr { v3 pos, gnor, nor, tex; float area; };      // area: get_prim_area of the primitive (hit_attributes_rec only)
TD HitAttr hit_attributes(const SceneView &s, v3 origin, v3 direction, int prim, float t, float u, float v)
{
    HitAttr h; h.pos = h.gnor = h.nor = h.tex = V(0.0f, 0.0f, 0.0f); h.area = 0.0f;
    const int *pr = s.primitive + (size_t)prim * PRI_VEC;
    v3 gn = V(0.0f, 0.0f, 0.0f), nn = gn;
    if (pr[0] == PRIMITIVE_TRI) {
        int vi = pr[1];
        float a = 1.0f - u - v, b = u, c = v;
        v3 v1 = vtx_pos(s, vi), v2 = vtx_pos(s, vi + 1), v3_ = vtx_pos(s, vi + 2);
        v3 n1 = vtx_nor(s, vi), n2 = vtx_nor(s, vi + 1), n3 = vtx_nor(s, vi + 2);
        v3 t1 = vtx_uv(s, vi), t2 = vtx_uv(s, vi + 1), t3 = vtx_uv(s, vi + 2);
        v3 v13 = v3_ - v1, v12 = v2 - v1;
        gn = cross(v12, v13);
        h.pos = (v1 * a + v2 * b) + v3_ * c;
        h.tex = (t1 * a + t2 * b) + t3 * c;
        nn = (n1 * a + n2 * b) + n3 * c;
    } else {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        if ((int)sh[0] == SHAPE_SPHERE) {
            float c;
            (void)intersect_sphere(origin, direction, V(sh[1], sh[2], sh[3]), sh[4], c);
            h.pos = origin + direction * t;
            nn = V(h.pos.x - c, h.pos.y - c, h.pos.z - c);          // quirk B3
            gn = nn;
        }
    }
    h.gnor = normalized(gn); h.nor = normalized(nn);
    return h;
}

// The same from the 128-byte shading record of the primitive (one cache line instead of a 12-byte primitive row plus three
// 36-byte vertex rows in three more lines; exact copies of the same floats, so the same results):
//   triangles: (v1.xyz, bits mat) (v2.xyz, bits PRIMITIVE_TRI) (v3.xyz, t3.u) (n1.xyz, t3.v) (n2.xyz, -) (n3.xyz, -) (gnor.xyz, area) (t1.u, t1.v, t2.u, t2.v)
//   shapes   : (centre.xyz, bits mat) (radius, shape type, area, bits 2)
// gnor = normalized(cross(v2 - v1, v3 - v1)) and area = get_prim_area depend on the primitive alone: k_shade_records evaluates them
// once, with the very expressions of hit_attributes / get_prim_area (a cross product, five correctly rounded square roots and three
// divisions less per shaded path).  A sphere's normal depends on the hit point and stays here; its gn IS its nn, so the one
// normalisation serves both.
// The uvs t1, t2, t3 of the three vertices (columns 6, 7 of their rows; column 8 is not carried) are in the record only while the scene is textured
// (SF_TEXTURE or SF_TEXTURE_PARAM); otherwise those words are zero, as they always were.  TEX -- the textured instantiation of k_shade alone -- reads them and returns
// tex = (t1 * a + t2 * b) + t3 * c as hit_attributes does, .z = 0; every other caller gets tex = 0 and loads nothing more than before.  Shapes have uv 0.
template <bool TEX = false>
TD HitAttr hit_attributes_rec(const float4 *rec, v3 origin, v3 direction, int prim, float t, float u, float v, int &mat_id)
{
    HitAttr h; h.pos = h.gnor = h.nor = h.tex = V(0.0f, 0.0f, 0.0f);
    const float4 *r = rec + (size_t)prim * 8;
    const float4 r0 = r[0], r1 = r[1];
    mat_id = __float_as_int(r0.w);
    h.area = r1.z;
    v3 nn = V(0.0f, 0.0f, 0.0f);
    const bool tri = __float_as_int(r1.w) == PRIMITIVE_TRI;
    if (tri) {
        const float4 r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6];
        float a = 1.0f - u - v, b = u, c = v;
        v3 v1 = V(r0.x, r0.y, r0.z), v2 = V(r1.x, r1.y, r1.z), v3_ = V(r2.x, r2.y, r2.z);
        v3 n1 = V(r3.x, r3.y, r3.z), n2 = V(r4.x, r4.y, r4.z), n3 = V(r5.x, r5.y, r5.z);
        h.gnor = V(r6.x, r6.y, r6.z); h.area = r6.w;
        h.pos = (v1 * a + v2 * b) + v3_ * c;
        nn = (n1 * a + n2 * b) + n3 * c;
        if constexpr (TEX) {
            const float4 r7 = r[7];
            h.tex = V((r7.x * a + r7.z * b) + r2.w * c, (r7.y * a + r7.w * b) + r3.w * c, 0.0f);
        }
    } else if ((int)r1.y == SHAPE_SPHERE) {
        float c;
        (void)intersect_sphere(origin, direction, V(r0.x, r0.y, r0.z), r1.x, c);
        h.pos = origin + direction * t;
        nn = V(h.pos.x - c, h.pos.y - c, h.pos.z - c);          // quirk B3
    }
    h.nor = normalized(nn);
    if (!tri) h.gnor = h.nor;                                   // gn = nn: the same expression on the same floats
    return h;
}

// ---- colour (UtilsFunc.py:76-94, 113-120) ----------------------------------------------------------
TD float srgb_to_lrgb1(float c) { return (c < 0.04045f) ? c / 12.92f : tm_pow((c + 0.055f) / 1.055f, 2.4f); }
TD v3 srgb_to_lrgb(v3 c) { return V(srgb_to_lrgb1(c.x), srgb_to_lrgb1(c.y), srgb_to_lrgb1(c.z)); }
TD float lrgb_to_srgb1(float c)
{
    const float e = (float)(1.0 / 2.4);
    float o = (c < 0.0031308f) ? c * 12.92f : 1.055f * tm_pow(c, e) - 0.055f;
    return clampf(o, 0.0f, 1.0f);
}
TD float tone_aces1(float x)
{
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    return clampf((x * (a * x + b)) / (x * (c * x + d) + e), 0.0f, 1.0f);
}

// ---- sampling helpers (UtilsFunc.py:352-387) ---------------------------------------------------------
TD v3 cosine_sample_hemisphere(float u1, float u2)
{
    const float two_pi = (float)(2.0 * 3.1415956);
    float r = tm_sqrt(u1);
    float phi = two_pi * u2;
    v3 p;
    float sn, cs; tm_sincos(phi, &sn, &cs);
    p.x = r * cs;
    p.y = r * sn;
    p.z = tm_sqrt(maxf(0.0f, 1.0f - p.x * p.x - p.y * p.y));
    return normalized(p);
}
TD v3 inverse_transform(v3 dir, v3 N)
{
    v3 Normal = normalized(N);
    v3 Binormal;
    if (absf(Normal.x) > absf(Normal.z)) Binormal = V(-Normal.y, Normal.x, 0.0f);
    else Binormal = V(0.0f, -Normal.z, Normal.y);
    Binormal = normalized(Binormal);
    v3 Tangent = normalized(cross(Binormal, Normal));
    return (Tangent * dir.x + Binormal * dir.y) + Normal * dir.z;
}

// ---- microfacet terms (UtilsFunc.py:393-438) -------------------------------------------------------------
TD float schlick_fresnel(float u) { float m = clampf(1.0f - u, 0.0f, 1.0f); float m2 = m * m; return m2 * m2 * m; }
TD float gtr2(float NDotH, float a) { float a2 = a * a; float t = 1.0f + (a2 - 1.0f) * NDotH * NDotH; return a2 / (PI_UF * t * t); }
TD float smithg_ggx(float NDotv, float alphaG) { float a = alphaG * alphaG, b = NDotv * NDotv; return 1.0f / (NDotv + tm_sqrt(a + b - a * b)); }
TD v3 refract_(v3 InRay, v3 N, float eta, float &suc)
{
    suc = -1.0f;
    float N_DOT_I = dot(N, InRay);
    float k = 1.0f - eta * eta * (1.0f - N_DOT_I * N_DOT_I);
    v3 R = V(0.0f, 0.0f, 0.0f);
    if (k > 0.0f) { R = InRay * eta - N * (eta * N_DOT_I + tm_sqrt(k)); suc = 1.0f; }
    return R;
}
TD float schlick(float cosine, float ior)
{
    float r0 = (1.0f - ior) / (1.0f + ior);
    r0 = r0 * r0;
    return r0 + (1.0f - r0) * tm_pow(1.0f - cosine, 5.0f);
}
TD v3 reflect_(v3 I, v3 N) { return I - N * (2.0f * dot(N, I)); }
TD float power_heuristic(float a, float b) { float t = a * a; return t / (b * b + t); }

// ---- UtilsFunc.py:440-461 ------------------------------------------------------------------------------
TD float offset_ray1(float p, float n)
{
    const float int_scale = 256.0f, float_scale = (float)(1.0 / 2048.0), origin = (float)(1.0 / 256.0);
    int i_of = (int)(int_scale * n);
    int i_p = (int)tm_f2u(p);
    if (p < 0.0f) i_p = i_p - i_of; else i_p = i_p + i_of;
    float f_p = tm_u2f((uint32_t)i_p);
    return (absf(p) < origin) ? p + float_scale * n : f_p;
}
TD v3 offset_ray(v3 p, v3 n) { return V(offset_ray1(p.x, n.x), offset_ray1(p.y, n.y), offset_ray1(p.z, n.z)); }

// ---- brdf/Disney.py:17-40, 65-108.  What evaluate_pdf and sample compute from the material row alone, and what evaluate_pdf computes from
// (N, V) alone, in one place: a path evaluates the BSDF twice at one hit (NEE sample, continuation) with the same N and V, and samples
// it once.  Every value is the expression of the reference on the same operands; only how often it is evaluated differs. ----
struct DisneySetup {
    float metal1, rough, Cspec0, specularAlpha, a2, roughg, diffuseRatio, specularRatio;      // material only (metal1 = 1 - metal)
    float NDotV, FV, GV;                                                                       // view: dot(N, V), schlick_fresnel, smithg_ggx
};
TD float gtr2_a2(float NDotH, float a2) { float t = 1.0f + (a2 - 1.0f) * NDotH * NDotH; return a2 / (PI_UF * t * t); }      // gtr2 with a * a given
TD void disney_setup_material(const float *m, DisneySetup &d)
{
    const float metal = m[5], rough = m[6];
    d.rough = rough;
    d.metal1 = 1.0f - metal;
    d.Cspec0 = mixf(0.04f, 1.0f, metal);
    d.specularAlpha = maxf(0.001f, rough);
    d.a2 = d.specularAlpha * d.specularAlpha;
    const float rg = rough * 0.5f + 0.5f; d.roughg = rg * rg;
    d.diffuseRatio = 0.5f * d.metal1;
    d.specularRatio = 1.0f - d.diffuseRatio;
}
TD DisneySetup disney_setup(const float *m, v3 N, v3 Vv)
{
    DisneySetup d;
    disney_setup_material(m, d);
    d.NDotV = dot(N, Vv);
    d.FV = schlick_fresnel(d.NDotV);
    d.GV = smithg_ggx(d.NDotV, d.roughg);
    return d;
}
TD v3 disney_sample_set(const DisneySetup &ds, v3 dir, v3 N, float probability, float r1, float r2)
{
    // Both lobes of the reference (diffuse: cosine_sample_hemisphere + inverse_transform, specular: GTR2
    // half vector + inverse_transform + reflect) take one sin/cos pair of a lobe-specific angle and one change
    // of basis around N.  Written so that a wave with lanes in both lobes evaluates the expensive shared
    // pieces (sincos, the three normalisations of the basis) once; every lane still performs exactly the
    // reference's operations for its lobe.
    const bool diffuse = probability < ds.diffuseRatio;
    const float two_pi = (float)(2.0 * 3.1415956);
    const float phi = diffuse ? two_pi * r2 : r1 * 2.0f * PI_UF;       // UtilsFunc.py:352-361 / Disney.py:28
    float sinPhi, cosPhi; tm_sincos(phi, &sinPhi, &cosPhi);
    v3 local;
    if (diffuse) {
        float r = tm_sqrt(r1);
        v3 p;
        p.x = r * cosPhi;
        p.y = r * sinPhi;
        p.z = tm_sqrt(maxf(0.0f, 1.0f - p.x * p.x - p.y * p.y));
        local = normalized(p);
    } else {
        float cosTheta = tm_sqrt((1.0f - r2) / (1.0f + (ds.a2 - 1.0f) * r2));
        float sinTheta = tm_sqrt(1.0f - (cosTheta * cosTheta));
        local = V(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta);
    }
    const v3 world = inverse_transform(local, N);
    return diffuse ? world : reflect_(dir, world);
}
// the reference's signature (BDPT, PT_Spec, the known-answer tests, the instantiations of k_shade that do not share a set-up): the same function
// with its own material terms.  (Not a wrapper around disney_sample_set: through one the generic k_shade needs 8 bytes of scratch.)
TD v3 disney_sample(const float *m, v3 dir, v3 N, float probability, float r1, float r2)
{
    float metal = m[5], rough = m[6];
    float diffuseRatio = 0.5f * (1.0f - metal);
    float specularAlpha = maxf(0.001f, rough);
    const bool diffuse = probability < diffuseRatio;
    const float two_pi = (float)(2.0 * 3.1415956);
    const float phi = diffuse ? two_pi * r2 : r1 * 2.0f * PI_UF;       // UtilsFunc.py:352-361 / Disney.py:28
    float sinPhi, cosPhi; tm_sincos(phi, &sinPhi, &cosPhi);
    v3 local;
    if (diffuse) {
        float r = tm_sqrt(r1);
        v3 p;
        p.x = r * cosPhi;
        p.y = r * sinPhi;
        p.z = tm_sqrt(maxf(0.0f, 1.0f - p.x * p.x - p.y * p.y));
        local = normalized(p);
    } else {
        float cosTheta = tm_sqrt((1.0f - r2) / (1.0f + (specularAlpha * specularAlpha - 1.0f) * r2));
        float sinTheta = tm_sqrt(1.0f - (cosTheta * cosTheta));
        local = V(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta);
    }
    const v3 world = inverse_transform(local, N);
    return diffuse ? world : reflect_(dir, world);
}
// ---- brdf/Disney.py:65-108: the part that depends on L ------------------------------------------------------
TD float disney_evaluate_pdf_set(const DisneySetup &ds, v3 N, v3 Vv, v3 L, float &pdf)
{
    float outputC = 0.0f; pdf = -1.0f;
    float NDotL = dot(N, L);
    if ((NDotL > 0.0f) & (ds.NDotV > 0.0f)) {
        const float inv_pi = (float)(1.0 / 3.1415956);
        v3 H = normalized(L + Vv);
        float NDotH = dot(H, N), LDotH = dot(H, L);
        float Csheen = 0.5f;
        float FL = schlick_fresnel(NDotL);
        float Fd90 = 0.5f + 2.0f * LDotH * LDotH * ds.rough;
        float Fd = mixf(1.0f, Fd90, FL) * mixf(1.0f, Fd90, ds.FV);
        float Ds = gtr2_a2(NDotH, ds.a2);
        float FH = schlick_fresnel(LDotH);
        float Fs = mixf(ds.Cspec0, 1.0f, FH);
        float Gs = smithg_ggx(NDotL, ds.roughg) * ds.GV;
        float Fsheen = FH * Csheen;
        outputC = (Fsheen + inv_pi) * Fd * ds.metal1 + Gs * Fs * Ds;
        float pdfGTR2 = Ds * NDotH;
        float pdfSpec = pdfGTR2 / (4.0f * absf(LDotH));
        float pdfDiff = inv_pi;                               // quirk B4
        pdf = ds.diffuseRatio * pdfDiff + ds.specularRatio * pdfSpec;
    }
    return outputC;
}
// the reference's signature: set-up and evaluation in one function, every term inside the early-out (see disney_sample)
TD float disney_evaluate_pdf(const float *m, v3 N, v3 Vv, v3 L, float &pdf)
{
    float outputC = 0.0f; pdf = -1.0f;
    float NDotL = dot(N, L), NDotV = dot(N, Vv);
    if ((NDotL > 0.0f) & (NDotV > 0.0f)) {
        const float inv_pi = (float)(1.0 / 3.1415956);
        v3 H = normalized(L + Vv);
        float NDotH = dot(H, N), LDotH = dot(H, L);
        float metal = m[5], rough = m[6];
        float Cspec0 = mixf(0.04f, 1.0f, metal);
        float Csheen = 0.5f;
        float FL = schlick_fresnel(NDotL), FV = schlick_fresnel(NDotV);
        float Fd90 = 0.5f + 2.0f * LDotH * LDotH * rough;
        float Fd = mixf(1.0f, Fd90, FL) * mixf(1.0f, Fd90, FV);
        float specularAlpha = maxf(0.001f, rough);
        float Ds = gtr2(NDotH, specularAlpha);
        float FH = schlick_fresnel(LDotH);
        float Fs = mixf(Cspec0, 1.0f, FH);
        float rg = rough * 0.5f + 0.5f; float roughg = rg * rg;
        float Gs = smithg_ggx(NDotL, roughg) * smithg_ggx(NDotV, roughg);
        float Fsheen = FH * Csheen;
        outputC = (Fsheen + inv_pi) * Fd * (1.0f - metal) + Gs * Fs * Ds;
        float diffuseRatio = 0.5f * (1.0f - metal);
        float specularRatio = 1.0f - diffuseRatio;
        float pdfGTR2 = Ds * NDotH;
        float pdfSpec = pdfGTR2 / (4.0f * absf(LDotH));
        float pdfDiff = inv_pi;                               // quirk B4
        pdf = diffuseRatio * pdfDiff + specularRatio * pdfSpec;
    }
    return outputC;
}
// ---- brdf/Glass.py:9-34 ----------------------------------------------------------------------------------
TD v3 glass_sample(const float *m, v3 dir, v3 N, float probability, float &f_or_b)
{
    v3 w_out = dir;
    float cos_theta_i = dot(w_out, N);
    float ior = m[5];
    float eta = ior;
    f_or_b = 1.0f;
    float R = probability + 1.0f;
    if (cos_theta_i > 0.0f) N = -N;
    else { cos_theta_i = -cos_theta_i; eta = 1.0f / ior; }
    float suc;
    v3 next_dir = refract_(w_out, N, eta, suc);
    if (suc > 0.0f) R = schlick(cos_theta_i, ior);
    if (probability < R) next_dir = reflect_(w_out, N);
    else f_or_b = -1.0f;
    return next_dir;
}

// ---- Scene.py:324-350 ------------------------------------------------------------------------------------
TD float get_prim_area(const SceneView &s, int index)
{
    float ret = 0.0f;
    const int *pr = s.primitive + (size_t)index * PRI_VEC;
    if (pr[0] == PRIMITIVE_TRI) {
        v3 v1 = vtx_pos(s, pr[1]), v2 = vtx_pos(s, pr[1] + 1), v3_ = vtx_pos(s, pr[1] + 2);
        float a = norm(v1 - v2), b = norm(v1 - v3_), c = norm(v3_ - v2);
        float sum = (a + b + c) * 0.5f;
        ret = tm_sqrt(sum * (sum - a) * (sum - b) * (sum - c));
    } else {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        int st = (int)sh[0];
        if (st == SHAPE_SPHERE || st == SHAPE_SPOT || st == SHAPE_LASER) { float r = sh[4]; ret = r * r * PI_SCENE; }   // quirk B2
    }
    return ret;
}
// ---- Scene.py:315-322 ------------------------------------------------------------------------------------
TD v3 uniform_sample_sphere(float u1, float u2)
{
    const float two_pi = (float)(2.0 * 3.1415926);
    float z = 1.0f - 2.0f * u1;
    float r = tm_sqrt(clampf(1.0f - z * z, 0.0f, 1.0f));
    float phi = two_pi * u2;
    float sn, cs; tm_sincos(phi, &sn, &cs);
    return V(r * cs, r * sn, z);
}
// ---- Scene.py:381-420 ------------------------------------------------------------------------------------
TD void get_prim_random_point_normal(const SceneView &s, int index, float a, float b, v3 &pos, v3 &nor)
{
    pos = V(0.0f, 0.0f, 0.0f); v3 normal = pos;
    const int *pr = s.primitive + (size_t)index * PRI_VEC;
    if (pr[0] == PRIMITIVE_TRI) {
        v3 v1 = vtx_pos(s, pr[1]), v2 = vtx_pos(s, pr[1] + 1), v3_ = vtx_pos(s, pr[1] + 2);
        v3 n1 = vtx_nor(s, pr[1]), n2 = vtx_nor(s, pr[1] + 1), n3 = vtx_nor(s, pr[1] + 2);
        if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        pos = (v1 + (v3_ - v1) * a) + (v2 - v1) * b;
        normal = normalized((n1 * (1.0f - a - b) + n2 * a) + n3 * b);
    } else {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        if ((int)sh[0] == SHAPE_SPHERE) {
            float r = sh[4];
            normal = uniform_sample_sphere(a, b);
            pos = V(sh[1], sh[2], sh[3]) + normal * r;
        } else if ((int)sh[0] == SHAPE_SPOT || (int)sh[0] == SHAPE_LASER) {      // Scene.py:413-418: the shape's own point and normal
            normal = V(sh[7], sh[8], sh[9]);
            pos = V(sh[1], sh[2], sh[3]);
        }
    }
    nor = normalized(normal);
}
// ---- Scene.py:491-516: what sample_li adds for the two shape emitters that have no surface -- the factor `visable` on the
// emission (spot: 1 inside the cone of half-angle x1, falling linearly to 0 at x2, measured between the light's normal and the
// direction to the shaded point; laser: 1 within `radius` of the beam's axis, else 0) and, for the laser, light_choice_pdf =
// 1 / light_count ----
TD float light_shape_visible(const SceneView &s, int light_prim, v3 light_dir, v3 light_normal, float light_dist, float &choice_pdf)
{
    float visable = 1.0f;
    const int *pr = s.primitive + (size_t)light_prim * PRI_VEC;
    if (pr[0] != PRIMITIVE_TRI) {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        const int st = (int)sh[0];
        if (st == SHAPE_SPOT) {
            const float NdotL = absf(dot(light_dir, light_normal));
            const float x1 = sh[4], x2 = sh[5];
            const float x = tm_acos(NdotL);
            if (x > x2) visable = 0.0f;
            else if (x > x1) visable *= 1.0f - (x - x1) / (x2 - x1);
        } else if (st == SHAPE_LASER) {
            choice_pdf = 1.0f / (float)s.light_count;
            const float proj = dot(light_dir, light_normal) * light_dist;
            const float r = tm_sqrt(light_dist * light_dist - proj * proj);
            if (r > sh[4]) visable = 0.0f;
        }
    }
    return visable;
}
// ---- the per-light record (k_light_records): what Scene.sample_li (Scene.py:477-518) reads of emitter light[lidx] that does not depend on
// the path, one 128-byte line per entry of `light` instead of a primitive row, three vertex rows (or a shape row) and a material row --
//   triangles: (v1.xyz, area) (v3 - v1, choice_pdf) (v2 - v1, bits -1) (n1.xyz, emission.r) (n2.xyz, emission.g) (n3.xyz, emission.b) - -
//   shapes   : (centre.xyz, area) (sh[4], sh[5], -, choice_pdf) (-, -, -, bits shape type) (sh[7..9], emission.r) (-, -, -, .g) (-, -, -, .b)
// area = get_prim_area (Heron: four correctly rounded square roots), choice_pdf = 1 / (light_count * area), or 1 / light_count for a laser
// (light_shape_visible overwrites it, Scene.py:509), the two edges of get_prim_random_point_normal's point and the emitter's material
// colour: each evaluated once by the expression of the function it replaces.  What depends on the sample (a, b) stays per path, in
// get_prim_random_point_normal's order, and so do the three normalisations of the light's normal. ----
constexpr int LIGHT_REC_QUADS = 8;
struct LightRec { v3 emission; float area, choice_pdf, p0, p1; int kind; };      // kind: -1 triangle, else the shape type; p0, p1 = sh[4], sh[5]
// FEAT (a scene feature word): emitter kinds the mask rules out are not compiled, and where it leaves one kind no test is made for it
template <unsigned FEAT = SF_ALL>
TD LightRec light_sample_rec(const float4 *lrec, int lidx, float a, float b, v3 &pos, v3 &nor)
{
    constexpr unsigned LK = FEAT & SF_LIGHT_KINDS;
    const float4 *r = lrec + (size_t)lidx * LIGHT_REC_QUADS;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
    LightRec L; L.emission = V(r3.w, r4.w, r5.w); L.area = r0.w; L.choice_pdf = r1.w; L.p0 = r1.x; L.p1 = r1.y; L.kind = __float_as_int(r2.w);
    pos = V(0.0f, 0.0f, 0.0f); v3 normal = pos;
    if ((LK & SF_LIGHT_TRI) && (LK == SF_LIGHT_TRI || L.kind == -1)) {
        const v3 v1 = V(r0.x, r0.y, r0.z), e31 = V(r1.x, r1.y, r1.z), e21 = V(r2.x, r2.y, r2.z);
        const v3 n1 = V(r3.x, r3.y, r3.z), n2 = V(r4.x, r4.y, r4.z), n3 = V(r5.x, r5.y, r5.z);
        if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        pos = (v1 + e31 * a) + e21 * b;
        normal = normalized((n1 * (1.0f - a - b) + n2 * a) + n3 * b);
    } else if ((LK & SF_LIGHT_SPHERE) && (LK == SF_LIGHT_SPHERE || L.kind == SHAPE_SPHERE)) {
        normal = uniform_sample_sphere(a, b);
        pos = V(r0.x, r0.y, r0.z) + normal * L.p0;
    } else if ((LK & SF_LIGHT_SPOT_LASER) && (L.kind == SHAPE_SPOT || L.kind == SHAPE_LASER)) {
        normal = V(r3.x, r3.y, r3.z);
        pos = V(r0.x, r0.y, r0.z);
    }
    nor = normalized(normal);
    return L;
}
// light_shape_visible on the record (the laser's choice pdf is already in it)
template <unsigned FEAT = SF_ALL>
TD float light_shape_visible_rec(const LightRec &L, v3 light_dir, v3 light_normal, float light_dist)
{
    float visable = 1.0f;
    if (!(FEAT & SF_LIGHT_SPOT_LASER)) return visable;
    if (L.kind == SHAPE_SPOT) {
        const float NdotL = absf(dot(light_dir, light_normal));
        const float x1 = L.p0, x2 = L.p1;
        const float x = tm_acos(NdotL);
        if (x > x2) visable = 0.0f;
        else if (x > x1) visable *= 1.0f - (x - x1) / (x2 - x1);
    } else if (L.kind == SHAPE_LASER) {
        const float proj = dot(light_dir, light_normal) * light_dist;
        const float r = tm_sqrt(light_dist * light_dist - proj * proj);
        if (r > L.p0) visable = 0.0f;
    }
    return visable;
}
// ---- UtilsFunc.py:321-345 ----
TD void map_to_disk(float u1, float u2, float &r, float &phi)
{
    phi = 0.0f; r = 0.0f;
    const float a = 2.0f * u1 - 1.0f, b = 2.0f * u2 - 1.0f;
    if (a > -b) {
        if (a > b) { r = a; phi = (PI_UF / 4.0f) * (b / a); }
        else { r = b; phi = (PI_UF / 4.0f) * (2.0f - a / b); }
    } else {
        if (a < b) { r = -a; phi = (PI_UF / 4.0f) * (4.0f + b / a); }
        else { r = -b; phi = (b == 0.0f) ? 0.0f : (PI_UF / 4.0f) * (6.0f - a / b); }
    }
}
// ---- Scene.py:353-377 ------------------------------------------------------------------------------------
TD float get_prim_angle(const SceneView &s, int index, v3 v)
{
    float ret = 0.0f;
    const int *pr = s.primitive + (size_t)index * PRI_VEC;
    if (pr[0] == PRIMITIVE_TRI) {
        v3 v1 = vtx_pos(s, pr[1]), v2 = vtx_pos(s, pr[1] + 1), v3_ = vtx_pos(s, pr[1] + 2);
        if (norm(v1 - v) < 0.00001f) ret = dot(normalized(v2 - v1), normalized(v3_ - v1));
        else if (norm(v2 - v) < 0.00001f) ret = dot(normalized(v1 - v2), normalized(v3_ - v2));
        else ret = dot(normalized(v1 - v3_), normalized(v2 - v3_));
    }
    return tm_acos(ret);
}

// ---- texture/Texture.py:41-69: `sample` and `texture2D` on an image of w x h packed texels (the environment's, or one albedo texture's) ----
TD v3 tex_sample(const int *img, int w, int h, float fx, float fy)
{
    int x = (int)fx, y = (int)fy;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    int RGBA = img[(size_t)x * h + y];
    float R = (float)((RGBA & 0x00FF0000) >> 16) / 255.0f;
    float G = (float)((RGBA & 0x0000FF00) >> 8) / 255.0f;
    float B = (float)(RGBA & 0x000000FF) / 255.0f;
    return V(R, G, B);
}
TD v3 texture2d(const int *img, int w, int h, float u, float v)
{
    float x = clampf(u * (float)w, 0.0f, (float)w - 1.0f);
    float y = clampf(v * (float)h, 0.0f, (float)h - 1.0f);
    float lx = tm_floor(x), ly = tm_floor(y);
    float wbt = y - tm_floor(y), wlr = x - tm_floor(x);
    v3 lt = tex_sample(img, w, h, lx, ly), rt = tex_sample(img, w, h, lx + 1.0f, ly);
    v3 lb = tex_sample(img, w, h, lx, ly + 1.0f), rb = tex_sample(img, w, h, lx + 1.0f, ly + 1.0f);
    return mix3(mix3(lt, rt, wlr), mix3(lb, rb, wlr), wbt);
}

// ---- HDR environment (include/tirt.h, "HDR environment"; no reference counterpart): RGBE8 texels (E << 24) | (R << 16) | (G << 8) | B at the index of an 8-bit image.
// A channel is mantissa * 2^(E - 136), linear radiance: one exact conversion and one exact scaling (v_ldexp_f32; f32 denormals are kept -- the library is
// compiled with -fno-fast-math and without -fgpu-flush-denormals-to-zero, the kernels' float_denorm_mode_32 is 3).  The upload has refused E == 0 with a mantissa,
// so an all-zero word is the only texel with E == 0 and decodes to 0 by the same expression: no special case.  Host and device (env_texel_lum_hdr runs on both).
TM_HD void hdr_decode(int texel, float c[3])
{
    const unsigned t = (unsigned)texel;
    const int e = (int)(t >> 24) - 136;
    c[0] = __builtin_ldexpf((float)((t >> 16) & 255u), e); c[1] = __builtin_ldexpf((float)((t >> 8) & 255u), e); c[2] = __builtin_ldexpf((float)(t & 255u), e);
}
TD v3 tex_sample_hdr(const int *img, int w, int h, float fx, float fy)
{
    int x = (int)fx, y = (int)fy;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    float c[3]; hdr_decode(img[(size_t)x * h + y], c);
    return V(c[0], c[1], c[2]);
}
// texture2d on decoded texels: the same clamp, lx / ly / wlr / wbt, four taps and mix order
TD v3 texture2d_hdr(const int *img, int w, int h, float u, float v)
{
    float x = clampf(u * (float)w, 0.0f, (float)w - 1.0f);
    float y = clampf(v * (float)h, 0.0f, (float)h - 1.0f);
    float lx = tm_floor(x), ly = tm_floor(y);
    float wbt = y - tm_floor(y), wlr = x - tm_floor(x);
    v3 lt = tex_sample_hdr(img, w, h, lx, ly), rt = tex_sample_hdr(img, w, h, lx + 1.0f, ly);
    v3 lb = tex_sample_hdr(img, w, h, lx, ly + 1.0f), rb = tex_sample_hdr(img, w, h, lx + 1.0f, ly + 1.0f);
    return mix3(mix3(lt, rt, wlr), mix3(lb, rb, wlr), wbt);
}
// the linear colour of the environment at lookup coordinates (tx, ty), before env_power: what shade_path's miss branch and its environment sample read
template <bool HDR>
TD v3 env_lookup(const int *img, int w, int h, float tx, float ty)
{
    if constexpr (HDR) return texture2d_hdr(img, w, h, tx, ty);
    else return srgb_to_lrgb(texture2d(img, w, h, tx, ty));
}

// ---- albedo textures (include/tirt.h, tirt_texture_upload; no reference counterpart: PT_RGB.py:86 takes the material colour) ----
// The texture a material row names: (int)row[1] - 1 where 1 <= (int)row[1], else -1.  The host has refused every row of a material that is not an emitter
// whose slot exceeds the number of uploaded textures, so a slot >= 1 found on the device names a table entry (no count is passed to any kernel).
// Only meaningful while textures are uploaded (SceneView::tex != nullptr, or the SF_TEXTURE instantiation).
// (the test before the subtraction: a slot below -2^31 converts to INT_MIN, and INT_MIN - 1 would come out as a texture number)
TD int material_texture(const float *m) { const int slot = (int)m[1]; return ((int)m[0] == MAT_LIGHT || slot < 1) ? -1 : slot - 1; }
// tex_albedo of include/tirt.h: a u or v that is not finite counts as 0; repeat takes the fractional part; then the environment's bilinear lookup.
// An encoded (sRGB-valued) colour, in the space of a material row's colour.
TD v3 tex_albedo(const int *tex, int id, float u, float v)
{
    const int4 e = ((const int4 *)tex)[id];                    // offset, w, h, wrap
    const float big = 3.4028234e38f;
    if (!(absf(u) <= big)) u = 0.0f;
    if (!(absf(v) <= big)) v = 0.0f;
    if (e.w == 1) { u = u - tm_floor(u); v = v - tm_floor(v); }
    return texture2d(tex + e.x, e.y, e.z, u, v);
}

// tex_alpha of include/tirt.h: the fourth channel of the same lookup -- the same non-finite rule, wrap, clamp, lx / ly / wlr / wbt, the four texels lt / rt / lb / rb
// and mix order as tex_albedo / texture2d; a texel's alpha is (255 - top byte) / 255 (the top byte holds the transparency: 0 in every texture packed without one)
TD float tex_sample_alpha(const int *img, int w, int h, float fx, float fy)
{
    int x = (int)fx, y = (int)fy;
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    const int RGBA = img[(size_t)x * h + y];
    return (float)(255 - ((RGBA >> 24) & 255)) / 255.0f;
}
TD float tex_alpha(const int *tex, int id, float u, float v)
{
    const int4 e = ((const int4 *)tex)[id];                    // offset, w, h, wrap
    const float big = 3.4028234e38f;
    if (!(absf(u) <= big)) u = 0.0f;
    if (!(absf(v) <= big)) v = 0.0f;
    if (e.w == 1) { u = u - tm_floor(u); v = v - tm_floor(v); }
    const int *img = tex + e.x; const int w = e.y, h = e.z;
    const float x = clampf(u * (float)w, 0.0f, (float)w - 1.0f);
    const float y = clampf(v * (float)h, 0.0f, (float)h - 1.0f);
    const float lx = tm_floor(x), ly = tm_floor(y);
    const float wbt = y - tm_floor(y), wlr = x - tm_floor(x);
    const float lt = tex_sample_alpha(img, w, h, lx, ly), rt = tex_sample_alpha(img, w, h, lx + 1.0f, ly);
    const float lb = tex_sample_alpha(img, w, h, lx, ly + 1.0f), rb = tex_sample_alpha(img, w, h, lx + 1.0f, ly + 1.0f);
    return mixf(mixf(lt, rt, wlr), mixf(lb, rb, wlr), wbt);
}

// ---- roughness, metallic and normal-map textures (include/tirt.h, "Roughness, metallic and normal-map textures"; no reference counterpart) ----
// The texture word `word` (7 roughness, 8 metallic, 9 normal map) of a material row names: (int)row[word] - 1 where 1 <= (int)row[word], else -1, by
// material_texture's rule.  An emitter's row names none; a glass row none in words 7 and 8 (its words 5 and 6 are ior and extinction).
TD int material_map(const float *m, int word)
{
    const int type = (int)m[0], slot = (int)m[word];
    return (type == MAT_LIGHT || (type == MAT_GLASS && word != 9) || slot < 1) ? -1 : slot - 1;
}
// roughness = .y of the roughness texture, metallic = .z of the metallic texture (glTF's channels; linear values, no sRGB decode): what takes the place of
// m[6] / m[5] of a Disney row.  The lookup is tex_albedo itself.
TD float tex_roughness(const int *tex, int id, float u, float v) { return tex_albedo(tex, id, u, v).y; }
TD float tex_metallic(const int *tex, int id, float u, float v) { return tex_albedo(tex, id, u, v).z; }
// The mapped shading normal N' of a hit at (u, v) on a triangle with vertex positions p0..p2 and vertex uvs (t0x, t0y) .. (t2x, t2y), N the interpolated,
// normalised shading normal.  Every operation in the order written, f32, one rounding each:
//   c = tex_albedo(tex, id, u, v);  n = c * 2 - 1 per channel
//   e1 = p1 - p0, e2 = p2 - p0;  d1 = t1 - t0, d2 = t2 - t0;  det = d1.x * d2.y - d2.x * d1.y
//   det == 0 or not finite (|det| <= 3.4028234e38 fails): N
//   T = (e1 * d2.y - e2 * d1.y) / det;  T = T - N * dot(N, T);  T = normalized(T);  a component of T not finite: N
//   B = cross(N, T);  Nraw = (T * n.x + B * n.y) + N * n.z;  N' = normalized(Nraw)
// k_shade, k_aov, the Debug normal views and tirt_kat_material_maps all come through here.
TD v3 tex_normal_raw(const int *tex, int id, float u, float v, v3 N, v3 p0, v3 p1, v3 p2, float t0x, float t0y, float t1x, float t1y, float t2x, float t2y, bool &mapped)
{
    mapped = false;
    const float big = 3.4028234e38f;
    const float d1x = t1x - t0x, d1y = t1y - t0y, d2x = t2x - t0x, d2y = t2y - t0y;
    const float det = d1x * d2y - d2x * d1y;
    if (det == 0.0f || !(absf(det) <= big)) return N;
    const v3 e1 = p1 - p0, e2 = p2 - p0;
    v3 T = (e1 * d2y - e2 * d1y) / det;
    T = T - N * dot(N, T);
    T = normalized(T);
    if (!(absf(T.x) <= big) || !(absf(T.y) <= big) || !(absf(T.z) <= big)) return N;
    const v3 c = tex_albedo(tex, id, u, v);
    const v3 n = V(c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f);
    const v3 B = cross(N, T);
    mapped = true;
    return (T * n.x + B * n.y) + N * n.z;
}
TD v3 tex_normal(const int *tex, int id, float u, float v, v3 N, v3 p0, v3 p1, v3 p2, float t0x, float t0y, float t1x, float t1y, float t2x, float t2y)
{
    bool mapped;
    const v3 raw = tex_normal_raw(tex, id, u, v, N, p0, p1, p2, t0x, t0y, t1x, t1y, t2x, t2y, mapped);
    return mapped ? normalized(raw) : N;
}
// the same for a hit on primitive `prim` from the vertex rows (k_aov, Debug, tirt_kat_material_maps) and from the shading record (k_shade): exact copies
// of the same floats.  uv is the hit's interpolated uv (HitAttr::tex).  An analytic shape keeps its normal.
TD v3 tex_normal_rows(const SceneView &s, int id, int prim, v3 uv, v3 N)
{
    const int *pr = s.primitive + (size_t)prim * PRI_VEC;
    if (pr[0] != PRIMITIVE_TRI) return N;
    const int vi = pr[1];
    const v3 t0 = vtx_uv(s, vi), t1 = vtx_uv(s, vi + 1), t2 = vtx_uv(s, vi + 2);
    return tex_normal(s.tex, id, uv.x, uv.y, N, vtx_pos(s, vi), vtx_pos(s, vi + 1), vtx_pos(s, vi + 2), t0.x, t0.y, t1.x, t1.y, t2.x, t2.y);
}
TD v3 tex_normal_rec(const int *tex, const float4 *rec, int id, int prim, v3 uv, v3 N)
{
    const float4 *r = rec + (size_t)prim * 8;
    const float4 r1 = r[1];
    if (__float_as_int(r1.w) != PRIMITIVE_TRI) return N;
    const float4 r0 = r[0], r2 = r[2], r7 = r[7]; const float t2y = r[3].w;
    return tex_normal(tex, id, uv.x, uv.y, N, V(r0.x, r0.y, r0.z), V(r1.x, r1.y, r1.z), V(r2.x, r2.y, r2.z), r7.x, r7.y, r7.z, r7.w, r2.w, t2y);
}
// what k_aov and the Debug normal views show: the mapped normal where the hit's material names a normal map (textures uploaded: s.tex != nullptr), else N
TD v3 shading_normal_rows(const SceneView &s, const float *m, int prim, v3 uv, v3 N)
{
    const int ni = material_map(m, 9);
    return ni >= 0 ? tex_normal_rows(s, ni, prim, uv, N) : N;
}

// ---- environment importance sampling (include/tirt.h, "Importance sampling of the environment"; tirt_envsample.hip builds the table; no reference counterpart) ----
// The table lives BEHIND the environment's texels in the same allocation, 16-byte aligned: (total u64, share f32, 0) (marginal u64[h]) (row sums u64[h * w], row j at j * w).
// SceneView does not change for it: the kernels compiled without SF_ENV_SAMPLE keep their argument block, and their code, to the bit.
typedef unsigned long long env_u64;
constexpr int ENV_SAMPLE_MAX_DIM = 16384;           // w, h of an environment that gets a table (row totals times 2^24 stay below 2^64)
constexpr long long ENV_SAMPLE_MAX_CELLS = 1ll << 25;     // and w * h: the table takes 8 bytes a cell (256 MiB at the cap; 16384 x 2048 fits)
TM_HD bool env_sample_dims_ok(int w, int h) { return w >= 1 && h >= 1 && w <= ENV_SAMPLE_MAX_DIM && h <= ENV_SAMPLE_MAX_DIM && (long long)w * h <= ENV_SAMPLE_MAX_CELLS; }
constexpr float ENV_SHADOW_DIST = 2000000.0f;       // the "unbounded" sh_dist of an environment shadow ray: beyond INF_VALUE, so any accepted hit settles a bounded walk
constexpr float ENV_TWO_PI_SQ = (2.0f * PI_SCENE) * PI_SCENE;
TM_HD size_t env_table_offset(int w, int h) { return (((size_t)w * (size_t)h) * 4u + 15u) & ~(size_t)15u; }
TM_HD size_t env_table_bytes(int w, int h) { return 16u + 8u * ((size_t)h + (size_t)w * (size_t)h); }
// q(i, j): step 1 of include/tirt.h.  Host and device (tm_* only): tirt_shade_features_host_env asks "is any q > 0" without a device.
TM_HD float env_texel_lum(const int *img, int w, int h, int x, int y)
{
    x = x > w - 1 ? w - 1 : x; y = y > h - 1 ? h - 1 : y;
    const int RGBA = img[(size_t)x * h + y];
    const float c[3] = {(float)((RGBA & 0x00FF0000) >> 16) / 255.0f, (float)((RGBA & 0x0000FF00) >> 8) / 255.0f, (float)(RGBA & 0x000000FF) / 255.0f};
    float l[3];
    for (int k = 0; k < 3; k++) l[k] = (c[k] < 0.04045f) ? c[k] / 12.92f : tm_pow((c[k] + 0.055f) / 1.055f, 2.4f);      // srgb_to_lrgb1
    return ((l[0] + l[1]) + l[2]) / 3.0f;                                                                                // the level of tirt_moments_converged
}
TM_HD unsigned env_cell_q(const int *img, int w, int h, int i, int j)
{
    const float m = ((env_texel_lum(img, w, h, i, j) + env_texel_lum(img, w, h, i + 1, j)) + (env_texel_lum(img, w, h, i, j + 1) + env_texel_lum(img, w, h, i + 1, j + 1))) * 0.25f;
    const float el = (((float)j + 0.5f) / (float)h - 0.5f) * PI_SCENE;
    const float wgt = m * tm_cos(el);
    const float s = __builtin_rintf(wgt * 16777216.0f);
    return s > 0.0f ? (unsigned)s : 0u;
}
// the same for an RGBE8 image: the level of the decoded texels, the same cell mean and cos(el), and the scale 2^(152 - e_max) in 2^24's place, applied by an exact ldexp
// (e_max: the largest exponent byte among texels with a mantissa, so every channel is below 2^(e_max - 128) and q <= 2^24; sums that overflow to +Inf -- possible
// only from e_max = 254 on -- give 2^24 by the clamp).  Adding a constant to every such texel's exponent byte scales m and the inverse scale by exact powers of two: the same q.
TM_HD float env_texel_lum_hdr(const int *img, int w, int h, int x, int y)
{
    x = x > w - 1 ? w - 1 : x; y = y > h - 1 ? h - 1 : y;
    float l[3]; hdr_decode(img[(size_t)x * h + y], l);
    return ((l[0] + l[1]) + l[2]) / 3.0f;
}
TM_HD unsigned env_cell_q_hdr(const int *img, int w, int h, int i, int j, int e_max)
{
    const float m = ((env_texel_lum_hdr(img, w, h, i, j) + env_texel_lum_hdr(img, w, h, i + 1, j)) + (env_texel_lum_hdr(img, w, h, i, j + 1) + env_texel_lum_hdr(img, w, h, i + 1, j + 1))) * 0.25f;
    const float el = (((float)j + 0.5f) / (float)h - 0.5f) * PI_SCENE;
    const float wgt = m * tm_cos(el);
    const float s = __builtin_rintf(__builtin_ldexpf(wgt, 152 - e_max));
    return s > 0.0f ? (s < 16777216.0f ? (unsigned)s : 16777216u) : 0u;
}
struct EnvTable { const env_u64 *marg, *rows; env_u64 total; float share; };
TD EnvTable env_table(const SceneView &sc)
{
    const char *b = (const char *)sc.env + env_table_offset(sc.env_w, sc.env_h);
    EnvTable t; t.total = *(const env_u64 *)b; t.share = *(const float *)(b + 8);
    t.marg = (const env_u64 *)(b + 16); t.rows = t.marg + sc.env_h;
    return t;
}
// step 3: entry of an inclusive sum `cum[n]` (last entry `tot` > 0) picked by the 24-bit random k, and the offset inside it: all integers, then one exact conversion
TD int env_pick(const env_u64 *cum, int n, unsigned k, env_u64 tot, float &off)
{
    const env_u64 a = (env_u64)k << 40;
    const env_u64 t = __umul64hi(a, tot);                    // floor(k * tot / 2^24)
    const env_u64 fb = (a * tot) >> 40;                      // (k * tot) mod 2^24
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[mid] > t) hi = mid; else lo = mid + 1; }
    const env_u64 below = lo > 0 ? cum[lo - 1] : 0ull;
    env_u64 q = cum[lo] - below;
    if (q == 0ull) q = 1ull;                                 // (never with tot > 0; keeps the division defined on a table that is not one)
    off = (float)((((t - below) << 24) | fb) / q) * 5.9604644775390625e-08f;
    return lo;
}
struct EnvSample { int i, j; float tx, ty; v3 d; };
TD EnvSample env_sample(const EnvTable &t, int w, int h, float ra, float rb)
{
    EnvSample s; float offx, offy;
    const unsigned ka = (unsigned)(ra * 16777216.0f) & 0xffffffu, kb = (unsigned)(rb * 16777216.0f) & 0xffffffu;
    s.j = env_pick(t.marg, h, ka, t.total, offy);
    const env_u64 rowtot = t.marg[s.j] - (s.j > 0 ? t.marg[s.j - 1] : 0ull);
    s.i = env_pick(t.rows + (size_t)s.j * w, w, kb, rowtot, offx);
    s.tx = ((float)s.i + offx) / (float)w; s.ty = ((float)s.j + offy) / (float)h;
    const float az = (s.tx * 2.0f) * PI_SCENE - PI_SCENE, el = (s.ty - 0.5f) * PI_SCENE;
    float sa, ca, se, ce; tm_sincos(az, &sa, &ca); tm_sincos(el, &se, &ce);
    s.d = V(ce * ca, se, ce * sa);
    return s;
}
// step 4: the lookup coordinates of the miss branch (tirt_render.hip, shade_path) and the pdf over solid angle of the cell they land in
struct EnvPdf { int i, j; float tx, ty, pdf; };
TD EnvPdf env_pdf(const EnvTable &t, int w, int h, v3 d)
{
    EnvPdf p;
    const float dis = tm_sqrt(d.x * d.x + d.z * d.z);
    p.tx = (tm_atan2(d.z, d.x) + PI_SCENE) / PI_SCENE / 2.0f;
    p.ty = tm_atan2(d.y, dis) / PI_SCENE + 0.5f;
    const float x = clampf(p.tx * (float)w, 0.0f, (float)w - 1.0f), y = clampf(p.ty * (float)h, 0.0f, (float)h - 1.0f);
    int i = (int)tm_floor(x), j = (int)tm_floor(y);
    i = i < 0 ? 0 : (i > w - 1 ? w - 1 : i); j = j < 0 ? 0 : (j > h - 1 ? h - 1 : j);
    p.i = i; p.j = j; p.pdf = 0.0f;
    if (dis >= 0.000001f) {
        const env_u64 *row = t.rows + (size_t)j * w;
        const env_u64 q = row[i] - (i > 0 ? row[i - 1] : 0ull);
        p.pdf = (((float)q / (float)t.total) * ((float)w * (float)h)) / (ENV_TWO_PI_SQ * dis);
    }
    return p;
}

// ---- emitter choice by power (include/tirt.h, "Choosing emitters by power"; tirt_envsample.hip builds the table; no reference counterpart: Scene.sample_li picks uniformly) ----
// The table lives BEHIND the 8 * light_count quads of the light records in the same allocation: a 32-byte head (total u64, uniform share f32, e_max i32, bits of the
// largest weight u32, -) and the inclusive 64-bit sums C[light_count] of the quantised weights.  SceneView does not change for it, and the light records stay what
// BDPT and the spectral path read.  The binary search walks the dense 8-byte sums; the chosen 128-byte record is read once afterwards (light_sample_rec).
constexpr size_t LIGHT_TABLE_HEAD = 32u;
TM_HD size_t light_table_offset(int light_count) { return sizeof(float) * 4u * 8u * (size_t)(light_count > 0 ? light_count : 1); }
TM_HD size_t light_table_bytes(int light_count) { return LIGHT_TABLE_HEAD + 8u * (size_t)(light_count > 0 ? light_count : 1); }
// w_i and q_i of include/tirt.h: level of the emission times the area; the bits of a weight that takes part (finite and > 0), else 0
TM_HD unsigned light_weight_bits(float er, float eg, float eb, float area)
{
    const float w = (((er + eg) + eb) / 3.0f) * area;
    unsigned u; __builtin_memcpy(&u, &w, 4);
    return (w > 0.0f && w <= 3.4028234e38f) ? u : 0u;
}
TM_HD int light_weight_emax(unsigned max_bits)
{
    float m; __builtin_memcpy(&m, &max_bits, 4);
    int e = 0; (void)__builtin_frexpf(m, &e);
    return max_bits ? e : 0;
}
TM_HD unsigned light_weight_q(unsigned bits, int e_max)
{
    if (!bits) return 0u;
    float w; __builtin_memcpy(&w, &bits, 4);
    const float s = __builtin_rintf(__builtin_ldexpf(w, 24 - e_max));
    return s > 1.0f ? (unsigned)s : 1u;
}
struct LightTable { const env_u64 *cum; env_u64 total; float u; };
TD LightTable light_table(const SceneView &sc)
{
    const char *b = (const char *)sc.light_rec + light_table_offset(sc.light_count);
    LightTable t; t.total = *(const env_u64 *)b; t.u = *(const float *)(b + 8); t.cum = (const env_u64 *)(b + LIGHT_TABLE_HEAD);
    return t;
}
// P_i = u / N + (1 - u) * ((float)q_i / (float)total): a quotient, a quotient, a difference, a product, a sum -- in that order
TM_HD float light_choice_P(env_u64 q, env_u64 total, float u, int n) { return u / (float)n + (1.0f - u) * ((float)q / (float)total); }
// the entry a light random r in [0, 1] picks, and its P: below u the reference's index on r / u, else the integer inverse of env_pick on the 24 bits of (r - u) / (1 - u)
TD int light_pick(const LightTable &t, int n, float r, float &P)
{
    int i;
    if (r < t.u) {
        i = (int)((r / t.u) * (float)n);
        if (i >= n) i = n - 1;
    } else {
        unsigned k = (unsigned)(((r - t.u) / (1.0f - t.u)) * 16777216.0f);
        if (k > 16777215u) k = 16777215u;                    // (a rescaled random that rounds to 1)
        const env_u64 tt = __umul64hi((env_u64)k << 40, t.total);      // floor(k * total / 2^24)
        int lo = 0, hi = n - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (t.cum[mid] > tt) hi = mid; else lo = mid + 1; }
        i = lo;
    }
    P = light_choice_P(t.cum[i] - (i > 0 ? t.cum[i - 1] : 0ull), t.total, t.u, n);
    return i;
}
// P of the entry that names a hit primitive: the spare word of its shading record (k_light_phit writes it while the feature is active, 0 otherwise)
TD float shade_rec_phit(const float4 *rec, int prim)
{
    const float4 *r = rec + (size_t)prim * 8;
    return __float_as_int(r[1].w) == PRIMITIVE_TRI ? r[4].w : r[2].x;
}

// ---- Camera.py:122-142 ----------------------------------------------------------------------------------------
TD v3 camera_ray_direction(const CameraView &c, int i, int j, float jx, float jy)
{
    float x = ((float)i + jx - c.cx) / c.fx;
    float y = ((float)j + jy - c.cy) / c.fy;
    float z = -1.0f, w = 0.0f;
    const float *M = c.view_inv;
    float wx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * w;
    float wy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7] * w;
    float wz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11] * w;
    return normalized(V(wx, wy, wz));
}

}  // namespace tirt
