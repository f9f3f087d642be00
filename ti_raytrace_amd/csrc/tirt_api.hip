// tirt_api.hip -- the C-ABI of include/tirt.h: context, uploads/downloads, camera, film,
// tone map, Scene.process_normal / total_area kernels, stats.  (The known-answer entries tirt_kat_*: tirt_kat.hip.)
#include "tirt_internal.h"
#include "tirt_spectral.h"
#include "tirt_multi_hit.h"
#include <stddef.h>
#include <algorithm>
#include <mutex>
#include <string.h>

namespace tirt {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

SceneView scene_view(const tirt_ctx *c)
{
    SceneView s;
    s.vertex = c->vertex.as<float>(); s.primitive = c->primitive.as<int>(); s.material = c->material.as<float>();
    s.shape = c->shape.as<float>(); s.light = c->light.as<int>(); s.env = c->env.as<int>();
    s.mat_lrgb = c->mat_lrgb.as<float>(); s.shade_rec = c->shade_rec.as<float4>(); s.light_rec = c->light_rec.as<float4>();
    s.tex = c->tex_count > 0 ? c->tex.as<int>() : nullptr;
    s.n = c->n; s.light_count = c->light_count; s.env_w = c->env_w; s.env_h = c->env_h; s.env_power = c->env_power;
    return s;
}
BvhView bvh_view(const tirt_ctx *c)
{
    BvhView b;
    b.wnode = c->wnode.as<float4>(); b.tri = c->tri.as<float4>();
    b.cnode = c->cnode.as<uint4>(); b.top_count = c->wide_nodes + c->n_far_nodes < TR_TOP_SLOTS ? c->wide_nodes + c->n_far_nodes : TR_TOP_SLOTS; b.compact = c->compact.as<float>(); b.cparent = c->cparent.as<int>();
    for (int k = 0; k < 3; k++) { b.grid_min[k] = c->grid_min[k]; b.cell[k] = c->grid_cell[k]; b.inv_cell[k] = c->grid_inv_cell[k]; b.inv_extent[k] = c->grid_inv_extent[k]; }
    for (int k = 0; k < 3; k++) { b.root_min[k] = c->root_min[k]; b.root_max[k] = c->root_max[k]; }
    b.root_code = c->root_code;
    b.root_qcode = c->root_code;        // >= 0: wide node 0
    b.far_qcode = c->n_far_nodes ? c->wide_nodes : c->root_code;
    return b;
}
int flush_pending(tirt_ctx *c)
{
    if (!c->pend.valid) return 0;
    c->pend.valid = false;
    return pt_render(c, c->pend.begin, c->pend.count, c->pend.seed, c->pend.max_depth, c->pend.stack_size, c->pend.flags,
                     c->pend.spectral ? (const SpecView *)c->spec_view : nullptr);
}
int sync_all(tirt_ctx *c)
{
    if (int rc = flush_pending(c)) return rc;
    for (Lane &L : c->lanes) if (L.stream) TIRT_HIP(hipStreamSynchronize(L.stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    c->batches_since_sync = 0;
    return 0;
}
int ensure_counters(tirt_ctx *c)
{
    if (!c->dev_counters.p) {
        if (c->dev_counters.ensure(sizeof(DevCounters))) return TIRT_ERR_HIP;
        TIRT_HIP(hipMemsetAsync(c->dev_counters.p, 0, sizeof(DevCounters), c->stream));
    }
    return 0;
}

// ---- per-material srgb_to_lrgb(colour) table (integrator/PT_RGB.py:86 evaluates it per path vertex) ----
__global__ void k_material_lrgb(const float *material, int nm, float *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nm) return;
    const float *m = material + (size_t)i * MAT_VEC;
    v3 c = srgb_to_lrgb(V(m[2], m[3], m[4]));
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
}
static int refresh_material_table(tirt_ctx *c)
{
    if (c->mat_lrgb.ensure(sizeof(float) * 3 * (size_t)c->nm)) return TIRT_ERR_HIP;
    hipLaunchKernelGGL(k_material_lrgb, dim3((c->nm + 63) / 64), dim3(64), 0, c->stream, c->material.as<float>(), c->nm, c->mat_lrgb.as<float>());
    return 0;
}

// ---- 128-byte shading record per primitive (tirt_device.h, hit_attributes_rec) -----------------------
// gnor and area: the expressions of hit_attributes (Scene.py:537-561) and get_prim_area (Scene.py:324-350), evaluated here once per primitive
// textured (the scene's feature word has SF_TEXTURE): the uvs of the three vertices go into the free words; otherwise those stay zero
__global__ void k_shade_records(SceneView s, float4 *rec, int textured)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const int *pr = s.primitive + (size_t)i * PRI_VEC;
    float4 *r = rec + (size_t)i * 8;
    const float mat = __int_as_float(pr[2]);
    const float area = get_prim_area(s, i);
    r[6] = r[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pr[0] == PRIMITIVE_TRI) {
        const v3 v1 = vtx_pos(s, pr[1]), v2 = vtx_pos(s, pr[1] + 1), v3_ = vtx_pos(s, pr[1] + 2);
        const v3 n1 = vtx_nor(s, pr[1]), n2 = vtx_nor(s, pr[1] + 1), n3 = vtx_nor(s, pr[1] + 2);
        const v3 v13 = v3_ - v1, v12 = v2 - v1;
        const v3 gnor = normalized(cross(v12, v13));
        r[0] = make_float4(v1.x, v1.y, v1.z, mat); r[1] = make_float4(v2.x, v2.y, v2.z, __int_as_float(PRIMITIVE_TRI));
        r[2] = make_float4(v3_.x, v3_.y, v3_.z, 0.0f);
        r[3] = make_float4(n1.x, n1.y, n1.z, 0.0f); r[4] = make_float4(n2.x, n2.y, n2.z, 0.0f); r[5] = make_float4(n3.x, n3.y, n3.z, 0.0f);
        r[6] = make_float4(gnor.x, gnor.y, gnor.z, area);
        if (textured) {
            const v3 t1 = vtx_uv(s, pr[1]), t2 = vtx_uv(s, pr[1] + 1), t3 = vtx_uv(s, pr[1] + 2);
            r[2].w = t3.x; r[3].w = t3.y;
            r[7] = make_float4(t1.x, t1.y, t2.x, t2.y);
        }
    } else {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        r[0] = make_float4(sh[1], sh[2], sh[3], mat); r[1] = make_float4(sh[4], sh[0], area, __int_as_float(2));
        r[2] = r[3] = r[4] = r[5] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}
// ---- 128-byte record per entry of the light list (tirt_device.h, light_sample_rec): Scene.sample_li's reads of the emitter (Scene.py:477-518) ----
__global__ void k_light_records(SceneView s, float4 *rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.light_count) return;
    const int light_prim = s.light[i];
    const int *pr = s.primitive + (size_t)light_prim * PRI_VEC;
    float4 *r = rec + (size_t)i * LIGHT_REC_QUADS;
    const float *lm = s.material + (size_t)pr[2] * MAT_VEC;
    const v3 em = V(lm[2], lm[3], lm[4]);
    const float light_area = get_prim_area(s, light_prim);
    float light_choice_pdf = 1.0f / ((float)s.light_count * light_area);
    if (pr[0] == PRIMITIVE_TRI) {
        const v3 v1 = vtx_pos(s, pr[1]), v2 = vtx_pos(s, pr[1] + 1), v3_ = vtx_pos(s, pr[1] + 2);
        const v3 n1 = vtx_nor(s, pr[1]), n2 = vtx_nor(s, pr[1] + 1), n3 = vtx_nor(s, pr[1] + 2);
        const v3 e31 = v3_ - v1, e21 = v2 - v1;
        r[0] = make_float4(v1.x, v1.y, v1.z, light_area); r[1] = make_float4(e31.x, e31.y, e31.z, light_choice_pdf);
        r[2] = make_float4(e21.x, e21.y, e21.z, __int_as_float(-1));
        r[3] = make_float4(n1.x, n1.y, n1.z, em.x); r[4] = make_float4(n2.x, n2.y, n2.z, em.y); r[5] = make_float4(n3.x, n3.y, n3.z, em.z);
    } else {
        const float *sh = s.shape + (size_t)pr[1] * SHA_VEC;
        int st = (int)sh[0];
        if (st == SHAPE_LASER) light_choice_pdf = 1.0f / (float)s.light_count;       // Scene.py:509 (light_shape_visible)
        if (st == -1) st = -2;                                                       // (-1 marks a triangle; no shape type is negative)
        r[0] = make_float4(sh[1], sh[2], sh[3], light_area); r[1] = make_float4(sh[4], sh[5], 0.0f, light_choice_pdf);
        r[2] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(st));
        r[3] = make_float4(sh[7], sh[8], sh[9], em.x); r[4] = make_float4(0.0f, 0.0f, 0.0f, em.y); r[5] = make_float4(0.0f, 0.0f, 0.0f, em.z);
    }
    r[6] = r[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// ---- scene feature word (tirt_device.h, SF_*) ------------------------------------------------------------
// the kind of every emitter on the light list as k_light_records writes it into the light record: -1 a triangle, else the shape type
static void light_kinds(const int32_t *primitive, const float *shape, const int32_t *light, int light_count, std::vector<int> &kind)
{
    kind.resize((size_t)(light_count > 0 ? light_count : 0));
    for (int i = 0; i < light_count; i++) {
        const int32_t *pr = primitive + (size_t)light[i] * PRI_VEC;
        int st = -1;
        if (pr[0] != PRIMITIVE_TRI) { st = (int)shape[(size_t)pr[1] * SHA_VEC]; if (st == -1) st = -2; }
        kind[(size_t)i] = st;
    }
}
static bool env_is_lit(const int32_t *texel, size_t count, float power)
{
    if (power != 0.0f) return true;
    for (size_t k = 0; k < count; k++) if (texel[k] & 0x00FFFFFF) return true;      // (tex_sample reads the low 24 bits)
    return false;
}
// the slot a material row names in `word` (1 albedo, 7 roughness, 8 metallic, 9 normal map; as the device's (int) conversion reads it: saturating,
// NaN -> 0): >= 1 names texture slot - 1
static int material_texture_slot(const float *row, int word = 1)
{
    const float s = row[word];
    return s >= 2147483648.0f ? 0x7fffffff : s >= 1.0f ? (int)s : 0;
}
// the words of a row that name textures, and whether the row's type honours that word: an emitter none, glass not 7 and 8 (its words 5, 6 are ior and extinction)
static const int MAT_TEX_WORDS[4] = {1, 7, 8, 9};
static bool material_honours(const float *row, int word)
{
    const int type = (int)row[0];
    return type != MAT_LIGHT && !(type == MAT_GLASS && (word == 7 || word == 8));
}
// every material row that is not an emitter's names no texture, or one of the tex_count uploaded ones (tex_count == 0: nothing is textured, nothing to check)
static int check_material_textures(const char *fn, const float *material, int nm, int tex_count)
{
    if (tex_count <= 0) return TIRT_OK;
    for (int i = 0; i < nm; i++) {
        const float *row = material + (size_t)i * MAT_VEC;
        TIRT_REQUIRE((int)row[0] == MAT_LIGHT || material_texture_slot(row) <= tex_count,
                     std::string(fn) + ": material " + std::to_string(i) + " names texture " + std::to_string(material_texture_slot(row)) + " of " + std::to_string(tex_count) +
                     " uploaded (slot 1 of the row: 0 or -1 = none; tirt_texture_upload with count 0 removes all textures)");
        for (int k = 1; k < 4; k++) {
            const int word = MAT_TEX_WORDS[k];
            TIRT_REQUIRE(!material_honours(row, word) || material_texture_slot(row, word) <= tex_count,
                         std::string(fn) + ": material " + std::to_string(i) + " names texture " + std::to_string(material_texture_slot(row, word)) + " of " + std::to_string(tex_count) +
                         " uploaded in word " + std::to_string(word) + " (7 roughness, 8 metallic, 9 normal map: 0 = none; tirt_texture_upload with count 0 removes all textures)");
        }
    }
    return TIRT_OK;
}
static unsigned shade_features_core(const float *material, int nm, const int *light_kind, int light_count, bool env_lit, int tex_count = 0)
{
    unsigned f = 0u;
    for (int i = 0; i < nm; i++) if ((int)material[(size_t)i * MAT_VEC] == MAT_GLASS) f |= SF_GLASS;
    for (int i = 0; i < nm && tex_count > 0; i++) {
        const float *row = material + (size_t)i * MAT_VEC;
        const int slot = material_texture_slot(row);
        if ((int)row[0] != MAT_LIGHT && slot >= 1 && slot <= tex_count) f |= SF_TEXTURE;
        for (int k = 1; k < 4; k++) {
            const int ps = material_texture_slot(row, MAT_TEX_WORDS[k]);
            if (material_honours(row, MAT_TEX_WORDS[k]) && ps >= 1 && ps <= tex_count) f |= SF_TEXTURE_PARAM;
        }
    }
    if (env_lit) f |= SF_ENV;
    if (light_count <= 0) f |= SF_NO_LIGHT;
    for (int i = 0; i < light_count; i++) {
        const int k = light_kind[i];
        f |= k == -1 ? SF_LIGHT_TRI : k == SHAPE_SPHERE ? SF_LIGHT_SPHERE : (k == SHAPE_SPOT || k == SHAPE_LASER) ? SF_LIGHT_SPOT_LASER : SF_LIGHT_OTHER;
    }
    return f;
}
void refresh_shade_features(tirt_ctx *c)
{
    c->shade_features = c->h_material.empty() ? SF_ALL
        : shade_features_core(c->h_material.data(), c->nm, c->h_light_kind.data(), c->light_count, c->env_lit, c->tex_count);
    // SF_CUTOUT, kept beside the word (tirt_shade_features puts it in): a material row some triangle uses, not an emitter's, whose word 1 names a flagged texture
    c->has_cutout = false;
    for (int i = 0; i < c->nm && !c->h_material.empty() && !c->tex_cutout.empty(); i++) {
        const float *row = c->h_material.data() + (size_t)i * MAT_VEC;
        const int slot = material_texture_slot(row);
        if ((size_t)i < c->h_mat_on_tri.size() && c->h_mat_on_tri[(size_t)i] && (int)row[0] != MAT_LIGHT && slot >= 1 && slot <= c->tex_count &&
            (size_t)slot <= c->tex_cutout.size() && c->tex_cutout[(size_t)slot - 1]) c->has_cutout = true;
    }
    c->cut_rec_valid = false;      // every caller has changed one of the tables the tags are derived from
}

// ---- alpha cut-outs: the tag in every record of `tri` and the side array of vertex uvs (tirt_internal.h, trace_leaf_step) ----
// flags == nullptr: every tag back to 0 (a scene that has lost its last cut-out triangle; cut_uv is not touched)
__global__ void k_cutout_records(SceneView s, const int *prim_slot, const int *flags, int tex_count, float4 *tri, float4 *cut_uv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const int *pr = s.primitive + (size_t)i * PRI_VEC;
    const size_t slot = (size_t)prim_slot[i];
    int tag = 0;
    float4 ua = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ub = ua;
    if (flags && pr[0] == PRIMITIVE_TRI) {
        const int id = material_texture(s.material + (size_t)pr[2] * MAT_VEC);
        if (id >= 0 && id < tex_count && flags[id]) {
            tag = id + 1;
            const v3 t1 = vtx_uv(s, pr[1]), t2 = vtx_uv(s, pr[1] + 1), t3 = vtx_uv(s, pr[1] + 2);
            ua = make_float4(t1.x, t1.y, t2.x, t2.y); ub = make_float4(t3.x, t3.y, __int_as_float(id), 0.0f);
        }
    }
    tri[slot * TRI_STRIDE + 1].w = __int_as_float(tag);
    if (flags) { cut_uv[slot * 2] = ua; cut_uv[slot * 2 + 1] = ub; }
}
int ensure_cutout_records(tirt_ctx *c)
{
    if (c->cut_rec_valid || !c->built) return TIRT_OK;
    if (c->has_cutout || c->cut_tagged) {
        const int *flags = nullptr;
        if (c->has_cutout) {
            if (c->cut_uv.ensure(sizeof(float4) * 2 * (size_t)c->n) || c->cut_flags.ensure(sizeof(int) * (size_t)c->tex_count)) return TIRT_ERR_HIP;
            TIRT_HIP(hipMemcpyAsync(c->cut_flags.p, c->tex_cutout.data(), sizeof(int) * (size_t)c->tex_count, hipMemcpyHostToDevice, c->stream));
            flags = c->cut_flags.as<int>();
        }
        hipLaunchKernelGGL(k_cutout_records, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, scene_view(c), c->prim_slot.as<int>(), flags, c->tex_count,
                           c->tri.as<float4>(), c->cut_uv.as<float4>());
        TIRT_HIP(hipStreamSynchronize(c->stream));      // (rare: after an upload; the launch that follows may be on a lane's stream, and tex_cutout may change)
        c->cut_tagged = c->has_cutout;
    }
    c->cut_rec_valid = true;
    return TIRT_OK;
}

int ensure_shade_records(tirt_ctx *c)
{
    if (!(c->shade_rec_valid && c->shade_rec.p)) {
        if (c->shade_rec.ensure(sizeof(float4) * 8 * (size_t)c->n)) return TIRT_ERR_HIP;
        hipLaunchKernelGGL(k_shade_records, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, scene_view(c), c->shade_rec.as<float4>(), (c->shade_features & (SF_TEXTURE | SF_TEXTURE_PARAM)) ? 1 : 0);
        c->shade_rec_valid = true;
        c->light_phit_written = false;             // (the spare words are zero again)
    }
    if (!(c->light_rec_valid && c->light_rec.p)) {
        // (never an empty allocation; no record is read when light_count is 0.  Behind the records: room for the table of tirt_light_sampling, 8 bytes an entry)
        if (c->light_rec.ensure(light_table_offset(c->light_count) + light_table_bytes(c->light_count))) return TIRT_ERR_HIP;
        if (c->light_count > 0)
            hipLaunchKernelGGL(k_light_records, dim3((c->light_count + 63) / 64), dim3(64), 0, c->stream, scene_view(c), c->light_rec.as<float4>());
        c->light_rec_valid = true;
        c->light_tab_valid = false;
    }
    return light_table_sync(c);
}

// ---- Scene.total_area (Scene.py:747-750): serial so the f32 sum order is defined --------------
__global__ void k_total_area(SceneView s, int count, float *out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float a = 0.0f;
        for (int i = 0; i < count; i++) a += get_prim_area(s, s.light[i]);
        *out = a;
    }
}

// ---- Scene.process_normal (Scene.py:754-798): BVH point query per vertex ------------------------
__global__ void k_smooth_normal(SceneView s, int nv, const float *compact, const int *vertex_index, float *smooth)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    constexpr int MAX_STACK_SIZE = 32;              // Scene.py:19
    int stack[MAX_STACK_SIZE + 2];
    v3 v = vtx_pos(s, i);
    v3 n = normalized(vtx_nor(s, i));
    int f = vertex_index[i];
    v3 sm = (n * get_prim_angle(s, f, v)) * get_prim_area(s, f);
    stack[0] = 0;
    int stack_pos = 0;
    while ((stack_pos >= 0) & (stack_pos < MAX_STACK_SIZE)) {
        int node = stack[stack_pos];
        stack_pos -= 1;
        const float *cn = compact + (size_t)node * CPN_VEC;
        if ((((int)cn[0]) & 1) == 1) {
            int prim = (int)cn[1];
            const int *pr = s.primitive + (size_t)prim * PRI_VEC;
            if (pr[0] == PRIMITIVE_TRI) {
                for (int j = 0; j < 3; j++) {
                    int nb = j + pr[1];
                    if (i != nb) {
                        v3 nvp = vtx_pos(s, nb);
                        v3 nn = normalized(vtx_nor(s, nb));
                        if ((int)(norm(v - nvp) < 0.000001f) & (int)(dot(nn, n) > 0.5f)) {      // (Scene.py:781: both sides evaluated, as the reference's `&` does)
                            float angle = get_prim_angle(s, prim, nvp);
                            sm = sm + (nn * angle) * get_prim_area(s, prim);
                        }
                    }
                }
            }
        } else {
            if ((v.x >= cn[2]) & (v.y >= cn[3]) & (v.z >= cn[4]) & (v.x <= cn[5]) & (v.y <= cn[6]) & (v.z <= cn[7])) {
                stack_pos += 1; stack[stack_pos] = node + 1;
                stack_pos += 1; stack[stack_pos] = (int)cn[1];
            }
        }
    }
    smooth[3 * i] = sm.x; smooth[3 * i + 1] = sm.y; smooth[3 * i + 2] = sm.z;
}
__global__ void k_write_normal(float *vertex, int nv, const float *smooth)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    v3 nn = normalized(V(smooth[3 * i], smooth[3 * i + 1], smooth[3 * i + 2]));
    float *p = vertex + (size_t)i * VER_VEC;
    p[3] = nn.x; p[4] = nn.y; p[5] = nn.z;
}

// UtilsFunc.py:583-586
__global__ void k_tone_map(const float *hdr, float *rgb, long nvals, float exposure)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nvals) return;
    rgb[i] = lrgb_to_srgb1(tone_aces1(hdr[i] * exposure));
}

// ---- bench helper: ceiling of scattered 64-byte record gathers (the node-fetch pattern of k_trace) ----
TD uint32_t mg_mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
__global__ __launch_bounds__(256) void k_micro_gather(const float4 *rec, uint32_t nrec, int iters, float *out)
{
    uint32_t s = mg_mix(blockIdx.x * 256 + threadIdx.x + 1);
    float acc = 0.0f;
    for (int it = 0; it < iters; it++) {
        s = mg_mix(s + it);
        const uint32_t idx = (uint32_t)(((unsigned long long)s * nrec) >> 32);
        const float4 *p = rec + (size_t)idx * 4;
        const float4 a = p[0], b = p[1], c = p[2], d = p[3];
        acc += a.x + b.y + c.z + d.w;
    }
    out[blockIdx.x * 256 + threadIdx.x] = acc;
}

static int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t st)
{
    if (b.ensure(bytes)) return TIRT_ERR_HIP;
    if (bytes) TIRT_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

}  // namespace tirt

using namespace tirt;

extern "C" {

const char *tirt_last_error(void) { return g_error.c_str(); }
int tirt_version(void) { return 102; }

int tirt_device_count(int *out)
{
    TIRT_REQUIRE(out, "tirt_device_count: null out");
    TIRT_HIP(hipGetDeviceCount(out));
    return TIRT_OK;
}

int tirt_create(int device_id, tirt_ctx **out)
{
    TIRT_REQUIRE(out, "tirt_create: null out");
    int ndev = 0;
    TIRT_HIP(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) { set_error("tirt_create: device " + std::to_string(device_id) + " of " + std::to_string(ndev)); return TIRT_ERR_ARG; }
    TIRT_HIP(hipSetDevice(device_id));
    tirt_ctx *c = new tirt_ctx();
    c->device = device_id;
    TIRT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    TIRT_HIP(hipEventCreate(&c->ev0));
    TIRT_HIP(hipEventCreate(&c->ev1));
    TIRT_HIP(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    for (Lane &L : c->lanes) {
        TIRT_HIP(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        TIRT_HIP(hipEventCreateWithFlags(&L.film_done, hipEventDisableTiming));
        TIRT_HIP(hipEventCreateWithFlags(&L.aov_done, hipEventDisableTiming));
    }
    memset(&c->cam, 0, sizeof(c->cam));
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device_id) == hipSuccess && optin > 0) c->lds_optin = (size_t)optin;
    else { (void)hipGetLastError(); if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && optin > 0) c->lds_optin = (size_t)optin; }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) {
        const int g = 5 * cus < 2048 ? 5 * cus : 2048;            // five 256-thread k_trace blocks per CU (tirt_internal.h, TR_TOP_CAP)
        c->tr_grid = g; c->tr_grid_alone = g; c->cu_count = cus;
    } else (void)hipGetLastError();
    *out = c;
    return TIRT_OK;
}

void tirt_destroy(tirt_ctx *c)
{
    if (!c) return;
    if (c->comm) { tirt_ctx *one[1] = {c}; (void)tirt_comm_destroy(one, 1); }
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    retire_render_events(c, false);
    DevBuf *bufs[] = {&c->vertex, &c->primitive, &c->material, &c->shape, &c->light, &c->env, &c->tex, &c->cut_uv, &c->cut_flags, &c->mat_lrgb, &c->shade_rec, &c->light_rec, &c->morton_unsorted, &c->keys_a,
                      &c->keys_b, &c->vals_a, &c->vals_b, &c->hist, &c->morton_sorted, &c->bvh_node, &c->compact, &c->parent,
                      &c->flag, &c->subtree, &c->build_status, &c->leaf_compact, &c->wnode, &c->tri, &c->prim_slot, &c->cnode, &c->cparent, &c->csize, &c->wide_queue, &c->wide_levels, &c->sah_compact, &c->sah_csize, &c->sah_parent, &c->wide_dp, &c->sah_box, &c->sah_idx, &c->sah_tasks, &c->sah_counts, &c->hdr, &c->rgb, &c->aov, &c->mom, &c->mom_cnt, &c->pixset, &c->pixset_tmp, &c->tp_mem, &c->mv_rec, &c->mv_snap, &c->dn_mem, &c->dn_out,
                      &c->counters_mem, &c->spill, &c->trace_stage, &c->debug_mem, &c->query_mem, &c->sd_tab, &c->sd_state, &c->wn_tab, &c->wn_sums, &c->dyn_mem, &c->dev_counters, &c->bdpt_px, &c->bd_rec, &c->timeline, &c->pvb_set[0].count, &c->pvb_set[0].cand, &c->pvb_set[0].bound, &c->pvb_set[1].count, &c->pvb_set[1].cand, &c->pvb_set[1].bound, &c->pvb_stat, &c->pvb_tmp};
    for (DevBuf *b : bufs) b->release();
    for (auto &bl : c->bd) {
        DevBuf *bb[] = {&bl.items, &bl.state, &bl.rays, &bl.hits, &bl.qidx, &bl.ctr, &bl.rad};
        for (DevBuf *b : bb) b->release();
        if (bl.delta_done) (void)hipEventDestroy(bl.delta_done);
        if (bl.film_done) (void)hipEventDestroy(bl.film_done);
    }
    for (Lane &L : c->lanes) {
        DevBuf *lb[] = {&L.path_mem, &L.counters_mem, &L.spill};
        for (DevBuf *b : lb) b->release();
        if (L.film_done) (void)hipEventDestroy(L.film_done);
        if (L.aov_done) (void)hipEventDestroy(L.aov_done);
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    c->spec_mem.release(); c->spec_dev.release();
    if (c->spec_view) { delete (SpecView *)c->spec_view; c->spec_view = nullptr; }
    if (c->ev_main) (void)hipEventDestroy(c->ev_main);
    if (c->query_ev_in) (void)hipEventDestroy(c->query_ev_in);
    if (c->query_ev_out) (void)hipEventDestroy(c->query_ev_out);
    (void)hipEventDestroy(c->ev0); (void)hipEventDestroy(c->ev1);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

// film readers/writers on the main stream run after the last film update of the render lanes
#define AFTER_RENDER(c)                                                            \
    do { if ((c)->last_film) TIRT_HIP(hipStreamWaitEvent((c)->stream, (c)->last_film, 0)); } while (0)

// the same for the feature buffers (tirt_aov.hip): after the last k_aov
#define AFTER_AOV(c)                                                               \
    do { if ((c)->last_aov) TIRT_HIP(hipStreamWaitEvent((c)->stream, (c)->last_aov, 0)); } while (0)

int tirt_sync(tirt_ctx *c)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int tirt_set_option(tirt_ctx *c, const char *name, double value)
{
    CTX(c);
    TIRT_REQUIRE(name, "tirt_set_option: null name");
    if (!strcmp(name, "time_kernels")) { c->time_kernels = value != 0.0; return TIRT_OK; }
    if (!strcmp(name, "overlap_lanes")) { TIRT_REQUIRE(value >= 1.0 && value <= (double)TIRT_MAX_LANES, "overlap_lanes: 1..8"); if (sync_all(c)) return TIRT_ERR_HIP; c->n_lanes = (int)value; return TIRT_OK; }
#ifndef TIRT_EXPERIMENTS
    if (!strcmp(name, "wide_collapse")) {
        TIRT_REQUIRE(value == 0.0, "this option is an experiment (cost-optimal wide collapse): build with -DTIRT_EXPERIMENTS (make experiments)");
        return TIRT_OK;
    }
#endif
    if (!strcmp(name, "split_lone_batch")) { TIRT_REQUIRE(value >= 0.0 && value <= 8.0, "split_lone_batch: 0 (off) or the number of parts, 2..8"); c->split_lone = (int)value; return TIRT_OK; }
    if (!strcmp(name, "wide_collapse")) { TIRT_REQUIRE(value == 0.0 || value == 1.0, "wide_collapse: 0 (greedy) or 1 (cost-optimal)"); c->wide_dp_on = (int)value; return TIRT_OK; }
    if (!strcmp(name, "traversal_tree")) {       // takes effect at the next tirt_lbvh_build
        TIRT_REQUIRE(value == 0.0 || value == 1.0, "traversal_tree: 0 (the reference's LBVH) or 1 (binned SAH)");
        c->use_sah = (int)value; return TIRT_OK;
    }
    if (!strcmp(name, "plan_batches")) { TIRT_REQUIRE(value >= 0.0 && value <= 64.0, "plan_batches: 0 (automatic) .. 64"); if (flush_pending(c)) return TIRT_ERR_HIP; c->plan_nb = (int)value; return TIRT_OK; }
    if (!strcmp(name, "plan_lanes")) { TIRT_REQUIRE(value >= 0.0 && value <= TIRT_MAX_LANES, "plan_lanes: 0 (automatic) .. the lane count"); if (flush_pending(c)) return TIRT_ERR_HIP; c->plan_lanes = (int)value; return TIRT_OK; }
    if (!strcmp(name, "job_frames")) { TIRT_REQUIRE(value >= 0.0 && value <= 1.0e9, "job_frames out of range"); c->job_frames = (long)value; return TIRT_OK; }
    if (!strcmp(name, "merge_paths")) { TIRT_REQUIRE(value >= 0.0 && value <= 1.0e9, "merge_paths out of range"); c->merge_paths = (size_t)value; c->merge_user = true; return TIRT_OK; }
    if (!strcmp(name, "batch_paths")) {
        TIRT_REQUIRE(value >= 1.0 && value <= 1.0e9, "tirt_set_option: batch_paths out of range");
        c->batch_paths = (size_t)value; c->batch_user = true; return TIRT_OK;
    }
    if (!strcmp(name, "trace_lds_depth")) {
        TIRT_REQUIRE(value >= 12 && value <= 64, "trace_lds_depth: 12..64");
        TIRT_REQUIRE(trace_lds_bytes((int)value) <= c->lds_optin, "trace_lds_depth: stacks + tree top exceed the LDS a block can have on this device");
        c->tr_lds_depth = (int)value; return TIRT_OK;
    }
    if (!strcmp(name, "bdpt_stack_size")) { TIRT_REQUIRE(value >= 16 && value <= 4096, "bdpt_stack_size: 16..4096"); c->bdpt_stack = (int)value; return TIRT_OK; }
    if (!strcmp(name, "trace_timeline")) { c->timeline_arm = (int)value; c->timeline_waves = 0; return TIRT_OK; }
    if (!strcmp(name, "trace_refill_min")) { TIRT_REQUIRE(value >= 1 && value <= 64, "trace_refill_min: 1..64"); c->tr_refill_min = (int)value; return TIRT_OK; }
    if (!strcmp(name, "trace_node_min")) { TIRT_REQUIRE(value >= 1 && value <= 64, "trace_node_min: 1..64"); c->tr_node_min = (int)value; return TIRT_OK; }
    if (!strcmp(name, "bdpt_bounded")) { c->bdpt_bounded = value != 0.0 ? 1 : 0; return TIRT_OK; }
    if (!strcmp(name, "bdpt_state_fill")) { TIRT_REQUIRE(value == 0.0 || value == 1.0 || value == 2.0, "bdpt_state_fill: 0 (none), 1 (zeros) or 2 (poison)"); c->bdpt_state_fill = (int)value; return TIRT_OK; }
    if (!strcmp(name, "primary_beams")) { TIRT_REQUIRE(value == 0.0 || value == 1.0, "primary_beams: 0 or 1"); if (flush_pending(c)) return TIRT_ERR_HIP; c->primary_beams = (int)value; return TIRT_OK; }
    // "primary_beams_rebuild": forget the camera rays' candidate lists -- the next batch that uses lists makes them again (bench.py: a list build inside its clock)
    if (!strcmp(name, "primary_beams_rebuild")) { if (flush_pending(c)) return TIRT_ERR_HIP; c->pvb_valid = false; return TIRT_OK; }
    if (!strcmp(name, "primary_beams_diag")) { if (flush_pending(c)) return TIRT_ERR_HIP; c->pvb_diag = value != 0.0; return TIRT_OK; }
    if (!strcmp(name, "primary_beams_edges")) { TIRT_REQUIRE(value == 0.0 || value == 1.0, "primary_beams_edges: 0 or 1"); if (flush_pending(c)) return TIRT_ERR_HIP; c->pvb_edges = (int)value; return TIRT_OK; }      // (part of the lists' key: pvb_prepare makes them again)
    if (!strcmp(name, "primary_fused")) { TIRT_REQUIRE(value == 0.0 || value == 1.0, "primary_fused: 0 or 1"); if (flush_pending(c)) return TIRT_ERR_HIP; c->primary_fused = (int)value; return TIRT_OK; }
    if (!strcmp(name, "primary_beams_min_frames")) { TIRT_REQUIRE(value >= 1.0 && value <= 1.0e6, "primary_beams_min_frames out of range"); if (flush_pending(c)) return TIRT_ERR_HIP; c->primary_beams_min_frames = (int)value; return TIRT_OK; }
    if (!strcmp(name, "bdpt_lanes")) { TIRT_REQUIRE(value >= 1.0 && value <= 4.0, "bdpt_lanes: 1..4"); if (sync_all(c)) return TIRT_ERR_HIP; c->bdpt_lanes = (int)value; return TIRT_OK; }
    if (!strcmp(name, "bdpt_batch_items")) { TIRT_REQUIRE(value >= 1.0 && value <= 1.0e9, "bdpt_batch_items out of range"); c->bdpt_batch_items = (size_t)value; return TIRT_OK; }
    if (!strcmp(name, "bdpt_mem_budget")) { TIRT_REQUIRE(value >= 0, "bdpt_mem_budget: bytes >= 0"); c->bdpt_mem_budget = (size_t)value; return TIRT_OK; }
    if (!strcmp(name, "trace_slices")) {
        const int iv = (int)value;
        TIRT_REQUIRE(iv >= 1 && iv <= 64 && (iv & (iv - 1)) == 0, "trace_slices: power of two, 1..64");
        int l = 0; while ((1 << l) < iv) l++;
        c->tr_slice_log2 = l; return TIRT_OK;
    }
    if (!strcmp(name, "shade_specialize")) { TIRT_REQUIRE(value == 0.0 || value == 1.0, "shade_specialize: 0 (generic kernel) or 1"); if (flush_pending(c)) return TIRT_ERR_HIP; c->shade_specialize = (int)value; return TIRT_OK; }
    if (!strcmp(name, "shade_grid")) { TIRT_REQUIRE(value >= 1 && value <= 65536, "shade_grid: 1..65536"); c->sh_grid = (int)value; c->grid_user = true; return TIRT_OK; }
    if (!strcmp(name, "path_order_blocks")) { c->path_order_blocks = value != 0.0; return TIRT_OK; }
    if (!strcmp(name, "slices_contiguous")) { c->slices_contiguous = value != 0.0; return TIRT_OK; }
    if (!strcmp(name, "trace_grid_alone")) { TIRT_REQUIRE(value >= 1 && value <= 16384, "trace_grid_alone: 1..16384"); c->tr_grid_alone = (int)value; return TIRT_OK; }
    if (!strcmp(name, "query_chunk_rays")) {       // rays per chunk of tirt_query_closest / tirt_query_occluded (the scratch is sized to one chunk, 48 bytes per ray)
        TIRT_REQUIRE(value >= 256.0 && value <= (double)(1 << 27), "query_chunk_rays: 256 .. 2^27");
        c->query_chunk = (size_t)value; return TIRT_OK;
    }
    if (!strcmp(name, "trace_grid")) { TIRT_REQUIRE(value >= 1 && value <= 16384, "trace_grid: 1..16384"); c->tr_grid = (int)value; c->grid_user = true; return TIRT_OK; }
    set_error(std::string("tirt_set_option: unknown option ") + name);
    return TIRT_ERR_ARG;
}

int tirt_scene_upload(tirt_ctx *c, const float *vertex, int nv, const int32_t *primitive, int n, const float *material, int nm,
                      const float *shape, int ns, const int32_t *light, int nl, int light_count, const float bmin[3], const float bmax[3])
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    TIRT_REQUIRE(n >= 1 && nv >= 0 && nm >= 1 && ns >= 1 && nl >= 1, "tirt_scene_upload: need n,nm,ns,nl >= 1");
    TIRT_REQUIRE(vertex && primitive && material && shape && light && bmin && bmax, "tirt_scene_upload: null pointer");
    TIRT_REQUIRE(light_count >= 0 && light_count <= nl, "tirt_scene_upload: light_count out of range");
    TIRT_REQUIRE((long long)2 * n - 1 < (1ll << 24), "tirt_scene_upload: node indices are stored as f32 (exact below 2^24 nodes)");
    // validate indices on the host so that device code can trust them
    for (int i = 0; i < n; i++) {
        const int32_t *pr = primitive + (size_t)i * 3;
        if (pr[0] == PRIMITIVE_TRI) { TIRT_REQUIRE(pr[1] >= 0 && pr[1] + 2 < nv, "tirt_scene_upload: vertex index out of range"); }
        else { TIRT_REQUIRE(pr[1] >= 0 && pr[1] < ns, "tirt_scene_upload: shape index out of range"); }
        TIRT_REQUIRE(pr[2] >= 0 && pr[2] < nm, "tirt_scene_upload: material index out of range");
    }
    for (int i = 0; i < nl; i++) TIRT_REQUIRE(light[i] >= 0 && light[i] < n, "tirt_scene_upload: light index out of range");
    if (int rc = check_material_textures("tirt_scene_upload", material, nm, c->tex_count)) return rc;
    c->sphere_prims.clear(); c->sphere_geom.clear();
    c->h_mat_on_tri.assign((size_t)nm, 0);
    for (int i = 0; i < n; i++) {
        const int32_t *pr = primitive + (size_t)i * 3;
        if (pr[0] == PRIMITIVE_TRI) c->h_mat_on_tri[(size_t)pr[2]] = 1;
        if (pr[0] != PRIMITIVE_TRI && (int)shape[(size_t)pr[1] * 10] == SHAPE_SPHERE) {
            c->sphere_prims.push_back(i);
            for (int k = 1; k <= 4; k++) c->sphere_geom.push_back(shape[(size_t)pr[1] * 10 + k]);
        }
    }
    hipStream_t st = c->stream;
    c->built = false; c->sd_tab_valid = false; c->wn_tab_valid = false;
    c->tp_valid = false; c->mv_moved = false;  // another world: the temporal history (tirt_temporal.hip) and its snapshot of the vertex rows describe the old one
    if (upload(c->vertex, vertex, sizeof(float) * 9 * (size_t)nv, st)) return TIRT_ERR_HIP;
    if (upload(c->primitive, primitive, sizeof(int) * 3 * (size_t)n, st)) return TIRT_ERR_HIP;
    if (upload(c->material, material, sizeof(float) * 10 * (size_t)nm, st)) return TIRT_ERR_HIP;
    if (upload(c->shape, shape, sizeof(float) * 10 * (size_t)ns, st)) return TIRT_ERR_HIP;
    if (upload(c->light, light, sizeof(int) * (size_t)nl, st)) return TIRT_ERR_HIP;
    c->nv = nv; c->n = n; c->nm = nm; c->ns = ns; c->nl = nl; c->light_count = light_count; c->shade_rec_valid = false; c->light_rec_valid = false;
    for (int k = 0; k < 3; k++) { c->bmin[k] = bmin[k]; c->bmax[k] = bmax[k]; }
    if (refresh_material_table(c)) return TIRT_ERR_HIP;
    if (!c->env.p) {        // default: 1x1 black (Scene.py:295-296 loads image/black.png)
        int32_t z = 0;
        if (upload(c->env, &z, sizeof(int32_t), st)) return TIRT_ERR_HIP;
        c->env_w = 1; c->env_h = 1; c->env_power = 0.0f; c->env_lit = false; c->env_format = 0; c->env_emax = 0;
    }
    c->h_material.assign(material, material + (size_t)MAT_VEC * nm);
    light_kinds(primitive, shape, light, light_count, c->h_light_kind);
    refresh_shade_features(c);
    TIRT_HIP(hipStreamSynchronize(st));
    return TIRT_OK;
}

int tirt_material_upload(tirt_ctx *c, const float *material, int nm)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    TIRT_REQUIRE(material && nm == c->nm, "tirt_material_upload: material count differs from the uploaded scene");
    if (int rc = check_material_textures("tirt_material_upload", material, nm, c->tex_count)) return rc;
    if (upload(c->material, material, sizeof(float) * 10 * (size_t)nm, c->stream)) return TIRT_ERR_HIP;
    if (refresh_material_table(c)) return TIRT_ERR_HIP;
    c->light_rec_valid = false;                // the light records carry the emitters' colours
    c->shade_rec_valid = false;                // the shading records carry uvs iff a material is textured
    c->h_material.assign(material, material + (size_t)MAT_VEC * nm);
    refresh_shade_features(c);                 // (a material may have become glass, or stopped being it)
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_env_upload(tirt_ctx *c, const int32_t *rgb_packed, int w, int h, float power)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    TIRT_REQUIRE(rgb_packed && w >= 1 && h >= 1, "tirt_env_upload: bad image");
    if (upload(c->env, rgb_packed, sizeof(int32_t) * (size_t)w * h, c->stream)) return TIRT_ERR_HIP;
    c->env_w = w; c->env_h = h; c->env_power = power;
    c->env_format = 0; c->env_emax = 0;
    c->env_lit = env_is_lit(rgb_packed, (size_t)w * h, power);
    refresh_shade_features(c);
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return env_table_refresh(c);               // (tirt_env_sampling on: the table of the new image, or none)
}

// the same for RGBE8 texels (include/tirt.h, "HDR environment"): what needs no context first
int tirt_env_upload_hdr(tirt_ctx *c, const int32_t *rgbe_packed, int w, int h, float power)
{
    TIRT_REQUIRE(rgbe_packed && w >= 1 && h >= 1, "tirt_env_upload_hdr: bad image");
    int e_max = 0;
    if (int rc = env_hdr_check("tirt_env_upload_hdr", rgbe_packed, w, h, &e_max)) return rc;
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    if (upload(c->env, rgbe_packed, sizeof(int32_t) * (size_t)w * h, c->stream)) return TIRT_ERR_HIP;
    c->env_w = w; c->env_h = h; c->env_power = power;
    c->env_format = 1; c->env_emax = e_max;
    c->env_lit = env_is_lit(rgbe_packed, (size_t)w * h, power);      // the same rule: power != 0 or a mantissa that is not 0
    refresh_shade_features(c);
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return env_table_refresh(c);
}

int tirt_env_format(tirt_ctx *c, int32_t out[2])
{
    TIRT_REQUIRE(c, "null context");
    TIRT_REQUIRE(out, "tirt_env_format: null pointer");
    out[0] = c->env_format; out[1] = c->env_emax;
    return TIRT_OK;
}

int tirt_env_sampling(tirt_ctx *c, int on, float share)
{
    // what needs no context first
    TIRT_REQUIRE(on == 0 || on == 1, "tirt_env_sampling: on is 0 or 1");
    TIRT_REQUIRE(share > 0.0f && share < 1.0f, "tirt_env_sampling: share outside (0, 1)");
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // the kernels in flight read the share, and the texels the table may move
    const bool share_only = on == 1 && c->env_sample_on == 1 && c->env_tab_valid;
    c->env_sample_on = on; c->env_share = share;
    return share_only ? env_table_set_share(c) : env_table_refresh(c);
}

int tirt_env_table_download(tirt_ctx *c, uint32_t *q, uint64_t *row_sums, uint64_t *marginal, int32_t info[4])
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;
    return env_table_download(c, q, row_sums, marginal, info);
}

int tirt_light_sampling(tirt_ctx *c, int mode, float uniform_share)
{
    // what needs no context first
    TIRT_REQUIRE(mode == 0 || mode == 1, "tirt_light_sampling: mode is 0 (uniform) or 1 (power)");
    TIRT_REQUIRE(uniform_share >= 0.0f && uniform_share < 1.0f, "tirt_light_sampling: uniform_share outside [0, 1)");
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // the kernels in flight read the table's head and the emitters' spare words
    c->light_sample_mode = mode; c->light_uniform_share = uniform_share;
    c->light_tab_valid = false;                // rebuilt with the next render or query, as the light records are (ensure_shade_records)
    return TIRT_OK;
}

int tirt_light_table_download(tirt_ctx *c, uint32_t *q, uint64_t *prefix, float *P, int32_t info[4])
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;
    return light_table_download(c, q, prefix, P, info);
}

int tirt_kat_light_pick(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(in && out && n >= 0, "tirt_kat_light_pick: null pointer or negative n");
    TIRT_REQUIRE(in_stride >= 1 && out_stride >= 2, "tirt_kat_light_pick: stride too small (1 word in, 2 out)");
    CTX(c);
    return kat_light_pick(c, in, in_stride, out, out_stride, n);
}

// One buffer for all textures: `count` quads (offset in ints from the buffer's start, w, h, wrap), then the caller's texels.
int tirt_texture_upload(tirt_ctx *c, int count, const int32_t *texels, int64_t total, const int64_t *offset, const int32_t *w, const int32_t *h, const int32_t *wrap)
{
    // what needs no context first (and no device: these refusals hold for a null context too)
    TIRT_REQUIRE(count >= 0 && count <= (1 << 20), "tirt_texture_upload: count outside 0 .. 2^20");
    TIRT_REQUIRE(count == 0 || (texels && offset && w && h && wrap), "tirt_texture_upload: null pointer");
    TIRT_REQUIRE(total >= 0 && total < ((int64_t)1 << 31) - 4 * (int64_t)count, "tirt_texture_upload: total outside 0 .. 2^31 - 4 * count (texels are indexed by int)");
    std::vector<std::pair<int64_t, int64_t>> span((size_t)count);
    for (int i = 0; i < count; i++) {
        const std::string t = "tirt_texture_upload: texture " + std::to_string(i);
        TIRT_REQUIRE(w[i] >= 1 && h[i] >= 1, t + ": w and h must be >= 1");
        TIRT_REQUIRE(wrap[i] == 0 || wrap[i] == 1, t + ": wrap is 0 (clamp) or 1 (repeat)");
        const int64_t sz = (int64_t)w[i] * h[i];
        TIRT_REQUIRE(offset[i] >= 0 && offset[i] <= total && sz <= total - offset[i], t + ": its texels run past `total`");
        span[(size_t)i] = {offset[i], offset[i] + sz};
    }
    std::sort(span.begin(), span.end());
    for (int i = 1; i < count; i++) TIRT_REQUIRE(span[(size_t)i].first >= span[(size_t)i - 1].second, "tirt_texture_upload: two textures overlap");
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    if (!c->h_material.empty())
        if (int rc = check_material_textures("tirt_texture_upload", c->h_material.data(), c->nm, count)) return rc;
    if (count > 0) {
        std::vector<int32_t> table(4 * (size_t)count);
        for (int i = 0; i < count; i++) {
            table[4 * (size_t)i] = (int32_t)(4 * (int64_t)count + offset[i]); table[4 * (size_t)i + 1] = w[i];
            table[4 * (size_t)i + 2] = h[i]; table[4 * (size_t)i + 3] = wrap[i];
        }
        const size_t tb = sizeof(int32_t) * table.size(), xb = sizeof(int32_t) * (size_t)total;
        if (c->tex.ensure(tb + xb)) return TIRT_ERR_HIP;
        TIRT_HIP(hipMemcpyAsync(c->tex.p, table.data(), tb, hipMemcpyHostToDevice, c->stream));
        if (xb) TIRT_HIP(hipMemcpyAsync((char *)c->tex.p + tb, texels, xb, hipMemcpyHostToDevice, c->stream));
        TIRT_HIP(hipStreamSynchronize(c->stream));      // (table is a local)
    } else c->tex.release();
    c->tex_count = count;
    c->tex_cutout.clear();                     // no texture is a cut-out mask until tirt_texture_cutout says so
    c->shade_rec_valid = false;                // the shading records carry uvs iff a material is textured
    refresh_shade_features(c);
    return TIRT_OK;
}

int tirt_texture_cutout(tirt_ctx *c, const int32_t *flags, int count)
{
    // what needs no context first (and no device: these refusals hold for a null context too)
    TIRT_REQUIRE(count >= 0 && (count == 0 || flags), "tirt_texture_cutout: null pointer or negative count");
    for (int i = 0; i < count; i++) TIRT_REQUIRE(flags[i] == 0 || flags[i] == 1, "tirt_texture_cutout: flag " + std::to_string(i) + " is neither 0 nor 1");
    CTX(c);
    TIRT_REQUIRE(count == c->tex_count, "tirt_texture_cutout: count " + std::to_string(count) + " differs from the " + std::to_string(c->tex_count) + " uploaded textures");
    if (sync_all(c)) return TIRT_ERR_HIP;      // the tags must not change under batches still in flight
    c->tex_cutout.assign(flags, flags + count);
    c->pvb_valid = false;                      // the candidate lists of an opaque scene are not those of one with holes, and the other way round
    refresh_shade_features(c);
    return TIRT_OK;
}

int tirt_shade_features(tirt_ctx *c, uint32_t *out)
{
    TIRT_REQUIRE(c, "null context");
    TIRT_REQUIRE(out, "tirt_shade_features: null pointer");
    if (c->light_sample_mode == 1 && c->n >= 1 && !(c->shade_rec_valid && c->light_rec_valid && c->light_tab_valid)) {
        // bit 4096 needs the table's total: built here as a render would build it (whatever invalidated it has drained the work in flight)
        TIRT_HIP(hipSetDevice(c->device));
        if (sync_all(c) || ensure_shade_records(c)) return TIRT_ERR_HIP;
    }
    out[0] = shade_word(c) | (c->has_cutout ? (unsigned)SF_CUTOUT : 0u);
    out[1] = c->shade_specialize ? 1u : 0u;
    return TIRT_OK;
}

int tirt_shade_instantiation(uint32_t word, int specialize, int spectral, uint32_t *feat)
{
    TIRT_REQUIRE(feat, "tirt_shade_instantiation: null pointer");
    TIRT_REQUIRE((specialize == 0 || specialize == 1) && (spectral == 0 || spectral == 1), "tirt_shade_instantiation: specialize and spectral are 0 or 1");
    TIRT_REQUIRE(word < 8192u, "tirt_shade_instantiation: the word has bits at or above 8192");
    TIRT_REQUIRE(!spectral || (word & ~(unsigned)SF_ALL) == 0u, "tirt_shade_instantiation: PT_Spec renders no textured scene and never sees the derived bits: a spectral word lies within 127");
    unsigned f = 0;
    TIRT_REQUIRE(shade_instantiation(word, specialize, spectral != 0, &f), "tirt_shade_instantiation: no instantiation serves the word");
    *feat = f;
    return TIRT_OK;
}

int tirt_shade_features_host(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                             const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power, uint32_t *out)
{
    TIRT_REQUIRE(material && primitive && shape && out && nm >= 1 && n >= 1 && ns >= 1, "tirt_shade_features_host: null pointer or empty table");
    TIRT_REQUIRE(light_count >= 0 && (light_count == 0 || light), "tirt_shade_features_host: bad light list");
    for (int i = 0; i < light_count; i++) {
        TIRT_REQUIRE(light[i] >= 0 && light[i] < n, "tirt_shade_features_host: light index out of range");
        const int32_t *pr = primitive + (size_t)light[i] * 3;
        TIRT_REQUIRE(pr[0] == PRIMITIVE_TRI || (pr[1] >= 0 && pr[1] < ns), "tirt_shade_features_host: shape index out of range");
    }
    std::vector<int> kind;
    light_kinds(primitive, shape, light, light_count, kind);
    const bool lit = env ? env_is_lit(env, (size_t)(env_w > 0 ? env_w : 0) * (size_t)(env_h > 0 ? env_h : 0), env_power) : env_power != 0.0f;
    *out = shade_features_core(material, nm, kind.data(), light_count, lit);
    return TIRT_OK;
}
// the same with the switch of tirt_env_sampling as an input: bit 1024 where the context would report it (a table needs the image: env == NULL never sets it)
int tirt_shade_features_host_env(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                 const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power, int env_sampling, uint32_t *out)
{
    if (int rc = tirt_shade_features_host(material, nm, primitive, n, shape, ns, light, light_count, env, env_w, env_h, env_power, out)) return rc;
    if (env_sampling && (*out & SF_ENV) && env_table_exists_host(env, env_w, env_h, env_power)) *out |= SF_ENV_SAMPLE;
    return TIRT_OK;
}

// the same with the texel format as an input: env_format 0 is tirt_shade_features_host_env; env_format 1 reads RGBE8 texels -- the image is then required and
// checked as tirt_env_upload_hdr checks it --, sets bit 2048 where the environment is lit and bit 1024 by the RGBE8 table's rule
int tirt_shade_features_host_env_hdr(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                     const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power, int env_sampling, int env_format, uint32_t *out)
{
    TIRT_REQUIRE(env_format == 0 || env_format == 1, "tirt_shade_features_host_env_hdr: env_format is 0 (8 bits per channel) or 1 (RGBE8)");
    if (env_format == 0)
        return tirt_shade_features_host_env(material, nm, primitive, n, shape, ns, light, light_count, env, env_w, env_h, env_power, env_sampling, out);
    TIRT_REQUIRE(env && env_w >= 1 && env_h >= 1, "tirt_shade_features_host_env_hdr: bad image");
    int e_max = 0;
    if (int rc = env_hdr_check("tirt_shade_features_host_env_hdr", env, env_w, env_h, &e_max)) return rc;
    if (int rc = tirt_shade_features_host(material, nm, primitive, n, shape, ns, light, light_count, env, env_w, env_h, env_power, out)) return rc;
    if (*out & SF_ENV) *out |= SF_ENV_HDR;
    if (env_sampling && (*out & SF_ENV) && env_table_exists_host_hdr(env, env_w, env_h, env_power, e_max)) *out |= SF_ENV_SAMPLE;
    return TIRT_OK;
}

// the same with the mode of tirt_light_sampling as an input: bit 4096 where a context would report it (a triangle's weight needs the vertex rows)
int tirt_shade_features_host_lights(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                    const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power, int env_sampling, int env_format,
                                    const float *vertex, int nv, int light_sampling, uint32_t *out)
{
    TIRT_REQUIRE(light_sampling == 0 || light_sampling == 1, "tirt_shade_features_host_lights: light_sampling is 0 (uniform) or 1 (power)");
    if (int rc = tirt_shade_features_host_env_hdr(material, nm, primitive, n, shape, ns, light, light_count, env, env_w, env_h, env_power, env_sampling, env_format, out)) return rc;
    if (!light_sampling || light_count <= 0 || (*out & (SF_LIGHT_SPOT_LASER | SF_LIGHT_OTHER))) return TIRT_OK;
    TIRT_REQUIRE(nv >= 0 && (vertex || nv == 0), "tirt_shade_features_host_lights: bad vertex table");
    for (int i = 0; i < light_count; i++) {
        const int32_t *pr = primitive + (size_t)light[i] * 3;
        TIRT_REQUIRE(pr[2] >= 0 && pr[2] < nm, "tirt_shade_features_host_lights: material index out of range");
        TIRT_REQUIRE(pr[0] != PRIMITIVE_TRI || (pr[1] >= 0 && pr[1] + 2 < nv), "tirt_shade_features_host_lights: vertex index out of range");
    }
    if (light_table_exists_host(material, nm, primitive, n, shape, ns, vertex, nv, light, light_count)) *out |= SF_LIGHT_POWER;
    return TIRT_OK;
}

int tirt_lbvh_build(tirt_ctx *c)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    return lbvh_build(c);
}

#ifdef TIRT_EXPERIMENTS
int tirt_exp_download(tirt_ctx *c, int which, void *out, uint64_t bytes)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;
    DevBuf *b = which == 0 ? &c->tri : which == 1 ? &c->prim_slot : which == 2 ? &c->leaf_compact : which == 3 ? &c->cnode : which == 5 ? &c->bd[0].qidx : &c->cparent;
    TIRT_REQUIRE(bytes <= b->bytes, "tirt_exp_download: too many bytes");
    TIRT_HIP(hipMemcpy(out, b->p, bytes, hipMemcpyDeviceToHost));
    return TIRT_OK;
}
int tirt_exp_wide_from_tree(tirt_ctx *c, const float *compact_host, const int32_t *csize_host)
{
    CTX(c);
    TIRT_REQUIRE(c->built && c->n >= 2, "tirt_exp_wide_from_tree: LBVH not built");
    if (sync_all(c)) return TIRT_ERR_HIP;
    return exp_wide_from_tree(c, compact_host, csize_host);
}
#endif

int tirt_lbvh_download(tirt_ctx *c, int32_t *morton_sorted, float *bvh_node, float *compact_node)
{
    CTX(c);
    TIRT_REQUIRE(c->built, "tirt_lbvh_download: LBVH not built");
    const size_t n = c->n, N = 2 * n - 1;
    if (morton_sorted) TIRT_HIP(hipMemcpyAsync(morton_sorted, c->morton_sorted.p, sizeof(int) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    if (bvh_node) TIRT_HIP(hipMemcpyAsync(bvh_node, c->bvh_node.p, sizeof(float) * NOD_VEC * N, hipMemcpyDeviceToHost, c->stream));
    if (compact_node) TIRT_HIP(hipMemcpyAsync(compact_node, c->compact.p, sizeof(float) * CPN_VEC * N, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_traversal_tree_download(tirt_ctx *c, float *rows)
{
    CTX(c);
    TIRT_REQUIRE(c->built && rows, "tirt_traversal_tree_download: LBVH not built / null pointer");
    const size_t N = 2 * (size_t)c->n - 1;
    const bool sah = c->built_sah != 0;
    TIRT_HIP(hipMemcpyAsync(rows, sah ? c->sah_compact.p : c->compact.p, sizeof(float) * N * CPN_VEC, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_wide_tree_download(tirt_ctx *c, uint32_t *cnode, float *tri, float *wnode, int32_t *prim_slot, float grid[19], int32_t info[6])
{
    CTX(c);
    TIRT_REQUIRE(c->built && grid && info, "tirt_wide_tree_download: LBVH not built / null pointer");
    if (int rc = ensure_cutout_records(c)) return rc;      // (the records' tag words as the next trace would see them)
    const size_t n = c->n, N = 2 * n - 1, nodes = (size_t)c->wide_nodes + (size_t)c->n_far_nodes;
    if (cnode && nodes) TIRT_HIP(hipMemcpyAsync(cnode, c->cnode.p, 64 * nodes, hipMemcpyDeviceToHost, c->stream));
    if (tri) TIRT_HIP(hipMemcpyAsync(tri, c->tri.p, sizeof(float4) * TRI_STRIDE * n, hipMemcpyDeviceToHost, c->stream));
    if (wnode) TIRT_HIP(hipMemcpyAsync(wnode, c->wnode.p, sizeof(float4) * 4 * N, hipMemcpyDeviceToHost, c->stream));
    if (prim_slot) TIRT_HIP(hipMemcpyAsync(prim_slot, c->prim_slot.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    const BvhView b = bvh_view(c);
    for (int k = 0; k < 3; k++) {
        grid[k] = b.grid_min[k]; grid[3 + k] = b.cell[k]; grid[6 + k] = b.inv_cell[k]; grid[9 + k] = b.inv_extent[k];
        grid[12 + k] = b.root_min[k]; grid[15 + k] = b.root_max[k];
    }
    grid[18] = c->wide_pad;
    info[0] = c->wide_nodes; info[1] = c->n_far_nodes; info[2] = b.root_code; info[3] = b.far_qcode; info[4] = c->built_sah; info[5] = c->shapes_boxed;
    return TIRT_OK;
}

int tirt_morton_download(tirt_ctx *c, int32_t *out)
{
    CTX(c);
    TIRT_REQUIRE(c->built && out, "tirt_morton_download: LBVH not built");
    TIRT_HIP(hipMemcpyAsync(out, c->morton_unsorted.p, sizeof(int) * 2 * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_process_normal(tirt_ctx *c, const int32_t *vertex_index)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;      // scene data must not change under batches still in flight
    TIRT_REQUIRE(c->built && vertex_index, "tirt_process_normal: LBVH not built");
    if (c->nv == 0) return TIRT_OK;
    for (int i = 0; i < c->nv; i++) TIRT_REQUIRE(vertex_index[i] >= 0 && vertex_index[i] < c->n, "tirt_process_normal: vertex_index out of range");
    DevBuf vi, smooth;
    if (upload(vi, vertex_index, sizeof(int) * (size_t)c->nv, c->stream)) return TIRT_ERR_HIP;
    if (smooth.ensure(sizeof(float) * 3 * (size_t)c->nv)) { vi.release(); return TIRT_ERR_HIP; }
    const int B = 128, G = (c->nv + B - 1) / B;
    hipLaunchKernelGGL(k_smooth_normal, dim3(G), dim3(B), 0, c->stream, scene_view(c), c->nv, c->compact.as<float>(), vi.as<int>(), smooth.as<float>());
    hipLaunchKernelGGL(k_write_normal, dim3(G), dim3(B), 0, c->stream, c->vertex.as<float>(), c->nv, smooth.as<float>());
    c->shade_rec_valid = false; c->light_rec_valid = false;
    hipError_t e = hipStreamSynchronize(c->stream);
    vi.release(); smooth.release();
    TIRT_HIP(e);
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int tirt_vertex_download(tirt_ctx *c, float *vertex)
{
    CTX(c);
    TIRT_REQUIRE(vertex, "tirt_vertex_download: null");
    TIRT_HIP(hipMemcpyAsync(vertex, c->vertex.p, sizeof(float) * 9 * (size_t)c->nv, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_total_area(tirt_ctx *c, float *out)
{
    CTX(c);
    TIRT_REQUIRE(out && c->n >= 1, "tirt_total_area: no scene");
    DevBuf d;
    if (d.ensure(sizeof(float))) return TIRT_ERR_HIP;
    int cnt = c->light_count > 0 ? c->light_count : 1;      // the light field always has >= 1 entry (Scene.py:258-261)
    hipLaunchKernelGGL(k_total_area, dim3(1), dim3(64), 0, c->stream, scene_view(c), cnt, d.as<float>());
    hipError_t e = hipMemcpyAsync(out, d.p, sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    TIRT_HIP(e);
    return TIRT_OK;
}

int tirt_camera_set(tirt_ctx *c, const float view[16], const float view_inv[16], const float eye[3], float fx, float fy, float cx, float cy)
{
    CTX(c);
    TIRT_REQUIRE(view && view_inv && eye, "tirt_camera_set: null");
    memcpy(c->view, view, sizeof(float) * 16);
    memcpy(c->cam.view_inv, view_inv, sizeof(float) * 12);
    memcpy(c->cam.eye, eye, sizeof(float) * 3);
    c->cam.fx = fx; c->cam.fy = fy; c->cam.cx = cx; c->cam.cy = cy;
    c->cam_set = true;
    return TIRT_OK;
}

// ---- the per-pixel buffers beside the film: `words` f32 per pixel, pixel p = i * H + j as hdr ----
enum RecordOrder { ORDER_NONE, ORDER_RENDER, ORDER_AOV };      // what a main-stream reader waits for: nothing, last_film, last_aov
struct FilmRecord { tirt::DevBuf tirt_ctx::*buf; int words; const char *missing; RecordOrder order; };
enum { REC_AOV, REC_MOM, REC_DENOISED };
static const FilmRecord RECORDS[3] = {
    {&tirt_ctx::aov, TIRT_AOV_WORDS, "feature buffers not enabled (tirt_aov_enable)", ORDER_AOV},
    {&tirt_ctx::mom, TIRT_MOM_WORDS, "moment buffers not enabled (tirt_moments_enable)", ORDER_RENDER},
    {&tirt_ctx::dn_out, 3, "nothing filtered yet (tirt_denoise)", ORDER_NONE},      // written by the filter on the main stream itself
};

static size_t record_bytes(const tirt_ctx *c, const FilmRecord &r) { return sizeof(float) * r.words * (size_t)c->W * c->H; }

// tirt_*_enable: on != 0 allocates and zeroes the record, on == 0 frees it
static int record_enable(tirt_ctx *c, const FilmRecord &r, int on, const char *fn)
{
    TIRT_REQUIRE(c->hdr.p, std::string(fn) + ": film not created");
    TIRT_REQUIRE(on || !c->tp_mem.p, std::string(fn) + ": temporal accumulation is on and needs these records (tirt_temporal_enable(0) first)");
    if (sync_all(c)) return TIRT_ERR_HIP;      // no kernel of the render in flight while the records come or go
    if (r.order == ORDER_AOV) c->last_aov = nullptr;
    if (!on) { (c->*r.buf).release(); return TIRT_OK; }
    if ((c->*r.buf).ensure(record_bytes(c, r))) return TIRT_ERR_HIP;
    TIRT_HIP(hipMemsetAsync((c->*r.buf).p, 0, record_bytes(c, r), c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

// tirt_*_download (kind = hipMemcpyDeviceToHost) and tirt_*_export_device (hipMemcpyDeviceToDevice): the whole record, and wait for it
static int record_copy_out(tirt_ctx *c, const FilmRecord &r, void *dst, hipMemcpyKind kind, const char *fn)
{
    if (r.order == ORDER_RENDER) AFTER_RENDER(c);
    if (r.order == ORDER_AOV) AFTER_AOV(c);
    TIRT_REQUIRE(c->hdr.p, std::string(fn) + ": film not created");
    TIRT_REQUIRE((c->*r.buf).p, std::string(fn) + ": " + r.missing);
    TIRT_REQUIRE(dst, std::string(fn) + ": null pointer");
    TIRT_HIP(hipMemcpyAsync(dst, (c->*r.buf).p, record_bytes(c, r), kind, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_film_create(tirt_ctx *c, int W, int H, int tile_rank, int tile_count, int tile_size)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 30), "tirt_film_create: bad size");
    TIRT_REQUIRE(tile_count >= 1 && tile_rank >= 0 && tile_rank < tile_count && tile_size >= 1, "tirt_film_create: bad tiling");
    const long NP = (long)W * H;
    if (c->pixset_n >= 0) {                      // a pixel set is a list of THIS film's pixels: it goes with the film
        if (sync_all(c)) return TIRT_ERR_HIP;
        c->pixset_n = -1;
    }
    for (const FilmRecord &r : RECORDS)          // the records the render writes belong to the film: a new film starts without them
        if (r.order != ORDER_NONE && (c->*r.buf).p) {
            if (sync_all(c)) return TIRT_ERR_HIP;
            (c->*r.buf).release();
            if (r.order == ORDER_AOV) c->last_aov = nullptr;
        }
    if (c->dn_mem.p || c->dn_out.p || c->tp_mem.p) {      // so do the denoiser's buffer and its scratch and the temporal history; a filter or an accumulation may still be queued on the main stream
        TIRT_HIP(hipStreamSynchronize(c->stream));
        c->dn_mem.release(); c->dn_out.release();
        c->tp_mem.release(); c->tp_valid = false;
        c->mv_rec.release(); c->mv_snap.release(); c->mv_moved = false; c->mv_rec_valid = false;
    }
    if (c->hdr.ensure(sizeof(float) * 3 * (size_t)NP) || c->rgb.ensure(sizeof(float) * 3 * (size_t)NP)) return TIRT_ERR_HIP;
    c->W = W; c->H = H; c->tile_rank = tile_rank; c->tile_count = tile_count; c->tile_size = tile_size;
    c->tile_blocked = (H % 8 == 0 && tile_size % (8 * H) == 0 && ((long)W * H) % tile_size == 0) ? 1 : 0;       // local_to_pixel
    long ntiles = (NP + tile_size - 1) / tile_size, local = 0;
    for (long t = tile_rank; t < ntiles; t += tile_count) {
        long beg = t * tile_size, end = beg + tile_size; if (end > NP) end = NP;
        local += end - beg;
    }
    c->npix_local = local;
    c->bdpt_px.release();                        // BDPT vertex arrays belong to the film: start from zeros
    TIRT_HIP(hipMemsetAsync(c->hdr.p, 0, sizeof(float) * 3 * (size_t)NP, c->stream));
    TIRT_HIP(hipMemsetAsync(c->rgb.p, 0, sizeof(float) * 3 * (size_t)NP, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_film_clear(tirt_ctx *c)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p, "tirt_film_clear: film not created");
    if (c->bdpt_px.p) TIRT_HIP(hipMemsetAsync(c->bdpt_px.p, 0, c->bdpt_px.bytes, c->stream));
    TIRT_HIP(hipMemsetAsync(c->hdr.p, 0, sizeof(float) * 3 * (size_t)c->W * c->H, c->stream));
    TIRT_HIP(hipMemsetAsync(c->rgb.p, 0, sizeof(float) * 3 * (size_t)c->W * c->H, c->stream));
    for (const FilmRecord &r : RECORDS)          // (the denoiser's buffer stays; k_moments lies before last_film)
        if (r.order != ORDER_NONE && (c->*r.buf).p) {
            if (r.order == ORDER_AOV) AFTER_AOV(c);
            TIRT_HIP(hipMemsetAsync((c->*r.buf).p, 0, record_bytes(c, r), c->stream));
        }
    return TIRT_OK;
}

int tirt_aov_enable(tirt_ctx *c, int on) { CTX(c); return record_enable(c, RECORDS[REC_AOV], on, "tirt_aov_enable"); }
int tirt_aov_download(tirt_ctx *c, float *out) { CTX(c); return record_copy_out(c, RECORDS[REC_AOV], out, hipMemcpyDeviceToHost, "tirt_aov_download"); }
int tirt_aov_export_device(tirt_ctx *c, void *dev_dst) { CTX(c); return record_copy_out(c, RECORDS[REC_AOV], dev_dst, hipMemcpyDeviceToDevice, "tirt_aov_export_device"); }

// ---- sample moments (tirt_moments.hip).  Their last update lies before last_film: ORDER_RENDER orders the main stream after it ----
int tirt_moments_enable(tirt_ctx *c, int on) { CTX(c); return record_enable(c, RECORDS[REC_MOM], on, "tirt_moments_enable"); }
int tirt_moments_download(tirt_ctx *c, float *out) { CTX(c); return record_copy_out(c, RECORDS[REC_MOM], out, hipMemcpyDeviceToHost, "tirt_moments_download"); }
int tirt_moments_export_device(tirt_ctx *c, void *dev_dst) { CTX(c); return record_copy_out(c, RECORDS[REC_MOM], dev_dst, hipMemcpyDeviceToDevice, "tirt_moments_export_device"); }

int tirt_moments_converged(tirt_ctx *c, float threshold, uint64_t out[3])
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p, "tirt_moments_converged: film not created");
    TIRT_REQUIRE(c->mom.p, "tirt_moments_converged: moment buffers not enabled (tirt_moments_enable)");
    TIRT_REQUIRE(out, "tirt_moments_converged: null pointer");
    TIRT_REQUIRE(threshold > 0.0f, "tirt_moments_converged: threshold must be > 0 (and not NaN)");
    return moments_converged(c, threshold * threshold, out);
}

// ---- pixel set and adaptive sampling (tirt_adaptive.hip).  Every entry point waits for pending work before it touches the list ----
#define NO_PIXEL_SET(c, fn)                                                        \
    TIRT_REQUIRE((c)->pixset_n < 0, std::string(fn) + ": a pixel set is installed (it restricts tirt_pt_rgb_render alone): tirt_pixel_set_clear first")

static int select_args(tirt_ctx *c, const char *fn, float threshold, int min_samples, int max_samples)
{
    TIRT_REQUIRE(c->hdr.p, std::string(fn) + ": film not created");
    TIRT_REQUIRE(c->mom.p, std::string(fn) + ": moment buffers not enabled (tirt_moments_enable)");
    TIRT_REQUIRE(threshold >= 0.0f && threshold < __builtin_inff(), std::string(fn) + ": threshold must be finite and >= 0");
    TIRT_REQUIRE(min_samples >= 1, std::string(fn) + ": min_samples must be >= 1");
    TIRT_REQUIRE(max_samples >= min_samples && max_samples <= (1 << 24), std::string(fn) + ": max_samples must be >= min_samples (and <= 2^24, where the f32 count stops being exact)");
    return TIRT_OK;
}

int tirt_pixel_set_upload(tirt_ctx *c, const int32_t *pixels, int64_t n) { CTX(c); return pixel_set_upload(c, pixels, n); }
int tirt_pixel_set_clear(tirt_ctx *c) { CTX(c); return pixel_set_clear(c); }

int tirt_pixel_set_from_moments(tirt_ctx *c, float threshold, int min_samples, int max_samples, int64_t *count)
{
    CTX(c);
    if (int rc = select_args(c, "tirt_pixel_set_from_moments", threshold, min_samples, max_samples)) return rc;
    return pixel_set_select(c, threshold * threshold, min_samples, max_samples, -1, count, nullptr);
}

int tirt_pixel_set_download(tirt_ctx *c, int32_t *out, int64_t cap, int64_t *n)
{
    CTX(c);
    TIRT_REQUIRE(n && cap >= 0, "tirt_pixel_set_download: null count or negative capacity");
    TIRT_REQUIRE(!out || cap >= c->pixset_n, "tirt_pixel_set_download: the list has " + std::to_string(c->pixset_n) + " entries, more than the capacity");
    *n = c->pixset_n < 0 ? -1 : (int64_t)c->pixset_n;
    if (out && c->pixset_n > 0) {
        if (sync_all(c)) return TIRT_ERR_HIP;
        TIRT_HIP(hipMemcpy(out, c->pixset.p, sizeof(int32_t) * (size_t)c->pixset_n, hipMemcpyDeviceToHost));
    }
    return TIRT_OK;
}

int tirt_pt_rgb_render_adaptive(tirt_ctx *c, uint32_t frame_begin, uint32_t seed, int max_depth, int stack_size, int flags, const tirt_adaptive_t *a,
                                tirt_adaptive_result_t *out)
{
    CTX(c);
    TIRT_REQUIRE(a, "tirt_pt_rgb_render_adaptive: null parameters");
    NO_PIXEL_SET(c, "tirt_pt_rgb_render_adaptive");
    if (int rc = select_args(c, "tirt_pt_rgb_render_adaptive", a->threshold, a->min_samples, a->max_samples)) return rc;
    TIRT_REQUIRE(a->pass_frames >= 1, "tirt_pt_rgb_render_adaptive: pass_frames must be >= 1");
    TIRT_REQUIRE(c->built && c->cam_set, "tirt_pt_rgb_render_adaptive: LBVH not built or camera not set");
    TIRT_REQUIRE(max_depth >= 1 && max_depth <= 4096, "tirt_pt_rgb_render_adaptive: bad max_depth");
    TIRT_REQUIRE((uint64_t)frame_begin + (uint64_t)a->max_samples < ((uint64_t)1 << 31), "tirt_pt_rgb_render_adaptive: frame_begin + max_samples must stay below 2^31");
    return render_adaptive(c, frame_begin, seed, max_depth, stack_size, flags, a, out);
}

// ---- denoiser (tirt_denoise.hip): the film routes wait for the last film update (which covers the moments) and the last k_aov ----
static int denoise_entry(tirt_ctx *c, const tirt_denoise_t *params, bool var)
{
    CTX(c);
    AFTER_RENDER(c);
    AFTER_AOV(c);
    return denoise_film(c, params, var);
}
int tirt_denoise(tirt_ctx *c, const tirt_denoise_t *params) { return denoise_entry(c, params, false); }
int tirt_denoise_var(tirt_ctx *c, const tirt_denoise_var_t *params) { return denoise_entry(c, params, true); }

int tirt_denoise_device(tirt_ctx *c, const float *hdr, const float *aov, float *out, int W, int H, const tirt_denoise_t *params, void *stream)
{
    CTX(c);
    return denoise_device(c, false, hdr, aov, nullptr, out, W, H, params, stream);
}

int tirt_denoise_var_device(tirt_ctx *c, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_var_t *params, void *stream)
{
    CTX(c);
    return denoise_device(c, true, hdr, aov, mom, out, W, H, params, stream);
}

int tirt_denoise_download(tirt_ctx *c, float *out)
{
    CTX(c);
    if (int rc = record_copy_out(c, RECORDS[REC_DENOISED], out, hipMemcpyDeviceToHost, "tirt_denoise_download")) return rc;
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}
int tirt_denoise_export_device(tirt_ctx *c, void *dev_dst) { CTX(c); return record_copy_out(c, RECORDS[REC_DENOISED], dev_dst, hipMemcpyDeviceToDevice, "tirt_denoise_export_device"); }

// ---- temporal accumulation (tirt_temporal.hip): what reads the film and the records waits as the denoiser does ----
int tirt_temporal_device(tirt_ctx *c, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                         const tirt_temporal_camera_t *cur, const tirt_temporal_camera_t *prev, float *hdr_o, float *mom_o, int W, int H,
                         const tirt_temporal_t *params, void *stream)
{
    CTX(c);
    return temporal_device(c, hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cur, prev, hdr_o, mom_o, W, H, params, nullptr, stream);
}
int tirt_motion_temporal_device(tirt_ctx *c, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                            const tirt_temporal_camera_t *cur, const tirt_temporal_camera_t *prev, float *hdr_o, float *mom_o, int W, int H,
                            const tirt_temporal_t *params, const float *motion, void *stream)
{
    CTX(c);
    TIRT_REQUIRE(motion, "tirt_motion_temporal_device: null pointer");
    return temporal_device(c, hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cur, prev, hdr_o, mom_o, W, H, params, motion, stream);
}
int tirt_temporal_enable(tirt_ctx *c, int on) { CTX(c); return temporal_enable(c, on); }
int tirt_temporal_accumulate(tirt_ctx *c, const tirt_temporal_t *params)
{
    CTX(c);
    AFTER_RENDER(c);
    AFTER_AOV(c);
    return temporal_accumulate(c, params);
}
int tirt_temporal_reset(tirt_ctx *c)
{
    CTX(c);
    TIRT_REQUIRE(c->tp_mem.p, "tirt_temporal_reset: temporal accumulation not enabled (tirt_temporal_enable)");
    c->tp_valid = false; c->mv_moved = false;
    return TIRT_OK;
}
int tirt_motion_enable(tirt_ctx *c, int on) { CTX(c); return motion_enable(c, on); }
int tirt_motion_download(tirt_ctx *c, float *out) { CTX(c); return motion_copy_out(c, "tirt_motion_download", out, hipMemcpyDeviceToHost); }
int tirt_motion_export_device(tirt_ctx *c, void *dev_dst) { CTX(c); return motion_copy_out(c, "tirt_motion_export_device", dev_dst, hipMemcpyDeviceToDevice); }
int tirt_temporal_download(tirt_ctx *c, float *hdr_out, float *mom_out) { CTX(c); return temporal_copy_out(c, "tirt_temporal_download", hdr_out, mom_out, hipMemcpyDeviceToHost); }
int tirt_temporal_export_device(tirt_ctx *c, void *hdr_dst, void *mom_dst) { CTX(c); return temporal_copy_out(c, "tirt_temporal_export_device", hdr_dst, mom_dst, hipMemcpyDeviceToDevice); }
int tirt_temporal_denoise_var(tirt_ctx *c, const tirt_denoise_var_t *params) { CTX(c); return temporal_denoise_var(c, params); }

static int submit_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed, int max_depth, int stack_size, int flags, bool spectral)
{
    TIRT_REQUIRE(c->built, "render: LBVH not built");
    TIRT_REQUIRE(c->cam_set, "render: camera not set");
    TIRT_REQUIRE(c->hdr.p && c->npix_local >= 0, "render: film not created");
    TIRT_REQUIRE(frame_count >= 0 && max_depth >= 1 && max_depth <= 4096, "render: bad frame_count/max_depth");
    if (spectral) NO_PIXEL_SET(c, "tirt_pt_spec_render");
    if (frame_count == 0 || c->pixset_n == 0) return TIRT_OK;      // (an empty pixel set: nothing to render)
    auto &p = c->pend;
    if (p.valid && p.begin + (uint32_t)p.count == frame_begin && p.seed == seed && p.max_depth == max_depth &&
        p.stack_size == stack_size && p.flags == flags && p.spectral == spectral) {
        p.count += frame_count;
    } else {
        if (int rc = flush_pending(c)) return rc;
        p.valid = true; p.begin = frame_begin; p.count = frame_count; p.seed = seed;
        p.max_depth = max_depth; p.stack_size = stack_size; p.flags = flags; p.spectral = spectral;
    }
    const int P = render_pixels(c);
    if ((size_t)p.count * (size_t)(P > 0 ? P : 1) >= effective_merge_paths(c)) return flush_pending(c);
    return TIRT_OK;
}
// albedo textures are PT_RGB's (and the feature buffers', Debug's): the other integrators refuse a textured scene instead of rendering it flat
#define NO_TEXTURES(c, fn)                                                         \
    TIRT_REQUIRE(!((c)->shade_features & SF_TEXTURE), std::string(fn) + ": a material of the scene has an albedo texture (PT_RGB only): tirt_texture_upload with count 0 removes all textures"); \
    TIRT_REQUIRE(!((c)->shade_features & SF_TEXTURE_PARAM), std::string(fn) + ": a material of the scene has a roughness, metallic or normal-map texture (PT_RGB only): tirt_texture_upload with count 0 removes all textures")
int tirt_pt_rgb_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed, int max_depth, int stack_size, int flags)
{
    CTX_NOFLUSH(c);
    return submit_render(c, frame_begin, frame_count, seed, max_depth, stack_size, flags, false);
}
int tirt_pt_spec_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed, int max_depth, int stack_size, int flags)
{
    CTX_NOFLUSH(c);
    TIRT_REQUIRE(c->spec_set && c->spec_view, "tirt_pt_spec_render: spectral tables not uploaded (tirt_spectral_upload)");
    NO_TEXTURES(c, "tirt_pt_spec_render");
    return submit_render(c, frame_begin, frame_count, seed, max_depth, stack_size, flags, true);
}

int tirt_bdpt_rgb_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed)
{
    CTX(c);
    NO_PIXEL_SET(c, "tirt_bdpt_rgb_render");
    NO_TEXTURES(c, "tirt_bdpt_rgb_render");
    return bdpt_render(c, frame_begin, frame_count, seed);
}
int tirt_bdpt_spec_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed)
{
    CTX(c);
    NO_PIXEL_SET(c, "tirt_bdpt_spec_render");
    NO_TEXTURES(c, "tirt_bdpt_spec_render");
    TIRT_REQUIRE(c->spec_set && c->spec_dev.p, "tirt_bdpt_spec_render: spectral tables not uploaded (tirt_spectral_upload)");
    return bdpt_render(c, frame_begin, frame_count, seed, true);
}

int tirt_debug_render(tirt_ctx *c, uint32_t frame, uint32_t seed, int mode, int stack_size, int flags)
{
    CTX(c);
    NO_PIXEL_SET(c, "tirt_debug_render");
    AFTER_RENDER(c);                 // the view overwrites pixels the lanes' last film update may still be writing
    return debug_render(c, frame, seed, mode, stack_size, flags);
}

int tirt_tone_map(tirt_ctx *c, float exposure)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p, "tirt_tone_map: film not created");
    long nvals = 3l * c->W * c->H;
    hipLaunchKernelGGL(k_tone_map, dim3((unsigned)((nvals + 255) / 256)), dim3(256), 0, c->stream, c->hdr.as<float>(), c->rgb.as<float>(), nvals, exposure);
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int tirt_film_download(tirt_ctx *c, float *hdr, float *rgb)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p, "tirt_film_download: film not created");
    size_t bytes = sizeof(float) * 3 * (size_t)c->W * c->H;
    if (hdr) TIRT_HIP(hipMemcpyAsync(hdr, c->hdr.p, bytes, hipMemcpyDeviceToHost, c->stream));
    if (rgb) TIRT_HIP(hipMemcpyAsync(rgb, c->rgb.p, bytes, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int tirt_film_export_device(tirt_ctx *c, void *dev_dst)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p && dev_dst, "tirt_film_export_device: film not created");
    TIRT_HIP(hipMemcpyAsync(dev_dst, c->hdr.p, sizeof(float) * 3 * (size_t)c->W * c->H, hipMemcpyDeviceToDevice, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_film_import_device(tirt_ctx *c, const void *dev_src)
{
    CTX(c);
    AFTER_RENDER(c);
    TIRT_REQUIRE(c->hdr.p && dev_src, "tirt_film_import_device: film not created");
    TIRT_HIP(hipMemcpyAsync(c->hdr.p, dev_src, sizeof(float) * 3 * (size_t)c->W * c->H, hipMemcpyDeviceToDevice, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

int tirt_trace_closest(tirt_ctx *c, const float *rays, int nr, int stack_size, int flags, float *out_hit, int32_t *out_prim, int32_t *counts)
{
    CTX(c);
    TIRT_REQUIRE(rays && out_hit && out_prim, "tirt_trace_closest: null");
    return trace_host(c, rays, nr, stack_size, flags, false, out_hit, out_prim, counts);
}

int tirt_trace_shadow(tirt_ctx *c, const float *rays, int nr, int stack_size, int flags, float *out_t, int32_t *out_prim, int32_t *counts)
{
    CTX(c);
    TIRT_REQUIRE(rays && out_t && out_prim, "tirt_trace_shadow: null");
    return trace_host(c, rays, nr, stack_size, flags, true, out_t, out_prim, counts);
}

int tirt_query_closest(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, int stack_size, int flags,
                       float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *counts, void *stream)
{
    CTX(c);
    return query_closest(c, rays, nr, ray_stride, stack_size, flags, out_t, out_prim, out_hit, hit_stride, counts, stream);
}

int tirt_query_occluded(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, const float *tmax, int64_t tmax_stride, float tmax_all,
                        int stack_size, int flags, uint8_t *out_occluded, void *stream)
{
    CTX(c);
    return query_occluded(c, rays, nr, ray_stride, tmax, tmax_stride, tmax_all, stack_size, flags, out_occluded, stream);
}

// (the checks of k need no context: they come first)
#define HITS_K_CHECKS(fn)                                                                                     \
    TIRT_REQUIRE(k >= 0 && k <= TIRT_HITS_MAX, fn ": k outside 0..TIRT_HITS_MAX (64)");                       \
    TIRT_REQUIRE(k > 0 || out_count, fn ": k == 0 without out_count (nothing to return)")
int tirt_query_hits(tirt_ctx *c, const float *rays, int64_t nr, int64_t ray_stride, const float *tmax, int64_t tmax_stride, float tmax_all, int k,
                    int stack_size, int flags, float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *out_count, int32_t *counts,
                    void *stream)
{
    HITS_K_CHECKS("tirt_query_hits");
    CTX(c);
    return query_hits(c, rays, nr, ray_stride, tmax, tmax_stride, tmax_all, k, stack_size, flags, out_t, out_prim, out_hit, hit_stride, out_count, counts, stream);
}

int tirt_trace_hits(tirt_ctx *c, const float *rays, int nr, const float *tmax, int k, int stack_size, int flags, float *out_t, int32_t *out_prim,
                    float *out_hit, int32_t *out_count, int32_t *counts)
{
    HITS_K_CHECKS("tirt_trace_hits");
    CTX(c);
    return trace_hits_host(c, rays, nr, tmax, k, stack_size, flags, out_t, out_prim, out_hit, out_count, counts);
}
#undef HITS_K_CHECKS

// host only, no context: candidates (t, u, v, bits leaf) in the order given through MhList (tirt_multi_hit.h), the text k_multi_hit runs
int tirt_kat_hit_list(const float *cand, int n, int k, float bound, float *out_list, int32_t *out_info)
{
    TIRT_REQUIRE(cand && out_info && n >= 0, "tirt_kat_hit_list: null pointer or negative n");
    TIRT_REQUIRE(k >= 0 && k <= TIRT_HITS_MAX && (k == 0 || out_list), "tirt_kat_hit_list: k outside 0..TIRT_HITS_MAX (64), or no out_list");
    struct HostList {
        float *p;
        MhEntry get(int e) const { MhEntry r; r.t = p[4 * e]; r.u = p[4 * e + 1]; r.v = p[4 * e + 2]; memcpy(&r.leaf, p + 4 * e + 3, 4); return r; }
        void set(int e, const MhEntry c) { p[4 * e] = c.t; p[4 * e + 1] = c.u; p[4 * e + 2] = c.v; memcpy(p + 4 * e + 3, &c.leaf, 4); }
    } list = {out_list};
    const float B = bound < INF_VALUE ? bound : INF_VALUE;
    MhList L(k, B);
    int accepted = 0;
    for (int i = 0; i < n; i++) {
        MhEntry c; c.t = cand[4 * i]; c.u = cand[4 * i + 1]; c.v = cand[4 * i + 2]; memcpy(&c.leaf, cand + 4 * i + 3, 4);
        TIRT_REQUIRE(c.leaf >= 0, "tirt_kat_hit_list: a candidate's leaf index is negative");
        if (!(bound > 0.0f)) continue;                                     // tmax <= 0 or NaN finds nothing
        if ((c.t > 0.0f) & hit_before(c.t, c.leaf, B, -1)) accepted++;      // membership of H: trace_leaf_step against (B, -1)
        if (L.wants(c.t, c.leaf)) L.insert(list, c);
    }
    out_info[0] = L.n; out_info[1] = accepted; memcpy(&out_info[2], &L.thr_t, 4); out_info[3] = L.thr_leaf;
    return TIRT_OK;
}

int tirt_bvh_info(tirt_ctx *c, uint64_t out[4])
{
    CTX(c);
    TIRT_REQUIRE(out && c->built, "tirt_bvh_info: LBVH not built");
    const int nq = c->wide_nodes + c->n_far_nodes;      // the chain nodes of far-origin rays are walked, and kept in LDS, like any other (bvh_view: top_count)
    out[0] = (uint64_t)nq * 64u; out[1] = (uint64_t)c->n * sizeof(float4) * TRI_STRIDE; out[2] = (uint64_t)nq;
    const int top = TR_TOP_SLOTS;
    out[3] = (uint64_t)(nq < top ? nq : top);
    return TIRT_OK;
}

int tirt_micro_gather_rate(tirt_ctx *c, uint64_t working_set_bytes, int iters, double *gbps_out)
{
    CTX(c);
    if (sync_all(c)) return TIRT_ERR_HIP;
    TIRT_REQUIRE(gbps_out && iters >= 1 && working_set_bytes >= 64 && working_set_bytes <= ((uint64_t)1 << 36), "tirt_micro_gather_rate: bad arguments");
    const uint32_t nrec = (uint32_t)(working_set_bytes / 64);
    const int blocks = 1536;
    DevBuf rec, out;
    if (rec.ensure((size_t)nrec * 64) || out.ensure(sizeof(float) * blocks * 256)) { rec.release(); out.release(); return TIRT_ERR_HIP; }
    hipError_t e = hipMemsetAsync(rec.p, 0, (size_t)nrec * 64, c->stream);
    float best = 1.0e30f;
    for (int rep = 0; rep < 4 && e == hipSuccess; rep++) {          // first launch warms the caches
        (void)hipEventRecord(c->ev0, c->stream);
        hipLaunchKernelGGL(k_micro_gather, dim3(blocks), dim3(256), 0, c->stream, rec.as<float4>(), nrec, iters, out.as<float>());
        (void)hipEventRecord(c->ev1, c->stream);
        e = hipEventSynchronize(c->ev1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
        if (rep > 0 && ms < best) best = ms;
    }
    rec.release(); out.release();
    TIRT_HIP(e);
    *gbps_out = (double)blocks * 256.0 * (double)iters * 64.0 / ((double)best * 1.0e-3) / 1.0e9;
    return TIRT_OK;
}

int tirt_stats(tirt_ctx *c, tirt_stats_t *out)
{
    CTX(c);
    TIRT_REQUIRE(out, "tirt_stats: null");
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    DevCounters h;
    if (sync_all(c)) return TIRT_ERR_HIP;
    TIRT_HIP(hipMemcpyAsync(&h, c->dev_counters.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    retire_render_events(c, false);
    out->rays_closest = h.rays_closest; out->rays_shadow = h.rays_shadow;
    out->box_closest = h.box_closest; out->leaf_closest = h.leaf_closest;
    out->box_shadow = h.box_shadow; out->leaf_shadow = h.leaf_shadow;
    out->shaded = h.shaded; out->paths = h.paths; out->stack_overflow = h.stack_overflow;
    out->diag_it_node = h.it_node; out->diag_lanes_node = h.lanes_node; out->diag_it_leaf = h.it_leaf;
    out->diag_lanes_leaf = h.lanes_leaf; out->diag_refills = h.refills; out->diag_it_outer = h.it_outer;
    out->diag_wave_ticks = h.wave_ticks; out->diag_drain_ticks = h.drain_ticks; out->diag_waves = h.waves;
    out->ms_build = c->ms_build; out->ms_render = c->ms_render;
    out->ms_trace_closest = c->ms_trace_closest; out->ms_trace_shadow = c->ms_trace_shadow; out->ms_shade = c->ms_shade;
    out->launches_trace_closest = c->launches_trace_closest; out->launches_trace_shadow = c->launches_trace_shadow;
    out->launches_shade = c->launches_shade; out->launches_tail = 0;      // (the persistent tail kernel left the library in round 6; the field stays for the ABI)
    if (h.stack_overflow > 0) {      // results are wrong (subtrees were dropped): the statistics are filled in, the call reports it
        set_error("traversal stack overflow on " + std::to_string((unsigned long long)h.stack_overflow) + " rays: raise stack_size");
        // reported once: the counter is cleared, so that later tirt_stats calls of unrelated consumers do not keep failing
        TIRT_HIP(hipMemsetAsync((char *)c->dev_counters.p + offsetof(DevCounters, stack_overflow), 0, sizeof(h.stack_overflow), c->stream));
        TIRT_HIP(hipStreamSynchronize(c->stream));
        return TIRT_ERR_STACK;
    }
    return TIRT_OK;
}

static void drain_pvb_events(tirt_ctx *c)
{
    for (auto &pr : c->pvb_ev) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) c->pvb_build_ns += (unsigned long long)((double)ms * 1.0e6);
        (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
    }
    c->pvb_ev.clear();
    (void)hipGetLastError();
}

int tirt_primary_beam_stats(tirt_ctx *c, uint64_t out[12])
{
    TIRT_REQUIRE(c && out, "tirt_primary_beam_stats: null arguments");
    for (int k = 0; k < 12; k++) out[k] = 0;
    if (sync_all(c)) return TIRT_ERR_HIP;
    drain_pvb_events(c);
    out[5] = c->pvb_builds; out[6] = c->pvb_build_ns; out[7] = c->pvb_skipped;
    if (!c->pvb_stat.p) return TIRT_OK;
    unsigned long long h[12];
    TIRT_HIP(hipMemcpy(h, c->pvb_stat.p, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 5; k++) out[k] = h[k];
    for (int k = 8; k < 12; k++) out[k] = h[k];
    return TIRT_OK;
}

int tirt_trace_timeline(tirt_ctx *c, uint64_t *out, int max_waves, int *n_waves)
{
    CTX(c);
    TIRT_REQUIRE(out && n_waves && max_waves >= 0, "tirt_trace_timeline: null / negative arguments");
    if (sync_all(c)) return TIRT_ERR_HIP;
    const int n = c->timeline_waves < max_waves ? c->timeline_waves : max_waves;
    if (n > 0) TIRT_HIP(hipMemcpy(out, c->timeline.p, sizeof(uint64_t) * 4 * (size_t)n, hipMemcpyDeviceToHost));
    *n_waves = c->timeline_waves;
    return TIRT_OK;
}

int tirt_stats_reset(tirt_ctx *c)
{
    CTX(c);
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    if (sync_all(c)) return TIRT_ERR_HIP;
    retire_render_events(c, false);
    TIRT_HIP(hipMemsetAsync(c->dev_counters.p, 0, sizeof(DevCounters), c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    c->ms_render = c->ms_trace_closest = c->ms_trace_shadow = c->ms_shade = 0.0;
    c->launches_trace_closest = c->launches_trace_shadow = c->launches_shade = 0;
    drain_pvb_events(c); c->pvb_builds = c->pvb_build_ns = c->pvb_skipped = 0;
    return TIRT_OK;
}

int tirt_shade_table_download(tirt_ctx *c, int which, float *out, uint64_t floats)
{
    CTX(c);
    TIRT_REQUIRE(out && (which == 0 || which == 1), "tirt_shade_table_download: bad args");
    TIRT_REQUIRE(c->n >= 1, "tirt_shade_table_download: no scene");
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (ensure_shade_records(c)) return TIRT_ERR_HIP;
    const uint64_t have = which == 0 ? (uint64_t)32 * c->n : (uint64_t)4 * LIGHT_REC_QUADS * c->light_count;
    TIRT_REQUIRE(floats == have, "tirt_shade_table_download: 32 floats per primitive (which 0) or per light (which 1)");
    if (floats) TIRT_HIP(hipMemcpyAsync(out, which == 0 ? c->shade_rec.p : c->light_rec.p, sizeof(float) * floats, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

}  // extern "C"
