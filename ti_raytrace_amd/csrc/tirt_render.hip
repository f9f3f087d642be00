// tirt_render.hip -- the PT_RGB / PT_Spec wavefront pipeline.
//
// Reference path: integrator/PT_RGB.py:44-136 is ONE per-pixel megakernel that inlines
// Scene.closet_hit (Scene.py:702-744), the shading branch, Scene.closet_hit_shadow (:671-699) and the film
// update.  Here the same arithmetic is split into a wavefront of kernels over struct-of-arrays
// path state in HBM:
//
//   k_generate        camera rays                                   Camera.py:122-142
//   k_trace<closest>  closest hit of every live path                Scene.py:702-744
//   k_shade           light / glass / disney branch, NEE set-up,    integrator/PT_RGB.py:66-132
//                     next ray, throughput; compacts live paths
//                     into the next dense state (ballots + one
//                     packed atomic per block)
//   k_trace<shadow>   NEE visibility, adds the stored contribution  Scene.py:671-699, PT_RGB.py:104-109
//   k_film            running-mean film update                      integrator/PT_RGB.py:134-136
//
// PT_RGB keeps a path's radiance in one place from bounce 0 on: PathState::fr / fg / fb[slot], which k_film reads.  k_shade of bounce 0 stores every path's first
// value there (slot == q: coalesced); at a later bounce only a path with something to add -- an emitter hit, a miss under a lit environment -- reads, adds and
// writes its three words, and every shadow ray carries ~slot, so k_trace's write-back adds the light sample's contribution there too.  Per path the additions
// come in the reference's order: a lane's launches are on one stream, and within a launch a path has one writer.  A path that goes on moves 11 words from one
// PathSoA to the other (ray, throughput, brdf_pdf, and the slot word with perfect_spec in its bit 31); the rr / rg / rb / flags arrays are PT_Spec's.
//
// A PT_RGB batch whose camera rays go through the pixels' candidate lists (tirt_pvb.hip) does k_generate, the list pass and k_shade of bounce 0 in one kernel,
// k_pvb_cand_shade below (option "primary_fused"): the direction and the first hit record never reach HBM.
//
// The three persistent shading kernels -- k_shade, k_pvb_cand_shade, PT_Spec's k_shade_spec -- differ in their shading body and in what a path carries.  What
// surrounds the body is one text for all three ("the path queues", below): the loop head (shade_loop), the hit-record load, the dense compaction with its one
// packed atomic per block and round (queue_slots; the fused kernel's leftover list is an option of it), the store blocks and the `shaded` statistic.
//
// k_trace and its launchers (the walk, its two visiting rules, the tie rule) are in tirt_trace.hip; this file holds the shading kernels, the tables of
// their instantiations and the scheduler that submits a batch's launches (pt_render), in that order.
#include "tirt_pvb.h"
#include "tirt_spectral.h"

namespace tirt {

// One path at one bounce: what integrator/PT_RGB.py:66-132 does between the closest hit and the next one -- emission (with MIS), the glass / disney
// branch, the NEE sample (its shadow ray and the contribution it adds IF the ray arrives), the next ray and the throughput, the environment
// for a miss.  The body of k_shade, kept apart from its queue handling.  `throughout`, `brdf_pdf`, `perfect_spec` are the path's state coming in.  The radiance so far is
// not: the step reports the term it adds to it (`adds`, `add`: an emitter hit or a miss; a Disney or glass hit adds nothing) and the caller performs `radiance + add`.
struct ShadeStep {
    bool want_next = false, want_shadow = false, shaded = false, adds = false;
    v3 add = V(0.0f, 0.0f, 0.0f);
    v3 next_o = V(0.0f, 0.0f, 0.0f), next_d = next_o, next_thr = next_o, sh_o = next_o, sh_d = next_o, sh_c = next_o;
    float next_pdf = 0.0f, sh_dist = 0.0f; int next_spec = 0, sh_expect = -2;
};
// FEAT: the feature word (tirt_device.h, SF_*) this copy is compiled for -- a superset of the scene's.  A scene without glass, without a lit environment, with one
// kind of emitter compiles none of the code of the others; what is left performs the same operations on the same operands in the same order.
// LIST: the batch's local pixels are a pixel set's list (mapped_pixel, tirt_internal.h) -- the pixel is the random numbers' and nothing else here.
template <unsigned FEAT, bool LIST = false>
TD void shade_path(const SceneView &sc, const TileMap &tm, int P, uint32_t frame_begin, uint32_t seed, int bounce, int last_bounce, int slot,
                   const v3 origin, const v3 direction, const float4 hrec, v3 throughout, float brdf_pdf, int perfect_spec, ShadeStep &s)
{
    int f, k; slot_to_frame_pixel(tm, P, slot, f, k);
    const uint32_t pixel = (uint32_t)mapped_pixel<LIST>(tm, k);
    const uint32_t frame = frame_begin + (uint32_t)f;
    const uint32_t dim0 = TM_DIM_BOUNCE0 + TM_DIMS_PER_BOUNCE * (uint32_t)bounce;
    const float t = hrec.x;
    // environment importance sampling (SF_ENV_SAMPLE instantiations only; include/tirt.h): the share of the light samples that go to the environment
    constexpr bool ENV_NEE = (FEAT & SF_ENV_SAMPLE) != 0u;
    // an RGBE8 environment (SF_ENV_HDR instantiations only; include/tirt.h, "HDR environment"): the two lookups below decode linear texels, no srgb_to_lrgb
    constexpr bool ENV_HDR = (FEAT & SF_ENV_HDR) != 0u;
    // emitters chosen by power (SF_LIGHT_POWER instantiations only; include/tirt.h, "Choosing emitters by power"): the entry and its P come from the table behind the light
    // records, an emitter hit reads the P of its entry from the spare word of its shading record
    constexpr bool LIGHT_POW = (FEAT & SF_LIGHT_POWER) != 0u;
    [[maybe_unused]] float p_env = 0.0f;
    if constexpr (ENV_NEE) p_env = sc.light_count == 0 ? 1.0f : env_table(sc).share;
    if (t < INF_VALUE) {
        const int prim_id = __float_as_int(hrec.w);
        int mat_id;
        const HitAttr h = hit_attributes_rec<(FEAT & (SF_TEXTURE | SF_TEXTURE_PARAM)) != 0u>(sc.shade_rec, origin, direction, prim_id, t, hrec.y, hrec.z, mat_id);
        v3 normal = h.nor;
        // a normal-mapped material (SF_TEXTURE_PARAM instantiation only): the mapped normal takes h.nor's place before fnormal is formed; h.gnor stays
        if constexpr ((FEAT & SF_TEXTURE_PARAM) != 0u) {
            const int nor_id = material_map(sc.material + (size_t)mat_id * MAT_VEC, 9);
            if (nor_id >= 0) normal = tex_normal_rec(sc.tex, sc.shade_rec, nor_id, prim_id, h.tex, normal);
        }
        const v3 fnormal = normal * signf(dot(-direction, h.gnor));            // UtilsFunc.py:465-467
        const float *m = sc.material + (size_t)mat_id * MAT_VEC;
        const v3 mat_color = V(m[2], m[3], m[4]);
        const int mat_type = (int)m[0];
        if (mat_type == MAT_LIGHT) {                                           // PT_RGB.py:72-81
            const float fCosTheta = absf(dot(direction, h.gnor));
            s.adds = true;
            if (perfect_spec == 1) {
                s.add = throughout * mat_color;
            } else {
                const float area = h.area * (float)sc.light_count;              // get_prim_area of the emitter, from its shading record
                float light_pdf = (t * t) / (area * fCosTheta);
                if constexpr (LIGHT_POW) light_pdf = (t * t) * (shade_rec_phit(sc.shade_rec, prim_id) / h.area) / fCosTheta;
                if constexpr (ENV_NEE) light_pdf = light_pdf * (1.0f - p_env);
                s.add = (throughout * power_heuristic(brdf_pdf, light_pdf)) * mat_color;
            }
        } else {
            s.shaded = true;
            // UF.srgb_to_lrgb(material colour) (PT_RGB.py:86): per-material table filled by the same device function
            v3 reflect_color;
            // a textured material (SF_TEXTURE instantiation only): srgb_to_lrgb of the texture's colour at the hit's uv takes the place of the table's entry
            const int tex_id = (FEAT & SF_TEXTURE) ? material_texture(m) : -1;
            if ((FEAT & SF_TEXTURE) && tex_id >= 0) reflect_color = srgb_to_lrgb(tex_albedo(sc.tex, tex_id, h.tex.x, h.tex.y));
            else reflect_color = V(sc.mat_lrgb[mat_id * 3], sc.mat_lrgb[mat_id * 3 + 1], sc.mat_lrgb[mat_id * 3 + 2]);
            v3 next_dir; float f_or_b = 1.0f, brdf = 1.0f;
            if ((FEAT & SF_GLASS) && mat_type == MAT_GLASS) {                  // PT_RGB.py:89-92
                perfect_spec = 1;
                next_dir = glass_sample(m, direction, normal, tm_rand(seed, pixel, frame, dim0 + TM_SLOT_GLASS), f_or_b);
                brdf = 1.0f; brdf_pdf = 1.0f;
            } else {
                perfect_spec = 0;
                // roughness / metallic textures (SF_TEXTURE_PARAM instantiation only): a local copy of the whole row with the looked-up values in words 5
                // and 6, which the Disney functions read through the pointer they always took (they read those two words; the rest is copied so that a
                // function that comes to read another word through `md` finds it)
                float mp[MAT_VEC];
                const float *md = m;
                if constexpr ((FEAT & SF_TEXTURE_PARAM) != 0u) {
                    for (int w = 0; w < MAT_VEC; w++) mp[w] = m[w];
                    const int metal_id = material_map(m, 8), rough_id = material_map(m, 7);
                    if (metal_id >= 0) mp[5] = tex_metallic(sc.tex, metal_id, h.tex.x, h.tex.y);
                    if (rough_id >= 0) mp[6] = tex_roughness(sc.tex, rough_id, h.tex.x, h.tex.y);
                    md = mp;
                }
                // Scene.py:477-518 sample_li.  No emitters (env-lit scene): the reference would index light[-1]
                // (Scene.py:423-428, undefined) -- defined here, as in the oracle, as "no NEE sample"
                // the view-only and material-only terms of the BSDF, once for the NEE sample, the lobe choice and the continuation (tirt_device.h)
                // (only where the glass branch is not compiled: with it the body sits on the 96-VGPR limit of SH_MIN_WAVES and the set-up's live values go
                // to scratch -- there every evaluation makes its own, as before)
                constexpr bool SHARE_SETUP = !(FEAT & SF_GLASS);
                DisneySetup ds;
                if (SHARE_SETUP) ds = disney_setup(md, fnormal, -direction);
                [[maybe_unused]] bool env_taken = false;
                if constexpr (ENV_NEE) {
                    // the environment's turn: r < p_env.  The sample, its pdf and the lookup coordinates of its OWN direction (what a BSDF ray in that direction
                    // would fetch in the miss branch below) come from the table behind the texels; one shadow ray that arrives iff it hits nothing
                    if (tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LIGHT) < p_env) {
                        env_taken = true;
                        const EnvTable et = env_table(sc);
                        const EnvSample es = env_sample(et, sc.env_w, sc.env_h, tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LA), tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LB));
                        const EnvPdf ep = env_pdf(et, sc.env_w, sc.env_h, es.d);
                        const float NdotL = dot(fnormal, es.d);
                        if ((NdotL > 0.0f) & (ep.pdf > 0.0f)) {
                            s.want_shadow = true;
                            float e_pdf;
                            const float e_brdf = SHARE_SETUP ? disney_evaluate_pdf_set(ds, fnormal, -direction, es.d, e_pdf)
                                                             : disney_evaluate_pdf(md, fnormal, -direction, es.d, e_pdf);
                            const float pdf_l = p_env * ep.pdf;
                            v3 c = V(0.0f, 0.0f, 0.0f);
                            int expect = -2;
                            if (e_pdf > 0.0f) {
                                const float w = power_heuristic(pdf_l, e_pdf) / maxf(0.0001f, pdf_l);
                                c = (env_lookup<ENV_HDR>(sc.env, sc.env_w, sc.env_h, ep.tx, ep.ty) * sc.env_power) * w;
                                c = c * throughout;
                                c = c * reflect_color;
                                c = c * e_brdf;
                                c = c * absf(NdotL);
                                // The reference draws its diffuse lobe with density cos / pi and states 1 / pi (quirk B4, disney_evaluate_pdf), so a BSDF sample
                                // weighted by 1 / e_pdf -- the switch-off estimator -- converges to the integral of (drawn / e_pdf) * f * cos * L, not of
                                // f * cos * L.  The light sample carries the same ratio: both strategies then estimate one integrand and their MIS weights,
                                // which sum to 1, leave its integral where the switch-off render has it.  A metal (diffuseRatio 0) has the ratio exactly 1.
                                const float dr = SHARE_SETUP ? ds.diffuseRatio : 0.5f * (1.0f - md[5]);
                                const float drawn = maxf(0.0f, e_pdf + (dr * (float)(1.0 / 3.1415956)) * (NdotL - 1.0f));
                                c = c * (drawn / e_pdf);
                                expect = -1;                   // k_trace's hit_prim of a ray that hits nothing
                            }
                            s.sh_o = offset_ray(h.pos, fnormal); s.sh_d = es.d; s.sh_c = c; s.sh_expect = expect; s.sh_dist = ENV_SHADOW_DIST;
                        }
                    }
                }
                if (!env_taken && (!(FEAT & SF_NO_LIGHT) || sc.light_count > 0)) {
                float r_light = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LIGHT);
                if constexpr (ENV_NEE) r_light = (r_light - p_env) / (1.0f - p_env);
                int lidx = (int)(r_light * (float)sc.light_count);
                if (lidx >= sc.light_count) lidx = sc.light_count - 1;
                [[maybe_unused]] float P_light = 0.0f;
                if constexpr (LIGHT_POW) lidx = light_pick(light_table(sc), sc.light_count, r_light, P_light);
                const float ra = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LA);
                const float rb = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LB);
                v3 light_pos, light_normal;
                // the emitter's area, choice pdf, emission and the edges of its sampled point: per-light record (tirt_device.h, k_light_records)
                // (chosen by power: the list holds triangles and spheres only, the other kinds are not compiled)
                const LightRec lr = light_sample_rec<LIGHT_POW ? (FEAT & ~(SF_LIGHT_SPOT_LASER | SF_LIGHT_OTHER)) : FEAT>(sc.light_rec, lidx, ra, rb, light_pos, light_normal);
                const float light_choice_pdf = LIGHT_POW ? P_light / lr.area : lr.choice_pdf;
                light_normal = normalized(light_normal);
                v3 light_dir = h.pos - light_pos;
                const float light_dist = norm(light_dir);
                light_dir = light_dir / light_dist;
                const v3 light_emission = lr.emission * light_shape_visible_rec<LIGHT_POW ? (FEAT & ~SF_LIGHT_SPOT_LASER) : FEAT>(lr, light_dir, light_normal, light_dist);   // spot / laser (Scene.py:491-516)
                const float NdotL_surface = dot(fnormal, light_dir);            // PT_RGB.py:101-109
                const float NdotL_light = dot(light_normal, light_dir);
                if ((NdotL_surface < 0.0f) & (NdotL_light > 0.0f)) {
                    s.want_shadow = true;
                    float e_pdf;
                    const float e_brdf = SHARE_SETUP ? disney_evaluate_pdf_set(ds, fnormal, -direction, -light_dir, e_pdf)
                                                     : disney_evaluate_pdf(md, fnormal, -direction, -light_dir, e_pdf);
                    float light_pdf = light_dist * light_dist * light_choice_pdf / NdotL_light;
                    if constexpr (ENV_NEE) light_pdf = light_pdf * (1.0f - p_env);
                    v3 c = V(0.0f, 0.0f, 0.0f);
                    int expect = -2;                       // never equals a primitive id
                    if (e_pdf > 0.0f) {
                        const float w = power_heuristic(light_pdf, e_pdf) / maxf(0.0001f, light_pdf);
                        c = light_emission * w;
                        c = c * throughout;
                        c = c * reflect_color;
                        c = c * e_brdf;
                        c = c * absf(NdotL_surface);
                        expect = prim_id;
                    }
                    s.sh_o = light_pos; s.sh_d = light_dir; s.sh_c = c; s.sh_expect = expect; s.sh_dist = light_dist;
                }
                }   // light_count > 0
                const float r_lobe = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LOBE), r_1 = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_R1),
                            r_2 = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_R2);
                next_dir = SHARE_SETUP ? disney_sample_set(ds, direction, fnormal, r_lobe, r_1, r_2) : disney_sample(md, direction, fnormal, r_lobe, r_1, r_2);
                f_or_b = 1.0f;
                brdf = SHARE_SETUP ? disney_evaluate_pdf_set(ds, fnormal, -direction, next_dir, brdf_pdf)
                                   : disney_evaluate_pdf(md, fnormal, -direction, next_dir, brdf_pdf);
                brdf *= absf(dot(normal, next_dir));
            }
            const v3 next_origin = offset_ray(h.pos, fnormal * signf(f_or_b));   // PT_RGB.py:115
            if (brdf_pdf > 0.0f) {
                bool alive = true;
                if ((FEAT & SF_GLASS) && f_or_b < 0.0f) {                        // PT_RGB.py:118-122
                    const float extinction = m[6];
                    const float R = tm_exp(-t / extinction);
                    if (tm_rand(seed, pixel, frame, dim0 + TM_SLOT_EXT) >= R) alive = false;
                }
                if (alive) {
                    throughout = throughout * (reflect_color * (brdf / brdf_pdf));
                    s.want_next = !last_bounce;      // depth reaches MAX_DEPTH after the last bounce: the loop ends
                    s.next_o = next_origin; s.next_d = next_dir; s.next_thr = throughout;
                    s.next_pdf = brdf_pdf; s.next_spec = perfect_spec;
                }
            }
        }
    } else if ((!(FEAT & SF_ENV) || sc.env_power == 0.0f) && (direction.x - direction.x == 0.0f) && (direction.y - direction.y == 0.0f) &&
               (direction.z - direction.z == 0.0f)) {
        // black environment (PT_RGB.py:127-132 with env_power == 0): for a finite direction the lookup returns a
        // finite e >= 0, so (e * throughput) * 0 is +-0 with throughput's sign, or NaN where throughput is not
        // finite -- exactly throughput * env_power, without the two atan2, four texel fetches and three pow
        s.adds = true; s.add = throughout * sc.env_power;
    } else if (!(FEAT & SF_ENV)) {
        // a direction that is not finite under a black environment (env_power == 0 and every texel 0: the SF_ENV bit is clear).  The lookup below then
        // fetches zeros whatever the texel indices are, and mixes them with the weights x - floor(x) of the clamped coordinates: 0 where tx and ty are
        // numbers (a clamped coordinate is finite), NaN where one of them is NaN -- and srgb_to_lrgb keeps both.  tm_atan2 returns NaN for a NaN
        // argument and for two infinite ones (its quotient), a number otherwise; `dis` is the lookup's own expression.  So e is all NaN or all zero:
        const float dis = tm_sqrt(direction.x * direction.x + direction.z * direction.z);
        const float big = 3.4028234e38f;
        const bool e_nan = direction.x != direction.x || direction.y != direction.y || direction.z != direction.z ||
                           (absf(direction.x) > big && absf(direction.z) > big) || (absf(direction.y) > big && dis > big);
        const float e1 = e_nan ? tm_nan() : 0.0f;
        s.adds = true; s.add = (V(e1, e1, e1) * throughout) * sc.env_power;
    } else {                                                                     // PT_RGB.py:127-132
        const float dis = tm_sqrt(direction.x * direction.x + direction.z * direction.z);
        const float tx = (tm_atan2(direction.z, direction.x) + PI_SCENE) / PI_SCENE / 2.0f;
        const float ty = tm_atan2(direction.y, dis) / PI_SCENE + 0.5f;
        const v3 e = env_lookup<ENV_HDR>(sc.env, sc.env_w, sc.env_h, tx, ty);
        s.adds = true;
        if constexpr (ENV_NEE) {
            // MIS against the environment sample the previous vertex could have taken: weight 1 behind a camera or glass vertex (no NEE there)
            float w = 1.0f;
            if (perfect_spec != 1) w = power_heuristic(brdf_pdf, p_env * env_pdf(env_table(sc), sc.env_w, sc.env_h, direction).pdf);
            s.add = ((e * throughout) * sc.env_power) * w;
        } else
        s.add = (e * throughout) * sc.env_power;
    }
}

// ---------------------------------------------------------------------------------------------
// Wavefront PT_RGB
// ---------------------------------------------------------------------------------------------
// The camera ray of path s of a batch: its pixel, the frame's sub-pixel jitter, the direction through it (Camera.py:122-142).  k_generate stores it; the fused
// first step (k_pvb_cand_shade) keeps it in registers.
template <bool LIST>
TD v3 camera_path_direction(const CameraView &cam, const TileMap &tm, int P, int s, uint32_t frame_begin, uint32_t seed)
{
    int f, k; slot_to_frame_pixel(tm, P, s, f, k);
    int p = mapped_pixel<LIST>(tm, k);
    int i = p / tm.H, j = p - i * tm.H;
    uint32_t frame = frame_begin + (uint32_t)f;
    float jx = 0.0f, jy = 0.0f;
    if (frame != 0) {                                    // Camera.py:135-137
        jx = tm_rand(seed, (uint32_t)p, frame, TM_DIM_JX) - 0.5f;
        jy = tm_rand(seed, (uint32_t)p, frame, TM_DIM_JY) - 0.5f;
    }
    return camera_ray_direction(cam, i, j, jx, jy);
}

template <bool LIST>
__global__ void k_generate(PathSoA ps, CameraView cam, TileMap tm, int P, int S, uint32_t frame_begin, uint32_t seed,
                           DevCounters *ctr)
{
    // Camera rays.  Only the direction is stored: the origin is the eye for every path and the rest of the
    // bounce-0 state is constant (throughput 1, radiance 0, pdf 1, specular flag set, path id = index), which
    // k_trace / k_shade of bounce 0 know without reading 48 bytes per path back from HBM.
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    v3 d = camera_path_direction<LIST>(cam, tm, P, s, frame_begin, seed);
    __builtin_nontemporal_store(d.x, &ps.dx[s]); __builtin_nontemporal_store(d.y, &ps.dy[s]); __builtin_nontemporal_store(d.z, &ps.dz[s]);      // (a stream: k_trace reads it once)
    if (s == 0) atomicAdd(&ctr->paths, (unsigned long long)S);
}

// Block size of the shading kernels: the unit that appends to the path queues with one atomic (queue_slots, below).  (512-thread blocks
// halve the atomics again but measured 4 % slower end to end: a 4-wave block needs 112 VGPRs per SIMD and fits next to the resident
// k_trace waves of another lane's batch, an 8-wave block does not.)
#ifndef SH_BLOCK
#define SH_BLOCK 256
#endif
#ifndef SH_MIN_WAVES
#define SH_MIN_WAVES 5
#endif
#ifndef SH_MIN_WAVES_NARROW      // the instantiations without glass and environment (82 VGPRs at 5 waves, 80 and still no scratch at 6)
#define SH_MIN_WAVES_NARROW 5
#endif
#ifndef SH_MIN_WAVES_MAPS        // the instantiation with every texture slot (SF_TEXTURE_PARAM): see DESIGN.md, "Roughness, metallic and normal-map textures"
#define SH_MIN_WAVES_MAPS 4      // at 5 (96 VGPRs) it has 20 bytes of scratch (12 LIST), at 4 110 VGPRs (107 LIST) and none
#endif
#ifndef SH_MIN_WAVES_ENV         // the instantiations with environment importance sampling (SF_ENV_SAMPLE): see DESIGN.md, "Importance sampling of the environment"
#define SH_MIN_WAVES_ENV 4
#endif
#ifndef SH_MIN_WAVES_POWER       // the generic kernel's twin that chooses emitters by power (SF_LIGHT_POWER): see DESIGN.md, "Choosing emitters by power"
#define SH_MIN_WAVES_POWER 4     // at 5 (96 VGPRs) it has 12 bytes of scratch where its sibling has none; its RGBE8 twin (SF_ENV_HDR | SF_LIGHT_POWER) likewise
#endif
#ifndef SH_MIN_WAVES_HDR         // the generic kernel's twin for an RGBE8 environment (SF_ENV_HDR): see DESIGN.md, "HDR environment"
#define SH_MIN_WAVES_HDR 5       // as its 8-bit sibling: no scratch at 5 (96 VGPRs) since the radiance is no longer live across shade_path (it had 12 bytes, and sat at 4)
#endif
#ifndef SH_MIN_WAVES_FUSED_NARROW      // k_pvb_cand_shade<.., true> of the two narrow kernels: 85 VGPRs at 5 waves, 80 and still no scratch at 6 -- and the list walk
#define SH_MIN_WAVES_FUSED_NARROW 6    // in it waits on memory, which a sixth wave covers: +0.6 % on the headline against 5, every pair (profiles/primary_fused_ab.txt)
#endif
#ifndef SH_MIN_WAVES_FUSED_WIDE  // k_pvb_cand_shade<.., true> of the generic kernels that sit at 5 waves (SF_ALL, + SF_TEXTURE, + SF_ENV_HDR): the leftover rays' direction is live
#define SH_MIN_WAVES_FUSED_WIDE 4      // across shade_path; at 5 (96 VGPRs) they have 20-24 bytes of scratch where k_shade has none, at 4 none (profiles/primary_fused.txt)
#endif
// The 78 array pointers of the path state are the first kernel argument and are never read from it directly: each of the three places
// that needs some of them (a path's state in, the survivor's state out, the shadow ray out) reads those from the kernel-argument segment in
// one batch of scalar loads -- as k_trace does (TR_COLD), and for the same reason: kept in SGPRs across the loop they overflow the scalar
// register file and come back through v_readlane, 700 VALU instructions of the 4 476 in this kernel.
struct ShadeArgs { PathState ps; PathSoA in, out; };
typedef const __attribute__((address_space(4))) ShadeArgs *cold_shade_t;
#define SH_COLD(ca) cold_shade_t ca = (cold_shade_t)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(ca))
#define SH_LD(x) __builtin_nontemporal_load(&(x))
#define SH_ST(x, v) __builtin_nontemporal_store((v), &(x))

// ---- the path queues: what the three persistent shading kernels (k_shade, k_pvb_cand_shade, k_shade_spec) do around their shading body, written once ----
// The head of the persistent loop: block b takes paths [it * total + b * SH_BLOCK, + SH_BLOCK) in round `it`; the path count comes from the counter the previous
// bounce appended to, or is the batch's (bounce 0).  The kernel passes its own blockDim.x and gridDim.x: read in a device function, blockDim.x comes out as
// the select between the full and the partial work-group's size (a 16-bit global load), which the compiler drops only where it sees the kernel's attributes.
struct ShadeLoop {
    int lane, wid, count, first, total, rounds;      // first: the thread's path in round 0
    unsigned long long lt_mask;                      // the lanes of the wave below this one
    TD int path(int it) const { return it * total + first; }
};
TD ShadeLoop shade_loop(const int *count_ptr, int count_fixed, unsigned block_dim, unsigned grid_dim)
{
    ShadeLoop lp;
    lp.lane = threadIdx.x & 63; lp.wid = threadIdx.x >> 6;
    lp.lt_mask = (lp.lane == 0) ? 0ull : (~0ull >> (64 - lp.lane));
    lp.count = count_ptr ? *count_ptr : count_fixed;
    lp.total = grid_dim * block_dim;
    lp.rounds = (lp.count + lp.total - 1) / lp.total;
    lp.first = blockIdx.x * block_dim + threadIdx.x;
    return lp;
}
// k_trace's 16-byte hit record of path q: a stream, read once
TD float4 load_hit_record(const float4 *hit, int q)
{
    typedef float f4nt__ __attribute__((ext_vector_type(4)));
    const f4nt__ h = __builtin_nontemporal_load((const f4nt__ *)&hit[q]);
    return make_float4(h.x, h.y, h.z, h.w);
}
// Dense compaction of a round: the block's survivors go to consecutive indices of the other PathSoA (`next`), its shadow rays to a dense list of their own
// (`shadow`); with LEFT the rays the fused kernel leaves to k_trace take their places in a third list (`left`; its counter fb_count, its statistic stat[3])
// between the same two barriers.  Two ballots, the wave's counts packed 16|16 into s_wcnt, and ONE 64-bit atomic per block and round (low word: next-bounce
// paths, high word: shadow rays; none for a block that appends nothing): same-address device atomics retire at ~11 ns each on MI355X, so one atomic per wave
// and queue (2 x 524k per 33.5 M paths) bounded the kernel at ~6 ms; per 256-thread block it is 131k (SH_BLOCK, above).  The LDS words are the calling kernel's
// and double-buffered by the round's parity: a wave may enter round it + 1 while another still reads the bases of round it.
struct QueueSlots { int next, shadow, left; };
template <bool LEFT = false>
TD QueueSlots queue_slots(const ShadeLoop &lp, int it, bool want_next, bool want_shadow, unsigned (&s_wcnt)[2][SH_BLOCK / 64], unsigned long long (&s_base)[2],
                          unsigned long long *append_ctr, bool left = false, unsigned (*s_fcnt)[SH_BLOCK / 64] = nullptr, int *s_fbase = nullptr,
                          int *fb_count = nullptr, unsigned long long *stat = nullptr)
{
    const int par = it & 1;
    const unsigned long long nmask = __ballot(want_next), smask = __ballot(want_shadow), fmask = LEFT ? __ballot(left) : 0ull;
    if (lp.lane == 0) { s_wcnt[par][lp.wid] = (unsigned)__popcll(nmask) | ((unsigned)__popcll(smask) << 16); if (LEFT) s_fcnt[par][lp.wid] = (unsigned)__popcll(fmask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tn = 0, tsd = 0, tf = 0;
#pragma unroll
        for (int w = 0; w < SH_BLOCK / 64; w++) { tn += s_wcnt[par][w] & 0xffffu; tsd += s_wcnt[par][w] >> 16; if (LEFT) tf += s_fcnt[par][w]; }
        s_base[par] = (tn | tsd) ? atomicAdd(append_ctr, (unsigned long long)tn | ((unsigned long long)tsd << 32)) : 0ull;
        if (LEFT) {
            s_fbase[par] = tf ? atomicAdd(fb_count, (int)tf) : 0;
            if (stat && tf) atomicAdd(&stat[3], (unsigned long long)tf);
        }
    }
    __syncthreads();
    unsigned pn = 0, psd = 0, pf = 0;
#pragma unroll
    for (int w = 0; w < SH_BLOCK / 64; w++) if (w < lp.wid) { pn += s_wcnt[par][w] & 0xffffu; psd += s_wcnt[par][w] >> 16; if (LEFT) pf += s_fcnt[par][w]; }
    const unsigned long long bb = s_base[par];
    QueueSlots at;
    at.next = (int)(unsigned)(bb & 0xffffffffull) + (int)pn + __popcll(nmask & lp.lt_mask);
    at.shadow = (int)(unsigned)(bb >> 32) + (int)psd + __popcll(smask & lp.lt_mask);
    at.left = LEFT ? s_fbase[par] + (int)pf + __popcll(fmask & lp.lt_mask) : 0;
    return at;
}
// PT_RGB: a survivor's 11 words into the other PathSoA (the slot word carries perfect_spec in bit 31), a shadow ray's 12 into its list, a camera path's first
// radiance into fr / fg / fb[slot] (slot == q but for the fused kernel's leftovers: coalesced).  Each reads its array pointers from the kernel-argument segment in
// one batch of scalar loads (SH_COLD, above); the empty asm keeps the batch together.
TD void store_survivor(int at, int slot, const ShadeStep &s)
{
    SH_COLD(ca);
    float *const o_ox = ca->out.ox, *const o_oy = ca->out.oy, *const o_oz = ca->out.oz, *const o_dx = ca->out.dx, *const o_dy = ca->out.dy, *const o_dz = ca->out.dz;
    float *const o_tr = ca->out.tr, *const o_tg = ca->out.tg, *const o_tb = ca->out.tb;
    float *const o_pdf = ca->out.brdf_pdf; int *const o_slot = ca->out.slot;
    asm volatile("" :: "s"(o_ox), "s"(o_oy), "s"(o_oz), "s"(o_dx), "s"(o_dy), "s"(o_dz), "s"(o_tr), "s"(o_tg), "s"(o_tb), "s"(o_pdf), "s"(o_slot));
    SH_ST(o_ox[at], s.next_o.x); SH_ST(o_oy[at], s.next_o.y); SH_ST(o_oz[at], s.next_o.z);
    SH_ST(o_dx[at], s.next_d.x); SH_ST(o_dy[at], s.next_d.y); SH_ST(o_dz[at], s.next_d.z);
    SH_ST(o_tr[at], s.next_thr.x); SH_ST(o_tg[at], s.next_thr.y); SH_ST(o_tb[at], s.next_thr.z);
    SH_ST(o_pdf[at], s.next_pdf); SH_ST(o_slot[at], (int)((uint32_t)slot | ((uint32_t)s.next_spec << 31)));
}
TD void store_shadow_ray(int at, int slot, const ShadeStep &s)
{
    SH_COLD(ca);
    float *const s_ox = ca->ps.sox, *const s_oy = ca->ps.soy, *const s_oz = ca->ps.soz, *const s_dx = ca->ps.sdx, *const s_dy = ca->ps.sdy, *const s_dz = ca->ps.sdz;
    float *const s_cr = ca->ps.scr, *const s_cg = ca->ps.scg, *const s_cb = ca->ps.scb, *const s_dist = ca->ps.sdist;
    int *const s_prim = ca->ps.sprim, *const s_dst = ca->ps.sdst;
    asm volatile("" :: "s"(s_ox), "s"(s_oy), "s"(s_oz), "s"(s_dx), "s"(s_dy), "s"(s_dz), "s"(s_cr), "s"(s_cg), "s"(s_cb), "s"(s_dist), "s"(s_prim), "s"(s_dst));
    SH_ST(s_ox[at], s.sh_o.x); SH_ST(s_oy[at], s.sh_o.y); SH_ST(s_oz[at], s.sh_o.z);
    SH_ST(s_dx[at], s.sh_d.x); SH_ST(s_dy[at], s.sh_d.y); SH_ST(s_dz[at], s.sh_d.z);
    SH_ST(s_cr[at], s.sh_c.x); SH_ST(s_cg[at], s.sh_c.y); SH_ST(s_cb[at], s.sh_c.z);
    SH_ST(s_prim[at], s.sh_expect); SH_ST(s_dist[at], s.sh_dist);
    SH_ST(s_dst[at], ~slot);               // always the per-path accumulator (k_trace's dst < 0 case), whether the path goes on or not
}
TD void store_first_radiance(int slot, const v3 radiance)
{
    SH_COLD(ca);
    float *const f_r = ca->ps.fr, *const f_g = ca->ps.fg, *const f_b = ca->ps.fb;
    asm volatile("" :: "s"(f_r), "s"(f_g), "s"(f_b));
    SH_ST(f_r[slot], radiance.x); SH_ST(f_g[slot], radiance.y); SH_ST(f_b[slot], radiance.z);
}
// PT_Spec: a survivor carries four-channel throughput and radiance (15 words; tw in brdf_pdf's array, rw in flags'), a shadow ray a four-channel contribution
// and, as destination, its path's place in the other PathSoA if the path goes on (k_trace's dst >= 0 case) or ~slot; plain stores
TD void store_survivor_spec(int at, int slot, const v3 next_o, const v3 next_d, const f4s &next_thr, const f4s &radiance)
{
    SH_COLD(ca);
    float *const o_ox = ca->out.ox, *const o_oy = ca->out.oy, *const o_oz = ca->out.oz, *const o_dx = ca->out.dx, *const o_dy = ca->out.dy, *const o_dz = ca->out.dz;
    float *const o_tr = ca->out.tr, *const o_tg = ca->out.tg, *const o_tb = ca->out.tb, *const o_rr = ca->out.rr, *const o_rg = ca->out.rg, *const o_rb = ca->out.rb;
    float *const o_tw = ca->out.brdf_pdf, *const o_rw = (float *)ca->out.flags; int *const o_slot = ca->out.slot;
    asm volatile("" :: "s"(o_ox), "s"(o_oy), "s"(o_oz), "s"(o_dx), "s"(o_dy), "s"(o_dz), "s"(o_tr), "s"(o_tg), "s"(o_tb), "s"(o_rr), "s"(o_rg), "s"(o_rb),
                 "s"(o_tw), "s"(o_rw), "s"(o_slot));
    o_ox[at] = next_o.x; o_oy[at] = next_o.y; o_oz[at] = next_o.z;
    o_dx[at] = next_d.x; o_dy[at] = next_d.y; o_dz[at] = next_d.z;
    o_tr[at] = next_thr.v[0]; o_tg[at] = next_thr.v[1]; o_tb[at] = next_thr.v[2]; o_tw[at] = next_thr.v[3];
    o_rr[at] = radiance.v[0]; o_rg[at] = radiance.v[1]; o_rb[at] = radiance.v[2]; o_rw[at] = radiance.v[3];
    o_slot[at] = slot;
}
TD void store_shadow_ray_spec(int at, int dst, const v3 sh_o, const v3 sh_d, const f4s &sh_c, int sh_expect, float sh_dist)
{
    SH_COLD(ca);
    float *const s_ox = ca->ps.sox, *const s_oy = ca->ps.soy, *const s_oz = ca->ps.soz, *const s_dx = ca->ps.sdx, *const s_dy = ca->ps.sdy, *const s_dz = ca->ps.sdz;
    float *const s_cr = ca->ps.scr, *const s_cg = ca->ps.scg, *const s_cb = ca->ps.scb, *const s_cw = ca->ps.scw, *const s_dist = ca->ps.sdist;
    int *const s_prim = ca->ps.sprim, *const s_dst = ca->ps.sdst;
    asm volatile("" :: "s"(s_ox), "s"(s_oy), "s"(s_oz), "s"(s_dx), "s"(s_dy), "s"(s_dz), "s"(s_cr), "s"(s_cg), "s"(s_cb), "s"(s_cw), "s"(s_dist), "s"(s_prim), "s"(s_dst));
    s_ox[at] = sh_o.x; s_oy[at] = sh_o.y; s_oz[at] = sh_o.z;
    s_dx[at] = sh_d.x; s_dy[at] = sh_d.y; s_dz[at] = sh_d.z;
    s_cr[at] = sh_c.v[0]; s_cg[at] = sh_c.v[1]; s_cb[at] = sh_c.v[2]; s_cw[at] = sh_c.v[3];
    s_prim[at] = sh_expect; s_dist[at] = sh_dist;
    s_dst[at] = dst;
}
// The `shaded` statistic: wave sum, LDS atomic, one global atomic per block -- not per wave, for the reason given at queue_slots
TD void count_shaded(unsigned long long n_shaded, unsigned long long &s_shaded, DevCounters *ctr)
{
    if (threadIdx.x == 0) s_shaded = 0ull;
    __syncthreads();
    n_shaded = wave_sum(n_shaded);
    if ((threadIdx.x & 63) == 0 && n_shaded) atomicAdd(&s_shaded, n_shaded);
    __syncthreads();
    if (threadIdx.x == 0 && s_shaded) atomicAdd(&ctr->shaded, s_shaded);
}

template <unsigned FEAT, int MIN_WAVES, bool LIST = false>
__global__ __launch_bounds__(SH_BLOCK, MIN_WAVES) void k_shade(ShadeArgs paths_in_kernarg_segment, SceneView sc, TileMap tm, int P,
                                                   uint32_t frame_begin, uint32_t seed, int bounce, int last_bounce,
                                                   const int *count_ptr, int count_fixed, unsigned long long *append_ctr,
                                                   DevCounters *ctr, v3 eye)
{
    __shared__ unsigned s_wcnt[2][SH_BLOCK / 64];
    __shared__ unsigned long long s_base[2];
    const ShadeLoop lp = shade_loop(count_ptr, count_fixed, blockDim.x, gridDim.x);
    unsigned long long n_shaded = 0;
    for (int it = 0; it < lp.rounds; it++) {
        const int q = lp.path(it);
        bool live = q < lp.count, adds = false;
        int slot = 0;
        // `radiance`: at bounce 0 the path's radiance after this step (0 + the step's term), at a later bounce the term alone -- the radiance so far is fr / fg / fb[slot]
        v3 radiance = V(0.0f, 0.0f, 0.0f);
        ShadeStep ss;
        const bool first = bounce == 0;              // camera rays: constant state, see k_generate
        if (live) {
            SH_COLD(ca);
            const int *const c_slot = ca->in.slot; const float4 *const c_hit = ca->ps.hit;
            const float *const c_ox = ca->in.ox, *const c_oy = ca->in.oy, *const c_oz = ca->in.oz, *const c_dx = ca->in.dx, *const c_dy = ca->in.dy, *const c_dz = ca->in.dz;
            const float *const c_tr = ca->in.tr, *const c_tg = ca->in.tg, *const c_tb = ca->in.tb;
            const float *const c_pdf = ca->in.brdf_pdf;
            asm volatile("" :: "s"(c_slot), "s"(c_hit), "s"(c_ox), "s"(c_oy), "s"(c_oz), "s"(c_dx), "s"(c_dy), "s"(c_dz), "s"(c_tr), "s"(c_tg), "s"(c_tb), "s"(c_pdf));
            // the stored slot word: the path id (>= 0) with perfect_spec in bit 31 (PathSoA::slot)
            const uint32_t slot_word = first ? (uint32_t)q | 0x80000000u : (uint32_t)SH_LD(c_slot[q]);
            slot = (int)(slot_word & 0x7fffffffu);
            const v3 origin = first ? eye : V(SH_LD(c_ox[q]), SH_LD(c_oy[q]), SH_LD(c_oz[q]));
            const v3 direction = V(SH_LD(c_dx[q]), SH_LD(c_dy[q]), SH_LD(c_dz[q]));
            const float4 hrec = load_hit_record(c_hit, q);
            v3 throughout = first ? V(1.0f, 1.0f, 1.0f) : V(SH_LD(c_tr[q]), SH_LD(c_tg[q]), SH_LD(c_tb[q]));
            float brdf_pdf = first ? 1.0f : SH_LD(c_pdf[q]);
            int perfect_spec = (int)(slot_word >> 31);
            shade_path<FEAT, LIST>(sc, tm, P, frame_begin, seed, bounce, last_bounce, slot, origin, direction, hrec, throughout, brdf_pdf, perfect_spec, ss);
            if (ss.shaded) n_shaded++;
            if (first) {
                if (ss.adds) radiance = radiance + ss.add;       // 0 + term: the add stays, 0 + (-0) is +0
            } else {
                radiance = ss.add;
                // A miss whose term is +-0 in every channel (a black environment, a finite throughput: every miss of such a scene) leaves the accumulator as it is,
                // bit for bit: the accumulator is never -0 (it starts as 0 + x, and a sum is -0 only if both operands are), so acc + (+-0) == acc.  A NaN term
                // compares unequal and is added.
                const bool nothing = !(hrec.x < INF_VALUE) && ss.add.x == 0.0f && ss.add.y == 0.0f && ss.add.z == 0.0f;
                adds = ss.adds && !nothing;
            }
        }
        // survivors go to consecutive indices of the other PathSoA, shadow rays get their own dense list with the path whose radiance (fr / fg / fb[slot]) their
        // contribution must be added to
        const QueueSlots at = queue_slots(lp, it, ss.want_next, ss.want_shadow, s_wcnt, s_base, append_ctr);
        if (ss.want_next) store_survivor(at.next, slot, ss);
        // the path's radiance lives in fr / fg / fb[slot] from bounce 0 on (k_trace's shadow write-back adds into it there: store_shadow_ray's ~slot): every camera
        // path stores its first value, a later bounce adds its term, if it has one, where the path's slot is; a path that ends has nothing left to store
        if (first ? live : adds) {
            if (first) store_first_radiance(slot, radiance);
            else {
                SH_COLD(ca);
                float *const f_r = ca->ps.fr, *const f_g = ca->ps.fg, *const f_b = ca->ps.fb;
                asm volatile("" :: "s"(f_r), "s"(f_g), "s"(f_b));
                f_r[slot] = f_r[slot] + radiance.x; f_g[slot] = f_g[slot] + radiance.y; f_b[slot] = f_b[slot] + radiance.z;
            }
        }
        if (ss.want_shadow) store_shadow_ray(at.shadow, slot, ss);
    }
    __shared__ unsigned long long s_shaded;
    count_shaded(n_shaded, s_shaded, ctr);
}

// The first step of a camera path in ONE kernel (option "primary_fused"): what k_generate, k_pvb_cand and k_shade of bounce 0 do one after the other, without the
// direction (12 B written, 24 B read per path) and the hit record (16 B written, 16 B read) going through HBM in between.  k_shade's loop, literally -- shade_loop,
// queue_slots, store_survivor / store_first_radiance / store_shadow_ray, count_shaded -- around camera_path_direction, pvb_walk_list (tirt_pvb.h) and shade_path.
//   WALK:   path q of the batch: its direction, its pixel's list; a ray the list resolves is shaded on the spot (k_shade's `first` state: origin = eye, throughput 1,
//           pdf 1, perfect_spec set, slot == q) and stores its first radiance; a ray it does not resolve is appended to the leftover list -- its slot in in.ox, its
//           direction in in.dx / dy / dz: the arrays k_generate would have filled -- with a second atomic of the block between queue_slots' two barriers (its LEFT option).
//   !WALK:  after k_trace has written the leftovers' hit records to ps.hit[0 .. n): entry q of that list, shaded with the same state and the slot from the list,
//           its survivors and shadow rays appended behind the others through the same counter of bounce 0.  Nothing is scattered.
// The device counters are the three kernels': paths, rays_closest and stat[3], stat[4] (WALK), shaded (both).
template <unsigned FEAT, int MIN_WAVES, bool WALK>
__global__ __launch_bounds__(SH_BLOCK, MIN_WAVES) void k_pvb_cand_shade(ShadeArgs paths_in_kernarg_segment, SceneView sc, BvhView bv, PvbView pv, CameraView cam, TileMap tm, int P,
                                                            uint32_t frame_begin, uint32_t seed, int last_bounce,
                                                            const int *count_ptr, int count_fixed, unsigned long long *append_ctr, int *fb_count,
                                                            DevCounters *ctr, unsigned long long *stat)
{
    __shared__ unsigned s_wcnt[2][SH_BLOCK / 64], s_fcnt[2][SH_BLOCK / 64];
    __shared__ unsigned long long s_base[2];
    __shared__ int s_fbase[2];
    const ShadeLoop lp = shade_loop(count_ptr, count_fixed, blockDim.x, gridDim.x);
    const v3 eye = V(cam.eye[0], cam.eye[1], cam.eye[2]);
    unsigned long long n_shaded = 0;
    for (int it = 0; it < lp.rounds; it++) {
        const int q = lp.path(it);
        const bool live = q < lp.count;
        bool shade = false, left = false;
        int slot = 0;
        v3 direction = V(0.0f, 0.0f, 1.0f);
        float4 hrec = make_float4(INF_VALUE, 0.0f, 0.0f, __int_as_float(-1));
        if constexpr (WALK) {
            // the ray's local pixel, as k_pvb_cand finds it (pixel-block-major numbering: the 64-path chunk is the wave's, its division by F scalar)
            int k = 0;
            if (tm.F > 0) { const int ch = __builtin_amdgcn_readfirstlane(q >> 6); k = ((ch / tm.F) << 6) | (q & 63); }
            else if (live) { int f; slot_to_frame_pixel(tm, P, q, f, k); }
            slot = q;
            if (live) direction = camera_path_direction<false>(cam, tm, P, q, frame_begin, seed);
            float hit_t, hit_u, hit_v; int hit_prim, steps = 0, trips = 0;
            shade = pvb_walk_list(bv, pv, P, k, live, eye, direction, hit_t, hit_u, hit_v, hit_prim, steps, trips);
            hrec = make_float4(hit_t, hit_u, hit_v, __int_as_float(hit_prim));
            left = live && !shade;
        } else if (live) {
            SH_COLD(ca);
            const int *const c_slot = (const int *)ca->in.ox; const float4 *const c_hit = ca->ps.hit;
            const float *const c_dx = ca->in.dx, *const c_dy = ca->in.dy, *const c_dz = ca->in.dz;
            asm volatile("" :: "s"(c_slot), "s"(c_hit), "s"(c_dx), "s"(c_dy), "s"(c_dz));
            slot = SH_LD(c_slot[q]);
            direction = V(SH_LD(c_dx[q]), SH_LD(c_dy[q]), SH_LD(c_dz[q]));
            hrec = load_hit_record(c_hit, q);
            shade = true;
        }
        v3 radiance = V(0.0f, 0.0f, 0.0f);
        ShadeStep ss;
        if (shade) {
            shade_path<FEAT, false>(sc, tm, P, frame_begin, seed, 0, last_bounce, slot, eye, direction, hrec, V(1.0f, 1.0f, 1.0f), 1.0f, 1, ss);
            if (ss.shaded) n_shaded++;
            if (ss.adds) radiance = radiance + ss.add;       // 0 + term: the add stays, 0 + (-0) is +0 (k_shade at bounce 0)
        }
        // the leftover rays of the block take their places in their list between the barriers of the other two
        const QueueSlots at = queue_slots<WALK>(lp, it, ss.want_next, ss.want_shadow, s_wcnt, s_base, append_ctr, left, s_fcnt, s_fbase, fb_count, stat);
        if (WALK && left) {
            SH_COLD(ca);
            int *const l_slot = (int *)ca->in.ox; float *const l_dx = ca->in.dx, *const l_dy = ca->in.dy, *const l_dz = ca->in.dz;
            asm volatile("" :: "s"(l_slot), "s"(l_dx), "s"(l_dy), "s"(l_dz));
            l_slot[at.left] = slot; l_dx[at.left] = direction.x; l_dy[at.left] = direction.y; l_dz[at.left] = direction.z;
        }
        if (ss.want_next) store_survivor(at.next, slot, ss);
        // the path's first radiance (k_shade at bounce 0; WALK: slot == q, coalesced).  A leftover ray stores none yet: its !WALK pass does
        if (shade) store_first_radiance(slot, radiance);
        if (ss.want_shadow) store_shadow_ray(at.shadow, slot, ss);
    }
    __shared__ unsigned long long s_shaded;
    count_shaded(n_shaded, s_shaded, ctr);
    if (WALK && blockIdx.x == 0 && threadIdx.x == 0) {          // what k_generate and k_pvb_cand count
        atomicAdd(&ctr->paths, (unsigned long long)lp.count); atomicAdd(&ctr->rays_closest, (unsigned long long)lp.count);
        if (stat) atomicAdd(&stat[4], (unsigned long long)lp.count);
    }
}

// integrator/PT_RGB.py:134-136, frames applied in order
template <bool LIST>
__global__ void k_film(PathState ps, TileMap tm, int P, int F, uint32_t frame_begin, float *hdr)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    int p = mapped_pixel<LIST>(tm, k);
    float *px = hdr + (size_t)p * 3;
    float r = px[0], g = px[1], b = px[2];
    for (int f = 0; f < F; f++) {
        int s = frame_pixel_to_slot(tm, P, f, k);
        float frame = (float)(int)(frame_begin + (uint32_t)f);
        float coff = 1.0f / (frame + 1.0f);
        r = __builtin_nontemporal_load(&ps.fr[s]) * coff + r * (1.0f - coff);
        g = __builtin_nontemporal_load(&ps.fg[s]) * coff + g * (1.0f - coff);
        b = __builtin_nontemporal_load(&ps.fb[s]) * coff + b * (1.0f - coff);
    }
    px[0] = r; px[1] = g; px[2] = b;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PT_Spec (integrator/PT_Spec.py:181-279) on the same wavefront: k_generate and the traversal launches are PT_RGB's, the
// shading kernel and the film update are spectral.  Path state in the same PathSoA arrays: throughput[4] in (tr, tg, tb, brdf_pdf),
// radiance[4] in (rr, rg, rb, flags) -- PT_Spec carries no brdf_pdf and no perfect_spec flag from one bounce to the next (its
// `perfect_spec` is reset to 1 at the top of every loop iteration, PT_Spec.py:214, so the emission hit is never MIS-weighted) --;
// the hero wavelength is not stored: Lambda = 360 + 100 * rand(pixel, frame, TM_DIM_SPEC_LAMBDA) is recomputed where it is needed.
// Reference behaviours kept: the NEE sample is tinted with the colour of the surface that was HIT (`light_tint` of :213), not with
// the light's emission; Disney.evaluate_pdf for the continuation is called with (N, V = next_dir, L = -direction) (:251).
//
// KAT: the known-answer instantiation behind tirt_kat_shade_spec_step (include/tirt.h) -- this kernel's shading body, the same text, on row q of a table in place of
// path q of a queue.  What differs is compiled under `if constexpr (KAT)` and nowhere else: the path's state and its (seed, pixel, frame, bounce, last_bounce) come
// from the row's 23 words, and the step's answers go to the 29 words of the output row instead of the queues (no compaction, no atomics, no statistic).  Its
// arguments: paths.in.ox = the input rows, paths.out.ox = the output rows, count_fixed = the number of rows, P = the input stride, tm.H = the output stride,
// count_ptr = nullptr; the others are unused.  The render's instantiations (KAT == false) hold no trace of it: their instruction text is the kernel's before
// the parameter was added (tools/isa_stats.py; docs/HISTORY.md).
[[maybe_unused]] constexpr int KAT_SPEC_STEP_IN = 23, KAT_SPEC_STEP_OUT = 29;
template <unsigned FEAT, bool KAT = false>
__global__ __launch_bounds__(SH_BLOCK, 4) void k_shade_spec(ShadeArgs paths_in_kernarg_segment, SceneView sc, SpecView sp, TileMap tm, int P,
                                                   uint32_t frame_begin, uint32_t seed_of_batch, int bounce_of_launch, int last_bounce_of_launch,
                                                   const int *count_ptr, int count_fixed, unsigned long long *append_ctr,
                                                   DevCounters *ctr, v3 eye)
{
    __shared__ unsigned s_wcnt[2][SH_BLOCK / 64];
    __shared__ unsigned long long s_base[2];
    const ShadeLoop lp = shade_loop(count_ptr, count_fixed, blockDim.x, gridDim.x);
    unsigned long long n_shaded = 0;
    for (int it = 0; it < lp.rounds; it++) {
        const int q = lp.path(it);
        bool live = q < lp.count, want_next = false, want_shadow = false;
        int slot = 0;
        f4s radiance = f4_set(0.0f), next_thr = radiance, sh_c = radiance;
        v3 next_o = V(0.0f, 0.0f, 0.0f), next_d = next_o, sh_o = next_o, sh_d = next_o;
        float sh_dist = 0.0f; int sh_expect = -2;
        [[maybe_unused]] const unsigned long long n_shaded_before = n_shaded;
        if (live) {
            // a row's words (KAT); integers travel as their bit patterns
            [[maybe_unused]] const float *const row = KAT ? paths_in_kernarg_segment.in.ox + (size_t)q * (size_t)P : nullptr;
            const uint32_t seed = KAT ? (uint32_t)__float_as_int(row[0]) : seed_of_batch;
            const int bounce = KAT ? __float_as_int(row[3]) : bounce_of_launch;
            const int last_bounce = KAT ? (int)(__float_as_int(row[4]) != 0) : last_bounce_of_launch;
            const bool first = KAT ? false : bounce == 0;
            SH_COLD(ca);          // (the path-state pointers: read here, in one batch of scalar loads -- see k_shade)
            const int *const c_slot = ca->in.slot; const float4 *const c_hit = ca->ps.hit;
            const float *const c_ox = ca->in.ox, *const c_oy = ca->in.oy, *const c_oz = ca->in.oz, *const c_dx = ca->in.dx, *const c_dy = ca->in.dy, *const c_dz = ca->in.dz;
            const float *const c_tr = ca->in.tr, *const c_tg = ca->in.tg, *const c_tb = ca->in.tb, *const c_rr = ca->in.rr, *const c_rg = ca->in.rg, *const c_rb = ca->in.rb;
            const float *const c_tw = ca->in.brdf_pdf, *const c_rw = (const float *)ca->in.flags;
            asm volatile("" :: "s"(c_slot), "s"(c_hit), "s"(c_ox), "s"(c_oy), "s"(c_oz), "s"(c_dx), "s"(c_dy), "s"(c_dz), "s"(c_tr), "s"(c_tg), "s"(c_tb),
                         "s"(c_rr), "s"(c_rg), "s"(c_rb), "s"(c_tw), "s"(c_rw));
            uint32_t pixel, frame;
            if constexpr (KAT) { pixel = (uint32_t)__float_as_int(row[1]); frame = (uint32_t)__float_as_int(row[2]); }
            else {
                slot = first ? q : c_slot[q];
                int f, k; slot_to_frame_pixel(tm, P, slot, f, k);
                pixel = (uint32_t)local_to_pixel(tm, k);
                frame = frame_begin + (uint32_t)f;
            }
            const uint32_t dim0 = TM_DIM_BOUNCE0 + TM_DIMS_PER_BOUNCE * (uint32_t)bounce;
            const float Lambda = HERO_LAMBDA_MIN + HERO_LAMBDA_STEP * tm_rand(seed, pixel, frame, TM_DIM_SPEC_LAMBDA);     // PT_Spec.py:191
            v3 origin, direction; float4 hrec;
            f4s throughout = f4_set(1.0f);
            if constexpr (KAT) {
                origin = V(row[5], row[6], row[7]); direction = V(row[8], row[9], row[10]); hrec = make_float4(row[11], row[12], row[13], row[14]);
                for (int w = 0; w < HERO_N; w++) { throughout.v[w] = row[15 + w]; radiance.v[w] = row[19 + w]; }
            } else {
                origin = first ? eye : V(c_ox[q], c_oy[q], c_oz[q]);
                direction = V(c_dx[q], c_dy[q], c_dz[q]);
                hrec = load_hit_record(c_hit, q);
                if (!first) {
                    throughout.v[0] = c_tr[q]; throughout.v[1] = c_tg[q]; throughout.v[2] = c_tb[q]; throughout.v[3] = c_tw[q];
                    radiance.v[0] = c_rr[q]; radiance.v[1] = c_rg[q]; radiance.v[2] = c_rb[q]; radiance.v[3] = c_rw[q];
                }
            }
            const float t = hrec.x;
            const f4s light_rad = hero_sample(sp.spd[0], Lambda);                                   // :212
            if (t < INF_VALUE) {
                const int prim_id = __float_as_int(hrec.w);
                int mat_id;
                const HitAttr h = hit_attributes_rec(sc.shade_rec, origin, direction, prim_id, t, hrec.y, hrec.z, mat_id);
                const v3 normal = h.nor;
                const v3 fnormal = normal * signf(dot(-direction, h.gnor));
                const float *m = sc.material + (size_t)mat_id * MAT_VEC;
                const v3 mat_color = V(m[2], m[3], m[4]);
                const int mat_type = (int)m[0];
                const f4s light_tint = emission_to_rad(sp, mat_color, Lambda);                      // :213 (the HIT material's colour)
                if (mat_type == MAT_LIGHT) {                                                        // :216-226
                    const float fCosTheta = dot(direction, normal);
                    if (fCosTheta < 0.0f) radiance = radiance + ((throughout * light_rad) * light_tint);
                } else {
                    n_shaded++;
                    const f4s reflect_spec = get_spec_power(sp, m, Lambda);
                    v3 next_dir; float f_or_b = 1.0f, brdf = 1.0f, brdf_pdf = 1.0f;
                    if ((FEAT & SF_GLASS) && mat_type == MAT_GLASS) {                               // :234-238
                        const int index = (int)(tm_rand(seed, pixel, frame, dim0 + TM_SLOT_HERO) * (float)HERO_N);
                        const float rnd_lambda = Lambda + (float)index * HERO_LAMBDA_STEP;
                        next_dir = glass_sample_lambda(direction, normal, rnd_lambda, tm_rand(seed, pixel, frame, dim0 + TM_SLOT_GLASS), f_or_b);
                    } else {
                        if (!(FEAT & SF_NO_LIGHT) || sc.light_count > 0) {                          // :240-249, Scene.sample_li
                            int lidx = (int)(tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LIGHT) * (float)sc.light_count);
                            if (lidx >= sc.light_count) lidx = sc.light_count - 1;
                            const float ra = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LA);
                            const float rb = tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LB);
                            v3 light_pos, light_normal;
                            const LightRec lr = light_sample_rec<FEAT>(sc.light_rec, lidx, ra, rb, light_pos, light_normal);
                            const float light_choice_pdf = lr.choice_pdf;          // (of light_shape_visible only the laser's pdf is used by :245: it is in the record)
                            light_normal = normalized(light_normal);
                            v3 light_dir = h.pos - light_pos;
                            const float light_dist = norm(light_dir);
                            light_dir = light_dir / light_dist;
                            const float NdotL_surface = dot(fnormal, light_dir);
                            const float NdotL_light = dot(light_normal, light_dir);
                            if ((NdotL_surface < 0.0f) & (NdotL_light > 0.0f)) {
                                want_shadow = true;
                                float e_pdf;
                                const float e_brdf = disney_evaluate_pdf(m, fnormal, -direction, -light_dir, e_pdf);
                                const float light_pdf = light_dist * light_dist * light_choice_pdf / NdotL_light;
                                f4s c = f4_set(0.0f);
                                int expect = -2;
                                if (e_pdf > 0.0f) {
                                    const float w = power_heuristic(light_pdf, e_pdf) / maxf(0.0001f, light_pdf);
                                    c = light_rad * w;
                                    c = c * light_tint;
                                    c = c * throughout;
                                    c = c * reflect_spec;
                                    c = c * e_brdf;
                                    c = c * absf(NdotL_surface);
                                    expect = prim_id;
                                }
                                sh_o = light_pos; sh_d = light_dir; sh_c = c; sh_expect = expect; sh_dist = light_dist;
                            }
                        }
                        next_dir = disney_sample(m, direction, fnormal, tm_rand(seed, pixel, frame, dim0 + TM_SLOT_LOBE),
                                                 tm_rand(seed, pixel, frame, dim0 + TM_SLOT_R1), tm_rand(seed, pixel, frame, dim0 + TM_SLOT_R2));
                        f_or_b = 1.0f;
                        brdf = disney_evaluate_pdf(m, fnormal, next_dir, -direction, brdf_pdf);     // (N, V = next_dir, L = -direction): :251
                        brdf *= absf(dot(normal, next_dir));
                    }
                    const v3 next_origin = offset_ray(h.pos, fnormal * signf(f_or_b));             // :254
                    if ((brdf_pdf > 0.0f) & (maxf(throughout.v[2], maxf(throughout.v[0], throughout.v[1])) > 0.0f)) {      // :256-258
                        throughout = throughout * ((reflect_spec * brdf) / brdf_pdf);
                        want_next = !last_bounce;
                        next_o = next_origin; next_d = next_dir; next_thr = throughout;
                    }
                }
            } else {                                                                                // :262-270: the analytic sky
                const float dis = tm_sqrt(direction.x * direction.x + direction.z * direction.z);
                const float beta = tm_atan2(direction.y, dis);
                const float gamma = tm_acos(dot(direction, V(sp.sun_dir[0], sp.sun_dir[1], sp.sun_dir[2])));
                const float theta = clampf(0.5f * PI_SCENE - beta, 0.0f, 0.5f * PI_SCENE);
                f4s ibl;
                for (int w = 0; w < HERO_N; w++) ibl.v[w] = sky_radiance(sp, theta, gamma, Lambda + (float)w * HERO_LAMBDA_STEP);
                radiance = radiance + ((throughout * ibl) * light_rad);
            }
        }
        if constexpr (KAT) {          // the row's answers: what the stores below would write, and whether the row was counted as shaded
            if (live) {
                float *const o = paths_in_kernarg_segment.out.ox + (size_t)q * (size_t)tm.H;
                for (int w = 0; w < HERO_N; w++) { o[w] = radiance.v[w]; o[12 + w] = next_thr.v[w]; o[23 + w] = sh_c.v[w]; }
                o[4] = __int_as_float(n_shaded != n_shaded_before ? 1 : 0); o[5] = __int_as_float(want_next ? 1 : 0);
                o[6] = next_o.x; o[7] = next_o.y; o[8] = next_o.z; o[9] = next_d.x; o[10] = next_d.y; o[11] = next_d.z;
                o[16] = __int_as_float(want_shadow ? 1 : 0);
                o[17] = sh_o.x; o[18] = sh_o.y; o[19] = sh_o.z; o[20] = sh_d.x; o[21] = sh_d.y; o[22] = sh_d.z;
                o[27] = __int_as_float(sh_expect); o[28] = sh_dist;
            }
            continue;
        }
        const QueueSlots at = queue_slots(lp, it, want_next, want_shadow, s_wcnt, s_base, append_ctr);
        // a path that goes on carries its radiance along; one that ends stores it where k_film_spec reads it
        if (want_next) store_survivor_spec(at.next, slot, next_o, next_d, next_thr, radiance);
        else if (live) {
            SH_COLD(ca);
            float *const f_r = ca->ps.fr, *const f_g = ca->ps.fg, *const f_b = ca->ps.fb, *const f_w = ca->ps.fw;
            asm volatile("" :: "s"(f_r), "s"(f_g), "s"(f_b), "s"(f_w));
            f_r[slot] = radiance.v[0]; f_g[slot] = radiance.v[1]; f_b[slot] = radiance.v[2]; f_w[slot] = radiance.v[3];
        }
        if (want_shadow) store_shadow_ray_spec(at.shadow, want_next ? at.next : ~slot, sh_o, sh_d, sh_c, sh_expect, sh_dist);
    }
    if constexpr (KAT) return;
    __shared__ unsigned long long s_shaded;
    count_shaded(n_shaded, s_shaded, ctr);
}

// integrator/PT_Spec.py:141-158 (AddSplat) + :273-274, frames applied in order
__global__ void k_film_spec(PathState ps, const float *fw, SpecView sp, TileMap tm, int P, int F, uint32_t frame_begin, uint32_t seed, float *hdr)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = local_to_pixel(tm, k);
    float *px = hdr + (size_t)p * 3;
    float r = px[0], g = px[1], b = px[2];
    for (int f = 0; f < F; f++) {
        const int s = frame_pixel_to_slot(tm, P, f, k);
        const uint32_t frame = frame_begin + (uint32_t)f;
        const float coff = 1.0f / ((float)(int)frame + 1.0f);
        const float Lambda = HERO_LAMBDA_MIN + HERO_LAMBDA_STEP * tm_rand(seed, (uint32_t)p, frame, TM_DIM_SPEC_LAMBDA);
        f4s spec; spec.v[0] = ps.fr[s]; spec.v[1] = ps.fg[s]; spec.v[2] = ps.fb[s]; spec.v[3] = fw[s];
        spec_add_splat(sp, spec, Lambda, coff, r, g, b);
    }
    px[0] = r; px[1] = g; px[2] = b;
}

// ---- known-answer evaluation of one shading step (tirt_kat_shade_step, include/tirt.h): shade_path<FEAT> -- the body of k_shade<FEAT> -- on row i of a table of
// hit records and path states, on the context's own tables.  (pixel, frame) reach it the way they reach k_shade, through a TileMap: one tile that holds every
// pixel (local pixel = pixel), frame-major paths with P = INT_MAX (slot = pixel gives frame 0 of the batch) and frame_begin = the row's frame.  Rows: the 23
// words in / 28 words out of include/tirt.h; integers travel as their bit patterns. ----
[[maybe_unused]] constexpr int KAT_STEP_IN = 23, KAT_STEP_OUT = 28;
template <unsigned FEAT, int MIN_WAVES>
__global__ __launch_bounds__(SH_BLOCK, MIN_WAVES) void k_kat_shade_step(SceneView sc, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + (size_t)i * in_stride;
    float *o = out + (size_t)i * out_stride;
    const TileMap tm = {0, 1, 0x7fffffff, 1, 0, 0};
    v3 radiance = V(a[18], a[19], a[20]);
    ShadeStep ss;
    shade_path<FEAT>(sc, tm, 0x7fffffff, (uint32_t)__float_as_int(a[2]), (uint32_t)__float_as_int(a[0]), __float_as_int(a[3]), __float_as_int(a[4]) != 0, __float_as_int(a[1]),
                     V(a[5], a[6], a[7]), V(a[8], a[9], a[10]), make_float4(a[11], a[12], a[13], a[14]), V(a[15], a[16], a[17]), a[21], __float_as_int(a[22]), ss);
    if (ss.adds) radiance = radiance + ss.add;      // the plain add, whatever the term: a row's radiance may be -0, which k_shade's accumulator never is
    o[0] = radiance.x; o[1] = radiance.y; o[2] = radiance.z; o[3] = __int_as_float(ss.shaded ? 1 : 0); o[4] = __int_as_float(ss.want_next ? 1 : 0);
    o[5] = ss.next_o.x; o[6] = ss.next_o.y; o[7] = ss.next_o.z; o[8] = ss.next_d.x; o[9] = ss.next_d.y; o[10] = ss.next_d.z;
    o[11] = ss.next_thr.x; o[12] = ss.next_thr.y; o[13] = ss.next_thr.z; o[14] = ss.next_pdf; o[15] = __int_as_float(ss.next_spec); o[16] = __int_as_float(ss.want_shadow ? 1 : 0);
    o[17] = ss.sh_o.x; o[18] = ss.sh_o.y; o[19] = ss.sh_o.z; o[20] = ss.sh_d.x; o[21] = ss.sh_d.y; o[22] = ss.sh_d.z;
    o[23] = ss.sh_c.x; o[24] = ss.sh_c.y; o[25] = ss.sh_c.z; o[26] = __int_as_float(ss.sh_expect); o[27] = ss.sh_dist;
}

// ---- the instantiations of the shading kernels.  One table for PT_RGB (SHADE_RGB: k_shade, its LIST variant and the known-answer twin k_kat_shade_step of every
// word), one for PT_Spec (SHADE_SPEC_INST), and one rule that chooses from either (pick_shade).  The stored words, narrowest first: sphere lights, mesh lights, SF_ALL
// -- every feature of an untextured scene; it serves every other one of those, and all of them when the option "shade_specialize" is 0 --, SF_ALL with the albedo
// lookup, and that with the roughness / metallic / normal-map lookups (SF_TEXTURE_PARAM).  Behind them the twins of SF_ALL and of the kernel with every texture slot
// for each combination of the three derived bits (SF_DERIVED, tirt_internal.h: the environment's light sample, RGBE8 texels, emitters chosen by power); launch
// bounds: DESIGN.md, "HDR environment" and the sections before it. ----
typedef void (*shade_fn_t)(ShadeArgs, SceneView, TileMap, int, uint32_t, uint32_t, int, int, const int *, int, unsigned long long *, DevCounters *, v3);
typedef void (*shade_spec_fn_t)(ShadeArgs, SceneView, SpecView, TileMap, int, uint32_t, uint32_t, int, int, const int *, int, unsigned long long *, DevCounters *, v3);
typedef void (*kat_step_fn_t)(SceneView, const float *, int, float *, int, int);
typedef void (*fused_fn_t)(ShadeArgs, SceneView, BvhView, PvbView, CameraView, TileMap, int, uint32_t, uint32_t, int, const int *, int, unsigned long long *, int *, DevCounters *, unsigned long long *);
// fn_list: the same kernel for the batches of a pixel set (LIST); kat: tirt_kat_shade_step's; fused, fused_rest: the first step of a camera path in one kernel
// (k_pvb_cand_shade with WALK) and its pass over the rays the lists left to k_trace (without)
struct ShadeInst { unsigned feat; shade_fn_t fn, fn_list; kat_step_fn_t kat; fused_fn_t fused, fused_rest; };
struct ShadeSpecInst { unsigned feat; shade_spec_fn_t fn, kat; };      // kat: tirt_kat_shade_spec_step's (k_shade_spec<feat, true>)
template <unsigned F, int MW, int MW_WALK = MW>      // MW_WALK: the bound of the fused kernel that walks the lists, where it differs (SH_MIN_WAVES_FUSED_WIDE)
constexpr ShadeInst shade_inst() { return {F, k_shade<F, MW>, k_shade<F, MW, true>, k_kat_shade_step<F, MW>, k_pvb_cand_shade<F, MW_WALK, true>, k_pvb_cand_shade<F, MW, false>}; }
// (Built and left out: SF_GLASS | SF_ENV | SF_LIGHT_SPHERE for Teapot and the gallery spheres -- 3 509 VALU against the generic 3 872, but 12 bytes of scratch at
// the 96-VGPR limit where the generic kernel has none; those scenes stay on the generic kernel.)
constexpr unsigned SF_I_MAPS = SF_ALL | SF_TEXTURE | SF_TEXTURE_PARAM;               // every texture slot of a material row
constexpr unsigned SF_E = SF_ENV_SAMPLE, SF_H = SF_ENV_HDR, SF_P = SF_LIGHT_POWER;
static const ShadeInst SHADE_RGB[] = {
    shade_inst<SF_LIGHT_SPHERE, SH_MIN_WAVES_NARROW, SH_MIN_WAVES_FUSED_NARROW>(),      // Disney, sphere lights, black environment: the synthetic headline scene
    shade_inst<SF_LIGHT_TRI, SH_MIN_WAVES_NARROW, SH_MIN_WAVES_FUSED_NARROW>(),         // Disney, mesh lights, black environment: Cornell box, Veach
    shade_inst<SF_ALL, SH_MIN_WAVES, SH_MIN_WAVES_FUSED_WIDE>(),
    shade_inst<SF_ALL | SF_TEXTURE, SH_MIN_WAVES, SH_MIN_WAVES_FUSED_WIDE>(),         // textured scenes: the generic kernel + the albedo lookup
    shade_inst<SF_I_MAPS, SH_MIN_WAVES_MAPS>(),              // + roughness, metallic and normal maps
    shade_inst<SF_ALL | SF_E, SH_MIN_WAVES_ENV>(), shade_inst<SF_I_MAPS | SF_E, SH_MIN_WAVES_ENV>(),
    shade_inst<SF_ALL | SF_H, SH_MIN_WAVES_HDR, SH_MIN_WAVES_FUSED_WIDE>(), shade_inst<SF_I_MAPS | SF_H, SH_MIN_WAVES_MAPS>(),
    shade_inst<SF_ALL | SF_E | SF_H, SH_MIN_WAVES_ENV>(), shade_inst<SF_I_MAPS | SF_E | SF_H, SH_MIN_WAVES_ENV>(),
    shade_inst<SF_ALL | SF_P, SH_MIN_WAVES_POWER>(), shade_inst<SF_I_MAPS | SF_P, SH_MIN_WAVES_MAPS>(),
    shade_inst<SF_ALL | SF_E | SF_P, SH_MIN_WAVES_ENV>(), shade_inst<SF_I_MAPS | SF_E | SF_P, SH_MIN_WAVES_ENV>(),
    shade_inst<SF_ALL | SF_H | SF_P, SH_MIN_WAVES_POWER>(), shade_inst<SF_I_MAPS | SF_H | SF_P, SH_MIN_WAVES_MAPS>(),
    shade_inst<SF_ALL | SF_E | SF_H | SF_P, SH_MIN_WAVES_ENV>(), shade_inst<SF_I_MAPS | SF_E | SF_H | SF_P, SH_MIN_WAVES_ENV>()};
static const ShadeSpecInst SHADE_SPEC_INST[] = {
    {SF_LIGHT_SPHERE, k_shade_spec<SF_LIGHT_SPHERE>, k_shade_spec<SF_LIGHT_SPHERE, true>}, {SF_LIGHT_TRI, k_shade_spec<SF_LIGHT_TRI>, k_shade_spec<SF_LIGHT_TRI, true>},
    {SF_ALL, k_shade_spec<SF_ALL>, k_shade_spec<SF_ALL, true>}};
// The rule: the first entry, in table order, that carries exactly the word's derived bits and covers its other bits (SF_CUTOUT aside: no instantiation depends on it);
// with specialize == 0 only the entries that carry all of SF_ALL.  Null where the table has none: no word that a context can hold
template <class T, size_t N>
static const T *pick_shade(const T (&tab)[N], unsigned word, int specialize)
{
    for (const T &e : tab)
        if ((e.feat & SF_DERIVED) == (word & SF_DERIVED) && (word & ~SF_CUTOUT & ~e.feat) == 0u && (specialize || (e.feat & SF_ALL) == SF_ALL)) return &e;
    return nullptr;
}
bool shade_instantiation(unsigned word, int specialize, bool spectral, unsigned *feat)      // behind tirt_shade_instantiation: the rule, no context
{
    if (spectral) { const ShadeSpecInst *e = pick_shade(SHADE_SPEC_INST, word, specialize); if (e) *feat = e->feat; return e != nullptr; }
    const ShadeInst *e = pick_shade(SHADE_RGB, word, specialize); if (e) *feat = e->feat; return e != nullptr;
}

// ---- the entry behind tirt_kat_shade_step: the known-answer twin of the instantiation whose word is exactly `feat` ----
static kat_step_fn_t kat_step_inst(unsigned feat)
{
    for (const ShadeInst &e : SHADE_RGB) if (e.feat == feat) return e.kat;
    return nullptr;
}
bool kat_shade_step_has_inst(unsigned feat) { return kat_step_inst(feat) != nullptr; }
// the arguments that need no context were checked by the caller (tirt_api.hip); here: what depends on the scene, then the launch
int kat_shade_step(tirt_ctx *c, unsigned feat, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(c->n >= 1, "tirt_kat_shade_step: no scene");
    const unsigned word = shade_word(c);           // (bit 4096 of it counts only after ensure_shade_records: read again below)
    TIRT_REQUIRE((word & ~SF_DERIVED & ~feat) == 0u, "tirt_kat_shade_step: feat does not cover the scene's feature word (tirt_shade_features)");
    TIRT_REQUIRE(((feat ^ word) & SF_ENV_HDR) == 0u, "tirt_kat_shade_step: an instantiation with bit 2048 reads RGBE8 texels and one without it 8-bit texels: feat must carry the bit exactly when tirt_shade_features does");
    TIRT_REQUIRE((feat & SF_ENV_SAMPLE & ~word) == 0u, "tirt_kat_shade_step: an instantiation with bit 1024 needs the environment's sampling table (tirt_env_sampling on, a lit environment)");
    if (feat & SF_LIGHT_POWER) {                   // the table is built with the light records, lazily
        if (sync_all(c) || ensure_shade_records(c)) return TIRT_ERR_HIP;
        TIRT_REQUIRE(shade_word(c) & SF_LIGHT_POWER, "tirt_kat_shade_step: an instantiation with bit 4096 needs the emitters' table (tirt_light_sampling mode 1, triangle and sphere emitters only, total > 0)");
    }
    const kat_step_fn_t fn = kat_step_inst(feat);
    TIRT_REQUIRE(fn, "tirt_kat_shade_step: feat is not an instantiation of k_shade");
    TIRT_REQUIRE(!(feat & (SF_TEXTURE | SF_TEXTURE_PARAM)) || c->tex_count > 0, "tirt_kat_shade_step: the textured instantiation needs uploaded textures (tirt_texture_upload): without them no material row's slot is checked");
    for (int i = 0; i < n; i++) {
        const float *a = in + (size_t)i * in_stride;
        const int32_t *w = (const int32_t *)a; const int32_t prim = w[14], pixel = w[1];
        TIRT_REQUIRE(!(a[11] < INF_VALUE) || (prim >= 0 && prim < c->n), "tirt_kat_shade_step: row " + std::to_string(i) + ": prim outside [0, n_prims) of a hit (t < INF)");
        TIRT_REQUIRE(pixel >= 0 && pixel < 0x7fffffff, "tirt_kat_shade_step: row " + std::to_string(i) + ": pixel outside [0, 2^31 - 1)");
    }
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (ensure_shade_records(c)) return TIRT_ERR_HIP;
    return kat_round_trip(c, "tirt_kat_shade_step", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(fn, dim3((n + SH_BLOCK - 1) / SH_BLOCK), dim3(SH_BLOCK), 0, c->stream, scene_view(c), (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

// ---- the entry behind tirt_kat_shade_spec_step: the known-answer twin of the instantiation of k_shade_spec whose word is exactly `feat` ----
static shade_spec_fn_t kat_spec_step_inst(unsigned feat)
{
    for (const ShadeSpecInst &e : SHADE_SPEC_INST) if (e.feat == feat) return e.kat;
    return nullptr;
}
bool kat_shade_spec_step_has_inst(unsigned feat) { return kat_spec_step_inst(feat) != nullptr; }
// the arguments that need no context were checked by the caller (tirt_kat.hip); here: what depends on the scene and the tables, then the launch
int kat_shade_spec_step(tirt_ctx *c, unsigned feat, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(c->n >= 1, "tirt_kat_shade_spec_step: no scene");
    TIRT_REQUIRE(c->spec_set && c->spec_view, "tirt_kat_shade_spec_step: no spectral tables (tirt_spectral_upload first)");
    // the word pt_render picks k_shade_spec's instantiation by: the context's stored word, without the derived bits PT_Spec never sees
    TIRT_REQUIRE((c->shade_features & ~SF_CUTOUT & ~feat) == 0u, "tirt_kat_shade_spec_step: feat does not cover the scene's feature word (tirt_shade_features)");
    const shade_spec_fn_t fn = kat_spec_step_inst(feat);
    TIRT_REQUIRE(fn, "tirt_kat_shade_spec_step: feat is not an instantiation of k_shade_spec");
    for (int i = 0; i < n; i++) {
        const float *a = in + (size_t)i * in_stride;
        const int32_t *w = (const int32_t *)a; const int32_t prim = w[14], pixel = w[1];
        TIRT_REQUIRE(!(a[11] < INF_VALUE) || (prim >= 0 && prim < c->n), "tirt_kat_shade_spec_step: row " + std::to_string(i) + ": prim outside [0, n_prims) of a hit (t < INF)");
        TIRT_REQUIRE(pixel >= 0 && pixel < 0x7fffffff, "tirt_kat_shade_spec_step: row " + std::to_string(i) + ": pixel outside [0, 2^31 - 1)");
    }
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (ensure_shade_records(c)) return TIRT_ERR_HIP;
    return kat_round_trip(c, "tirt_kat_shade_spec_step", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        // the arguments of k_shade_spec<feat, true>: rows in and out where a render has its path arrays, the strides in P and tm.H, n as the fixed count
        ShadeArgs rows{}; rows.in.ox = (float *)const_cast<void *>(din[0]); rows.out.ox = (float *)dout;
        TileMap tm{}; tm.H = out_stride;
        hipLaunchKernelGGL(fn, dim3((n + SH_BLOCK - 1) / SH_BLOCK), dim3(SH_BLOCK), 0, c->stream, rows, scene_view(c), *(const SpecView *)c->spec_view, tm, in_stride,
                           0u, 0u, 0, 0, (const int *)nullptr, n, (unsigned long long *)nullptr, (DevCounters *)nullptr, V(0.0f, 0.0f, 0.0f));
    });
}

// ---------------------------------------------------------------------------------------------
// The scheduler: a batch's launches on a lane's stream
// ---------------------------------------------------------------------------------------------
// Per-batch device counters of a lane: one packed append counter per bounce (low word: paths that go on
// to bounce b+1, high word: shadow rays of bounce b), each in its own 128-byte line, then the sliced
// ray-fetch cursors of the max_depth + 1 traversal launches.
constexpr size_t LINE = 128;
static size_t lane_counter_bytes(int max_depth)
{ return LINE * (size_t)(max_depth + 1) + sizeof(int) * TR_FETCH_STRIDE * TR_FETCH_LINES * (size_t)(max_depth + 1); }

constexpr int PATH_WORDS = 2 * 15 + 4 + 12 + 3 + 2;  // two PathSoA + hit record + shadow ray + final radiance + the two fourth-wavelength words of PT_Spec
static size_t path_state_bytes(size_t S) { return sizeof(float) * PATH_WORDS * ((S + 3) & ~(size_t)3); }
static int ensure_paths(Lane &L, size_t S, int max_depth)
{
    if (S > L.path_capacity || !L.path_mem.p) {
        if (L.path_mem.ensure(path_state_bytes(S))) return TIRT_ERR_HIP;
        const size_t S_user = S;
        S = (S + 3) & ~(size_t)3;                     // array pitch: keeps every array (and the float4 hit records) 16-byte aligned
        float *w = L.path_mem.as<float>();
        PathState &p = L.ps;
        auto nxt = [&]() { float *r = w; w += S; return r; };
        for (int k = 0; k < 2; k++) {
            PathSoA &q = p.st[k];
            q.ox = nxt(); q.oy = nxt(); q.oz = nxt(); q.dx = nxt(); q.dy = nxt(); q.dz = nxt();
            q.tr = nxt(); q.tg = nxt(); q.tb = nxt(); q.rr = nxt(); q.rg = nxt(); q.rb = nxt();
            q.brdf_pdf = nxt(); q.flags = (uint32_t *)nxt(); q.slot = (int *)nxt();
        }
        p.hit = (float4 *)w; w += 4 * S;             // S is a multiple of 4 words from a 256-byte aligned base: 16-byte aligned
        p.sox = nxt(); p.soy = nxt(); p.soz = nxt(); p.sdx = nxt(); p.sdy = nxt(); p.sdz = nxt();
        p.scr = nxt(); p.scg = nxt(); p.scb = nxt(); p.sprim = (int *)nxt(); p.sdist = nxt(); p.sdst = (int *)nxt();
        p.fr = nxt(); p.fg = nxt(); p.fb = nxt();
        p.scw = nxt(); p.fw = nxt();
        L.path_capacity = S_user;
    }
    if (L.counters_mem.ensure(lane_counter_bytes(max_depth))) return TIRT_ERR_HIP;
    return 0;
}

void retire_render_events(tirt_ctx *c, bool finished_only)
{
    size_t keep = 0;
    for (auto &pr : c->ev_pool) {
        if (finished_only && hipEventQuery(pr.second) != hipSuccess) { c->ev_pool[keep++] = pr; continue; }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) c->ms_render += ms;
        (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second);
    }
    c->ev_pool.resize(keep);
    if (finished_only) (void)hipGetLastError();           // hipEventQuery's hipErrorNotReady is not an error
}

// Option "time_kernels": one (begin, end) event pair around every launch of the closest-hit, shadow and shading kernels of a batch, summed into the
// context's totals once the batch is done.  Without the option begin / end do nothing.
struct KernelTimers {
    typedef std::vector<std::pair<hipEvent_t, hipEvent_t>> Pairs;
    bool on; hipStream_t st;
    Pairs closest, shadow, shade;
    void begin(Pairs &v) { if (!on) return; hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b); v.push_back({a, b}); (void)hipEventRecord(a, st); }
    void end(Pairs &v) { if (on) (void)hipEventRecord(v.back().second, st); }
    static void sum(Pairs &v, double &acc)      // after the stream has been synchronised
    {
        for (auto &pr : v) { float ms = 0; (void)hipEventElapsedTime(&ms, pr.first, pr.second); acc += ms; (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        v.clear();
    }
};

// Frames per batch: up to batch_paths pixel-samples in flight (the per-bounce launches of a batch end in a latency-bound tail of a few long
// rays, so bigger batches amortise it), in batches of equal size, as many as come closest to the planned size (up to 1.5 x it: never a full batch and a sliver)
static int frames_per_batch(const tirt_ctx *c, int frame_count, int P)
{
    const size_t batch_paths = effective_batch_paths(c);
    size_t nb = ((size_t)frame_count * P + batch_paths / 2) / batch_paths; if (nb < 1) nb = 1;
    int FB = (int)((frame_count + nb - 1) / nb);
    // A rank of a wide multi-GPU job renders its whole share as ONE batch, with nothing to overlap the per-bounce tails with:
    // as two half batches on two lanes it is 3.4 % faster at 8 ranks (measured on one GPU rendering rank 0's tiles; at 4 ranks
    // and below, and for a single GPU's stream of full batches, the halves lose 1-9 %: there 32 Mi-path batches win).
    // (Only for the first batch after a synchronisation: a rank with several batches in flight overlaps them anyway.)
    if (c->split_lone >= 2 && c->tile_count >= 6 && c->batches_since_sync == 0 && FB == frame_count && frame_count >= 2 && c->n_lanes >= 2 &&
        !c->time_kernels && (size_t)frame_count * P >= ((size_t)12 << 20))
        { int parts = c->split_lone < c->n_lanes ? c->split_lone : c->n_lanes; if (parts > frame_count) parts = frame_count; FB = (frame_count + parts - 1) / parts; }
    return FB;
}

// what the batches of one pt_render call share
struct RenderCall {
    uint32_t seed; int max_depth, flags; const SpecView *spec;
    bool list, beams_ready;            // the batches' local pixels are a pixel set's list; the pixels' candidate lists stand (pvb_prepare)
    int P, n_lanes, spill_depth;
    SceneView sv; BvhView bv; TileMap tm; DevCounters *ctr;
};

// All lanes get their buffers up front (an allocation inside a later call would stall the pipeline), sized for what deferred submission can
// merge later (merge_paths + one call), so that a bigger merged batch does not re-allocate in the middle of a job; small films skip the head-room.
// Sets r.n_lanes and r.spill_depth.
static int prepare_lanes(tirt_ctx *c, RenderCall &r, int FB, int stack_size)
{
    const int P = r.P;
    const size_t batch_paths = effective_batch_paths(c), merge_paths = effective_merge_paths(c);
    r.n_lanes = c->time_kernels ? 1 : c->n_lanes;
    { const int need = plan_batches(c).lanes + 1; if (need < r.n_lanes) r.n_lanes = need; }      // a job of two big batches needs path state on two lanes (+ one for a call the hint did not cover), not on all
    r.spill_depth = 0;
    size_t cap = (size_t)FB * P;
    if (merge_paths > 0 && P >= 65536) {
        size_t want = batch_paths + batch_paths / 2;        // the largest batch a call can become (the same for every call: a lane never re-allocates mid-job)
        // "job_frames" hint (the example classes pass their sample count): a short job never merges more than itself
        if (c->job_frames > 0 && want > (size_t)c->job_frames * P) want = (size_t)c->job_frames * P;
        want = (want / P) * P;
        if (want > cap) cap = want;
    }
    for (int k = 0; k < r.n_lanes; k++) {
        // very large films (204 B per path and lane): use fewer lanes rather than run out of HBM
        if (k > 0 && cap > c->lanes[k].path_capacity) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < path_state_bytes(cap) + ((size_t)2 << 30)) { r.n_lanes = k; break; }
        }
        if (ensure_paths(c->lanes[k], cap, r.max_depth)) return TIRT_ERR_HIP;
        if (ensure_spill(c, c->lanes[k].spill, stack_size, r.spill_depth)) return TIRT_ERR_HIP;
    }
    return TIRT_OK;
}

// What every k_trace launch of a batch on lane L has in common: the tree, the shadow rays' arrays and the film-side target of their contributions (the
// fourth wavelength's with PT_Spec), the stack spill, the counters and the tunables.  A launch adds its rays, their count, its fetch cursors and the
// path-side target (rr / rg / rb, rw).
static TraceArgs batch_trace_args(const tirt_ctx *c, const RenderCall &r, const Lane &L)
{
    TraceArgs a = {};
    a.bvh = r.bv;
    a.sox = L.ps.sox; a.soy = L.ps.soy; a.soz = L.ps.soz; a.sdx = L.ps.sdx; a.sdy = L.ps.sdy; a.sdz = L.ps.sdz;
    a.sprim = L.ps.sprim; a.sdst = L.ps.sdst; a.sdist = L.ps.sdist; a.scr = L.ps.scr; a.scg = L.ps.scg; a.scb = L.ps.scb;
    a.fr = L.ps.fr; a.fg = L.ps.fg; a.fb = L.ps.fb;
    if (r.spec) { a.scw = L.ps.scw; a.fw = L.ps.fw; }
    a.spill = L.spill.as<int>(); a.spill_depth = r.spill_depth; a.ctr = r.ctr; a.per_ray_counts = nullptr;
    fill_tunables(c, a);
    return a;
}

// One batch -- frames [f0, f0 + F) of the call's pixels -- on lane L: camera rays, max_depth rounds of closest hits (with the previous round's shadow
// rays) and shading, the last round's shadow rays, the film update behind the previous batch's.
static int submit_batch(tirt_ctx *c, const RenderCall &r, Lane &L, uint32_t f0, int F)
{
    const int P = r.P, S = F * P, max_depth = r.max_depth, flags = r.flags, B = 256;
    const SpecView *const spec = r.spec;
    const uint32_t seed = r.seed;
    DevCounters *const ctr = r.ctr;
    hipStream_t st = L.stream;
    TileMap tm = r.tm;
    tm.F = (c->path_order_blocks && (P & 63) == 0) ? F : 0;
    const bool use_beams = r.beams_ready && F >= c->primary_beams_min_frames;
    char *cm = L.counters_mem.as<char>();
    auto append_ctr = [&](int b) { return (unsigned long long *)(cm + LINE * (size_t)b); };
    auto cnt_path = [&](int b) { return (const int *)append_ctr(b - 1); };           // live paths entering bounce b >= 1
    auto cnt_shadow = [&](int b) { return (const int *)append_ctr(b) + 1; };         // shadow rays made by bounce b
    auto fetch = [&](int launch) { return (int *)(cm + LINE * (size_t)(max_depth + 1)) + (size_t)launch * TR_FETCH_STRIDE * TR_FETCH_LINES; };
    // the batch's shading kernel (after pt_render's ensure_shade_records: shade_word).  PT_Spec never sees the derived bits, and refuses the textured scenes
    const ShadeInst *const rgb_inst = spec ? nullptr : pick_shade(SHADE_RGB, shade_word(c), c->shade_specialize);
    const ShadeSpecInst *const spec_inst = spec ? pick_shade(SHADE_SPEC_INST, c->shade_features, c->shade_specialize) : nullptr;
    TIRT_REQUIRE(rgb_inst || spec_inst, "render: no instantiation of the shading kernel serves the scene's feature word " + std::to_string(shade_word(c)) + " (tirt_shade_instantiation)");
    const shade_fn_t shade_fn = !rgb_inst ? nullptr : r.list ? rgb_inst->fn_list : rgb_inst->fn;
    const shade_spec_fn_t shade_spec_fn = spec_inst ? spec_inst->fn : nullptr;

    TIRT_HIP(hipStreamWaitEvent(st, c->ev_main, 0));
    hipEvent_t r0, r1;
    TIRT_HIP(hipEventCreate(&r0)); TIRT_HIP(hipEventCreate(&r1));
    TIRT_HIP(hipEventRecord(r0, st));
    KernelTimers t = {c->time_kernels != 0, st, {}, {}, {}};

    // the first step of the camera paths in one kernel (k_pvb_cand_shade, option "primary_fused") wherever nothing but bounce 0 itself reads the directions and
    // the hit records of the camera rays: the feature buffers do (aov_launch), PT_Spec and a pixel set have no fused kernel, the diagnostics are k_pvb_cand's
    const bool fused = use_beams && c->primary_fused && !spec && !r.list && !c->aov.p && !c->pvb_diag;

    TIRT_HIP(hipMemsetAsync(L.counters_mem.p, 0, lane_counter_bytes(max_depth), st));
    if (!fused) hipLaunchKernelGGL(r.list ? k_generate<true> : k_generate<false>, dim3((S + B - 1) / B), dim3(B), 0, st, L.ps.st[0], c->cam, tm, P, S, f0, seed, ctr);
    // a batch that will run next to the previous one (still in flight on another lane) uses fewer persistent
    // blocks, so that both traversal kernels find LDS on the CUs; a batch submitted to an idle GPU takes them all
    bool busy = false;
    if (c->last_film) { busy = hipEventQuery(c->last_film) == hipErrorNotReady; (void)hipGetLastError(); }
    // (two big batches side by side -- what plan_batches makes of a hinted job -- do best with all persistent blocks each and
    // twice the shading blocks: +2 % for 2 x 128 / 64 / 32 Mi paths; four batches in flight, or two small ones, do not: -2 %)
    const BatchPlan plan = plan_batches(c);
    const bool two_big = plan.lanes <= 2 && plan.batch >= ((size_t)24 << 20) && !c->grid_user;
    const int grid_cap = (busy && r.n_lanes > 1 && !two_big) ? c->tr_grid : c->tr_grid_alone;
    int grid_full = (S + TR_BLOCK - 1) / TR_BLOCK; if (grid_full > grid_cap) grid_full = grid_cap;
    const int sh_cap = two_big ? 2 * c->sh_grid : c->sh_grid;
    int grid_shade = (S + SH_BLOCK - 1) / SH_BLOCK; if (grid_shade > sh_cap) grid_shade = sh_cap;
    v3 eye_v; eye_v.x = c->cam.eye[0]; eye_v.y = c->cam.eye[1]; eye_v.z = c->cam.eye[2];
    const TraceArgs base = batch_trace_args(c, r, L);
    for (int b = 0; b < max_depth; b++) {
        const PathSoA &in = L.ps.st[b & 1], &out = L.ps.st[(b + 1) & 1];
        // closest hits of bounce b, together with the NEE shadow rays of bounce b-1: one launch instead of two (PT_RGB: they add into fr / fg / fb[slot],
        // which shade(b) adds to after them; PT_Spec: into `in`'s radiance, which nothing reads before shade(b) -- rr / rg / rb, rw below are PT_Spec's)
        TraceArgs a = base;
        a.dx = in.dx; a.dy = in.dy; a.dz = in.dz;
        if (b == 0) for (int k = 0; k < 3; k++) a.eye[k] = c->cam.eye[k];      // camera rays share their origin (ox stays nullptr)
        else { a.ox = in.ox; a.oy = in.oy; a.oz = in.oz; }
        a.count_ptr = (b == 0) ? nullptr : cnt_path(b); a.count_fixed = S;
        a.scount_ptr = (b == 0) ? nullptr : cnt_shadow(b - 1);
        a.hit = L.ps.hit;
        a.fetch = fetch(b);
        a.rr = in.rr; a.rg = in.rg; a.rb = in.rb;
        if (spec) a.rw = (float *)in.flags;
        a.timeline = timeline_for(c, flags, grid_full);
        // camera rays with candidate lists: each against the list of leaves its pixel's rays can hit first (tirt_pvb.hip); those that find nothing there go to k_trace.  Scratch
        // the batch does not touch before shade(0): the `out` arrays (slots, directions of the leftover rays), the shadow-ray arrays (their hit records)
        const bool beams = b == 0 && use_beams;
        int *const fb_count = (int *)append_ctr(0) + 4;          // (zeroed with the batch's counters; words 0, 1 of the line: the appends of bounce 0)
        float4 *const fb_hit = (float4 *)L.ps.sox;               // sox, soy, soz, sdx: four consecutive arrays of the lane's pitch
        // Fused: the kernel's own survivors and shadow rays go where those leftovers went, so they are listed in the `in` arrays (slots in in.ox), which nobody
        // has filled, their hit records in hit[0 .. n), which nothing reads before bounce 1 writes it; the second pass shades them from there
        const bool fuse = beams && fused;
        auto launch_fused = [&](fused_fn_t fn, const int *count_ptr) {
            const tirt_ctx::PvbSet &ps = c->pvb_set[c->pvb_cur];
            t.begin(t.shade);
            hipLaunchKernelGGL(fn, dim3(grid_shade), dim3(SH_BLOCK), 0, st, ShadeArgs{L.ps, in, out}, r.sv, r.bv, PvbView{ps.count.as<int>(), ps.cand.as<int2>(), ps.bound.as<float>()},
                               c->cam, tm, P, f0, seed, (max_depth == 1) ? 1 : 0, count_ptr, S, append_ctr(0), fb_count, ctr, c->pvb_stat.as<unsigned long long>());
            t.end(t.shade);
            c->launches_shade++;
        };
        if (fuse) {
            launch_fused(rgb_inst->fused, nullptr);
            a.count_ptr = fb_count; a.no_ray_count = 1;          // (a.dx .. a.hit: the `in` arrays and hit already)
        } else if (beams) {
            pvb_launch_cand(c, st, r.bv, in.dx, in.dy, in.dz, tm, P, S, L.ps.hit, fb_count, (int *)out.ox, out.dx, out.dy, out.dz, ctr);
            a.dx = out.dx; a.dy = out.dy; a.dz = out.dz; a.count_ptr = fb_count; a.hit = fb_hit; a.no_ray_count = 1;
        }
        t.begin(t.closest);                                      // (the traversal timers and counters see k_trace's launch, not the list pass)
        if (int rc = launch_trace(c, st, b == 0 ? KIND_CLOSEST : KIND_MIXED, a, flags, grid_full)) return rc;
        t.end(t.closest);
        if (beams && !fuse) pvb_launch_scatter(st, fb_count, (const int *)out.ox, fb_hit, L.ps.hit);
        c->launches_trace_closest++;
        if (b == 0 && c->aov.p) { if (int rc = aov_launch(c, L, tm, P, F, f0)) return rc; }      // the camera rays' hits are complete: the feature buffers read them

        if (fuse) launch_fused(rgb_inst->fused_rest, fb_count);      // the rays k_trace was asked about: their first shading step
        else {
            t.begin(t.shade);
            if (spec)
                hipLaunchKernelGGL(shade_spec_fn, dim3(grid_shade), dim3(SH_BLOCK), 0, st, ShadeArgs{L.ps, in, out}, r.sv, *spec, tm, P, f0, seed, b,
                                   (b == max_depth - 1) ? 1 : 0, (b == 0) ? (const int *)nullptr : cnt_path(b), S,
                                   append_ctr(b), ctr, eye_v);
            else
                hipLaunchKernelGGL(shade_fn, dim3(grid_shade), dim3(SH_BLOCK), 0, st, ShadeArgs{L.ps, in, out}, r.sv, tm, P, f0, seed, b,
                                   (b == max_depth - 1) ? 1 : 0, (b == 0) ? (const int *)nullptr : cnt_path(b), S,
                                   append_ctr(b), ctr, eye_v);
            t.end(t.shade);
            c->launches_shade++;
        }

        if (b == max_depth - 1) {          // the last bounce's shadow rays have no closest-hit launch to ride on
            TraceArgs sa = base;
            sa.ox = L.ps.sox; sa.oy = L.ps.soy; sa.oz = L.ps.soz; sa.dx = L.ps.sdx; sa.dy = L.ps.sdy; sa.dz = L.ps.sdz;
            sa.count_ptr = cnt_shadow(b); sa.count_fixed = 0;
            sa.fetch = fetch(max_depth);
            sa.rr = out.rr; sa.rg = out.rg; sa.rb = out.rb;
            if (spec) sa.rw = (float *)out.flags;
            t.begin(t.shadow);
            if (int rc = launch_trace(c, st, KIND_SHADOW_ACC, sa, flags, grid_full)) return rc;
            t.end(t.shadow);
            c->launches_trace_shadow++;
        }
    }
    // the running mean is order dependent: this batch's film update follows the previous batch's
    if (c->last_film) TIRT_HIP(hipStreamWaitEvent(st, c->last_film, 0));
    if (spec) hipLaunchKernelGGL(k_film_spec, dim3((P + B - 1) / B), dim3(B), 0, st, L.ps, L.ps.fw, *spec, tm, P, F, f0, seed, c->hdr.as<float>());
    else hipLaunchKernelGGL(r.list ? k_film<true> : k_film<false>, dim3((P + B - 1) / B), dim3(B), 0, st, L.ps, tm, P, F, f0, c->hdr.as<float>());
    if (c->mom.p && !spec) { if (int rc = moments_launch(c, L, tm, P, F)) return rc; }      // the sample moments read fr / fg / fb too: behind the same wait, before film_done (tirt_moments.hip)
    TIRT_HIP(hipEventRecord(L.film_done, st));
    L.film_recorded = true;
    c->last_film = L.film_done;
    if (use_beams) c->pvb_set[c->pvb_cur].busy = L.film_done;      // the last batch that reads this set of candidate lists (pvb_prepare)
    TIRT_HIP(hipEventRecord(r1, st));
    if (t.on) {
        TIRT_HIP(hipStreamSynchronize(st));
        KernelTimers::sum(t.closest, c->ms_trace_closest); KernelTimers::sum(t.shadow, c->ms_trace_shadow); KernelTimers::sum(t.shade, c->ms_shade);
    }
    c->ev_pool.push_back({r0, r1});        // retired (and destroyed) by tirt_stats / tirt_stats_reset
    if (c->ev_pool.size() > 64) retire_render_events(c, true);      // long render loops that never ask for stats: retire finished pairs
    return TIRT_OK;
}

int pt_render(tirt_ctx *c, uint32_t frame_begin, int frame_count, uint32_t seed, int max_depth, int stack_size, int flags, const SpecView *spec)
{
    TIRT_REQUIRE(c->built, "tirt_pt_rgb_render: LBVH not built");
    TIRT_REQUIRE(c->cam_set, "tirt_pt_rgb_render: camera not set");
    TIRT_REQUIRE(c->hdr.p && c->npix_local >= 0, "tirt_pt_rgb_render: film not created");
    TIRT_REQUIRE(frame_count >= 0 && max_depth >= 1 && max_depth <= 4096, "tirt_pt_rgb_render: bad frame_count/max_depth");
    // a pixel set (tirt_adaptive.hip): the batches' local pixels are its list -- P of them, planned and numbered as any P, through the LIST kernels
    const bool list = c->pixset_n >= 0;
    TIRT_REQUIRE(!(list && spec), "tirt_pt_spec_render: a pixel set is installed (PT_RGB only): tirt_pixel_set_clear first");
    if (frame_count == 0 || c->npix_local == 0 || c->pixset_n == 0) return TIRT_OK;
    if (ensure_counters(c)) return TIRT_ERR_HIP;
    if (ensure_shade_records(c)) return TIRT_ERR_HIP;          // on the main stream: the lanes wait for ev_main below
    if (int rc = ensure_cutout_records(c)) return rc;
    RenderCall r = {seed, max_depth, flags, spec, list, false, render_pixels(c), 0, 0, scene_view(c), bvh_view(c), render_tile_map(c), c->dev_counters.as<DevCounters>()};
    const int FB = frames_per_batch(c, frame_count, r.P);
    // the pixels' candidate lists for the camera rays (tirt_pvb.hip), made on the main stream when the scene, the camera or the film changed since
    // (indexed by the tiles' local pixel: the camera rays of a pixel set's batches all go through k_trace)
    // (and they assume opaque leaves: a scene with cut-outs traces its camera rays the ordinary way, as a pixel set's batches do)
    if (!list && !c->has_cutout && c->primary_beams && FB >= c->primary_beams_min_frames && !(flags & TIRT_TRAVERSE_EXHAUSTIVE)) {
        if (int rc = pvb_prepare(c)) return rc;
        r.beams_ready = c->pvb_valid;
    }
    // everything queued on the main stream (uploads, film clear, tone map) precedes the lanes' work
    TIRT_HIP(hipEventRecord(c->ev_main, c->stream));
    if (int rc = prepare_lanes(c, r, FB, stack_size)) return rc;
    for (int fb = 0; fb < frame_count; fb += FB) {
        Lane &L = c->lanes[r.n_lanes == 1 ? 0 : (c->lane_cursor++ % (unsigned)r.n_lanes)];
        c->batches_since_sync++;
        if (int rc = submit_batch(c, r, L, frame_begin + (uint32_t)fb, (frame_count - fb < FB) ? frame_count - fb : FB)) return rc;
    }
    // main-stream consumers of the film (tone map, downloads, clear) wait for c->last_film themselves
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

}  // namespace tirt
