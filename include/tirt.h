/*
 * tirt.h -- C-ABI of libtirt.so, the MI355X (gfx950) path-tracing core that sits behind
 * the ti-raytrace Scene / LBvh.Bvh / Camera / PT_RGB.PathTrace Python API.
 *
 * The reference has no FFI boundary for this path: every hot function is a @ti.kernel /
 * @ti.func JIT-compiled by Taichi and reached only from Python.  The
 * boundary is therefore defined here; each entry point cites the reference call it
 * replaces.  Plain pointers and sizes only, no torch types.  Host buffers are
 * C-contiguous f32/i32 (numpy); the caller owns them, the library copies on upload and
 * owns all device memory.  One host thread drives one tirt_ctx (one HIP device, one
 * stream).  Every function returns 0 on success, <0 on error (tirt_last_error() gives
 * the message); nothing throws across the boundary.
 *
 * Embedding.  The library itself touches no process state: no environment variable is read or written, no signal handler or
 * thread is installed (librccl is dlopen()ed by tirt_comm_init only).  A context runs up to `overlap_lanes` (default 4) HIP
 * streams side by side; the ROCm runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), so an embedder that
 * wants each lane on a queue of its own sets GPU_MAX_HW_QUEUES >= 5 before the HIP runtime initialises.  The Python package
 * ti_raytrace_amd does exactly that at import (setdefault to 8) and pre-loads PyTorch's bundled libamdhip64.so when torch is
 * installed, so that libtirt.so and torch share one runtime; TIRT_NO_ENV_TUNING=1 switches both off, TIRT_SYSTEM_HIP=1 only the
 * preload (ti_raytrace_amd/__init__.py, _native.py).  libtirt.so's DT_NEEDED entry is libamdhip64.so.7 by SONAME.
 */
#ifndef TIRT_H
#define TIRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tirt_ctx tirt_ctx;

#define TIRT_OK 0
#define TIRT_ERR_HIP (-1)      /* a HIP runtime call failed (no device, OOM, launch error) */
#define TIRT_ERR_ARG (-2)      /* bad argument / call order */
#define TIRT_ERR_BUILD (-3)    /* LBVH build did not complete (refit did not reach the root) */
#define TIRT_ERR_STACK (-4)    /* traversal stack overflow (reference: "overflow, need larger stack") */

/* tirt_pt_rgb_render / tirt_trace_* flags */
#define TIRT_TRAVERSE_ORDERED 0     /* near-first, t-culled traversal (product default)     */
#define TIRT_TRAVERSE_EXHAUSTIVE 1  /* reference visiting rule: no t-culling (Scene.py:702-744) */
#define TIRT_COUNT_NODES 2          /* accumulate N_box / N_leaf pop counts into tirt_stats  */

typedef struct {
    uint64_t rays_closest;   /* closet_hit calls        (integrator/PT_RGB.py:65)  */
    uint64_t rays_shadow;    /* closet_hit_shadow calls (integrator/PT_RGB.py:104) */
    uint64_t box_closest;    /* compact nodes popped by closest-hit rays (TIRT_COUNT_NODES) */
    uint64_t leaf_closest;   /* ... leaves among them */
    uint64_t box_shadow;
    uint64_t leaf_shadow;
    uint64_t shaded;         /* path vertices that ran the BSDF branch */
    uint64_t paths;          /* pixel-samples started */
    uint64_t stack_overflow; /* rays whose traversal overflowed stack_size */
    double ms_build;         /* last tirt_lbvh_build, HIP-event time on the ctx stream */
    double ms_render;        /* sum of tirt_pt_rgb_render calls since reset */
    double ms_trace_closest; /* sum over closest-hit kernel launches since reset */
    double ms_trace_shadow;
    double ms_shade;
    uint64_t launches_trace_closest;
    uint64_t launches_trace_shadow;
    uint64_t launches_shade;
    /* wave-occupancy diagnostics of the traversal kernels (TIRT_COUNT_NODES only): per-wave
     * loop trips and the number of busy lanes summed over those trips (64 = full wave) */
    uint64_t diag_it_node, diag_lanes_node, diag_it_leaf, diag_lanes_leaf, diag_refills, diag_it_outer;
    /* timeline of the traversal waves (TIRT_COUNT_NODES only), 100 MHz ticks: their lifetimes summed, the part of a lifetime after the wave
     * found the ray queue empty (it only finishes the rays it holds), and how many waves ran */
    uint64_t diag_wave_ticks, diag_drain_ticks, diag_waves;
    uint64_t launches_tail;   /* always 0 since round 6 (rounds 4-5, experiments builds: PT_RGB batches whose last bounces ran as one persistent launch); kept for the layout */
} tirt_stats_t;

const char *tirt_last_error(void);
int tirt_version(void);
int tirt_device_count(int *out);

/* one context = one HIP device + one stream */
int tirt_create(int device_id, tirt_ctx **out);
void tirt_destroy(tirt_ctx *ctx);
int tirt_sync(tirt_ctx *ctx);
/* options: "time_kernels" (0/1) -- bracket every trace/shade launch with HIP events on the
 *            ctx stream so that tirt_stats reports per-kernel time (bench/roofline only)
 *            (also confines the batches to one lane so that kernel times are not overlapped)
 *          "overlap_lanes" (1..8, default 4) -- wavefront batches in flight on separate streams
 *          "trace_lds_depth" / "trace_refill_min" / "trace_node_min" / "trace_grid" / "trace_grid_alone" / "trace_slices" /
 *          "shade_grid" -- kernel tuning
 *          "shade_specialize" (0/1, default 1) -- k_shade / k_shade_spec are compiled for a few scene feature sets (tirt_shade_features); 1 launches the
 *            narrowest instantiation that covers the scene, 0 the generic kernel for every scene.  Same films bit for bit either way
 *          "query_chunk_rays" (256 .. 2^27, default 2^21) -- rays per chunk of tirt_query_closest / tirt_query_occluded (48 B of scratch each; tirt_query_hits divides it by k)
 *          "bdpt_bounded" (0/1, default 1) -- BDPT connection rays are cut off at their target distance (same
 *            visibility answers as the full closest-hit query; 0 = reference-style full query, for cross-checks)
 *          "merge_paths" -- consecutive tirt_pt_rgb_render calls over contiguous frames are merged
 *            until this many pixel-samples are pending (default 32 Mi = one full batch; 0 submits every call at once);
 *            every other entry point submits what is pending first
 *          "job_frames" -- hint: frames the whole job will render (0 = unknown, default).  With it (and no explicit batch_paths)
 *            the job is cut into as few wavefront batches as fit 128 Mi pixel-samples each, at least two, run two at a time
 *            (round 5: a 640 Mi-sample job as 5 x 128 Mi instead of 8 x 80 Mi on four lanes: +1.7 %); lane buffers are sized for that and only as many lanes get one (a 512^2 x 8 spp job does
 *            not allocate 32 Mi-path lanes).  Set it before the first render call of the job
 *          "batch_paths" -- pixel-samples kept in flight per wavefront batch (default 32 Mi, or planned from "job_frames";
 *            204 B of HBM each, lanes hold 1.5 x that)
 *          "split_lone_batch" (0 = off, or the number of parts 2..8; default 0 since round 3) -- a context that owns 1/6 or less of the film
 *            (tile_count >= 6) and whose whole job is one batch runs it as that many smaller batches on as many lanes
 *          "path_order_blocks" (0/1, default 1 since round 5) -- the paths of a wavefront batch numbered pixel-block major (64-path chunk = one 8 x 8 pixel block
 *            of one frame, the frames of a block next to each other) instead of frame major: +1.5 % on the headline scene, +5 % on a 4 M-triangle one; same film
 *          "slices_contiguous" (0/1, default 0) -- k_trace's ray-fetch slices as contiguous stretches of the queue (each XCD one region of the film); no gain measured
 *          "wide_collapse" -- EXPERIMENT (cost-optimal grouping into 4-wide nodes): only in a library built with -DTIRT_EXPERIMENTS (`make experiments`); the product
 *            library answers it with an error unless the value means "off".  (Rounds 4-5 also carried "tail_paths" / "tail_bounce" there: the last bounces of a batch as one
 *            persistent launch -- bit-identical, slower at every switch point; tools/exp/patches/r06_persistent_tail_kernel.patch)
 *          "traversal_tree" (0/1, default 1) -- the tree tirt_lbvh_build collapses into the 4-wide traversal nodes: 1 = a binned-SAH
 *            tree over the same primitives built on the device after the LBVH, 0 = the reference's LBVH itself; results are
 *            bit-identical either way (tirt_traversal_tree_download) -- except for rays that lie, to fp32 rounding, IN the plane of a
 *            triangle: there the reference's Moller-Trumbore divides by a determinant of rounding noise and which "hit" such a ray
 *            gets depends on the visiting order (none in any render); takes effect at the next tirt_lbvh_build
 *          "bdpt_mem_budget" -- bytes a BDPT call may take for its batch state even when more is free (0 = off; tests)
 *          "primary_beams" -- (round 5, default 1) camera rays against per-pixel lists of the leaves they can hit first instead of the bounce-0 traversal launch
 *            (csrc/tirt_pvb.hip: the lists are made once per build / camera / film from five probe rays and a walk of the pixel's pyramid; rays that find no hit
 *            on their list are traced the ordinary way; the same hit records bit for bit: +15 % on the headline scene); 0 = off.  "primary_beams_min_frames"
 *            (default 16): batches of fewer frames keep the ordinary launch (making the lists costs 1.2 ms at 1024^2).  "primary_beams_rebuild" (any value):
 *            the lists are forgotten and made again by the next batch that uses them (bench.py times a build inside its clock).  When the memory for the
 *            lists is not to be had the render goes on without them (tirt_primary_beam_stats out[7]).
 *          "primary_beams_edges" -- (0/1, default 1) a triangle goes on a pixel's list only if, besides the four faces of the pixel's pyramid, none of the
 *            triangle's own three edge planes through the eye separates it from the pyramid (pvb_beam_triangle_off, csrc/tirt_pvb.h): a triangle whose screen
 *            rectangle covers the pixel while the triangle does not is dropped.  Shorter lists, the same hit records, films and counters bit for bit.  Setting it
 *            makes the next batch that uses lists build them again, as a camera change does; 0 = the lists of the four faces alone.
 *          "primary_fused" -- (default 1) a PT_RGB batch that uses the lists computes a camera ray's direction, walks its pixel's list and performs the path's first
 *            shading step in ONE kernel (k_pvb_cand_shade, csrc/tirt_render.hip): the direction and the hit record stay in registers instead of going through
 *            device memory between three kernels.  The rays the lists leave over are traced as before and shaded by a second, short launch.  Same film, same
 *            counters, bit for bit; with "time_kernels" both launches count as shading time.  0 = the separate launches (k_generate, k_pvb_cand, k_trace,
 *            k_pvb_scatter, k_shade).  Batches with feature buffers enabled (tirt_aov_enable reads the camera rays' hit records), of a pixel set, of PT_Spec
 *            or under "primary_beams_diag" take the separate launches whatever the value.
 *          "bdpt_batch_items" -- (frame, pixel) items per BDPT wavefront batch (default 16 Mi, ~2.2 KB of HBM each: 38 GB; 5 Mi = 12 GB runs config 5 at 2 900 Mrays/s), shared by the batches in flight on render lanes 0 and 1 ("bdpt_lanes", 1..4, default 2: three or four measured no faster)
 *            (config 5, round 3: 4 Mi 2 890, 8 Mi 2 900, 16 Mi 2 995, 32 Mi 2 980 Mrays/s; 256 frames: 8 Mi 2 912, 16 Mi 2 923, 32 Mi 3 032)
 *            A call never sizes its batches beyond what hipMemGetInfo reports free (less 2 GB): next to other users of the device it renders in smaller batches.
 *          "bdpt_state_fill" (diagnostic) -- what a BDPT batch does to its per-item vertex arrays first: 0 = nothing (default: no read reaches a slot
 *            its item has not written), 1 = zeros (rounds 1-3: +3.5 % time on config 5), 2 = 0xFF poison (the parity tests run under it)
 *          (trace_lds_depth is checked against the LDS a block can have on the device) */
int tirt_set_option(tirt_ctx *ctx, const char *name, double value);

/* Scene.setup_data_gpu field uploads (reference Scene.py:299-308).
 * vertex[nv*9] primitive[n*3] material[nm*10] shape[ns*10] light[nl]; light_count is
 * Scene.light_count (may be 0 while nl == 1, Scene.py:253-261); bmin/bmax = scene AABB
 * (LBvh.Bvh.min/max_boundary, accel/LBvh.py:193-194). */
int tirt_scene_upload(tirt_ctx *ctx, const float *vertex, int nv, const int32_t *primitive, int n,
                      const float *material, int nm, const float *shape, int ns,
                      const int32_t *light, int nl, int light_count,
                      const float bmin[3], const float bmax[3]);
/* Re-upload the material rows only (examples edit material_cpu before setup). */
int tirt_material_upload(tirt_ctx *ctx, const float *material, int nm);

/* Texture.setup_data_gpu (texture/Texture.py:38-39): rgb_packed[w*h] 0xRRGGBB, index x*h + y */
int tirt_env_upload(tirt_ctx *ctx, const int32_t *rgb_packed, int w, int h, float power);

/* Albedo textures on materials (csrc/tirt_device.h, tex_albedo; no reference counterpart: integrator/PT_RGB.py:86 takes the material colour, and the
 * reference's Scene.add_obj fails on a map_Kd line).  PT_RGB, its feature buffers and the Debug albedo view honour them; nothing else does.
 * Which materials are textured: with T >= 1 uploaded textures, a material row whose type is not MAT_LIGHT and whose slot 1 (SceneData.Material.alebdoTex)
 *   satisfies 1 <= (int)row[1] <= T is textured with texture number (int)row[1] - 1.  0 (the default) and -1 (what Scene.add_obj writes for "none") mean
 *   untextured; an emitter's row ignores its slot (emission is never textured).  With T == 0 nothing is textured, whatever the rows hold.  A row that is
 *   not an emitter's and names a texture beyond T is refused (TIRT_ERR_ARG) by tirt_scene_upload, tirt_material_upload and tirt_texture_upload alike, so
 *   that the device never needs the count.
 * Texel format: a texture is w x h packed texels exactly as the environment image: i32 (R<<16)|(G<<8)|B, index x*h + y, y = 0 the bottom image row
 *   (Texture.load_image), and a wrap flag: 0 clamp, 1 repeat.
 * tex_albedo(tex, u, v), all f32, one rounding per operation, no contraction (tests/texture_expected.py restates it; the device gives its bits):
 *   1. finite(x) := |x| <= 3.4028234e38 (false for a NaN).  u = finite(u) ? u : 0; the same for v
 *   2. wrap == 1:  u = u - floor(u);  v = v - floor(v)      (floor: t = (float)(int)x, t > x ? t - 1 : t; |x| < 2^31)
 *   3. the reference's texture2D (texture/Texture.py:41-69) with this texture's w, h -- the function the environment lookup runs, on (buffer, w, h):
 *        x = min(w - 1, max(0, u * w));  y = min(h - 1, max(0, v * h))   (w - 1 computed in f32);  lx = floor(x), ly = floor(y);  wlr = x - floor(x), wbt = y - floor(y)
 *        sample(fx, fy): xi = clamp((int)fx, 0, w - 1), yi = clamp((int)fy, 0, h - 1), texel = buffer[xi*h + yi], (R, G, B) = ((texel >> 16) & 255, (texel >> 8) & 255, texel & 255) / 255.0f
 *        lt = sample(lx, ly), rt = sample(lx + 1, ly), lb = sample(lx, ly + 1), rb = sample(lx + 1, ly + 1);  mix(a, b, t) = a * (1 - t) + b * t per channel
 *        c = mix(mix(lt, rt, wlr), mix(lb, rb, wlr), wbt)
 *   c is an encoded (sRGB-valued) colour, in the space of a material row's colour.  uv = (0, 0) reads texel (0, 0) with weight exactly 1.
 * Where c goes, at a hit on a textured material: k_shade's reflect_color = srgb_to_lrgb(c) instead of srgb_to_lrgb(material colour) (PT_RGB.py:86), in the
 *   NEE contribution and the continuation's throughput; TIRT_AOV_ALBEDO and TIRT_DEBUG_ALBEDO = c instead of the row's words 2..4.
 *   The hit's uv is (t1*a + t2*b) + t3*c per component over the vertex rows' columns 6, 7 (a = 1 - u - v, b = u, c = v of the hit record), as
 *   Scene.hit_attributes (Scene.py:537-561) interpolates it; column 8 is not used.  Analytic shapes have uv 0.
 * Kernels: a textured scene sets bit 128 of the feature word (tirt_shade_features) and is shaded by an instantiation of k_shade of its own, the generic
 *   kernel plus the lookup behind a test of the material row; the shading records then carry the three vertex uvs in words that are otherwise zero
 *   (tirt_shade_table_download).  A scene without a textured material runs the kernels and produces the bits it did before textures existed.
 *   tirt_vertex_update and tirt_vertex_update_device write columns 0..5 of the vertex rows: uvs survive them.
 * tirt_bdpt_rgb_render, tirt_pt_spec_render and tirt_bdpt_spec_render return TIRT_ERR_ARG while the feature word has bit 128 (textures there are out of
 *   scope); tirt_texture_upload with count 0 clears it.
 * tirt_texture_upload: replaces all textures by `count` new ones; texture i is the w[i]*h[i] texels from texels + offset[i], `total` = the ints at `texels`.
 *   count == 0 removes all textures (the pointers may be NULL).  TIRT_ERR_ARG before anything is written, the old textures staying: w or h < 1, a wrap
 *   flag other than 0 / 1, texels that run past `total` or overlap another texture's, total >= 2^31 - 4 * count, a material row that names a texture
 *   beyond count (see above).  The first three need no context.  Waits for work in flight and for the copy, as tirt_env_upload.  Textures outlive
 *   tirt_scene_upload exactly as the environment image does; the feature word follows every texture and material upload.
 * tirt_kat_texture: known-answer entry (tests/test_gpu_texture.py).  in, 3 words per row: texture number (its bits), u, v; out, 6 words: c3,
 *   srgb_to_lrgb(c)3.  One launch, row i on thread i.  TIRT_ERR_ARG: in_stride < 3, out_stride < 6, no textures, a number outside [0, count). */
int tirt_texture_upload(tirt_ctx *ctx, int count, const int32_t *texels, int64_t total, const int64_t *offset, const int32_t *w, const int32_t *h,
                        const int32_t *wrap);
int tirt_kat_texture(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);

/* Alpha cut-outs (csrc/tirt_device.h, tex_alpha; csrc/tirt_internal.h, trace_leaf_step; no reference counterpart).  A hit on a transparent texel of a cut-out
 * triangle is no hit, for every ray the library traces: camera, bounce and NEE shadow rays of PT_RGB, Debug, tirt_trace_closest / _shadow, tirt_query_*, the
 * feature buffers and the motion records.
 * Texel: bits 24..31 of a packed texel hold 255 - A (transparency), so a texture packed without them (every texture before this) is fully opaque; tex_albedo
 *   and everything built on it mask them off and do not change by a bit.
 * Which textures are masks: none, until tirt_texture_cutout(ctx, flags, count) says so: flags[i] = 1 makes the top byte of texture i a cut-out mask, 0 leaves it
 *   ignored.  count must equal the number of uploaded textures, every flag must be 0 or 1: TIRT_ERR_ARG otherwise, before anything is written (the flag values
 *   are checked first and need no context).  Every tirt_texture_upload clears all flags (its own behaviour and refusals are unchanged).  Waits for work in flight.
 * Which primitives: a triangle whose material row is not an emitter's and whose word 1 names an uploaded texture with its flag set is a cut-out triangle.  Analytic
 *   shapes and emitters are never cut out (an emitter's row ignores its slot, as for the albedo).
 * tex_alpha(tex, id, tu, tv): the fourth channel of the unchanged tex_albedo lookup -- steps 1 and 2, then texture2D's x, y, lx, ly, wlr, wbt and the four samples
 *   lt, rt, lb, rb with   alpha(texel) = (float)(255 - ((texel >> 24) & 255)) / 255.0f   in place of (R, G, B), and mix(mix(lt, rt, wlr), mix(lb, rb, wlr), wbt).
 *   All f32, one rounding per operation, no contraction (tests/cutout_expected.py restates it; the device gives its bits).
 * Hit uv: (tu, tv) = (t1*a + t2*b) + t3*c over columns 6, 7 of the vertex rows, a = 1 - u - v, b = u, c = v of the candidate -- exactly the albedo lookup's uv.
 * Rule: a candidate of the traversal's leaf step on a cut-out triangle replaces the current hit only if, besides everything it must satisfy anyway (0 < t < best,
 *   the equal-distance rule, the ordered walk's proof that the reference reaches the leaf), tex_alpha >= 0.5f.  The cutoff is fixed (glTF's MASK default).  A
 *   rejected candidate changes nothing: not the hit, not the equal-distance state, not the culling distance, not a bounded query's settled answer.
 * Feature word: bit 512 (SF_CUTOUT) = a cut-out triangle exists; reported by tirt_shade_features, refreshed by scene, material, texture, flag and vertex uploads,
 *   never set by tirt_shade_features_host.  No instantiation of k_shade depends on it (an albedo-only cut-out scene is shaded by 255, one with maps by 511): the
 *   hits k_shade, the feature buffers and the denoisers see are on opaque texels.  Bit 128 is set with it, so tirt_bdpt_rgb_render, tirt_pt_spec_render and
 *   tirt_bdpt_spec_render refuse such a scene.
 * Kernels: while bit 512 is set every k_trace launch is the CUTOUT twin of the instantiation it would have been; the triangle records of the traversal layout carry
 *   a tag (0, or texture number + 1) in the last word of their second quad (tirt_wide_tree_download), written lazily before the next trace; the camera-ray candidate
 *   lists (option "primary_beams") are not used.  A scene without a cut-out triangle launches the kernels, and downloads the records, it did before.
 * tirt_kat_texture_alpha: known-answer entry (tests/test_gpu_cutout.py).  in, 3 words per row: texture number (its bits), u, v; out, 2 words: tex_alpha and the
 *   decision (1.0f where alpha >= 0.5f, else 0.0f).  One launch, row i on thread i.  TIRT_ERR_ARG: in_stride < 3, out_stride < 2, no textures, a number outside
 *   [0, count).  Needs no flags: every texture has a top byte. */
int tirt_texture_cutout(tirt_ctx *ctx, const int32_t *flags, int count);
int tirt_kat_texture_alpha(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);

/* Roughness, metallic and normal-map textures on materials (csrc/tirt_device.h, tex_roughness / tex_metallic / tex_normal; no reference counterpart).  PT_RGB, its
 * feature buffers' normal and the Debug normal / fnormal views honour them; nothing else does.  Storage, upload and lookup are the albedo textures' own.
 * Slots: words 7, 8, 9 of a material row (SceneData.Material.roughTex, metalTex, normalTex; no reader before this) by word 1's convention: with T uploaded
 *   textures 1 <= (int)word <= T names texture word - 1, 0 and anything below mean none.  An emitter's row ignores all of them; a glass row ignores words 7 and
 *   8 (its words 5 and 6 are ior and extinction) and honours word 9.  A word that is not ignored and names a texture beyond T is refused (TIRT_ERR_ARG, before
 *   anything is written) by tirt_scene_upload, tirt_material_upload and tirt_texture_upload, as word 1 is.  With T == 0 nothing is textured, whatever the rows hold.
 * Values, all f32, one rounding per operation, no contraction, in the order written (tests/material_maps_expected.py restates them; the device gives its bits);
 *   (tu, tv) is the hit's uv as the albedo lookup takes it, c = tex_albedo(tex, id, tu, tv) the unchanged lookup:
 *   rough = c.y of the roughness texture, metal = c.z of the metallic texture (glTF's channels, so one occlusion-roughness-metallic image serves both slots);
 *     linear, no sRGB decode.  They take the place of row[6] / row[5] wherever the Disney functions read them (disney_setup, disney_evaluate_pdf, disney_sample, through
 *     a local copy of the two words): maxf(0.001, rough) and every other expression of those functions applies to them unchanged.
 *   normal map: n = c * 2 - 1 per channel (the product, then the difference).  With the triangle's vertex positions p0, p1, p2 and uvs t0, t1, t2 and N the
 *     interpolated, normalised shading normal (hit_attributes' nor):
 *       d1 = t1 - t0, d2 = t2 - t0;  det = d1.x * d2.y - d2.x * d1.y (two products, one difference)
 *       det == 0, or not |det| <= 3.4028234e38 (infinite, NaN), or the primitive is an analytic shape:  N' = N
 *       e1 = p1 - p0, e2 = p2 - p0;  T = (e1 * d2.y - e2 * d1.y) / det per component (two products, one difference, one quotient)
 *       T = T - N * dot(N, T), dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;  T = normalized(T), normalized(a) = a * (1 / sqrt(dot(a, a)))
 *       a component of T not |.| <= 3.4028234e38:  N' = N
 *       B = cross(N, T) = (N.y * T.z - N.z * T.y, N.z * T.x - N.x * T.z, N.x * T.y - N.y * T.x)
 *       Nraw = (T * n.x + B * n.y) + N * n.z;  N' = normalized(Nraw)      (a texel of 0.5, 0.5, 1 does not give N back exactly: 2 * (128 / 255) - 1 != 0)
 *     N' takes the place of the shading normal before k_shade forms fnormal = N' * sign(dot(-direction, gnor)); the geometric normal is untouched.
 *     TIRT_AOV_NORMAL, TIRT_DEBUG_NORMAL and TIRT_DEBUG_FNORMAL show N'.  The motion records (tirt_motion_enable) keep using the vertex normals: a mapped
 *     normal's own motion is not tracked.
 * Kernels: a row that is not an emitter's and names an uploaded texture in a word it honours sets bit 256 of the feature word (SF_TEXTURE_PARAM); the scene is
 *   then shaded by k_shade<SF_ALL | SF_TEXTURE | SF_TEXTURE_PARAM> (511), the albedo instantiation plus these lookups behind tests of the material row, and the
 *   shading records carry the vertex uvs exactly as under bit 128.  Every other scene runs the kernels and produces the bits it did before.
 * tirt_bdpt_rgb_render, tirt_pt_spec_render and tirt_bdpt_spec_render return TIRT_ERR_ARG while bit 256 is set; tirt_texture_upload with count 0 clears it;
 *   tirt_shade_features_host never sets it.
 * tirt_kat_material_maps: known-answer entry (tests/test_gpu_material_maps.py).  in, 3 words per row: primitive (its bits), hit u, hit v (the barycentrics of
 *   the hit record); out, 8 words: the hit's uv (2), rough, metal -- looked up, or the row's words 6 and 5 as they are --, N' (3), 0.  A triangle's N is
 *   normalized((n0 * a + n1 * u) + n2 * v), a = 1 - u - v; an analytic shape has uv 0 and, there being no ray, N = N' = (0, 0, 0).  One launch, row i on
 *   thread i.  TIRT_ERR_ARG: in_stride < 3, out_stride < 8, no scene, no textures, a primitive outside [0, n_prims). */
int tirt_kat_material_maps(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);

/* The scene feature word: which shading code the uploaded tables can reach, and so which instantiation of the shading kernels a render
 * launches (option "shade_specialize").  Bits: 1 a MAT_GLASS material row, 2 environment lit (power != 0 or a texel that is not black),
 * 4 / 32 / 8 / 64 a triangle / a sphere / a spot or laser / an emitter of unknown kind on the light list, 16 light_count == 0,
 * 128 a material row that is not an emitter's names an uploaded albedo texture (never set by tirt_shade_features_host, which sees no textures),
 * 256 such a row names an uploaded roughness, metallic or normal-map texture in a word it honours (likewise never set by tirt_shade_features_host).
 * tirt_shade_features: out[0] = the word the context holds (refreshed by every scene, material, environment, texture and vertex upload),
 * out[1] = the "shade_specialize" option.  tirt_shade_features_host: the same rule on host tables, without a context or a device
 * (env may be NULL: lit if env_power != 0).
 * tirt_shade_instantiation: the choice itself.  k_shade is compiled for 19 words, kept in one table in this order: 32, 4, 127, 255, 511, then 127 | d and 511 | d for
 * d = 1024, 2048, 3072, then the same eight (127, 511 and their six twins) | 4096; k_shade_spec for 32, 4, 127.  With M = 1024 | 2048 | 4096 (the derived bits:
 * "Environment importance sampling", "HDR environment", "Choosing emitters by power") a render launches the first entry e of the table with (e & M) == (word & M),
 * (word & ~512 & ~e) == 0 and, where specialize is 0, (e & 127) == 127.  feat[0] = e.  spectral 1: PT_Spec's table; its words lie within 127.
 * TIRT_ERR_ARG: a NULL feat, specialize or spectral neither 0 nor 1, a word with bits at or above 8192, spectral 1 with bits outside 127. */
int tirt_shade_features(tirt_ctx *ctx, uint32_t *out);
/* which instantiation a render launches for a feature word as tirt_shade_features reports it (bit 512 ignored); no context, no device */
int tirt_shade_instantiation(uint32_t word, int specialize, int spectral, uint32_t *feat);
int tirt_shade_features_host(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                             const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power,
                             uint32_t *out);

/* Importance sampling of the environment (csrc/tirt_envsample.hip, the table; csrc/tirt_device.h, env_sample / env_pdf; csrc/tirt_render.hip, shade_path under
 * SF_ENV_SAMPLE; no reference counterpart: integrator/PT_RGB.py:127-132 reads the environment only where a BSDF-sampled ray misses).  Opt-in, PT_RGB only: with the
 * switch off every kernel keeps its code and its bits; tirt_pt_spec_render, both BDPT integrators, the feature buffers, moments, denoisers and the temporal
 * history never read the switch.  The image is 8 bits per channel (tirt_env_upload) or RGBE8 (tirt_env_upload_hdr, "HDR environment" below).
 * All f32 below: one rounding per operation, no contraction, in the order written (tests/env_sampling_expected.py restates it; the device gives its bits).
 * 1. Cells and weights.  One cell per texel index (i, j), i < w, j < h: the lookup coordinates with floor(min(w - 1, max(0, tx * w))) = i and the same for
 *      (ty, h, j) -- the cell texture2D's lx, ly name; cell w - 1 / h - 1 takes what the clamp folds into it.
 *      lum(x, y) = ((l.r + l.g) + l.b) / 3.0f of l = srgb_to_lrgb(texel(min(x, w - 1), min(y, h - 1)) / 255.0f)   (the level of tirt_moments_converged, not Rec.709)
 *      m = ((lum(i, j) + lum(i + 1, j)) + (lum(i, j + 1) + lum(i + 1, j + 1))) * 0.25f          -- the four texels texture2D mixes in the cell
 *      el = ((j + 0.5f) / h - 0.5f) * PI_SCENE;   weight = m * cos(el);   q(i, j) = (uint32) rintf(weight * 16777216.0f)   (round half to even; 0 <= q <= 2^24)
 * 2. Sums, 64-bit integers: R_j[i] = q(0, j) + .. + q(i, j);  M[j] = R_0[w - 1] + .. + R_j[w - 1];  total = M[h - 1].  total == 0, env_power == 0,
 *      max(w, h) > 16384 or w * h > 2^25: no table, the feature is inactive.  Any summation order gives these values.
 * 3. Sample from two randoms ra, rb in [0, 1) (24 bits: k = (uint32)(r * 16777216.0f)).  pick(C, n, k, tot), C an inclusive sum with C[n - 1] = tot:
 *        t = floor(k * tot / 2^24), fb = (k * tot) mod 2^24 (exact: the high and low halves of (k << 40) * tot);  e = the first index with C[e] > t;
 *        below = e ? C[e - 1] : 0;  off = (float)(((t - below) * 2^24 + fb) / (C[e] - below)) * 2^-24    (integer quotient < 2^24: off is exact and < 1)
 *      (j, offy) = pick(M, h, ka, total);  (i, offx) = pick(R_j, w, kb, R_j[w - 1]);   tx = ((float)i + offx) / (float)w;  ty = ((float)j + offy) / (float)h
 *      az = (tx * 2.0f) * PI_SCENE - PI_SCENE;  el = (ty - 0.5f) * PI_SCENE;  d = (cos(el) * cos(az), sin(el), cos(el) * sin(az))   -- the inverse of the miss branch's
 *      tx = (atan2(d.z, d.x) + PI_SCENE) / PI_SCENE / 2.0f,  ty = atan2(d.y, dis) / PI_SCENE + 0.5f,  dis = sqrt(d.x * d.x + d.z * d.z)     (PI_SCENE = 3.1415926f)
 * 4. pdf over solid angle of a direction d: dis, tx, ty as the miss branch forms them; x = min(w - 1, max(0, tx * w)), i = clamp((int)floor(x), 0, w - 1), j likewise;
 *        pdf = (((float)q(i, j) / (float)total) * ((float)w * (float)h)) / (((2.0f * PI_SCENE) * PI_SCENE) * dis);   dis < 1e-6f: pdf = 0
 *      The pdf of a sample is the pdf of ITS direction by this lookup (a tx that rounds onto a cell's edge may land in the neighbour: both sides then agree).
 * 5. One bounce of k_shade with the table (bit 1024).  p_env = light_count == 0 ? 1 : share.  r = tm_rand(.., TM_SLOT_LIGHT):
 *      r < p_env: the environment sample d of (ra, rb) = (TM_SLOT_LA, TM_SLOT_LB), Disney branch only.  Taken iff dot(fnormal, d) > 0 and pdf(d) > 0:
 *        pdf_l = p_env * pdf(d);  e_brdf, e_pdf = the Disney evaluation towards d;  e_pdf > 0:  w = power_heuristic(pdf_l, e_pdf) / max(1e-4f, pdf_l),
 *        c = (srgb_to_lrgb(texture2D(env, tx, ty)) * env_power) * w, then * throughput, * reflect_color, * e_brdf, * |dot(fnormal, d)|, * (drawn / e_pdf) in that order, with (tx, ty)
 *        of step 4 for d and drawn = max(0, e_pdf + (dr * (float)(1.0 / 3.1415956)) * (dot(fnormal, d) - 1)), dr = 0.5f * (1 - metallic): the density Disney.sample
 *        draws d with (its diffuse lobe by cos / pi) where evaluate_pdf states 1 / pi for that lobe.  The switch-off estimator weights its draws by 1 / e_pdf and so
 *        converges to the integral of (drawn / e_pdf) * f * cos * L; with the ratio the light sample estimates that integrand too, the MIS weights sum to 1 over one
 *        integrand, and switch on and off have one expectation.  A metal has dr = 0 and the ratio exactly 1;
 *        LIMIT: the emitter sample keeps the reference's form (no ratio), and the share rescales its pdf, so on dielectrics in a scene WITH emitters the expectation
 *        depends on `share` to the extent that an emitter's MIS weights move with it (nothing where light_pdf dwarfs e_pdf, as for small lamps);  shadow ray from offset_ray(pos, fnormal) along d with expect = -1 (-2 and c = 0 where e_pdf <= 0) and distance 2e6: it contributes iff it
 *        hits nothing (k_trace is unchanged: -1 is the hit primitive of a ray without a hit; a bound beyond INF_VALUE lets any accepted hit end the walk)
 *      otherwise: the emitter sample as before with r' = (r - p_env) / (1 - p_env) in r's place and light_pdf * (1 - p_env)
 *      emitter hit: light_pdf * (1 - p_env).  Miss: the environment term times 1 where perfect_spec == 1, else power_heuristic(brdf_pdf, p_env * pdf(direction)).
 * tirt_env_sampling(ctx, on, share): the switch and the share (0 < share < 1, on 0 / 1: TIRT_ERR_ARG otherwise, before a context is needed).  Submits pending renders,
 *   waits for work in flight, builds or drops the table.  tirt_env_upload rebuilds or drops it; a scene upload keeps it (the feature bit follows the word's bit 2).
 * Feature word: bit 1024 (SF_ENV_SAMPLE) = switch on, bit 2 set, table exists; reported by tirt_shade_features, kept out of every other integrator's kernel choice.
 *   tirt_pt_rgb_render then launches k_shade<127 | 1024>, or k_shade<511 | 1024> where the word has bit 128 or 256.  tirt_shade_features_host_env is
 *   tirt_shade_features_host with the switch as an input (env == NULL never sets the bit: a table needs the image).
 * tirt_env_table_download: info = (w, h, table exists, bit 1024); with a table q[h * w] (row j at j * w), row_sums[h * w] (R_j) and marginal[h] (M); each may be NULL.
 * tirt_kat_env_sample: in 2 words (ra, rb in [0, 1)), out 10: i, j (bits), tx, ty, d3, pdf(d), and the cell (i, j bits) the lookup of d lands in.
 * tirt_kat_env_pdf: in 3 words (d), out 5: i, j (bits), tx, ty, pdf.  Both: one launch, row r on thread r; TIRT_ERR_ARG without a table or with strides too small. */
int tirt_env_sampling(tirt_ctx *ctx, int on, float share);
int tirt_env_table_download(tirt_ctx *ctx, uint32_t *q, uint64_t *row_sums, uint64_t *marginal, int32_t info[4]);
int tirt_kat_env_sample(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);
int tirt_kat_env_pdf(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);
int tirt_shade_features_host_env(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                 const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power,
                                 int env_sampling, uint32_t *out);

/* HDR environment (csrc/tirt_device.h, hdr_decode / texture2d_hdr / env_lookup / env_cell_q_hdr; no reference counterpart: texture/Texture.py packs 8 bits per channel).
 * PT_RGB only, as the 8-bit image: tirt_pt_spec_render and both BDPT integrators do not light from the image at all, so they neither read nor refuse it.
 * A scene with an 8-bit environment launches the kernels it launched before this format existed; they are compiled without bit 2048 and keep their code.
 * Texel format: RGBE8 in the word the environment already uses, w x h packed i32 at index x*h + y, y = 0 the bottom row: (E << 24) | (R << 16) | (G << 8) | B.
 *   channel = (float)mantissa * 2^(E - 136)  -- one exact integer-to-float conversion and one exact scaling (ldexp).  Linear radiance: no srgb_to_lrgb is applied.
 *   f32 denormals are kept as they come (E <= 17 reaches them): the library is built with -fno-fast-math and without denormal flushing (float_denorm_mode_32 = 3).
 *   E == 0 is allowed only with R = G = B = 0, which is black; tirt_env_upload_hdr refuses every other E == 0 texel (TIRT_ERR_ARG), so the decode above needs no
 *   special case: the all-zero word gives 0 * 2^-136 = 0.  The largest value is 255 * 2^119 < FLT_MAX: a texel is never Inf or NaN.
 *   (Not float3 / float4 texels: a tap stays one 4-byte gather, the allocation, env_table_offset and the kernels' SceneView argument stay what they are; and a
 *   Radiance .hdr file stores exactly these four bytes.)
 * Lookup L(tx, ty), all f32, one rounding per operation, in the order written (tests/env_hdr_expected.py restates it; the device gives its bits) -- texture2D on decoded texels:
 *   x = min(w - 1, max(0, tx * w)), y = min(h - 1, max(0, ty * h))   (max(a, b) = a > b ? a : b, min(a, b) = a < b ? a : b: a NaN coordinate stays NaN);
 *   lx = floor(x), ly = floor(y);  wlr = x - floor(x), wbt = y - floor(y);  texel(fx, fy) = decode(img[clamp((int)fx, 0, w - 1) * h + clamp((int)fy, 0, h - 1)]);
 *   lt = texel(lx, ly), rt = texel(lx + 1, ly), lb = texel(lx, ly + 1), rb = texel(lx + 1, ly + 1);  mix(a, b, t) = a * (1 - t) + b * t;
 *   L = mix(mix(lt, rt, wlr), mix(lb, rb, wlr), wbt).
 *   It takes the place of srgb_to_lrgb(texture2D(env, tx, ty)) in the miss branch -- radiance += (L * throughput) * env_power, times the MIS weight w last under bit 1024 --
 *   and in the environment sample of "Importance sampling of the environment", step 5: c = (L * env_power) * w, then the factors in the order given there.
 * Sampling table: steps 2..5 are unchanged; step 1 becomes
 *   lum(x, y) = ((c.r + c.g) + c.b) / 3.0f of c = decode(texel(min(x, w - 1), min(y, h - 1)));  m and el as there;  weight = m * cos(el);
 *   E_max = the largest exponent byte among the texels with a mantissa that is not 0 (found by the host at upload, passed to the kernel);
 *   s = rintf(ldexpf(weight, 152 - E_max));  q(i, j) = s > 0 ? (s < 2^24 ? (uint32) s : 2^24) : 0.   Every channel is below 2^(E_max - 128), so q <= 2^24 and every bound of
 *   steps 2..4 holds; the clamp only acts where a sum of channels overflowed to +Inf, which needs E_max >= 254.  The scale is applied by ldexp, never as a float factor
 *   (2^(152 - E_max) is no f32 for E_max < 25).  Adding a constant to the exponent byte of every texel with a mantissa gives the same table to the bit.
 * Feature word: bit 2048 (SF_ENV_HDR) = the uploaded image is RGBE8 and the environment is lit (bit 2: env_power != 0 or a texel whose low 24 bits are not 0 -- the
 *   8-bit rule).  Reported by tirt_shade_features.  tirt_pt_rgb_render then launches k_shade<127 | 2048>, or k_shade<511 | 2048> where the word has bit 128 or 256; with
 *   bit 1024 as well k_shade<127 | 1024 | 2048> or k_shade<511 | 1024 | 2048>.  "shade_specialize" does not matter to them: a lit environment means the generic kernel.
 * tirt_env_upload_hdr: as tirt_env_upload (waits for work in flight, refreshes the feature word, rebuilds or drops the sampling table) and sets the format; the
 *   E == 0 rule is checked first, without a context, and the message names the first offending texel's index.  tirt_env_upload sets the format back to 8 bits.
 * tirt_env_format: out = (format: 0 8-bit, 1 RGBE8;  E_max, 0 for format 0 or an image without a mantissa).
 * tirt_kat_env_lookup: in 2 words (tx, ty), out 3: the linear colour the miss branch adds before env_power, in the context's current format -- L above, or
 *   srgb_to_lrgb(texture2D(env, tx, ty)) for an 8-bit image.  One launch, row r on thread r.  TIRT_ERR_ARG: strides too small, no image.
 * tirt_shade_features_host_env_hdr: tirt_shade_features_host_env with the format as an input.  env_format 0: that function.  env_format 1: the image is required
 *   (NULL, w < 1, h < 1 and an E == 0 texel with a mantissa are TIRT_ERR_ARG); bit 2048 where bit 2 is set, bit 1024 by the table rule above. */
int tirt_env_upload_hdr(tirt_ctx *ctx, const int32_t *rgbe_packed, int w, int h, float power);
int tirt_env_format(tirt_ctx *ctx, int32_t out[2]);
int tirt_kat_env_lookup(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);
int tirt_shade_features_host_env_hdr(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                     const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power,
                                     int env_sampling, int env_format, uint32_t *out);

/* Choosing emitters by power (csrc/tirt_envsample.hip, the table; csrc/tirt_device.h, light_pick; csrc/tirt_render.hip, shade_path under SF_LIGHT_POWER; no reference
 * counterpart: Scene.sample_li picks light[(int)(r * light_count)], one entry per emissive PRIMITIVE, so an emitter is found as often as it has entries).  Opt-in, PT_RGB
 * only: with mode 0 every kernel keeps its code and its bits; tirt_pt_spec_render and both BDPT integrators never read the switch.
 * All f32 below: one rounding per operation, no contraction, in the order written (tests/light_sampling_expected.py restates it; the device gives its bits).
 * 1. Weight of entry i of the light list: w_i = (((e.r + e.g) + e.b) / 3.0f) * area_i, e = words 2..4 of the emitter's material row as they stand (shade_path does not
 *      sRGB-decode an emission), area_i = get_prim_area of the primitive (Heron for a triangle, r * r * PI_SCENE for a sphere: what the light record holds).
 *      An entry takes part iff w_i > 0 and w_i <= FLT_MAX (so not 0, negative, NaN or infinite -- a degenerate triangle's NaN area among them).
 * 2. e_max = the exponent frexpf gives for the largest w_i that takes part (w = f * 2^e, 0.5 <= f < 1).  q_i = max(1, rintf(ldexpf(w_i, 24 - e_max))) for an entry that
 *      takes part (round half to even; 1 <= q_i <= 2^24), q_i = 0 otherwise.  The floor of 1 keeps every emitter with a weight reachable: no uniform share is needed for an
 *      unbiased estimator.  Scaling every emission by a power of two gives the same q to the bit.  The maximum is taken over the bits of positive floats, which order as
 *      the floats do: exact and free of order.
 * 3. C[i] = q_0 + .. + q_i, 64-bit integers (any summation order gives them); total = C[N - 1], N = light_count.  The table exists, and the feature is active, iff
 *      mode == 1, N > 0, total > 0 and every entry of the list is a triangle or a sphere (bits 8 and 64 of the feature word clear).
 * 4. Choice from the light random r in [0, 1] with the uniform share u in [0, 1) (default 0):
 *        r < u:      i = min((int)((r / u) * (float)N), N - 1)                                     -- the reference's expression on the rescaled random
 *        otherwise:  k = min((uint32)(((r - u) / (1.0f - u)) * 16777216.0f), 2^24 - 1);  t = floor(k * total / 2^24) (exact: the high half of (k << 40) * total);
 *                    i = the first index with C[i] > t                                             -- env_pick's integer inverse; an entry with q = 0 is never its answer
 *      P_i = u / (float)N + (1.0f - u) * ((float)q_i / (float)total): quotient, quotient, difference, product, sum, in that order.  With u = 0, r' = r to the bit.
 * 5. One bounce of k_shade with the table (bit 4096).  Under bit 1024 r is the rescaled random r' of "Importance sampling of the environment", step 5, and every
 *      (1 - p_env) factor applies as there, last.
 *      light sample: entry i and P_i of step 4 in the place of lidx;  light_choice_pdf = P_i / area_i;  the point (a, b), the directions, visibility,
 *        light_pdf = light_dist * light_dist * light_choice_pdf / NdotL_light, the power heuristic, the contribution and the shadow ray (expect = the hit primitive, its distance)
 *        keep their form and operand order.  No drawn / stated factor ("Importance sampling of the environment"): the emitter sample keeps the reference's form.
 *      emitter hit with perfect_spec != 1: light_pdf = (t * t) * (P_hit / area) / fCosTheta -- a product, a quotient, a product, a quotient -- in the place of
 *        (t * t) / ((area * light_count) * fCosTheta).
 *      P_hit rides in a spare word of the hit primitive's 128-byte shading record: the last word of quad 4 of a triangle, the first word of quad 2 of a sphere.  Both are 0
 *        while the feature is inactive (written with the table, written back to 0 when the feature goes).  The record holds its entry's own P.  Scene (Python) lists a
 *        primitive at most once.  A list uploaded through this ABI may name one twice: the entries then have equal weights and equal P, the record holds that P, and a
 *        hit's light_pdf understates the chance of sampling the primitive by the number of its entries -- exactly as 1 / (area * light_count) does with the switch off.
 *      LIMIT: where metallic < 1 the reference's sampler does not draw from the pdf it states, so its MIS estimate depends on the weights; changing light_pdf moves them.
 *        On metals switch on and off have one expectation; on dielectrics they can differ where an emitter's solid-angle pdf is comparable to the BSDF's.
 * tirt_light_sampling(ctx, mode, uniform_share): mode 0 uniform (the default), 1 power; 0 <= uniform_share < 1 (TIRT_ERR_ARG otherwise, before a context is needed).
 *   Submits pending renders and waits for work in flight.  The switch persists across scene, material and vertex uploads and tirt_film_create; the table is rebuilt
 *   lazily with the light records (the next render, tirt_shade_features or query), which all three uploads invalidate.
 * Feature word: bit 4096 (SF_LIGHT_POWER) = active by step 3; reported by tirt_shade_features (which builds the table if it is stale), kept out of every other
 *   integrator's kernel choice.  tirt_pt_rgb_render then launches the twin with bit 4096 of k_shade<127>, <511> and of their twins with bits 1024 and / or 2048; a scene with
 *   a spot, a laser or an unknown emitter runs exactly the kernels it runs with mode 0.
 * tirt_light_table_download: info = (light_count, e_max, bit 4096, table built: mode 1 and a list of triangles and spheres); with a table q[N], prefix[N] (C) and
 *   P[N] (all 0 where total == 0); each may be NULL.
 * tirt_kat_light_pick: in 1 word (r in [0, 1]), out 2: i (bits), P_i.  One launch, row r on thread r.  TIRT_ERR_ARG: strides too small, r outside [0, 1], feature inactive.
 * tirt_shade_features_host_lights: tirt_shade_features_host_env_hdr with the mode as an input, and the vertex rows a triangle's area needs: bit 4096 by step 3.
 * tirt_kat_shade_step accepts the eight words with bit 4096 while the feature is active. */
int tirt_light_sampling(tirt_ctx *ctx, int mode, float uniform_share);
int tirt_light_table_download(tirt_ctx *ctx, uint32_t *q, uint64_t *prefix, float *P, int32_t info[4]);
int tirt_kat_light_pick(tirt_ctx *ctx, const float *in, int in_stride, float *out, int out_stride, int n);
int tirt_shade_features_host_lights(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns,
                                    const int32_t *light, int light_count, const int32_t *env, int env_w, int env_h, float env_power,
                                    int env_sampling, int env_format, const float *vertex, int nv, int light_sampling, uint32_t *out);

/* LBvh.Bvh.setup_data_gpu (accel/LBvh.py:192-226): Morton codes, stable radix sort, Karras
 * topology, leaf boxes, bottom-up refit, DFS flatten -- all on device. */
int tirt_lbvh_build(tirt_ctx *ctx);
/* any of the three may be NULL: morton_sorted[n*2] (code, prim), bvh_node[(2n-1)*11],
 * compact_node[(2n-1)*9] */
int tirt_lbvh_download(tirt_ctx *ctx, int32_t *morton_sorted, float *bvh_node, float *compact_node);
/* The tree the ordered traversal walks (option "traversal_tree" = 1, the default): a binned-SAH binary tree over the
 * same primitives, built on the device after the LBVH, in the layout of compact_node -- rows [(2n-1)*9], pre-order, row =
 * (1 | prim | box) for a leaf, (0 | index of the right child | box) otherwise, left child = row + 1.  No counterpart
 * in the reference: its LBVH (tirt_lbvh_download) still decides every hit -- a candidate is accepted only if the
 * reference's traversal would have visited that leaf (Scene.py:702-744) -- this tree only finds the candidates with fewer
 * node visits.  With traversal_tree = 0 the rows are those of compact_node. */
int tirt_traversal_tree_download(tirt_ctx *ctx, float *rows);
/* Diagnostic, read-only: the arrays k_trace<ordered>, the beam kernels and the ray queries actually walk, as tirt_lbvh_build left them.
 * Any of the four arrays may be NULL (call once with all four NULL to learn the node counts):
 *   cnode[(wide_nodes + n_far_nodes) * 16]  64-byte 4-wide nodes in breadth-first order, the chain nodes of far-origin rays behind them:
 *                                           dword 3 * slot + axis = half(min plane) | half(max plane) << 16 in grid cells, dwords 12..15 the
 *                                           child codes (>= 0: node index; < 0: ~(record index | shape << 30); 0x80000001: empty slot)
 *   tri[n * 12]        48-byte primitive records in the leaf order of the traversal tree
 *   wnode[(2n-1) * 16] two-child nodes of the exhaustive traversal, one per compact_node row (rows of leaves are not written)
 *   prim_slot[n]       index of primitive i's record in tri
 * grid[19] = grid_min[3] (the centre of the padded root box), cell[3], inv_cell[3], inv_extent[3], root_min[3], root_max[3], and the
 * padding of leaf boxes.  info[6] = wide_nodes, n_far_nodes, root_code, far_qcode, built_sah (1: the rows of
 * tirt_traversal_tree_download are the binned-SAH tree's), shapes_boxed (1: sphere slots carry their own padded boxes, 0: the whole grid). */
int tirt_wide_tree_download(tirt_ctx *ctx, uint32_t *cnode, float *tri, float *wnode, int32_t *prim_slot, float grid[19], int32_t info[6]);
/* unsorted Morton pairs [n*2] as produced by build_morton_3d (accel/LBvh.py:318-336) */
int tirt_morton_download(tirt_ctx *ctx, int32_t *morton_unsorted);

/* Scene.process_normal (Scene.py:754-798); vertex_index[nv] = owning primitive (Scene.py:128) */
int tirt_process_normal(tirt_ctx *ctx, const int32_t *vertex_index);
int tirt_vertex_download(tirt_ctx *ctx, float *vertex);
/* Move whole triangles of the uploaded scene in place (csrc/tirt_dynamic.hip): vertices first ..
 * first + count - 1 (multiples of 3) get position and normal, row i at pos + i * pos_stride floats; nrm == NULL: Scene.cal_normal's face
 * normals.  Host pointers, or (_device) memory of ctx's device, ordered after `stream`; the rows must not change during the call.  Waits for
 * all batches first and for its own work; tirt_lbvh_build must follow.  Columns 6..8 of the rows (the uvs of albedo textures) are not written: they survive.  The scene box becomes the fminf / fmaxf box of ALL vertex rows
 * (rows left non-finite by tirt_scene_upload are ignored; which zero a +-0 corner gets is not defined).  TIRT_ERR_ARG before anything is
 * queued (range, stride, pointer kind, capturing stream, no scene) or written (a NaN / infinite position): the old build stays usable. */
int tirt_vertex_update(tirt_ctx *ctx, int64_t first, int64_t count, const float *pos, int64_t pos_stride,
                       const float *nrm, int64_t nrm_stride);
int tirt_vertex_update_device(tirt_ctx *ctx, int64_t first, int64_t count, const float *pos, int64_t pos_stride,
                              const float *nrm, int64_t nrm_stride, void *stream);
/* the scene box as the context holds it: tirt_scene_upload's, or the one the last vertex update computed */
int tirt_scene_box(tirt_ctx *ctx, float bmin[3], float bmax[3]);
/* Scene.total_area (Scene.py:747-750) */
int tirt_total_area(tirt_ctx *ctx, float *out);

/* Camera.update field uploads (Camera.py:91-93) + intrinsics (Camera.py:31-34) */
int tirt_camera_set(tirt_ctx *ctx, const float view[16], const float view_inv[16], const float eye[3],
                    float fx, float fy, float cx, float cy);

/* PathTrace.setup_data_cpu (integrator/PT_RGB.py:34-37): hdr + rgb_film, W*H*3 f32 each,
 * index (i*H + j)*3.  This context renders the pixels whose linear index p = i*H + j lies
 * in a tile (p / tile_size) with tile % tile_count == tile_rank (tile_count 1: all).  A tile_size of a multiple of 8 whole
 * columns (8 * H pixels; H a multiple of 8, W * H a multiple of tile_size) lets the device walk a tile in 8 x 8 pixel blocks
 * -- the camera rays of a wave are then a compact bundle; any other tile_size works too. */
int tirt_film_create(tirt_ctx *ctx, int W, int H, int tile_rank, int tile_count, int tile_size);
int tirt_film_clear(tirt_ctx *ctx);       /* zeroes hdr, rgb_film and the enabled records; an installed pixel set (tirt_pixel_set_*) stays installed */

/* PathTrace.render x frame_count (integrator/PT_RGB.py:44-136), frames frame_begin ..
 * frame_begin+frame_count-1 accumulated into hdr as the running mean of :134-136.
 * Asynchronous, and possibly deferred: see option "merge_paths". */
int tirt_pt_rgb_render(tirt_ctx *ctx, uint32_t frame_begin, int frame_count, uint32_t seed,
                       int max_depth, int stack_size, int flags);

/* BDPT.render x frame_count (integrator/BDPT_RGB.py:595-642): eye + light sub-paths, all
 * connections up to MAX_DEPTH 5 with MIS, light-tracing splats; same film, camera and tiling as
 * PT_RGB (with tiles, every context accumulates splats into its full-size film: sum-reduce). */
int tirt_bdpt_rgb_render(tirt_ctx *ctx, uint32_t frame_begin, int frame_count, uint32_t seed);
/* BDPT.render x frame_count of integrator/BDPT_SPEC.py:660-691: the same bidirectional tracer carrying one wavelength per pixel sample
 * (reflectances and emitters through the RGB -> spectrum table, dispersive glass, AddSplat through the CIE observer).  Needs
 * tirt_spectral_upload.  The example that uses it: example/prism_rainbow.py (a laser through a prism). */
int tirt_bdpt_spec_render(tirt_ctx *ctx, uint32_t frame_begin, int frame_count, uint32_t seed);
/* ---- BDPT under test: the contributions and the sub-path vertices themselves (tests/test_gpu_bdpt_records.py) -----------------------------
 * A film shows BDPT's contributions only as sums formed by float atomics in no fixed order; these two show the numbers added and what they were made from.
 * tirt_bdpt_record_enable: capacity >= 0 turns the contribution record on with room for `capacity` records and restarts its count; capacity < 0 turns it off
 *   and frees it.  While on, tirt_bdpt_rgb_render / tirt_bdpt_spec_render write one record per contribution they EVALUATE with a target on the film: every
 *   connection whose ray met the primitive it was aimed at (k_bd_resolve's list) and every eye sub-path that ended on an emitter (k_bd_emitted), zero or
 *   not; an e == 1 connection that projects off the film has no target and no record.  A record is eight 32-bit words: frame, source pixel p (whose
 *   sub-paths made it), target pixel q (where it is added), e, l as int32, then the three values added as float32 (SPEC: after the sensor conversion) --
 *   before k_bd_resolve's pairwise pre-sum.  The order of the records is not defined.  Records beyond the capacity are dropped and still counted.
 *   The film is made as always (same atomics); the kernels launched are instantiations that differ from the usual ones by the store alone, and with
 *   the record off the usual ones are launched.  Waits for pending work.
 * tirt_bdpt_record_download: the first min(capacity, kept) records into `records`, and into *needed how many the renders since the enable needed
 *   (which may exceed either capacity).  TIRT_ERR_ARG when the record is off.
 * tirt_bdpt_vertices_download: what the kernels of the last BDPT call left in device memory, provided it ran as ONE batch: *items = its items (frames x
 *   owned pixels); with capacity >= *items also item_rows[4 * it] = frame, pixel, eye_depth | tail << 16 (tail: slot eye[eye_depth] holds a surface vertex of
 *   this item whose sampling ended the path), light_depth, and vertices[it][13][80 bytes]: eye slots 0..6, light slots 0..5, each (pos, prim) (snormal, mat)
 *   (normal, fpdf) (beta, rpdf) (wo, int16 type, int16 delta).  capacity <= 0 asks for *items alone.  Slots the item did not write hold what was there
 *   (option "bdpt_state_fill").  Launches nothing in a render.  TIRT_ERR_ARG when no BDPT call has rendered into this film or the last one used more than one batch. */
int tirt_bdpt_record_enable(tirt_ctx *ctx, long capacity);
int tirt_bdpt_record_download(tirt_ctx *ctx, void *records, long capacity, long *needed);
int tirt_bdpt_vertices_download(tirt_ctx *ctx, int32_t *item_rows, void *vertices, long capacity, long *items);

/* ---- spectral path: integrator/PT_Spec.py (hero-wavelength path tracer) -----------------------------
 * tirt_spec_table_build: spectrum/JakobSpecTable.py:1-439 on the device -- the RGB -> sigmoid-spectrum coefficient table that
 *   Rgb2Spec.load_table reads from spectrum/spec_table (a file the reference repository lacks).  cie_xyz [n*3] and d65 [n] for
 *   360..830 nm in 1 nm steps (n = 471; spectrum/ciexyz31_1.csv, spectrum/Illuminantd65.csv from 360 nm on);
 *   scale_out [res], coeff_out [3*res^3*3] in the order of the table file (res = 64 there).
 * tirt_spectral_upload: what PathTrace.setup_data_cpu / setup_data_gpu place (PT_Spec.py:56-99): the CIE 1931 observer rows
 *   (sensor [n_sensor*3], wavelengths s_min..s_max, step s_range), four tabulated spectra back to back in `spd` (D65 after
 *   normalize_spec, white, red, green: Spectrum.load_table; sizes spd_n, ranges spd_min / spd_max / spd_range), the Rgb2Spec table
 *   (tbl_scale [res], tbl_data [3*res^3*3]), and the sky (Sky.configs [11*9], Sky.radiances [11], Sky.sun_dir; sky/Sky.py:76-172).
 * tirt_pt_spec_render: PathTrace.render x frame_count (PT_Spec.py:181-279; MAX_DEPTH 10 there); film, camera, tiling, deferred
 *   submission and flags as tirt_pt_rgb_render. */
typedef struct {
    const float *sensor; int n_sensor; float s_min, s_max, s_range;
    const float *spd; int spd_n[4]; float spd_min[4], spd_max[4], spd_range[4];
    const float *tbl_scale, *tbl_data; int tbl_res;
    const float *sky_cfg, *sky_rad; float sun_dir[3];
} tirt_spectral_t;
int tirt_spec_table_build(tirt_ctx *ctx, int res, const float *cie_xyz, const float *d65, int n, float *scale_out, float *coeff_out);
int tirt_spectral_upload(tirt_ctx *ctx, const tirt_spectral_t *tables);
int tirt_pt_spec_render(tirt_ctx *ctx, uint32_t frame_begin, int frame_count, uint32_t seed, int max_depth, int stack_size, int flags);

/* Debug.render (integrator/Debug.py:44-67): for every pixel of this context's tiles, the camera ray of `frame` (jittered iff
 * frame != 0, the same ray as tirt_pt_rgb_render's at that frame and seed), its closest hit, and hdr[i, j] OVERWRITTEN with one
 * view of that hit -- (0, 0, 0) on a miss, no running mean:
 *   TIRT_DEBUG_ALBEDO   the material colour, words 2..4 (:65); on a textured material tex_albedo at the hit's uv (tirt_texture_upload)
 *   TIRT_DEBUG_FNORMAL  (faceforward(normal, -direction, gnormal) + 1) * 0.5 (:62); normal as below
 *   TIRT_DEBUG_NORMAL   (normal + 1) * 0.5 (:63); on a normal-mapped material the mapped normal N' (tirt_kat_material_maps)
 *   TIRT_DEBUG_GNORMAL  (gnormal + 1) * 0.5 (:64)
 * Pixels of other ranks' tiles are left as they are.  flags: TIRT_TRAVERSE_EXHAUSTIVE, TIRT_COUNT_NODES; stack_size 1..4096.
 * Asynchronous; the rays count in rays_closest, a traversal stack overflow is reported by tirt_stats (TIRT_ERR_STACK). */
#define TIRT_DEBUG_ALBEDO 0
#define TIRT_DEBUG_FNORMAL 1
#define TIRT_DEBUG_NORMAL 2
#define TIRT_DEBUG_GNORMAL 3
int tirt_debug_render(tirt_ctx *ctx, uint32_t frame, uint32_t seed, int mode, int stack_size, int flags);

/* UtilsFunc.tone_map(exposure, hdr, rgb_film) (UtilsFunc.py:583-586) */
int tirt_tone_map(tirt_ctx *ctx, float exposure);
/* field.to_numpy(): either pointer may be NULL */
int tirt_film_download(tirt_ctx *ctx, float *hdr, float *rgb);
/* device-to-device copy of hdr into / from a caller-owned device buffer of W*H*3 f32
 * (e.g. a torch tensor that is then reduced over RCCL) */
int tirt_film_export_device(tirt_ctx *ctx, void *dev_dst);
int tirt_film_import_device(tirt_ctx *ctx, const void *dev_src);

/* Feature buffers of the path tracer (csrc/tirt_aov.hip; no reference counterpart).  While enabled, every frame of tirt_pt_rgb_render /
 * tirt_pt_spec_render also folds, per pixel of this context's tiles, the closest hit of that frame's camera ray into TIRT_AOV_WORDS f32 with the
 * film's running mean (integrator/PT_RGB.py:134-136), frames in ascending order:
 *   TIRT_AOV_ALBEDO  3 words: the material colour, or the albedo texture's, as TIRT_DEBUG_ALBEDO reads it (no sRGB conversion)
 *   TIRT_AOV_NORMAL  3 words: the shading normal (a normal-mapped material's mapped normal) as TIRT_DEBUG_NORMAL reads it, NOT mapped to [0, 1] and not face-forwarded (a NaN stays a NaN)
 *   TIRT_AOV_DEPTH   1 word : the hit distance t
 *   TIRT_AOV_ALPHA   1 word : 1
 * and zeros on a miss.  hdr is not touched; pixels of other ranks' tiles are never written (zero: the ranks' records sum to the whole).
 * tirt_bdpt_rgb_render, tirt_bdpt_spec_render and tirt_debug_render leave the records alone.  tirt_film_clear zeroes them.
 * tirt_aov_enable: needs a film.  on != 0 allocates and zeroes the records, on == 0 frees them; tirt_film_create disables.  Waits for pending work.
 * tirt_aov_download: out[W*H*TIRT_AOV_WORDS], pixel p = i*H + j as hdr.  tirt_aov_export_device: the same into device memory, as
 * tirt_film_export_device.  TIRT_ERR_ARG when not enabled, without a film, or for a null pointer. */
#define TIRT_AOV_WORDS 8
#define TIRT_AOV_ALBEDO 0
#define TIRT_AOV_NORMAL 3
#define TIRT_AOV_DEPTH 6
#define TIRT_AOV_ALPHA 7
int tirt_aov_enable(tirt_ctx *ctx, int on);
int tirt_aov_download(tirt_ctx *ctx, float *out);
int tirt_aov_export_device(tirt_ctx *ctx, void *dev_dst);

/* Edge-avoiding a-trous denoiser over the film and its feature buffers (csrc/tirt_denoise.hip; no reference counterpart): the joint-bilateral wavelet filter of
 * Dammertz et al. 2010 on albedo-demodulated radiance, guided by the records' first-hit normal and depth.  It writes a buffer of its own; hdr, rgb_film and
 * the records are only read.  All f32, one rounding per operation in the order written (tests/denoise_expected.py restates it; the device gives its bits):
 *   prepare, per pixel p = i*H + j with record words alb[3], n[3], z, al:  d = fmaxf(alb + (1 - al), 1e-3) per channel (the missed share of a pixel counts as
 *     albedo 1),  e = hdr / d,  rz = 1 / fmaxf(z*z, 1e-12)
 *   level l = 0 .. levels-1, step = 1 << l, on the host ic = 1 / (s*s) with s = sigma_c * 2^-l, in = 1 / (sigma_n*sigma_n), iz = 1 / (sigma_z*sigma_z): the taps
 *     q = (i + di*step, j + dj*step), di = -2..2 outer, dj = -2..2 inner, those outside the film skipped, the centre included:
 *       k = h[|di|] * h[|dj|], h = {0.375, 0.25, 0.0625};  dc = ((e_p.r-e_q.r)^2 + (e_p.g-e_q.g)^2) + (e_p.b-e_q.b)^2;  dn the same over n;
 *       dz = ((z_p-z_q) * (z_p-z_q)) * rz_p;  x = (dc*ic + dn*in) + dz*iz;  w = k * exp(-x), exp as tirt_kat_math fn 2;
 *       a tap counts only if w and all of e_q are finite: sum_c += e_q * w per channel, sum_w += w
 *     e'_p = sum_c / sum_w; a pixel whose own e_p is not finite keeps it (the film's NaN pixels stay and poison no neighbour).  A NaN normal makes every w of its
 *     pixel NaN, its own centre tap included: such a pixel drops out of its neighbours' sums and comes out NaN itself (0 / 0)
 *   remodulate: out = e * d
 * tirt_denoise_t: levels 1..8, sigmas finite and > 0, else TIRT_ERR_ARG; a NULL pointer means the defaults {5, 1.0, 0.3, 0.1}.
 * tirt_denoise: the context's hdr with its records into a context-owned buffer, on the main stream after the last film and record update; asynchronous.
 *   TIRT_ERR_ARG without a film, without enabled feature buffers, or with tile_count > 1 (a rank's film is partial: reduce, then tirt_denoise_device).
 * tirt_denoise_download / tirt_denoise_export_device: out[W*H*3], as tirt_film_download / tirt_film_export_device; TIRT_ERR_ARG before the first tirt_denoise
 *   of this film.  tirt_film_create drops the buffer and the filter's scratch (60 B per pixel); tirt_film_clear leaves both alone.
 * tirt_denoise_device: the same filter on caller-owned device arrays hdr [W,H,3], aov [W,H,TIRT_AOV_WORDS] (16-byte aligned), out [W,H,3] (e.g. torch tensors);
 *   needs no film.  Ordering on `stream`, the pointer checks and the refusal of a capturing stream are tirt_query_closest's; out may not overlap the inputs.
 * First-hit guides know nothing of what is seen through glass or in a mirror: there the filter can blur detail the guides do not show. */
typedef struct { int levels; float sigma_c, sigma_n, sigma_z; } tirt_denoise_t;
int tirt_denoise(tirt_ctx *ctx, const tirt_denoise_t *params);
int tirt_denoise_download(tirt_ctx *ctx, float *out);
int tirt_denoise_export_device(tirt_ctx *ctx, void *dev_dst);
int tirt_denoise_device(tirt_ctx *ctx, const float *hdr, const float *aov, float *out, int W, int H, const tirt_denoise_t *params, void *stream);

/* Sample moments of the path tracer (csrc/tirt_moments.hip; no reference counterpart).  While enabled, every frame of tirt_pt_rgb_render also folds, per pixel of
 * this context's tiles, that frame's pixel-sample x = the final radiance (r, g, b) that the film's running mean takes in, into TIRT_MOM_WORDS f32:
 *   TIRT_MOM_N     1 word : n, the samples folded so far
 *   TIRT_MOM_MEAN  3 words: their mean
 *   TIRT_MOM_M2    3 words: their sum of squared deviations from the mean (sample variance = M2 / (n - 1), variance of the mean = M2 / (n * (n - 1)))
 *   TIRT_MOM_BAD   1 word : samples skipped because a channel was NaN or +-infinite
 * by Welford's update, frames in ascending order, all f32 with one rounding per operation in this order (tests/moments_expected.py restates it; the device
 * gives its bits):  a sample with a channel that is not finite: bad = bad + 1, nothing else;  otherwise n = n + 1 and per channel
 *   delta = x - mean;  mean = mean + delta / n;  M2 = M2 + delta * (x - mean)      (the new mean; the division is tirt_kat_math fn 8's; no FMA)
 * n is the record's own count, not a frame index: frames may start anywhere, come in any order or repeat with other seeds, and the record is the moments
 * of whatever was rendered since the last clear.  As an f32 it is exact up to 2^24 samples per pixel.  The result does not depend on how the same frames
 * are cut into calls, merges ("merge_paths"), batches, lanes and tiles, nor on the route of the camera rays.
 * hdr is not touched; pixels of other ranks' tiles are never written (zero: the ranks' records sum to the whole).  tirt_pt_spec_render, tirt_bdpt_rgb_render,
 * tirt_bdpt_spec_render and tirt_debug_render leave the records alone: their per-frame samples are not RGB radiance per pixel-sample (PT_RGB only).
 * tirt_moments_enable: needs a film.  on != 0 allocates and zeroes the records, on == 0 frees them; tirt_film_create disables, tirt_film_clear zeroes.  Waits
 *   for pending work.
 * tirt_moments_download: out[W*H*TIRT_MOM_WORDS], pixel p = i*H + j as hdr.  tirt_moments_export_device: the same into device memory, as
 *   tirt_film_export_device.  TIRT_ERR_ARG when not enabled, without a film, or for a null pointer.
 * tirt_moments_converged: over this context's own pixels, out[0] = the measured ones (n >= 2), out[1] = the measured ones that are still noisy:
 *     v > t2 * (Y * Y)  with  nn = n * (n - 1),  v = (M2.r / nn + M2.g / nn) + M2.b / nn,  Y = ((mean.r + mean.g) + mean.b) / 3,  t2 = threshold * threshold (host)
 *   -- the standard error exceeds `threshold` x the mean level; a measured black pixel without variance is converged --, out[2] = pixels with bad > 0.
 *   One pass on the device; waits for pending work and for the answer.  TIRT_ERR_ARG as the downloads, and for a threshold that is NaN or <= 0. */
#define TIRT_MOM_WORDS 8
#define TIRT_MOM_N 0
#define TIRT_MOM_MEAN 1
#define TIRT_MOM_M2 4
#define TIRT_MOM_BAD 7
int tirt_moments_enable(tirt_ctx *ctx, int on);
int tirt_moments_download(tirt_ctx *ctx, float *out);
int tirt_moments_export_device(tirt_ctx *ctx, void *dev_dst);
int tirt_moments_converged(tirt_ctx *ctx, float threshold, uint64_t out[3]);

/* Variance-guided mode of the denoiser (csrc/tirt_denoise.hip): the a-trous of SVGF (Schied et al. 2017) without its temporal part.  The colour edge-stopping
 * term of tirt_denoise is scaled by the pixel's own variance of the mean, from the sample moments, instead of one film-wide sigma_c, and that variance is
 * filtered along.  tirt_denoise and its structure are unchanged.  All f32, one rounding per operation in the order written (tests/denoise_var_expected.py):
 *   prepare, per pixel: d, e = hdr / d and z as tirt_denoise; from the moment record  s = -1  unless n >= 2 and, with nn = n * (n - 1), v = M2 / nn per channel,
 *     t = (v.r / (d.r*d.r) + v.g / (d.g*d.g)) + v.b / (d.b*d.b)  satisfies 0 <= t < inf: then s = t (the variance of the mean of e, summed over channels).
 *     A value s is KNOWN when 0 <= s < inf; -1, NaN and inf are not.  A pixel whose s is not known has its colour term switched off (it is filtered by the
 *     guides alone), keeps that s through every step, and is skipped wherever variances are summed: no weight is NaN because of it.
 *   prefilter, once: a pixel with a known s gets  s = sum(k * s_q) / sum(k)  over the taps q = (i + di, j + dj), di = -1..1 outer, dj = -1..1 inner, that are
 *     inside the film and have a known s_q;  k = g[|di|] * g[|dj|], g = {0.5, 0.25} (so 1/4, 1/8, 1/16); sums in tap order
 *   level l = 0 .. levels-1, step = 1 << l, on the host sc2 = sigma_c * sigma_c (the same at every level), in and iz as tirt_denoise; per pixel
 *     rz = 1 / fmaxf(z*z, 1e-12),  cden = sc2 * s_p + 1e-12;  taps, k, dc, dn, dz as tirt_denoise;
 *       xc = dc / cden if s_p is known, else 0;  x = (xc + dn*in) + dz*iz;  w = k * exp(-x);
 *       a tap counts only if w and all of e_q are finite: sum_c += e_q * w, sum_w += w, and if s_q is known also  sum_v += (w * w) * s_q, sum_wv += w
 *     e'_p as tirt_denoise (a pixel whose own e is not finite keeps it);  s'_p = sum_v / (sum_wv * sum_wv) if s_p is known and sum_wv > 0, else s_p
 *   remodulate: out = e * d
 * tirt_denoise_var_t: levels 1..8, sigmas finite and > 0, else TIRT_ERR_ARG; NULL means {5, TIRT_DENOISE_VAR_SIGMA_C, 0.3, 0.1}.
 * tirt_denoise_var: the context's hdr, feature records and moment records into the buffer tirt_denoise_download / tirt_denoise_export_device read.  Refusals:
 *   tirt_denoise's, and TIRT_ERR_ARG when the moment buffers are not enabled.
 * tirt_denoise_var_device: on caller-owned device arrays, mom [W,H,TIRT_MOM_WORDS] 16-byte aligned as aov; otherwise as tirt_denoise_device. */
#define TIRT_DENOISE_VAR_SIGMA_C 3.0f
typedef tirt_denoise_t tirt_denoise_var_t;
int tirt_denoise_var(tirt_ctx *ctx, const tirt_denoise_var_t *params);
int tirt_denoise_var_device(tirt_ctx *ctx, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_var_t *params, void *stream);

/* Temporal accumulation (csrc/tirt_temporal.hip; no reference counterpart; PT_RGB only): the temporal part of SVGF (Schied et al. 2017) beside
 * tirt_denoise_var.  The film and the moment records of the PREVIOUS view are reprojected through the current view's first-hit surface point, rejected
 * where the surfaces disagree, and merged with the current film as sample statistics; the result has the layout of hdr and of the moment records, so
 * tirt_denoise_var consumes it unchanged, with the current feature records as its guides.  The world must have stood still between the views (unless
 * the motion records of the next section are on), and first-hit guides know nothing of what is seen through glass or in a mirror.
 * The random numbers are counter-based on (seed, pixel, frame, dimension) and a cleared film restarts at frame 0: two views rendered with the same seed
 * draw the same numbers per pixel, so a caller who accumulates views must change the seed per view (seed + view, say).
 * One thread per current pixel p = i*H + j; all f32, one rounding per operation in the order written (tests/temporal_expected.py restates it; the device
 * gives its bits).  "c" = current, "h" = history; a comparison with a NaN is false:
 *   1. surface point: record words n_c[3], z, al of aov_c.  al > 0 fails (every camera ray missed): NO HISTORY.  zc = z / al;
 *      D = camera_ray_direction(cur, i, j, 0, 0) (the pixel centre: x = ((float)i + 0 - cx) / fx, ..., the view_inv rows summed left to right, normalised
 *      by 1 / sqrt);  X = eye_cur + D * zc per component
 *   2. into the previous view: q.r = ((V[r][0] * X.x + V[r][1] * X.y) + V[r][2] * X.z) + V[r][3], r = 0..2, V = prev.view.  q.z < 0 fails: NO HISTORY.
 *      nz = -q.z;  fi = (q.x / nz) * fx_prev + cx_prev;  fj = (q.y / nz) * fy_prev + cy_prev  (an integer fi is a pixel centre).
 *      -1 < fi < W and -1 < fj < H fails (no tap would lie inside the film): NO HISTORY.  i0 = floor(fi), j0 = floor(fj), wi = fi - i0, wj = fj - j0;
 *      e = X - eye_prev;  d_exp = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z), correctly rounded
 *   3. taps t = (i0 + a, j0 + b), a = 0..1 outer, b = 0..1 inner, weight k = (a ? wi : 1 - wi) * (b ? wj : 1 - wj).  A tap counts only if it lies inside
 *      the film, al_h > 0, dn = ((n_c.x-n_h.x)^2 + (n_c.y-n_h.y)^2) + (n_c.z-n_h.z)^2 <= sigma_n * sigma_n (host product),
 *      |d_exp - z_h / al_h| <= sigma_z * d_exp, its count n_h > 0, and its hdr_h[3] and its mean and M2 words are all finite.  Counted taps, in tap order:
 *      sw += k;  s_hdr[3] += hdr_h * k;  s_mom[8] += mom_h * k (all eight words: n, mean, M2 and bad interpolate linearly, which keeps M2 / n where the
 *      neighbourhood is uniform).  sw >= 1e-3 fails: NO HISTORY.  Otherwise hdr_h = s_hdr / sw and (n_h, mean_h, M2_h, bad_h) = s_mom / sw
 *   4. cap: if n_h > max_history:  f = max_history / n_h;  n_h = max_history;  M2_h = M2_h * f;  bad_h = bad_h * f  (mean_h and hdr_h stay: old samples
 *      fade once the history is full -- an exponential window written as a sample count)
 *   5. merge (the pairwise update of Chan et al.), with the current record (n_c, mean_c, M2_c, bad_c):  N = n_h + n_c.
 *      n_c == 0: mom_o = the history's eight words, hdr_o = hdr_h.  Else N == 0: NO HISTORY.  Else  w = n_c / N  and per channel
 *        delta = mean_c - mean_h;  mean_o = mean_h + delta * w;  M2_o = (M2_h + M2_c) + (delta * delta) * (n_h * w);  hdr_o = hdr_h + (hdr_c - hdr_h) * w
 *      and n_o = N, bad_o = bad_h + bad_c.  In both cases a pixel whose own hdr_c has a channel that is not finite keeps hdr_c in all three channels
 *      (the film's NaN pixels stay, as in tirt_denoise); its moment words still merge: they only ever held the finite samples
 *   6. NO HISTORY: hdr_o = hdr_c and mom_o = mom_c, bit for bit.
 * tirt_temporal_t: max_history, sigma_n, sigma_z finite and > 0, else TIRT_ERR_ARG; NULL means {TIRT_TEMPORAL_MAX_HISTORY, 0.3, 0.1}
 *   (profiles/temporal_quality.txt has the sweep behind them).
 * tirt_temporal_camera_t: what tirt_camera_set takes.  Of `cur` the kernel reads view_inv, eye and the intrinsics, of `prev` view, eye and the intrinsics.
 * tirt_temporal_device: on caller-owned device arrays (e.g. torch tensors) in the layouts of tirt_film_export_device, tirt_aov_export_device and
 *   tirt_moments_export_device: current hdr_c, aov_c, mom_c, history hdr_h, aov_h, mom_h (the output of an earlier call with the aov_c of that call, or a
 *   plain film with its records), out hdr_o [W,H,3], mom_o [W,H,TIRT_MOM_WORDS]; the guide record of the output is aov_c itself.  The feature and moment
 *   arrays must be 16-byte aligned; no output may overlap an input or the other output.  Needs no film and no scene.  Ordering on `stream`, the pointer
 *   checks and the refusal of a capturing stream are tirt_denoise_device's.
 * The context's own history (tile_count == 1; a rank's film is partial: reduce the films and the records, then tirt_temporal_device):
 * tirt_temporal_enable: needs a film with enabled feature buffers and moment records; on != 0 allocates two history sets of (3 + 8 + 8) f32 per pixel
 *   and marks the history empty, on == 0 frees them.  tirt_film_create disables; tirt_aov_enable(0) and tirt_moments_enable(0) return TIRT_ERR_ARG while
 *   it is on.  Waits for pending work.
 * tirt_temporal_accumulate: on the main stream after the last film and record update; asynchronous.  Current = the context's hdr, feature and moment
 *   records and the camera set now; history = the result of the previous call with the feature records and the camera of that call.  With an empty
 *   history the result is the current film and records copied.  The result, a copy of the feature records and the camera become the new history.
 *   hdr, rgb_film, the records, the denoised film and an installed pixel set are only read; an adaptively sampled film merges pixel by pixel with its
 *   own n.  Nothing is added to the render path.  TIRT_ERR_ARG when not enabled or without a camera.
 * tirt_temporal_reset: empties the history.  tirt_scene_upload, tirt_vertex_update and tirt_vertex_update_device empty it too (the reprojection assumes
 *   the world stood still; with tirt_motion_enable the two updates keep it); tirt_film_clear leaves it alone -- carrying samples across a cleared film is what this is for.
 * tirt_temporal_download / tirt_temporal_export_device: the accumulated hdr [W*H*3] and moment records [W*H*TIRT_MOM_WORDS]; either pointer may be NULL.
 *   TIRT_ERR_ARG while the history is empty.  They wait for the copy.
 * tirt_temporal_denoise_var: tirt_denoise_var's filter over the accumulated hdr and moments with the history's feature records (those of the last
 *   accumulated view), into the buffer tirt_denoise_download / tirt_denoise_export_device read.  tirt_denoise and tirt_denoise_var are unchanged. */
#define TIRT_TEMPORAL_MAX_HISTORY 32.0f
typedef struct { float max_history, sigma_n, sigma_z; } tirt_temporal_t;
typedef struct { float view[16], view_inv[16], eye[3], fx, fy, cx, cy; } tirt_temporal_camera_t;
int tirt_temporal_device(tirt_ctx *ctx, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                         const tirt_temporal_camera_t *cur, const tirt_temporal_camera_t *prev, float *hdr_o, float *mom_o, int W, int H,
                         const tirt_temporal_t *params, void *stream);
int tirt_temporal_enable(tirt_ctx *ctx, int on);
int tirt_temporal_accumulate(tirt_ctx *ctx, const tirt_temporal_t *params);
int tirt_temporal_reset(tirt_ctx *ctx);
int tirt_temporal_download(tirt_ctx *ctx, float *hdr_out, float *mom_out);
int tirt_temporal_export_device(tirt_ctx *ctx, void *hdr_dst, void *mom_dst);
int tirt_temporal_denoise_var(tirt_ctx *ctx, const tirt_denoise_var_t *params);

/* Temporal accumulation across MOVING geometry: per-pixel motion records (csrc/tirt_temporal.hip, csrc/tirt_dynamic.hip; no reference counterpart; opt-in).
 * The part of SVGF the section above leaves out: backprojection through the surface's own motion.  While tirt_motion_enable is off everything above holds as
 * stated, a geometry update emptying the history included.  While it is on and the history is not empty, tirt_vertex_update and tirt_vertex_update_device
 * -- after all their refusals, a refused call changes nothing -- copy the whole vertex buffer to a SNAPSHOT before they write, unless an earlier update
 * since the last accumulate has done so already, mark the geometry as moved, and leave the history in place: however many updates lie between two
 * accumulates, the snapshot holds the vertex rows of the last accumulated view.  tirt_scene_upload, tirt_temporal_reset, tirt_film_create and every
 * successful tirt_temporal_accumulate clear the mark; tirt_scene_upload and tirt_temporal_reset still empty the history.  Normals rewritten by
 * tirt_process_normal are not tracked: the snapshot is taken by the vertex updates alone, so a scene whose normals are smoothed again after an update is
 * compared with whatever normals the rows held when the update began.
 * Motion record, TIRT_MOTION_WORDS f32 per pixel p = i*H + j, 16-byte aligned, made by tirt_temporal_accumulate when the geometry is marked as moved:
 * the camera ray through the pixel centre (tirt_debug_render's ray at frame 0: no jitter) is traced to its closest hit (t, u, v, prim), stack size 64.
 * For a triangle with first vertex vi, a = 1.0f - u - v, on vertex rows R:
 *     P(R) = (v1*a + v2*u) + v3*v        N(R) = normalized((n1*a + n2*u) + n3*v)       (per component; normalized: x * (1 / sqrt((x.x*x.x + x.y*x.y) + x.z*x.z)))
 *   words 0..2  D  = P(snapshot) - P(current)      word 3  1.0
 *   words 4..6  dN = N(snapshot) - N(current)      word 7  0
 * A miss, and a hit on an analytic shape (shapes do not move): eight zeros.  All f32, one rounding per operation in the order written
 * (tests/motion_expected.py restates it; the device gives its bits).
 * With motion records the accumulation above changes in step 1 alone: after X = eye_cur + D * zc,  X = X + D_motion per component, and
 * n_c = n_c + dN per component before the taps' normal test.  A record of zeros is added like any other.  Steps 2 to 6 are as stated: d_exp and the
 * projection use the point where the surface WAS, and the depth and normal tests reject what the moved object uncovered.
 * tirt_motion_enable: needs tirt_temporal_enable; on != 0 allocates the records, on == 0 frees them and the snapshot (and empties a history whose
 *   geometry is marked as moved).  tirt_temporal_enable(0) returns TIRT_ERR_ARG while it is on; tirt_film_create disables it.  Waits for pending work.
 * tirt_temporal_accumulate while it is on: an empty history, or geometry not marked as moved: exactly as without it, and the records are zeroed.  Marked
 *   as moved: TIRT_ERR_ARG when the LBVH is not built (tirt_lbvh_build must follow the vertex update); otherwise the rays, the records and the
 *   accumulation with them on the main stream.  The rays count in rays_closest; a traversal stack overflow is reported by tirt_stats, as tirt_debug_render's.
 * tirt_motion_download / tirt_motion_export_device: out[W*H*TIRT_MOTION_WORDS], the records of the last accumulate; TIRT_ERR_ARG when not enabled, while
 *   the history is empty or before the first accumulate since tirt_motion_enable, or for a null pointer.  They wait for the copy.
 * tirt_motion_temporal_device: tirt_temporal_device with `motion` [W,H,TIRT_MOTION_WORDS] (device memory, 16-byte aligned, no output may overlap it)
 *   between `params` and `stream`: the same checks through the same code, and the accumulation with the records.  tirt_temporal_device is unchanged. */
#define TIRT_MOTION_WORDS 8
int tirt_motion_enable(tirt_ctx *ctx, int on);
int tirt_motion_download(tirt_ctx *ctx, float *out);
int tirt_motion_export_device(tirt_ctx *ctx, void *dev_dst);
int tirt_motion_temporal_device(tirt_ctx *ctx, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                                const tirt_temporal_camera_t *cur, const tirt_temporal_camera_t *prev, float *hdr_o, float *mom_o, int W, int H,
                                const tirt_temporal_t *params, const float *motion, void *stream);

/* Pixel set and adaptive sampling of the path tracer (csrc/tirt_adaptive.hip; no reference counterpart; PT_RGB only).  A pixel set is a list of linear pixel
 * indices p = i*H + j of this context's own tiles, strictly ascending in the context's LOCAL order (the order in which the device walks its tiles: tile by
 * tile, and inside a tile of whole 8-column groups in 8 x 8 pixel blocks -- tirt_film_create; for every other tiling ascending p).  While one is installed,
 * tirt_pt_rgb_render renders the n listed pixels instead of all of this context's: path s of a batch is (frame, list entry), and the camera jitter, the random
 * numbers, the film, the feature buffers and the sample moments all see the listed pixel.  The random numbers are counter-based on (seed, pixel, frame,
 * dimension) and the film's weight is 1 / (frame + 1), so a pixel rendered at frames 0 .. m-1 and left alone since holds, bit for bit, the film, feature and
 * moment records of a dense render of m frames at that pixel.  Pixels outside the set are neither read nor written.  An empty set (n == 0) makes
 * tirt_pt_rgb_render a no-op that returns TIRT_OK.  The camera rays of such batches all go through the ordinary traversal (option "primary_beams" does not apply).
 * tirt_pt_spec_render, tirt_bdpt_rgb_render, tirt_bdpt_spec_render and tirt_debug_render return TIRT_ERR_ARG while a set is installed (tirt_pixel_set_clear first).
 * Every call below waits for pending work (as tirt_moments_enable does): a list is never rewritten under a batch that reads it.
 * tirt_pixel_set_upload: installs the caller's list pixels[0 .. n).  Refused with TIRT_ERR_ARG, before anything is written and with an installed set left as it
 *   was: no film; n < 0; n > 0 with a null list; n == 0 with a non-null list; an entry outside [0, W*H), in another rank's tile, equal to its predecessor or
 *   before it in local order.  n == 0 with a null list installs the empty set.
 * tirt_pixel_set_from_moments: makes the list on the device from the moment records (needs tirt_moments_enable) and installs it; *count (may be NULL) = its
 *   length.  Pixel k of the local order, record (n, mean, M2, bad), all f32 in this order, t2 = threshold * threshold (host), a comparison with a NaN false:
 *     total = n + bad;  nn = n * (n - 1);  v = (M2.r / nn + M2.g / nn) + M2.b / nn;  Y = ((mean.r + mean.g) + mean.b) / 3      (tirt_moments_converged's v and Y)
 *     listed  <=>  total < max_samples  and  ( total < min_samples  or  n < 2  or  v > t2 * (Y * Y) )
 *   in ascending local order (an order-preserving compaction: the result does not depend on the scheduling).  TIRT_ERR_ARG, nothing changed: no film, no moment
 *   records, min_samples < 1, max_samples < min_samples, threshold negative or not finite.  One host wait, for the count.
 * tirt_pixel_set_clear: removes the set (no set installed: nothing to do).  tirt_film_create removes it too; tirt_film_clear leaves it alone.
 * tirt_pixel_set_download: *n = the length of the installed list, or -1 when no set is installed; the list into out[0 .. *n) when out is not NULL.
 *   TIRT_ERR_ARG, nothing written: n NULL, cap < 0, or out not NULL and cap < the length.
 * tirt_pt_rgb_render_adaptive: frames from frame_begin on, each pass on the pixels still listed by tirt_pixel_set_from_moments' rule:
 *     start = the total every pixel of this context has (see below);  done = 0
 *     repeat:  select(threshold, min_samples, max_samples);  stop if nothing is listed;  F = min(pass_frames, max_samples - start - done);
 *              render frames frame_begin + done .. + F - 1 on the list;  done += F;  stop if start + done == max_samples
 *   It needs the moment records and NO set installed; it owns the set meanwhile and leaves none installed, on errors too.  The film must be a dense prefix
 *   the caller rendered itself: every pixel of this context with total == frame_begin (start = frame_begin), or all its moment records zero (start = 0);
 *   checked on the device in the first pass, TIRT_ERR_ARG and nothing rendered otherwise.  TIRT_ERR_ARG also for select's refusals and pass_frames < 1.
 *   out (may be NULL): passes rendered, pixel-samples rendered, pixels that reached max_samples in this call, frames of the longest-running pixel (done).
 *   With tile_count > 1 every rank runs its own loop on its own pixels; the ranks' films and records still sum to the single context's.
 *   Waits for every pass's count; a pixel's per-pixel sample count is n + bad of its moment record.
 * The limit: a pixel is stopped on its OWN variance estimate, which is biased towards stopping early where a few samples happen to agree (a pixel whose first
 * min_samples paths all miss a small light is "converged" and black).  min_samples is the only guard; no neighbour-aware or hierarchical criterion is offered. */
typedef struct { float threshold; int32_t min_samples, max_samples, pass_frames; } tirt_adaptive_t;
typedef struct { int64_t passes, pixel_samples, pixels_at_max, frames; } tirt_adaptive_result_t;
int tirt_pixel_set_upload(tirt_ctx *ctx, const int32_t *pixels, int64_t n);
int tirt_pixel_set_from_moments(tirt_ctx *ctx, float threshold, int min_samples, int max_samples, int64_t *count);
int tirt_pixel_set_clear(tirt_ctx *ctx);
int tirt_pixel_set_download(tirt_ctx *ctx, int32_t *out, int64_t cap, int64_t *n);
int tirt_pt_rgb_render_adaptive(tirt_ctx *ctx, uint32_t frame_begin, uint32_t seed, int max_depth, int stack_size, int flags,
                                const tirt_adaptive_t *a, tirt_adaptive_result_t *out);

/* Scene.closet_hit / closet_hit_shadow on a batch of rays (Scene.py:702-744, 671-699).  The default (ordered) traversal returns the
 * reference's hit bit for bit for every ray but the in-plane rays named under "traversal_tree" above; rays that start more than 8
 * scene extents away are traced without distance culling (from there the reference's own distances are rounding noise), so they
 * are the reference's too (tests/test_gpu_trace.py::test_ordered_equals_exhaustive_on_two_million_stress_rays).
 * rays[nr*6] = origin, direction.  out_hit[nr*13] = t, pos3, gnormal3, normal3, tex3;
 * out_prim[nr]; counts[nr*2] = N_box, N_leaf per ray (NULL unless TIRT_COUNT_NODES). */
int tirt_trace_closest(tirt_ctx *ctx, const float *rays, int nr, int stack_size, int flags,
                       float *out_hit, int32_t *out_prim, int32_t *counts);
int tirt_trace_shadow(tirt_ctx *ctx, const float *rays, int nr, int stack_size, int flags,
                      float *out_t, int32_t *out_prim, int32_t *counts);

/* Ray queries on DEVICE memory (no reference entry point: the same traversal as tirt_trace_closest / tirt_trace_shadow, for rays that
 * already live on the GPU, e.g. in torch tensors).  Every pointer is device memory of ctx's device, allocated through the same HIP runtime
 * as libtirt.so (a process with two libamdhip64 runtimes cannot share pointers); `stream` is the caller's hipStream_t (NULL: the null
 * stream).  Row i of the rays starts at rays + i * ray_stride floats and holds origin, direction in its first six floats.
 * Asynchronous: the work runs on the context's own stream, after everything queued on `stream` before the call, and `stream` waits for
 * it; the call returns once the work is queued, with no host sync.  Rays go through in chunks of option "query_chunk_rays" (default 2^21,
 * 256 .. 2^27), whose scratch the context keeps.
 * tirt_query_closest: the closest hit, bit for bit tirt_trace_closest's.  Each output may be NULL: out_t[nr] = t (1e6 on a miss),
 *   out_prim[nr] = primitive (-1 on a miss), out_hit + i * hit_stride = the 13 floats of tirt_trace_closest (t, pos3, gnormal3, normal3,
 *   tex3), counts[nr*2] = N_box, N_leaf per ray (8-byte aligned; only with TIRT_COUNT_NODES).  The rays count in rays_closest.
 * tirt_query_occluded: out_occluded[nr] = 1 where tirt_trace_shadow's t satisfies t < 1e6 && t < tmax, else 0 -- exact, with the walk
 *   stopping early at a hit well inside tmax.  tmax[i * tmax_stride] per ray, or tmax_all for every ray when tmax is NULL; +inf asks for
 *   any hit, tmax <= 0 or NaN answers 0.  The rays count in rays_shadow.
 * flags: TIRT_TRAVERSE_EXHAUSTIVE, TIRT_COUNT_NODES; stack_size 1..4096; a stack overflow is reported by tirt_stats (TIRT_ERR_STACK).
 * Refused with TIRT_ERR_ARG before anything is queued: a pointer that is not device memory of ctx's device, ray_stride < 6, hit_stride < 13
 * with out_hit, tmax_stride < 1 with tmax, an LBVH that is not built, other flags, and a `stream` that is capturing a graph.  nr == 0 queues
 * nothing. */
int tirt_query_closest(tirt_ctx *ctx, const float *rays, int64_t nr, int64_t ray_stride, int stack_size, int flags,
                       float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *counts, void *stream);
int tirt_query_occluded(tirt_ctx *ctx, const float *rays, int64_t nr, int64_t ray_stride,
                        const float *tmax, int64_t tmax_stride, float tmax_all,
                        int stack_size, int flags, uint8_t *out_occluded, void *stream);

/* First K hits (no reference counterpart as an entry point; csrc/tirt_multi_hit.hip / .h): the first k surfaces a ray meets, in order, and the count of all
 * of them -- what a caller otherwise gets from k tirt_query_closest calls, each from the previous hit pushed along the ray by an epsilon (which skips or
 * repeats surfaces closer together than the epsilon and loses one of two coincident triangles).  Everything is fp32, in the order written.
 * Bound.  Ray i has a bound tmax (+inf when none is given) and B = min(1e6, tmax) (1e6 = INF_VALUE, the reference's "no hit").  A tmax that is <= 0 or NaN
 *   finds nothing.
 * The hit set H(i) holds every primitive p that meets all three conditions:
 *   1. the reference's exhaustive traversal (Scene.py:702-744) reaches p's leaf: `slabs` passes on every proper ancestor of the leaf in the reference's LBVH;
 *   2. the reference's primitive test gives 0 < t < B: Moller-Trumbore on E1 = v1 - v0, E2 = v2 - v0, or the analytic sphere's near root (Scene.py:529-638);
 *   3. on a scene with cut-outs ("Alpha cut-outs"), the triangle is untagged or tex_alpha at the hit's uv is >= 0.5.
 *   A ray with a NaN component has H = {}.  H is a set: it does not depend on the order of the visits.
 * Order.  t ascending; at equal t bits the LARGER compact leaf index comes first -- the equal-distance rule of the closest hit, so the first element of H is
 *   tirt_query_closest's hit, bit for bit, whenever tmax does not exclude it.
 * Outputs, for k in 0 .. TIRT_HITS_MAX, each optional: out_t[i * k + j] and out_prim[i * k + j] for j < k are the j-th element of H(i), and 1e6 and -1 where
 *   H has fewer; out_hit + (i * k + j) * hit_stride = the 13 floats of tirt_trace_closest for that hit (a miss as tirt_query_closest writes it);
 *   out_count[i] = |H(i)| as int32, which may exceed k.  k == 0 with out_count is the count alone.  With out_count the walk has to meet every element of H and
 *   culls by the bound only; without it, it also culls by the k-th nearest hit so far.
 * tirt_query_hits: device memory on the caller's stream with tirt_query_closest's plumbing, flags and refusals; tmax[i * tmax_stride] per ray, or tmax_all for
 *   every ray when tmax is NULL.  Rays go through in chunks of max(256, query_chunk_rays / max(k, 1)) (40 + 16 k bytes of scratch per ray); counts[nr*2] =
 *   N_box, N_leaf per ray (8-byte aligned; only with TIRT_COUNT_NODES).  TIRT_TRAVERSE_EXHAUSTIVE walks the reference's two-child tree by the reference's rule
 *   (no distance cull): the yardstick, same bits.  stack_size 1..4096 entries of 4 bytes per ray (the first 16 in LDS, the rest in the context's spill buffer);
 *   an entry that does not fit is dropped and the ray counted in stack_overflow (tirt_stats: TIRT_ERR_STACK).  The rays count in rays_closest.
 *   Refused with TIRT_ERR_ARG before anything is queued, beside tirt_query_closest's refusals: k outside 0 .. TIRT_HITS_MAX, k == 0 without out_count,
 *   hit_stride < 13 with out_hit, tmax_stride < 1 with tmax.  nr == 0 queues nothing.
 * tirt_trace_hits: host arrays (rays[nr*6], tmax[nr] or NULL = +inf, out_t[nr*k], out_prim[nr*k], out_hit[nr*k*13], out_count[nr], counts[nr*2]), staged and
 *   synchronous, as tirt_trace_closest is to tirt_query_closest.
 * tirt_kat_hit_list: host only, no context: the n candidates cand[4 i ..] = (t, u, v, bits leaf), leaf >= 0, in the order given through the list code the
 *   kernel runs (csrc/tirt_multi_hit.h) with this k and bound.  out_list[4 j ..] = entry j; out_info = {entries held, candidates with 0 < t < B,
 *   bits of the threshold distance, the threshold's leaf (-1: the list has room)}. */
#define TIRT_HITS_MAX 64
int tirt_query_hits(tirt_ctx *ctx, const float *rays, int64_t nr, int64_t ray_stride,
                    const float *tmax, int64_t tmax_stride, float tmax_all, int k, int stack_size, int flags,
                    float *out_t, int32_t *out_prim, float *out_hit, int64_t hit_stride, int32_t *out_count, int32_t *counts, void *stream);
int tirt_trace_hits(tirt_ctx *ctx, const float *rays, int nr, const float *tmax, int k, int stack_size, int flags,
                    float *out_t, int32_t *out_prim, float *out_hit, int32_t *out_count, int32_t *counts);
int tirt_kat_hit_list(const float *cand, int n, int k, float bound, float *out_list, int32_t *out_info);

/* Closest point (no reference counterpart; csrc/tirt_closest_point.h / .hip): the nearest surface point of the scene to a query point p.
 * Everything is fp32, every operation in the order written, no contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * D2(p, i), Q(p, i), u(p, i), v(p, i) of primitive i:
 *   Triangle with positions a, b, c (Ericson, Real-Time Collision Detection, 5.1.5):
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;
 *     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
 *     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.  The first region whose test holds, in this order:
 *       A   d1 <= 0 and d2 <= 0:                        Q = a (the vertex itself), (u, v) = (0, 0)
 *       B   d3 >= 0 and d4 <= d3:                       Q = b, (u, v) = (1, 0)
 *       AB  vc <= 0 and d1 >= 0 and d3 <= 0:            u = d1 / (d1 - d3), v = 0, Q = a + ab * u
 *       C   d6 >= 0 and d5 <= d6:                       Q = c, (u, v) = (0, 1)
 *       AC  vb <= 0 and d2 >= 0 and d6 <= 0:            v = d2 / (d2 - d6), u = 0, Q = a + ac * v
 *       BC  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), Q = b + (c - b) * w, (u, v) = (1 - w, w)
 *       interior otherwise:                             den = 1 / ((va + vb) + vc), u = vb * den, v = vc * den, Q = (a + ab * u) + ac * v
 *     D2 = dot(p - Q, p - Q).  (u, v) is the hit record's convention, pos = a + u E1 + v E2: normals and uvs interpolate as for a hit.  A comparison
 *     with a NaN is false (such a triangle falls through to the interior); a zero-area triangle yields whatever these expressions yield.
 *   Analytic sphere (SHAPE_SPHERE) with centre c, radius r: pc = p - c, len = sqrt(dot(pc, pc)), d = |len - r| (x < 0 ? -x : x), D2 = d * d,
 *     Q = c + pc * (r / len), and Q = c + (r, 0, 0) where len == 0; u = v = 0.  Spot and laser shapes have no surface and take no part.
 * The answer for p with bound dmax: lim2 = dmax * dmax, formed once (dmax < 0 or NaN: nothing is found; +inf: no bound).  Among the primitives with
 *   D2 <= lim2 the one with the smallest D2; at equal D2 bits the smallest primitive id.  A NaN D2 is never accepted, and neither is D2 = +inf: "nothing"
 *   is prim = -1, d2 = +inf, point and uv 0 -- so a NaN or infinite coordinate of p finds nothing.  This is the minimum of a total order on (D2, prim):
 *   it does not depend on the order of the visits, and the culled walk returns the bits of a scan over all primitives (the culling argument is in the
 *   head of csrc/tirt_point_walk.h).  Alpha cut-outs are ignored: a transparent texel is still surface.
 * tirt_query_closest_point: device memory on the caller's stream with the plumbing of tirt_query_closest -- asynchronous, ordered after and before
 *   `stream` by two events, no host sync, chunks of option "query_chunk_rays" (one launch each; it reads and writes the caller's arrays in place and
 *   needs 0 bytes of scratch per query).  Row i of the points starts at points + i * point_stride floats; dmax[i * dmax_stride] per query, or dmax_all
 *   for every query when dmax is NULL.  Each output may be NULL: out_d2[n], out_prim[n], out_point + i * point_out_stride = Q, out_uv + i * uv_stride =
 *   (u, v), counts[n*2] = N_box (four per node visit), N_leaf (primitive tests) per query (8-byte aligned; only with TIRT_COUNT_NODES).
 *   flags: TIRT_TRAVERSE_EXHAUSTIVE = the scan over all primitive records (the yardstick: N_box 0, N_leaf = primitives), TIRT_COUNT_NODES.  stack_size
 *   1..4096 entries of 8 bytes per query (the first 16 in LDS, the rest in the context's spill buffer); an entry that does not fit is dropped and the
 *   query counted in stack_overflow (tirt_stats: TIRT_ERR_STACK), as a ray's.  The queries are not rays: no ray counter moves.
 *   Refused with TIRT_ERR_ARG before anything is queued: a pointer that is not device memory of ctx's device, point_stride < 3, point_out_stride < 3
 *   with out_point, uv_stride < 2 with out_uv, dmax_stride < 1 with dmax, other flags, an LBVH that is not built, a capturing stream.  n == 0 queues nothing.
 * tirt_closest_point: host arrays (points[n*3], dmax[n] or NULL = +inf, out_point[n*3], out_uv[n*2]), staged in the context's staging buffer (the
 *   columns that are there, each aligned to its element) and synchronous, as tirt_trace_closest is to tirt_query_closest.
 * tirt_kat_closest_point: D2, Q, u, v of explicit operands through the same device function, one row per thread: rows of 12 floats (p3, a3, b3, c3) or,
 *   with is_sphere, 7 floats (p3, c3, r), to rows of 6 floats (d2, q3, u, v). */
int tirt_query_closest_point(tirt_ctx *ctx, const float *points, int64_t n, int64_t point_stride,
                             const float *dmax, int64_t dmax_stride, float dmax_all, int stack_size, int flags,
                             float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                             float *out_uv, int64_t uv_stride, int32_t *counts, void *stream);
int tirt_closest_point(tirt_ctx *ctx, const float *points, int n, const float *dmax, int stack_size, int flags,
                       float *out_d2, int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts);
int tirt_kat_closest_point(tirt_ctx *ctx, const float *in, int n, int is_sphere, float *out);

/* K nearest primitives (no reference counterpart; csrc/tirt_nearest.hip / .h): the k primitives of the scene nearest to a query point p, in order, and the
 * count of all primitives within the bound -- what a caller otherwise gets from repeated bounded closest-point queries or a KD-tree on the host.
 * Terms.  D2(p, i), Q(p, i), u(p, i), v(p, i) of primitive i, lim2 = dmax * dmax formed once (dmax < 0 or NaN: lim2 = -1; +inf: no bound) and "a NaN or +inf
 *   D2 is never accepted" are those of "Closest point", unchanged: fp32, every operation in the order written there.
 * The set.  N(p) = { i : D2(p, i) <= lim2 and D2(p, i) < +inf }.  A comparison with a NaN is false, so a primitive with a NaN D2 is no element; spot and
 *   laser shapes have no surface and take no part.  N is a set: it does not depend on the order of the visits.  A query with a NaN or infinite coordinate
 *   has N = {} (every D2 is NaN or +inf), and so does a negative or NaN bound (no D2 is <= -1).  Alpha cut-outs are ignored, as for the closest point.
 * Order.  D2 ascending; at equal D2 bits the smaller primitive id comes first.  That is a total order on the elements of N (ids are distinct), and its
 *   element 0 is tirt_query_closest_point's answer, bit for bit.
 * Outputs, for k in 0 .. TIRT_NEAREST_MAX, each optional: out_d2[i * k + j] and out_prim[i * k + j] for j < k are D2 and the id of element j of N(p_i),
 *   and +inf and -1 where N has fewer; out_point + (i * k + j) * point_out_stride = Q and out_uv + (i * k + j) * uv_stride = (u, v) of that element, 0 in
 *   the padding; out_count[i] = |N(p_i)| as int32, which may exceed k.  k == 0 with out_count is the count alone.
 * Culling and out_count.  With out_count the walk has to meet every element of N and culls by lim2 only; without it, it also culls by the k-th smallest D2
 *   so far.  A count without a bound (dmax = +inf) is allowed and degenerates to testing every primitive of the scene for every query.
 * tirt_query_nearest: device memory on the caller's stream with tirt_query_closest_point's plumbing, flags, stack and refusals: row i of the points at
 *   points + i * point_stride floats; dmax[i * dmax_stride] per query, or dmax_all for every query when dmax is NULL; counts[n*2] = N_box (four per node
 *   visit), N_leaf (primitive tests) per query (8-byte aligned; only with TIRT_COUNT_NODES).  Queries go through in chunks of max(256, query_chunk_rays /
 *   max(k, 1)), two launches each (the walk, then the pass that writes the caller's layout), with 8 + 8 k bytes of scratch per query: the list of (D2, prim)
 *   and (entries held, |N|).  TIRT_TRAVERSE_EXHAUSTIVE = all primitive records in id order through the same list code (the yardstick: same bits, N_box 0,
 *   N_leaf = primitives).  stack_size 1..4096 entries of 8 bytes per query (the first 16 in LDS, the rest in the context's spill buffer); an entry that
 *   does not fit is dropped and the query counted in stack_overflow (tirt_stats: TIRT_ERR_STACK).  The queries are not rays: no ray counter moves.
 *   Refused with TIRT_ERR_ARG before anything is queued, beside tirt_query_closest_point's refusals: k outside 0 .. TIRT_NEAREST_MAX, k == 0 without
 *   out_count, k > 0 with no output at all.  n == 0 queues nothing.
 * tirt_nearest: host arrays (points[n*3], dmax[n] or NULL = +inf, out_d2[n*k], out_prim[n*k], out_point[n*k*3], out_uv[n*k*2], out_count[n], counts[n*2]),
 *   staged in the context's staging buffer and synchronous, as tirt_closest_point is to tirt_query_closest_point.
 * tirt_kat_nearest_list: host only, no context: the n candidates (d2[i], prim[i]), prim >= 0 and distinct, in the order given through the list code the
 *   kernels run (csrc/tirt_nearest.h) with this k and lim2 (lim2 itself, not a distance: -1 finds nothing).  out_d2[j], out_prim[j] = element j, padded to
 *   k with (+inf, -1); out_info = {entries held, |N|, bits of the threshold's D2, the threshold's id (-1: the list has room)}. */
#define TIRT_NEAREST_MAX 64
int tirt_query_nearest(tirt_ctx *ctx, const float *points, int64_t n, int64_t point_stride,
                       const float *dmax, int64_t dmax_stride, float dmax_all, int k, int stack_size, int flags,
                       float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                       float *out_uv, int64_t uv_stride, int32_t *out_count, int32_t *counts, void *stream);
int tirt_nearest(tirt_ctx *ctx, const float *points, int n, const float *dmax, int k, int stack_size, int flags,
                 float *out_d2, int32_t *out_prim, float *out_point, float *out_uv, int32_t *out_count, int32_t *counts);
int tirt_kat_nearest_list(const float *d2, const int32_t *prim, int n, int k, float lim2,
                          float *out_d2, int32_t *out_prim, int32_t *out_info);

/* Triangle distance (no reference counterpart; csrc/tirt_triangle_query.hip / .h): the closest points between a query TRIANGLE T = (p0, p1, p2) and the
 * scene's triangles, and with a bound of 0 the contact test.  The distance between two triangles is attained vertex-to-face or edge-to-edge, and two
 * triangles that cross have an edge of one through the other: a query of T's vertices through "Closest point" sees the first case only.
 * Everything is fp32, every operation in the order written, no contraction; dot, cross and cp_triangle (= the triangle of "Closest point": D2, Q) as above.
 *   clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x)  (a NaN passes through).
 *   seg_seg(p1, q1, p2, q2) -> s, t, d2, P, Q  (Ericson 5.1.9 with exact zero tests in place of an epsilon):
 *     d1 = q1 - p1, d2v = q2 - p2, r = p1 - p2, A = dot(d1, d1), E = dot(d2v, d2v), F = dot(d2v, r);
 *     A <= 0 and E <= 0:  s = 0, t = 0
 *     else A <= 0:        s = 0, t = clamp(F / E)
 *     else C = dot(d1, r);
 *       E <= 0:           t = 0, s = clamp((-C) / A)
 *       else              B = dot(d1, d2v), den = A*E - B*B, s = den > 0 ? clamp((B*F - C*E) / den) : 0, t = (B*s + F) / E;
 *                         if t < 0: t = 0, s = clamp((-C) / A); else if t > 1: t = 1, s = clamp((B - C) / A)
 *     P = p1 + d1 * s, Q = p2 + d2v * t, d2 = dot(P - Q, P - Q).
 *   seg_tri(x0, x1, a, b, c) -> hit, u, v, t, X  (Moeller-Trumbore on the segment x0 -> x1):
 *     d = x1 - x0, E1 = b - a, E2 = c - a, h = cross(d, E2), det = dot(E1, h).  Unless det < 0 or det > 0: no hit, u = v = t = 0.  Otherwise
 *     inv = 1 / det, s = x0 - a, u = dot(s, h) * inv, q = cross(s, E1), v = dot(d, q) * inv, t = dot(E2, q) * inv,
 *     X = (a + E1 * u) + E2 * v, w = (x0 + d * t) - X, m2 = max(max(max(max(dot(x0, x0), dot(x1, x1)), dot(a, a)), dot(b, b)), dot(c, c)) with
 *     max(x, y) = x > y ? x : y;  hit iff u >= 0 and v >= 0 and u + v <= 1 and t >= 0 and t <= 1 and dot(w, w) <= m2 * 2^-38.
 *     The last condition confirms the hit by its two points: where the segment runs in the triangle's plane (an edge of a wall against a coplanar
 *     triangle) det is rounding noise and u, v, t fall in range by accident for triangles that are far apart; the segment's point and the triangle's
 *     point then disagree.  2^-19 of the largest vertex norm is about 55 roundings of a coordinate: a grazing crossing whose points disagree by more
 *     is no piercing by this arithmetic, and the other candidates give it its (tiny) distance.
 * The pair (T, scene triangle i = (a, b, c)) has 21 candidates (d2, P on T, Q on the scene triangle); the index is the `code`:
 *    0..2      vertex p_j against the scene triangle: r = cp_triangle(p_j, a, b, c); P = p_j, Q = r.Q, d2 = r.D2
 *    3..5      scene vertex s_j (a, b, c) against T: r = cp_triangle(s_j, p0, p1, p2); Q = s_j, P = r.Q, d2 = r.D2
 *    6+3e+f    edge e of T (p0p1, p1p2, p2p0) against edge f of the scene triangle (ab, bc, ca): seg_seg(edge e, edge f): its P, Q, d2
 *    15..17    edge e of T pierces the scene triangle: seg_tri(edge e, a, b, c); a candidate iff hit; d2 = 0, P = Q = X
 *    18..20    edge f of the scene triangle pierces T: seg_tri(edge f, p0, p1, p2); a candidate iff hit; d2 = 0, P = Q = X (formed on T)
 *   The pair's answer starts as (d2 = +inf, code = -1, P = Q = 0); going through the codes in order, a candidate replaces it iff its d2 < the answer's d2:
 *   the smallest d2, at equal bits the first in code order; a NaN d2 is never a candidate (and neither is +inf).  No d2 is -0, so once a d2 of 0 stands
 *   nothing replaces it and an implementation may skip the later candidates.  A degenerate T or scene triangle yields whatever these expressions yield.
 * The answer for T with bound dmax: lim2 = dmax * dmax formed once (dmax < 0 or NaN: -1; +inf: no bound) and the rule across primitives are those of
 *   "Closest point", unchanged, on D2(T, i) = the pair's d2: among the scene triangles with D2 <= lim2 the smallest D2, at equal bits the smallest
 *   primitive id; NaN and +inf are never accepted.  "Nothing" is prim = -1, d2 = +inf, code = -1, P = Q = 0.  A T with a NaN or infinite coordinate finds
 *   nothing, whatever its finite corners would yield (its lim2 is -1, as for a negative bound; it does not walk).  The minimum of a total order on (D2, prim): the culled walk returns the bits of the scan over all primitives (the
 *   culling argument is in the head of csrc/tirt_triangle_query.h).  dmax = 0 is the contact test: prim >= 0 iff some scene triangle touches or crosses T
 *   by this arithmetic.  Analytic spheres, spot and laser shapes take no part: they are reached and skipped.  Alpha cut-outs are ignored, as for the
 *   closest point.
 * tirt_query_mesh_distance: device memory on the caller's stream with tirt_query_closest_point's plumbing, flags (TIRT_TRAVERSE_EXHAUSTIVE = the scan over
 *   all primitive records in id order, the yardstick; TIRT_COUNT_NODES), stack (1..4096 entries of 8 bytes, the first 16 in LDS; a dropped entry is counted
 *   in stack_overflow), refusals and n == 0 behaviour: asynchronous, no host sync, one launch per chunk of "query_chunk_rays", 0 bytes of scratch per query.
 *   Row i of the triangles is 9 floats (p0, p1, p2) at tris + i * tri_stride floats (tri_stride >= 9); dmax[i * dmax_stride] per query, or dmax_all for
 *   every query when dmax is NULL.  Each output may be NULL: out_d2[n], out_prim[n], out_code[n], out_points + i * points_stride = P then Q (6 floats,
 *   points_stride >= 6), counts[n*2] = N_box, N_leaf per query (8-byte aligned; only with TIRT_COUNT_NODES).  The walk never culls on equality: with
 *   the answer at D2 = 0 every leaf whose box meets T's box is still tested, since a smaller id may tie -- a deep penetration costs that.
 *   Refused with TIRT_ERR_ARG before anything is queued: a pointer that is not device memory of ctx's device, tri_stride < 9, points_stride < 6 with
 *   out_points, dmax_stride < 1 with dmax, counts not 8-byte aligned, other flags, a stack_size outside 1..4096, an LBVH that is not built, a capturing stream.
 * tirt_mesh_distance: host arrays (tris[n*9], dmax[n] or NULL = +inf, out_points[n*6], counts[n*2]), staged in the context's staging buffer and
 *   synchronous, as tirt_closest_point is to tirt_query_closest_point.
 * tirt_kat_tri_tri: explicit operands through the same device functions, one row per thread: what = 0: rows of 18 floats (p0, p1, p2, a, b, c) to 8 floats
 *   (d2, P3, Q3, (float) code); what = 1: seg_seg rows of 12 floats (p1, q1, p2, q2) to (s, t, d2); what = 2: seg_tri rows of 15 floats (x0, x1, a, b, c)
 *   to (hit as 0 / 1, u, v, t).
 * tirt_kat_tri_tri_host: host only, no context: the same rows through the same text compiled for the host. */
int tirt_query_mesh_distance(tirt_ctx *ctx, const float *tris, int64_t n, int64_t tri_stride,
                             const float *dmax, int64_t dmax_stride, float dmax_all, int stack_size, int flags,
                             float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int64_t points_stride,
                             int32_t *counts, void *stream);
int tirt_mesh_distance(tirt_ctx *ctx, const float *tris, int n, const float *dmax, int stack_size, int flags,
                       float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int32_t *counts);
int tirt_kat_tri_tri(tirt_ctx *ctx, const float *in, int n, int what, float *out);
int tirt_kat_tri_tri_host(const float *in, int n, int what, float *out);

/* Point pairs (no reference counterpart; csrc/tirt_pairs.hip / .h): EVERY primitive within a distance of a query point -- the fixed-radius neighbour list
 * -- as the rows of a CSR layout.  "K nearest primitives" answers the first k <= 64 and how many; this says which, however many.
 * Terms.  D2(p, i), Q, u, v, lim2 = dmax * dmax formed once (dmax < 0 or NaN: -1; +inf: no bound) are those of "Closest point", unchanged.
 * The row of p is the set N(p) of "K nearest primitives", unchanged: { i : D2(p, i) <= lim2 and D2(p, i) < +inf }.  A NaN D2 is never a member.  A query
 *   with a NaN or infinite coordinate, or a negative or NaN bound, has the empty row.  Analytic spheres take part; spot and laser shapes have no surface and
 *   do not; alpha cut-outs are ignored.
 * Order inside a row.  D2 ascending; at equal D2 bits the smaller primitive id first: the total order of "K nearest primitives".  So element 0 of a row that
 *   is not empty is tirt_query_closest_point's answer bit for bit, the first min(k, length) elements are tirt_query_nearest's list bit for bit, and the row
 *   does not depend on the order of the visits (which follows the tree build's atomics and differs from one build to the next).
 * Layout.  row_start[n + 1] is int64: the exclusive prefix sums of the rows' lengths, row_start[n] the total.  Element j of row i is at row_start[i] + j
 *   of out_d2 and out_prim; out_point + (row_start[i] + j) * point_out_stride = Q and out_uv + (row_start[i] + j) * uv_stride = (u, v) of that pair, formed
 *   again from the record by the device function the walk ran: the bits tirt_query_closest_point gives for that pair.
 * mode.  TIRT_PAIRS_COUNT writes row_start and nothing else: the sizing call (capacity and the out arrays are not looked at).  TIRT_PAIRS_FILL reads a
 *   row_start that a COUNT call on the same queries, bounds and geometry produced, and writes the rows.  TIRT_PAIRS_BOTH counts, scans and fills in one call.
 * capacity (FILL, BOTH): the number of pairs the out arrays hold.  A row is written iff it fits entirely: 0 <= row_start[i] <= row_start[i + 1] <= capacity.
 *   A row that does not fit is neither walked a second time nor written, not even in part (a part's content would depend on the order of the walk); nothing
 *   at or behind the end of the last row that fits is touched.  row_start is complete whatever the capacity: row_start[n] > capacity says the result was cut.
 * flags.  TIRT_TRAVERSE_EXHAUSTIVE = every primitive record in id order through the same membership, store and order code (the yardstick: same bits, N_box 0,
 *   N_leaf = primitives); TIRT_COUNT_NODES as elsewhere (counts[n*2], from the counting walk, or the filling walk of a FILL call); TIRT_PAIRS_UNORDERED skips
 *   the order pass: the order inside a row is then unspecified (the walk's), the set is the same.
 * tirt_query_point_pairs: device memory on the caller's stream with tirt_query_closest_point's plumbing, stack and refusals, no host wait.  Per chunk of
 *   "query_chunk_rays" one launch of the counting walk (the row's length into row_start[i + 1]); three launches turn the lengths into row_start in place
 *   (block sums, one block over the block sums, add -- no kernel waits for another block; 8 bytes of scratch per 1024 queries); one launch per chunk of the
 *   filling walk (the same walk, the same cut: member number j of row i to row_start[i] + j, guarded by j < the row's length, so that a stack overflow never
 *   writes outside its row); one launch orders the rows in place, one wave per row (rows of up to 1024 pairs in LDS; longer rows by the same sorting network
 *   on the caller's arrays in global memory, which is correct for any length and not tuned); one launch forms the points.  A query whose walk dropped a stack
 *   entry is counted in stack_overflow once per walk.
 *   Refused with TIRT_ERR_ARG before anything is queued, beside tirt_query_closest_point's refusals: an unknown mode, a null row_start or one that is not
 *   8-byte aligned, and in FILL and BOTH: neither out_prim nor out_d2, a negative capacity, only one of out_d2 and out_prim without TIRT_PAIRS_UNORDERED
 *   (they are the key of the order), out_point or out_uv without out_prim.  (With capacity == 0 no row that has a pair fits: the out arrays are not looked
 *   at and may be NULL.)  n == 0 writes row_start[0] = 0 (COUNT, BOTH) and nothing else.
 * tirt_point_pairs: host arrays (points[n*3], dmax[n] or NULL = +inf, row_start[n + 1], out arrays of `capacity` pairs), staged and synchronous, as
 *   tirt_nearest is to tirt_query_nearest.  Only the rows that fit are copied back.
 * tirt_kat_pairs_host: host only, no context: n_rows rows of members (d2, prim) -- row i is the next row_len[i] entries, D2 >= 0 and finite, prim >= 0 and
 *   distinct inside a row -- in the order given, through the scan, the capacity rule and the sorting network the kernels run (csrc/tirt_pairs.h):
 *   row_start[n_rows + 1], and the rows that fit, ordered, at their offsets of out_d2 / out_prim; nothing else of those is written. */
#define TIRT_PAIRS_COUNT 0
#define TIRT_PAIRS_FILL 1
#define TIRT_PAIRS_BOTH 2
#define TIRT_PAIRS_UNORDERED 4      /* a flag beside TIRT_TRAVERSE_EXHAUSTIVE and TIRT_COUNT_NODES, of the pair lists alone */
int tirt_query_point_pairs(tirt_ctx *ctx, const float *points, int64_t n, int64_t point_stride,
                           const float *dmax, int64_t dmax_stride, float dmax_all, int mode, int64_t capacity, int stack_size, int flags,
                           int64_t *row_start, float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                           float *out_uv, int64_t uv_stride, int32_t *counts, void *stream);
int tirt_point_pairs(tirt_ctx *ctx, const float *points, int n, const float *dmax, int mode, int64_t capacity, int stack_size, int flags,
                     int64_t *row_start, float *out_d2, int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts);
int tirt_kat_pairs_host(const float *d2, const int32_t *prim, const int32_t *row_len, int n_rows, int64_t capacity,
                        int64_t *row_start, float *out_d2, int32_t *out_prim);

/* Triangle pairs (no reference counterpart; csrc/tirt_pairs.hip / .h): every scene triangle within a distance of a query TRIANGLE T -- with a bound of 0
 * the contact pair list of a mesh against the scene -- as the rows of the same CSR layout.
 * The row of T is the same set on D2(T, i) = the d2 of the pair's answer of "Triangle distance" over the scene's triangles, with that section's rules:
 *   { i : D2(T, i) <= lim2 and D2(T, i) < +inf }.  A T with a NaN or infinite coordinate has the empty row, and so has a negative or NaN bound.  Analytic
 *   spheres, spot and laser shapes are skipped; alpha cut-outs are ignored.  dmax = 0 gives every scene triangle that touches or crosses T by that arithmetic:
 *   the row is not empty exactly where the contact test of "Triangle distance" says prim >= 0.
 * Order, layout, mode, capacity, flags, launches and refusals are those of "Point pairs" (tri_stride >= 9 and points_stride >= 6 in the place of the point
 *   strides); element 0 of a row is tirt_query_mesh_distance's answer bit for bit.  out_code[row_start[i] + j] is the `code` of that pair's answer -- it
 *   travels with its pair through the order pass -- and out_points + (row_start[i] + j) * points_stride = P on T then Q on the scene triangle (6 floats),
 *   formed again by the pair's arithmetic after the order.
 * tirt_mesh_pairs: host arrays (tris[n*9], dmax[n] or NULL = +inf, out_points[capacity*6]), staged and synchronous. */
int tirt_query_mesh_pairs(tirt_ctx *ctx, const float *tris, int64_t n, int64_t tri_stride,
                          const float *dmax, int64_t dmax_stride, float dmax_all, int mode, int64_t capacity, int stack_size, int flags,
                          int64_t *row_start, float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int64_t points_stride,
                          int32_t *counts, void *stream);
int tirt_mesh_pairs(tirt_ctx *ctx, const float *tris, int n, const float *dmax, int mode, int64_t capacity, int stack_size, int flags,
                    int64_t *row_start, float *out_d2, int32_t *out_prim, int32_t *out_code, float *out_points, int32_t *counts);

/* Sphere sweep (no reference counterpart; csrc/tirt_sweep.hip / .h): the first contact of a sphere of radius r whose centre moves along c(t) = o + t d
 * with the scene -- continuous collision for a particle, a link sphere, a thick beam.  A ray on the centre line has no radius and passes between two
 * triangles the sphere would hit; stepping "Closest point" along the path tunnels through whatever is thinner than the step.
 * Everything is fp32, every operation in the order written, no contraction; dot, cross, cp_triangle (D2, Q, u, v of a triangle) and cp_sphere (of an
 * analytic sphere) are those of "Closest point", unchanged.  A comparison with a NaN is false.
 * Terms.  A query is (o, d, r, B): d is NOT normalised (d = p1 - p0 with B = 1: t is the time of impact within a step), B = tmax, +inf = no bound.
 *   c(t) = o + d * t.  Formed once per query, the way lim2 is: r2 = r * r, tol = r * 2^-16 + m, rh = r + tol, rhi2 = rh * rh, nn = dot(d, d).
 *   m is the query's length: with the scene's grid (cell[3], grid_min[3]; C = max(max(cell[0], cell[1]), cell[2]), iE = 1 / (C * 60000),
 *   rho_0 = max(max(|grid_min[0]|, |grid_min[1]|), |grid_min[2]|) * iE): rho_o = max(max(|o.x - grid_min[0]|, |o.y - grid_min[1]|), |o.z - grid_min[2]|) * iE,
 *   rho_q = rho_o + r * iE, m = (0.5 + 0.5 * (rho_q + rho_0)) * C -- the margin of the point walks for o with r / E added: half a cell near the scene,
 *   8e-6 of the extent, and a fixed share of |o| and of r beyond it.  Alpha cut-outs are ignored, as every distance query ignores them; spot and laser
 *   shapes have no surface.
 *   root(a, b, c, ok, sg): disc = b*b - a*c; where ok and a > 0 and disc >= 0: (-b + sg * sqrt(disc)) / a; else +inf.
 * Contact time of a triangle (a, b, c), T: first c0 = cp_triangle(o, a, b, c); code 0 (overlap at the start): c0.D2 <= r2 gives T = 0 with c0's Q, u, v.
 *   Otherwise, with ab = b - a, ac = c - a, bc = c - b, ca = a - c, ma = o - a, mb = o - b, mc = o - c, the candidates t1 .. t7 (+inf = none):
 *   code 1, face: n = cross(ab, ac), n2 = dot(n, n), s = dot(n, ma), nd = dot(n, d), sg = s < 0 ? -1 : 1, h = s * sg, v = nd * sg.  Where n2 > 0 (a zero-area
 *     triangle has no face candidate) and v < 0 (approaching): rl = r * sqrt(n2); where h >= rl (the centre starts at least r from the plane):
 *     t = (h - rl) / (-v), p = c(t), and t1 = t iff dot(cross(ab, p - a), n) >= 0 and dot(cross(bc, p - b), n) >= 0 and dot(cross(ca, p - c), n) >= 0
 *     (the touched point's foot lies in the triangle).
 *   codes 2, 3, 4, the edges (P, e) = (a, ab), (b, bc), (c, ca) with m = o - P (Ericson 5.3.7, the infinite cylinder about the edge's line):
 *     me = dot(m, e), de = dot(d, e), ee = dot(e, e), A = ee * nn - de * de, k = dot(m, m) - r2, C = ee * k - me * me, Bq = ee * dot(m, d) - de * me,
 *     t = root(A, Bq, C, true, -1), ax = me + t * de; the candidate is t iff t >= 0 and ax >= 0 and ax <= ee.  A ray parallel to the edge and an edge of
 *     length 0 have A = 0 and no candidate: the corners' spheres cover the ends.
 *   codes 5, 6, 7, the corners P = a, b, c with m = o - P: t = root(nn, dot(m, d), dot(m, m) - r2, true, -1); the candidate is t iff t >= 0.
 *   A candidate whose root is exactly 0 becomes 2^-126, the smallest positive normal number: T = 0 is kept for code 0, overlap by cp_triangle's own
 *   arithmetic -- exactly where tirt_query_nearest counts a primitive within r of o -- and a start that arithmetic puts an ulp outside r (a sphere resting
 *   on a floor) has its contact ahead by less than any step: never dropped, never 0.  A candidate outside 0 <= t <= B is none.  Verification: a candidate counts only if cp_triangle(c(t), a, b, c).D2 <= rhi2 -- k_trace's rule, "every
 *   accepted hit is re-checked": a root that is cancellation noise far from the triangle is rejected, the contact carries its own certificate (the centre
 *   is within r + tol of the primitive by the library's own distance function) and the verifying call's Q, u, v are the contact's attributes.  T is the
 *   smallest candidate that verifies, at equal bits the first in code order (candidates are verified smallest first; a failed one is struck out); none: T = +inf,
 *   code -1.  The candidates are the boundary pieces of the triangle's Minkowski sum with the ball: each lies inside the sum and the true first contact
 *   on one of them, so in exact arithmetic the smallest candidate in range is the first contact (Ericson 5.5.6's one-shot test is not exact and not used).
 *   d = 0: nn = 0, no candidate has a root or an approach; only code 0 can answer.
 * Analytic sphere (centre Cs, radius R), on cp_sphere's distance to the SURFACE: code 0: cp_sphere(o, Cs, R).D2 <= r2 gives T = 0.  Otherwise m = o - Cs,
 *   mm = dot(m, m), Ro = R + r, Ri = R - r, co = mm - Ro * Ro, ci = mm - Ri * Ri; outside = co > 0, inside = Ri > 0 and ci < 0;
 *   t = root(nn, dot(m, d), outside ? co : ci, outside or inside, outside ? -1 : +1): code 8 is the smaller root of radius R + r entered from outside,
 *   code 9 the larger root of radius R - r left from inside; a root of exactly 0 becomes 2^-126, as above.  It counts iff 0 <= t <= B, t < +inf and cp_sphere(c(t), Cs, R).D2 <= rhi2.
 * The answer: among the primitives with T <= B the smallest T, at equal bits the smallest primitive id -- "Closest point"'s rule on (T, prim): the minimum
 *   of a total order, independent of the order of the visits.  Nothing qualifies: t = +inf, prim = -1, code = -1, point, uv and normal 0 (the distance
 *   family's miss, not the ray family's 1e6).  A query with a NaN or infinite coordinate of o or d, with r < 0, NaN or infinite, or with B < 0 or NaN gets
 *   the miss without a look at any primitive.  r = 0 is allowed: the centre line against the surface BY THESE FORMULAS -- not tirt_query_closest's
 *   bits, which follow the reference's Moeller-Trumbore test.
 * Attributes: point = Q and (u, v) of the verifying call (code 0: of c0), in the hit record's convention; normal = w * (1 / sqrt(dot(w, w))) with
 *   w = c(T) - Q, and (0, 0, 0) where dot(w, w) is not positive.
 * blocked: 1 iff some primitive has T <= B.  That does not depend on the visiting order; asked for alone, the walk stops at the first accepted contact.
 * tirt_query_sweep: device memory on the caller's stream with tirt_query_closest_point's plumbing -- asynchronous, no host sync, one launch per chunk of
 *   "query_chunk_rays", 0 bytes of scratch per query.  Row i of the rays is (o3, d3) at rays + i * ray_stride floats (ray_stride >= 6);
 *   radius[i * radius_stride] per query, or radius_all for every query when radius is NULL; tmax likewise.  Each output may be NULL: out_t[n], out_prim[n],
 *   out_code[n], out_point + i * point_stride, out_uv + i * uv_stride, out_normal + i * normal_stride, out_blocked[n] (bytes), counts[n*2] = N_box, N_leaf
 *   per query (8-byte aligned; only with TIRT_COUNT_NODES).  flags: TIRT_TRAVERSE_EXHAUSTIVE = the scan over all primitive records in id order (the yardstick:
 *   same bits), TIRT_COUNT_NODES.  The walk grows every box of the 4-wide nodes by (r + tol) + m, enters it by slabs and never culls on equality (the
 *   argument is in the head of csrc/tirt_sweep.hip); with the answer at T = 0 every leaf whose grown box holds o is still tested, since a smaller id may
 *   tie.  stack_size 1..4096 entries of 8 bytes per query (the first 16 in LDS, the rest in the context's spill buffer); an entry that does not fit is
 *   dropped and the query counted in stack_overflow (tirt_stats: TIRT_ERR_STACK).  The queries are not rays: no ray counter moves.
 *   Refused with TIRT_ERR_ARG before anything is queued: a pointer that is not device memory of ctx's device, ray_stride < 6, radius_stride < 1 with
 *   radius, tmax_stride < 1 with tmax, point_stride < 3 with out_point, uv_stride < 2 with out_uv, normal_stride < 3 with out_normal, counts not 8-byte
 *   aligned, other flags, a stack_size outside 1..4096, an LBVH that is not built, a capturing stream.  n == 0 queues nothing.
 * tirt_sweep: host arrays (rays[n*6], radius[n] or NULL = radius_all, tmax[n] or NULL = +inf, out_point[n*3], out_uv[n*2], out_normal[n*3], out_blocked[n]),
 *   staged in the context's staging buffer and synchronous.
 * tirt_kat_sweep: explicit operands through the same device functions, one row per thread: rows of 18 floats (o3, d3, r, m, B, a3, b3, c3) or, with
 *   is_sphere, 13 floats (o3, d3, r, m, B, Cs3, R) -- m is given, not formed -- to rows of 8 floats (T, (float) code, Q3, u, v, the verifying call's D2);
 *   a miss is (+inf, -1, 0, 0, 0, 0, 0, 0).
 * tirt_kat_sweep_host: host only, no context: the same rows through the same text compiled for the host. */
int tirt_query_sweep(tirt_ctx *ctx, const float *rays, int64_t n, int64_t ray_stride, const float *radius, int64_t radius_stride, float radius_all,
                     const float *tmax, int64_t tmax_stride, float tmax_all, int stack_size, int flags,
                     float *out_t, int32_t *out_prim, int32_t *out_code, float *out_point, int64_t point_stride, float *out_uv, int64_t uv_stride,
                     float *out_normal, int64_t normal_stride, uint8_t *out_blocked, int32_t *counts, void *stream);
int tirt_sweep(tirt_ctx *ctx, const float *rays, int n, const float *radius, float radius_all, const float *tmax, int stack_size, int flags,
               float *out_t, int32_t *out_prim, int32_t *out_code, float *out_point, float *out_uv, float *out_normal, uint8_t *out_blocked,
               int32_t *counts);
int tirt_kat_sweep(tirt_ctx *ctx, const float *in, int n, int is_sphere, float *out);
int tirt_kat_sweep_host(const float *in, int n, int is_sphere, float *out);

/* Signed distance (no reference counterpart; csrc/tirt_signed_distance.hip, sd_sign in csrc/tirt_closest_point.h): the distance of "Closest point" with the
 * sign of the angle-weighted pseudo-normal of the closest FEATURE -- face, edge or vertex (Baerentzen & Aanaes, "Signed distance computation using the
 * angle weighted pseudonormal", 2005).  The face normal of the winning triangle alone is wrong at sharp and concave vertices and edges, where several
 * triangles tie.  All fp32, every operation in the order written, no contraction, dot as above, cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x); tm_sqrt / tm_atan2 are csrc/tirt_math.h's.
 * Feature of a closest point, from the (u, v) of "Closest point" alone -- the first line that holds:
 *     v == 0 and u == 0: A     v == 0 and u == 1: B     v == 0: AB     u == 0 and v == 1: C     u == 0: AC     u == 1.0f - v: BC     else: interior
 *   (the BC region forms u = 1 - w, v = w, so its test is exact; an interior result that rounding puts on an edge counts as that edge).
 * Per triangle t with corners a, b, c (the bits of its vertex rows): g = cross(b - a, c - a), l2 = dot(g, g); t is VALID iff 0 < l2 < +inf;
 *   n^ = g / tm_sqrt(l2) per component; the angle at a corner with leaving edges e1, e2 is alpha = tm_atan2(tm_sqrt(dot(x, x)), dot(e1, e2)), x = cross(e1, e2),
 *   with (e1, e2) = (b - a, c - a) at a, (c - b, a - b) at b, (a - c, b - c) at c.  I(x) = (int64) rintf(x * 1073741824.0f).
 * Vertex sum of a corner at position v: over all valid triangles t' of any primitive id (t included) with a corner at a position == v (three fp32 ==: -0
 *   equals +0, a NaN equals nothing), the 64-bit integer sums of I(alpha' * n^'.x), I(alpha' * n^'.y), I(alpha' * n^'.z), alpha' the angle at that corner.
 * Edge sum of an edge (v0, v1) of t: over all valid t' that SHARE it -- a corner of t' == v0 and the corner after or before it == v1 --, the sums of
 *   I(n^'.x), I(n^'.y), I(n^'.z).  Its class counts the sharing t' of another primitive id: 0 closed (one, running v1 -> v0), 1 boundary (none),
 *   2 non-manifold (two or more), 3 flipped (one, running v0 -> v1).  The edges of t are AB = (a, b), BC = (b, c), CA = (c, a).
 * The table: float4[7] per primitive id, rows interior, A, B, C, AB, AC, BC.  Row 0 .xyz = n^ (whatever the divisions yield for an invalid t), the others
 *   (float) of the three sums (round to nearest; not normalised, only the direction matters) with .w = 0.  Row 0 .w as an int: the classes of AB, BC, CA in bits
 *   0-1, 2-3, 4-5, bit 6 = t is invalid.  Spheres, spots and lasers: all zero.  Integer sums: the table does not depend on the order anything is visited in.
 * The answer: with D2, prim, Q, u, v of "Closest point", for a triangle s = dot(p - Q, N.xyz) with N the row of the feature, d = tm_sqrt(D2),
 *   sd = s < 0 ? -d : d (s == 0 and a NaN s: positive); for an analytic sphere sd = len < r ? -d : d with len as "Closest point" forms it; nothing found: +inf.
 *   Negative is inside for a closed, consistently oriented mesh (and for unions of disjoint ones), "behind the sheet" for an open one; solids that
 *   intersect are not resolved; alpha cut-outs are ignored as above.
 * The table is context state, built ON THE DEVICE by the first signed query after tirt_scene_upload, tirt_vertex_update[_device] or tirt_lbvh_build dropped it:
 *   one lane per triangle corner walks the quantised nodes to every triangle that touches the corner's position, on the context's stream, inside the
 *   query's own ordering: no host sync (allocating the table, on first use or for a larger scene, waits for the context's stream as growing any of its
 *   scratch buffers does).  Its stack is the query's stack_size (4-byte entries, the first 16 in LDS).  An entry that does not fit loses
 *   the table: every sd answered from it is NaN and the corners count in stack_overflow (tirt_stats: TIRT_ERR_STACK); the entries that wait for the
 *   device anyway -- tirt_signed_distance, _prepare, _table_download -- return TIRT_ERR_STACK themselves.  The next signed call with a larger stack_size
 *   builds it again.
 * tirt_query_signed_distance: tirt_query_closest_point with out_sd[n] (required; the other outputs stay optional); the same flags, chunks and refusals.
 * tirt_signed_distance: host arrays, synchronous, as tirt_closest_point (56 bytes of scratch per query).
 * tirt_signed_distance_prepare: builds the table now (with the largest stack, 4096, unless one stands), waits, and reports report[0..4] = triangle edges
 *   that are boundary, non-manifold, flipped; invalid triangles; primitives.  All four zero: every mesh of the scene is closed and consistently oriented.
 * tirt_signed_distance_table_download: the same, and the table as out[n * 28] floats.
 * tirt_kat_signed_distance: rows of 33 floats (p3, a3, b3, c3, N[7][3]) through cp_triangle and sd_sign to rows of 2 floats: sd, the feature's row index. */
int tirt_query_signed_distance(tirt_ctx *ctx, const float *points, int64_t n, int64_t point_stride,
                               const float *dmax, int64_t dmax_stride, float dmax_all, int stack_size, int flags,
                               float *out_d2, int32_t *out_prim, float *out_point, int64_t point_out_stride,
                               float *out_uv, int64_t uv_stride, int32_t *counts, void *stream, float *out_sd);
int tirt_signed_distance(tirt_ctx *ctx, const float *points, int n, const float *dmax, int stack_size, int flags,
                         float *out_d2, int32_t *out_prim, float *out_point, float *out_uv, int32_t *counts, float *out_sd);
int tirt_signed_distance_prepare(tirt_ctx *ctx, int64_t report[5]);
int tirt_signed_distance_table_download(tirt_ctx *ctx, float *out);
int tirt_kat_signed_distance(tirt_ctx *ctx, const float *in, int n, float *out);

/* Winding number (no reference counterpart; csrc/tirt_winding.hip, the terms in csrc/tirt_winding.h): the generalized winding number of Jacobson et al.
 * 2013, w(q) = (1 / 4 pi) sum_t Omega_t(q), evaluated with the far-field expansion of Barill et al. 2018 ("Fast winding numbers for soups and clouds",
 * orders 0 and 1) over the quantised 4-wide nodes.  0 or 1 for a closed mesh, smooth near holes, additive over overlapping shells; w > 0.5 is the inside
 * test that survives open, flipped and self-intersecting meshes, where the pseudo-normal sign of "Signed distance" flips behind every hole.
 * All fp32 unless stated, every operation in the order written, no contraction, dot and cross as above; tm_sqrt / tm_atan2 are csrc/tirt_math.h's.
 * Triangle term, for a query q and a triangle (A, B, C) that is VALID as above (g = cross(B - A, C - A), 0 < dot(g, g) < +inf): a = A - q, b = B - q,
 *   c = C - q; la = tm_sqrt(dot(a, a)), lb, lc alike; num = dot(a, cross(b, c));
 *   den = (((la * lb) * lc + dot(a, b) * lc) + dot(a, c) * lb) + dot(b, c) * la;   Omega = 2.0f * tm_atan2(num, den)   (Van Oosterom & Strackee 1983).
 *   An invalid triangle: Omega = 0.  Positive where the normal g points away from q.  A query on the triangle's plane is not special-cased: num is 0 where
 *   the arithmetic makes it so (an axis-aligned face), den > 0 outside the triangle and < 0 inside it, tm_atan2(+-0, den < 0) = +pi (tirt_math.h does not
 *   distinguish signed zeros): 0 outside, +2 pi -- half a turn -- inside, on either orientation.  q at a corner: tm_atan2(0, 0) = 0.
 * Analytic sphere with centre Cs and radius R: pc = q - Cs, len = tm_sqrt(dot(pc, pc)); Omega = len < R ? 12.566370614359172f : 0.  Spots and lasers: 0.
 * Quantisation: I(x) = (int64) rintf(x * 1073741824.0f) if |x * 1073741824.0f| < 2^62, else 0 (a NaN or overflowed term counts as nothing; an exact term
 *   is at most 2 pi (1 + 2^-22), so 2^24 primitives sum to less than 2^24 * 2^33 = 2^57 < 2^63).  The terms of a query are added in 64-bit integers: the
 *   sum S does not depend on the order of the visits, nor on how the build's atomics numbered the nodes.
 * The answer: w = ((float) S * 9.313225746154785e-10f) * 0.07957747154594767f (round to nearest: 2^-30, then 1 / 4 pi).  A query with a NaN or infinite
 *   coordinate answers NaN and adds nothing.  Alpha cut-outs are ignored as above.
 * The moment table: one row of 16 floats per (4-wide node, child slot) whose code names an inner node (index 4 * node + slot; all other rows are zero), over
 *   the valid triangles beneath that child.  ext = max_k(cell[k]) * 60000.0f = m 2^e with 0.5 <= m < 1 (e = the exponent field of ext - 126);
 *   s2 = 2^(37 - 2 e), s3 = 2^(37 - 3 e).  A position relative to grid_min is below 2^(e - 1) in magnitude and |g| / 2 below 1.5 * 2^(2 e), so every scaled
 *   term below is under 1.5 * 2^37 and 2^24 of them under 2^62.  Per triangle: h = 0.5f * g per component; ar = 0.5f * tm_sqrt(dot(g, g));
 *   cen = (((A - grid_min) + (B - grid_min)) + (C - grid_min)) * 0.3333333432674408f per component; J(x, s) = (int64) rint((double) x * s) in float64 (0 if the
 *   product is NaN or reaches 2^62).  The sixteen 64-bit sums: J(h.x, s2), J(h.y, s2), J(h.z, s2); J(ar, s2); J(ar * cen.k, s3), k = x, y, z;
 *   J(cen.i * h.j, s3), row-major in (i, j).  Integer sums over a set: the table is a function of the tree's structure alone.
 *   The row, in float64 with + - * / only and one rounding to fp32 per word: area = (double) S3 / s2 (as a product with 2^(2 e - 37)), N_j = S_j / s2,
 *   M_ij = S_(7 + 3 i + j) / s3; if S3 > 0: p_k = (S_(4 + k) / s3) / area and p~_k = (float)(p_k + (double) grid_min[k]), else p_k = 0 and
 *   p~_k = 0.5f * (mn_k + mx_k) of the slot's decoded box (mn_k = grid_min[k] + (float) h_lo * cell[k], mx_k alike from the slot's two fp16 planes: the decode
 *   of the closest-point walk); C_ij = (float)(M_ij - p_i * N_j).  r2 in fp32: f_k = max(|p~_k - mn_k|, |mx_k - p~_k|), r2 = (f_x * f_x + f_y * f_y) + f_z * f_z:
 *   the squared distance from p~ to the farthest corner of the decoded box.  Row words: p~ (3), r2, N (3), C (9, row-major).
 * The walk starts at the root (a one-primitive scene: at its leaf).  Per child slot of a node: empty -- skipped; a leaf -- its primitive's term, always;
 *   an inner child with row (p~, r2, N, C): d = p~ - q per component, d2 = dot(d, d); iff d2 > (beta * beta) * r2 as computed numbers it is APPROXIMATED:
 *   s = tm_sqrt(d2), d3 = d2 * s, t0 = dot(N, d) / d3, tr = (C00 + C11) + C22, cd_i = dot(row i of C, d), t1 = tr / d3 - (3.0f * dot(d, cd)) / (d2 * d3),
 *   and I(t0) + I(t1) is added; else it is descended.  beta >= 1, or +inf (the comparison is then never true: the exact sum); anything else is
 *   TIRT_ERR_ARG.  An analytic sphere beneath an approximated child adds nothing, rightly: q is outside the ball about p~ that holds the child's box.
 *   Nothing is sorted or culled.  Stack: 4-byte entries, the first 16 in LDS; an entry beyond stack_size loses a subtree: that query answers NaN and
 *   counts in stack_overflow (tirt_stats: TIRT_ERR_STACK).  TIRT_TRAVERSE_EXHAUSTIVE: every primitive in id order, no table use (beta is checked, not used).
 *   TIRT_COUNT_NODES: counts[2 q] = child slots examined (4 per node visited), counts[2 q + 1] = leaves evaluated (the scan: 0 and n).
 * The table is context state, built ON THE DEVICE by the first winding call after tirt_scene_upload, tirt_vertex_update[_device] or tirt_lbvh_build dropped
 *   it: bottom-up, one launch per level of the 4-wide tree, then one launch for the rows; on the context's stream, inside the query's own ordering, no
 *   host sync (allocating it, on first use or for a larger scene, waits for the context's stream as growing any scratch buffer does).
 * tirt_query_winding_number: points (row q at points + q * point_stride, point_stride >= 3) and out_w[n] in device memory, optional counts[2 n] (8-byte
 *   aligned), the caller's stream; chunks, flags and refusals as tirt_query_closest_point.  n == 0 queues nothing.
 * tirt_winding_number: host arrays (points[n * 3], out_w[n], counts or NULL), staged and synchronous.
 * tirt_winding_prepare: builds the table now unless it stands, and waits.
 * tirt_winding_table_download: the same, then table[wide_nodes * 64] floats and sums[wide_nodes * 16] (the sums of everything beneath each NODE) where not
 *   NULL, and info[0] = wide_nodes, info[1] = e.
 * tirt_kat_winding: rows of 12 floats (q3, A3, B3, C3) or, with is_sphere, 7 (q3, Cs3, R) through the same device functions to rows of four 32-bit words:
 *   the bits of Omega, the bits of the w of that term alone, I(Omega) low word, high word.
 * tirt_kat_winding_host: host only, no context: the same rows through the same text compiled for the host. */
int tirt_query_winding_number(tirt_ctx *ctx, const float *points, int64_t n, int64_t point_stride, float beta, int stack_size, int flags,
                              float *out_w, int32_t *counts, void *stream);
int tirt_winding_number(tirt_ctx *ctx, const float *points, int n, float beta, int stack_size, int flags, float *out_w, int32_t *counts);
int tirt_winding_prepare(tirt_ctx *ctx);
int tirt_winding_table_download(tirt_ctx *ctx, float *table, int64_t *sums, int32_t info[2]);
int tirt_kat_winding(tirt_ctx *ctx, const float *in, int n, int is_sphere, uint32_t *out);
int tirt_kat_winding_host(const float *in, int n, int is_sphere, uint32_t *out);

/* Multi-GPU without a Python framework in the loop (the reference has nothing here): ONE host thread drives
 * ndev contexts, one per device of the node, each created with tirt_film_create(..., tile_rank = i, tile_count = ndev, ...).
 * tirt_comm_init builds one RCCL communicator over them (librccl is loaded on first use); tirt_film_reduce sums the films
 * -- zero outside a context's own tiles -- onto ctxs[root] with one ncclReduce per device in a group (xGMI), and returns
 * when every stream has finished.  bench.py's one-process-per-GPU runs use tirt_film_export_device / import_device around
 * torch.distributed's RCCL reduce instead. */
int tirt_comm_init(tirt_ctx **ctxs, int ndev);
int tirt_film_reduce(tirt_ctx **ctxs, int ndev, int root);
int tirt_comm_destroy(tirt_ctx **ctxs, int ndev);

/* Measurement helpers for bench.py's roofline object (no counterpart in the reference).
 * tirt_bvh_info: bytes of the traversal data the ordered traversal walks (out[0] = quantised 4-wide nodes,
 *   out[1] = primitive records, out[2] = node count, out[3] = of those kept in LDS by every block; the chain nodes of far-origin
 *   rays, tirt_wide_tree_download, are counted: they are walked and kept in LDS like the others).
 * tirt_micro_gather_rate: the ceiling of the access pattern k_trace is bound by, measured on this device now --
 *   every lane of 1536 x 256 threads gathers `iters` random 64-byte records (4 x 16-byte loads) from an array of
 *   `working_set_bytes`; returns the rate in GB/s (best of 3 launches). */
int tirt_bvh_info(tirt_ctx *ctx, uint64_t out[4]);
int tirt_micro_gather_rate(tirt_ctx *ctx, uint64_t working_set_bytes, int iters, double *gbps_out);

/* Diagnostics of the traversal kernel's schedule.  tirt_set_option(ctx, "trace_timeline", k) arms the k-th counting launch (TIRT_COUNT_NODES)
 * from then on (-1 disarms); that launch records, per wave, four 64-bit words: start, the moment the wave found the ray queue empty (0: never),
 * end -- all in ticks of the device's 100 MHz wall clock -- and the wave's hardware id (HW_ID in the low word, XCC_ID in the high word).
 * tirt_trace_timeline copies up to max_waves records to `out` and reports how many the launch had.  (No reference counterpart: bench / tools.) */
int tirt_trace_timeline(tirt_ctx *ctx, uint64_t *out, int max_waves, int *n_waves);

/* Diagnostics of the camera rays' candidate lists (option "primary_beams", csrc/tirt_pvb.hip): out[0] = local pixels that have a list, out[1] = leaves on
 * all lists, out[2] = pixels whose five probe rays all hit, out[3] = camera rays since the lists were made that found no hit on their pixel's list and were
 * traced by k_trace, out[4] = camera rays that went through the lists; since the last tirt_stats_reset: out[5] = list builds (one per change of build /
 * camera / film seen by a batch that uses lists, or after option "primary_beams_rebuild"), out[6] = their device time in nanoseconds (HIP events on the
 * context's stream: probe rays + the walk of the pixels' pyramids), out[7] = builds given up for lack of memory (the camera rays then take the ordinary
 * launch); with option "primary_beams_diag" (slow: an atomic per wave) the list pass counts since the lists were made out[8] = leaf steps of all camera rays,
 * out[9] = rays that took more than one, out[10] = lane slots of the waves' trips (64 x the leaf steps of each wave's slowest ray), out[11] = rays that took more
 * than two.  Waits for pending work.  (No reference counterpart: bench / tests.) */
int tirt_primary_beam_stats(tirt_ctx *ctx, uint64_t out[12]);
/* The candidate lists themselves, for the tests that hold them to their definition (the header of csrc/tirt_pvb.hip; tests/beam_lists_expected.py).  Diagnostic,
 * no reference counterpart.
 * tirt_primary_beam_lists_download makes the lists of the current (build, camera, film) exactly as a batch that uses them would (pvb_prepare: nothing happens when
 *   they stand already), waits for the stream and copies out the set batches read, in LOCAL pixel order (the order of the context's tiles):
 *     count[P]               leaves on the pixel's list, -1: the pixel has no list (its camera rays are k_trace's)
 *     cand[PVB_CMAX][P][2]   entry a of pixel k at (a * P + k) * 2: the leaf's child code as the 4-wide nodes hold it (tirt_wide_tree_download) and the bits of
 *                            `nr`, the least distance at which a ray of the pixel can reach the leaf; entries a >= count[k] are not defined
 *     bound[P]               up to this distance the list is complete; 1e6 (the distance of a miss) for a list made without a bound
 *   count, cand and bound are given together or all NULL; with NULL arrays only info is filled: info[0] = P (the context's local pixels), info[1] = PVB_CMAX,
 *   info[2] = 1 if the context has lists that batches would use and at least one pixel has one, else 0 -- option "primary_beams" off, a scene with cut-outs, an empty
 *   film and no list memory all give 0 and count[k] = -1 for every k (cand and bound are then not written); a camera further than 8 extents from the scene gives 0
 *   with the arrays of the lists it was refused --, info[3] = pixels that have a list.  If the call has to make the lists it COUNTS AS A LIST BUILD in
 *   tirt_primary_beam_stats (out[5], out[6]), and it resets the counters out[0..4] as every build does.  Waits for pending work.
 *   TIRT_ERR_ARG, and nothing is changed or written: null ctx or info, only some of the three arrays, no scene / LBVH not built, camera not set, film not created.
 * tirt_kat_primary_list_walk: known-answer entry for the walk of one camera ray over its pixel's list.  Row r: the ray of local pixel local_pixel[r] with jitter
 *   (jx[r], jy[r]) is formed as a batch forms it (camera_ray_direction) and handed to pvb_walk_list -- the function the list pass and PT_RGB's fused first step call
 *   -- on the context's current lists (made first if they do not stand, as above).  One launch of 64-thread blocks, row r on lane r % 64 of block r / 64, so the
 *   caller's order decides which rays share a wave; the padding lanes of the last block make the call as the padding threads of a batch do.
 *   out, 9 words per row: direction (3), resolved (1.0f: the hit is k_trace's; 0.0f: the ray would be handed to k_trace), t, u, v, the primitive as its bits (-1: none),
 *   and the ray's leaf steps as a float.  A row that is not resolved still reports the best hit of the entries it walked.
 *   TIRT_ERR_ARG as above, and: out_stride < 9, a local pixel outside [0, P), a context without lists (info[2] = 0 for any reason but the far camera).
 * tirt_kat_beam_triangle_host: host only, no context: the triangle-against-pyramid test of the list build (pvb_beam_triangle_off, csrc/tirt_pvb.h, the text k_pvb_beam
 *   calls, compiled for the host).  Row r of `in`, 31 floats: the eye (3), the cell sizes of the tree's grid (3), the four corner directions of the pixel's pyramid
 *   in the order (-, -), (+, -), (+, +), (-, +) of the film's two axes (12), the rounding bounds eps of its four face planes (4), the triangle's corners (9), all
 *   in world units; the entry forms the grid units and the face normals as k_pvb_beam does.  out[r] = 1: off, the leaf would not be listed; 0: listed.
 *   edges = 0: the four faces alone; 1: and the triangle's edge planes.  TIRT_ERR_ARG: a null pointer, n < 0, edges not 0 or 1. */
int tirt_kat_beam_triangle_host(const float *in, int n, int edges, int32_t *out);
int tirt_primary_beam_lists_download(tirt_ctx *ctx, int32_t *count, int32_t *cand, float *bound, int32_t info[4]);
int tirt_kat_primary_list_walk(tirt_ctx *ctx, int n, const int32_t *local_pixel, const float *jx, const float *jy, float *out, int out_stride);

/* Fills *out.  Returns TIRT_ERR_STACK (with *out filled in) when stack_overflow > 0: rays dropped subtrees, what was
 * rendered since the last tirt_stats_reset is wrong -- the reference prints "overflow, need larger stack" (Scene.py:741). */
int tirt_stats(tirt_ctx *ctx, tirt_stats_t *out);
int tirt_stats_reset(tirt_ctx *ctx);

/* The known-answer entries tirt_kat_* (these and the ones further up; csrc/tirt_kat.hip): row i of `in` is evaluated on thread i of one launch into row i of `out`.
 * In every one of them the words of an output row beyond those the entry writes (an out_stride larger than it needs) are zero, and n == 0 returns TIRT_OK
 * without touching the device or `out`.
 * Device-side evaluation of the shared scalar functions:
 * fn 0 sin 1 cos 2 exp 3 log 4 pow(x,y) 5 atan2(x,y) 6 acos 7 sqrt 8 x/y */
int tirt_kat_math(tirt_ctx *ctx, int fn, const float *x, const float *y, float *out, int n);
/* which 0 Disney.evaluate_pdf  in: mat10,N3,V3,L3        out: f, pdf
 *       1 Disney.sample        in: mat10,dir3,N3,rnd3    out: dir3
 *       2 Glass.sample         in: mat10,dir3,N3,prob    out: dir3, f_or_b
 *       3 UF.offset_ray        in: p3,n3                 out: p3
 *       4 UF.CosineSampleHemisphere in: u1,u2  out: dir3     5 UF.mapToDisk in: u1,u2 out: r,phi      6 UF.powerHeuristic in: a,b out: w
 *       7 UF.inverse_transform in: dir3,N3 out: dir3         8 UF.srgb_to_lrgb / 9 UF.lrgb_to_srgb / 10 UF.tone_ACES in: c3 out: c3
 *       11 UF.refract in: I3,N3,eta out: R3,suc              12 UF.schlick in: cos,ior    13 UF.GTR2 in: NDotH,a    14 UF.smithG_GGX in: NDotv,alphaG
 *       15 UF.SchlickFresnel in: u                           16 Glass.sample_lambda in: dir3,N3,lambda,prob out: dir3,f_or_b
 *       17 Camera.get_ray_direction in: view_inv16,fx,fy,cx,cy,i,j,jx,jy out: dir3
 *       18 UF.slabs in: o3,d3,min3,max3 out: hit (0/1), hit by the branch-free form of the traversal kernel
 *       (4..18: the helpers behind 0..3 one by one, for tests/test_gpu_kat.py against tests/golden/refkat.npz -- values computed by the
 *       reference's own source text)
 * in: [n*in_stride] out: [n*out_stride] */
int tirt_kat_brdf(tirt_ctx *ctx, int which, const float *in, int in_stride, float *out, int out_stride, int n);
/* The spectral device functions one by one, on the tables of tirt_spectral_upload (tests/test_gpu_spectral.py against tests/golden/refkat_spec.npz --
 * values computed by the reference's own spectrum modules, sky/Sky.py and integrator/PT_Spec.py text).  which:
 *   0 Spectrum.sample (Spectrum.py:44-52) in: k (0 d65 1 white 2 red 3 green), Lambda out: 1      1 HeroSample.sample (:10-16) in: k, Lambda0 out: 4
 *   2 HeroSample.sample_xyz (:18-29) of PathTrace.sample (PT_Spec.py:131-139) in: Lambda0 out: x4,y4,z4
 *   3 Rgb2Spec.fetch (Rgb2Spec.py:101-137) in: rgb3 out: coff3     4 Rgb2Spec.eval (:139-143) in: coff3, Lambda out: 1
 *   5 HeroSample.srgb_to_spec (:46-58) in: srgb3, Lambda0 out: 4    6 HeroSample.sky_sample (:60-71; Sky.get_solar_radiance, sky/Sky.py:232-264) in: theta, gamma, Lambda0 out: 4
 *   7 PathTrace.emission_to_rad (PT_Spec.py:102-109) in: emission3, Lambda out: 4     8 HeroSample.get_extinction_hero (:37-43) in: Lambda0, t out: 4
 *   9 PathTrace.AddSplat (PT_Spec.py:141-158) in: spec4, Lambda0, coff, hdr3 out: hdr3      10 PathTrace.get_spec_power (:111-127) in: mat10, Lambda out: 4
 *  11 HeroSample.get_rnd_hero (:31-35) in: ti.random(), Lambda0 out: index, Lambda */
int tirt_kat_spec(tirt_ctx *ctx, int which, const float *in, int in_stride, float *out, int out_stride, int n);

/* The tables k_shade reads instead of recomputing what depends on a primitive or a light alone (tests/test_gpu_shade_tables.py).  They are built on
 * the device after a scene upload, a material upload or tirt_process_normal, by the first call that needs them.
 * tirt_shade_table_download: which 0 the shading records, 32 floats (128 bytes) per primitive -- triangles (v1, bits mat) (v2, bits 1) (v3, -) (n1, -) (n2, -)
 *   (n3, -) (gnor, area) -, and while the feature word has bit 128 (a textured scene) the vertex uvs in three of the free places: (v3, t3.u) (n1, t3.v) and the
 *   last quad (t1.u, t1.v, t2.u, t2.v); shapes (centre, bits mat) (radius, type, area, bits 2) --, which 1 the light records, 32 floats per entry of the light list --
 *   triangles (v1, area) (v3 - v1, choice pdf) (v2 - v1, bits -1) (n1, emission.r) (n2, .g) (n3, .b); shapes (centre, area) (shape[4], shape[5], -, choice pdf)
 *   (-, -, -, bits type) (shape[7..9], emission.r) (-, .g) (-, .b).  floats: the size of out, which must be the table's.
 * tirt_kat_shade_tables: the un-hoisted device functions.  which 0, n = primitives: out 4 per primitive, gnor3 (zero for shapes), Scene.get_prim_area;
 *   which 1, n = light_count: out 5 per light, area, light_choice_pdf of Scene.sample_li, emission3;  which 2: in 6 per sample (random number of the light
 *   choice, a, b, shaded point3), out 2 x 12: (light_pos3, light_normal3, emission3 x visible, area, choice pdf, light_dist) by the un-hoisted functions,
 *   then from the light records. */
int tirt_shade_table_download(tirt_ctx *ctx, int which, float *out, uint64_t floats);
int tirt_kat_shade_tables(tirt_ctx *ctx, int which, const float *in, float *out, int n);

/* One shading step of PT_RGB (integrator/PT_RGB.py:66-132 between a closest hit and the next: emission with MIS, glass / Disney, the NEE set-up, the next ray, the
 * miss) by the body of one instantiation of k_shade, on the context's own tables (shading and light records, material colours, environment) -- for
 * tests/test_gpu_shade_step.py against the CPU oracle's orc_kat_shade_step.  One launch, row i on thread i.
 * feat: the feature word of the instantiation, one of the 19 that tirt_shade_instantiation can return (its table, above) -- 32 (sphere lights), 4 (mesh lights), 127 (generic),
 *   255 (generic + albedo textures), 511 (+ roughness, metallic and normal maps), and 127 and 511 with each combination of bits 1024, 2048 and 4096.
 *   Bit 1024 needs the context's environment table and bit 4096 its emitters' table (those bits of tirt_shade_features); feat carries bit 2048 exactly when
 *   tirt_shade_features does (TIRT_ERR_ARG otherwise).
 * in, 23 words per row (integers as their bit patterns): seed, pixel, frame, bounce, last_bounce; origin3, direction3; t, u, v, prim (t >= 1e6: a miss, prim unused);
 *   throughout3, radiance3, brdf_pdf, perfect_spec.  NaN and infinity in the ray, the barycentrics and the state are data.
 * out, 28 words per row: radiance3, shaded, want_next, next_o3, next_d3, next_thr3, next_pdf, next_spec, want_shadow, sh_o3, sh_d3, sh_c3, sh_expect, sh_dist -- what
 *   k_shade writes to the path state and the shadow-ray queue; a field the step does not set is 0, sh_expect -2.  sh_c counts if the shadow ray finds sh_expect first.
 * TIRT_ERR_ARG before anything is launched: in_stride < 23, out_stride < 28, a feat that is not one of those listed (both also with a NULL ctx), a feat that does not
 * cover the context's feature word, feat 255 or 511 on a context without uploaded textures, a hit row (t < 1e6) whose prim is outside [0, n_prims), a pixel outside [0, 2^31 - 1). */
int tirt_kat_shade_step(tirt_ctx *ctx, uint32_t feat, const float *in, int in_stride, float *out, int out_stride, int n);

/* One shading step of PT_Spec (integrator/PT_Spec.py:207-274 between a closest hit and the next: the emitter hit, glass with its wavelength pick / Disney, the NEE
 * set-up with its four-channel contribution, the next ray, the analytic sky for a miss) by the body of one instantiation of k_shade_spec, on the context's own
 * tables and the spectral tables of tirt_spectral_upload -- for tests/test_gpu_shade_spec_step.py against the CPU oracle's orc_kat_shade_spec_step.  One launch,
 * row i on thread i.  The hero wavelength is the row's: 360 + 100 * rand(seed, pixel, frame).
 * feat: 32 (sphere lights), 4 (mesh lights) or 127 (generic): the three words tirt_shade_instantiation returns for a spectral render.
 * in, 23 words per row (integers as their bit patterns): words 0..14 as tirt_kat_shade_step's -- seed, pixel, frame, bounce, last_bounce; origin3, direction3; t, u,
 *   v, prim (t >= 1e6: a miss, prim unused) --, then throughout4 (15..18) and radiance4 (19..22).  NaN and infinity in the ray, the barycentrics and the state are data.
 * out, 29 words per row: radiance4 (0..3), shaded, want_next, next_o3 (6..8), next_d3 (9..11), next_thr4 (12..15), want_shadow (16), sh_o3, sh_d3, sh_c4 (23..26),
 *   sh_expect (27), sh_dist (28) -- what k_shade_spec writes to the path state and the shadow-ray queue; a field the step does not set is 0, sh_expect -2.  sh_c counts
 *   if the shadow ray finds sh_expect first.
 * TIRT_ERR_ARG before anything is launched: in_stride < 23, out_stride < 29, a feat that is not one of the three (both also with a NULL ctx), no scene, no spectral
 * tables, a feat that does not cover the context's feature word, a hit row (t < 1e6) whose prim is outside [0, n_prims), a pixel outside [0, 2^31 - 1). */
int tirt_kat_shade_spec_step(tirt_ctx *ctx, uint32_t feat, const float *in, int in_stride, float *out, int out_stride, int n);

/* ---- native Wavefront OBJ/MTL ingest (host only; no device, no context) -----------------------------
 * Replaces the reference's use of the third-party PyWavefront 1.3.3 package in Scene.add_obj
 * (Scene.py:66-127: `pywavefront.Wavefront(filename)`, `scene.materials[name].vertices / vertex_format /
 * diffuse / emissive / transparency / optical_density / shininess`): materials in first-appearance order,
 * ONE interleaved float list per material (fan-triangulated faces in file order), vertex format chosen
 * by the material's first face.
 *   params[19] = diffuse rgba, ambient rgba, specular rgba, emissive rgba, transparency, optical_density, shininess
 *   vertex_format: 4 "V3F", 5 "T2F_V3F", 6 "N3F_V3F", 7 "T2F_N3F_V3F", 0 when the material owns no face */
typedef struct tirt_obj tirt_obj;
int tirt_obj_load(const char *path, tirt_obj **out);
void tirt_obj_free(tirt_obj *obj);
int tirt_obj_material_count(const tirt_obj *obj);
int tirt_obj_material_info(const tirt_obj *obj, int index, char *name, int name_cap, double *params, int *vertex_format,
                           int *is_default, long long *n_floats);
int tirt_obj_material_vertices(const tirt_obj *obj, int index, double *out, long long n_floats);
/* the image of the material's map_Kd statement (options before the file name skipped), resolved against the directory of the MTL file, NUL-terminated
 * into path[cap]; the empty string when the material has none.  TIRT_ERR_ARG when cap is too small. */
int tirt_obj_material_texture(const tirt_obj *obj, int index, char *path, int cap);
/* the same for the material's map_Pr (kind 0: roughness), map_Pm (kind 1: metallic) and norm / map_Bump / bump statement (kind 2: a tangent-space normal map,
 * not a height field; -bm and the other options are skipped as map_Kd's are).  TIRT_ERR_ARG: a kind outside 0..2, cap too small. */
int tirt_obj_material_map(const tirt_obj *obj, int index, int kind, char *path, int cap);
/* the same for the material's map_d statement (an opacity mask: Scene.add_obj makes an alpha cut-out texture of it, see "Alpha cut-outs").  An entry of its
 * own: tirt_obj_material_map's kinds stay 0..2. */
int tirt_obj_material_opacity(const tirt_obj *obj, int index, char *path, int cap);

#ifdef __cplusplus
}
#endif
#endif /* TIRT_H */
