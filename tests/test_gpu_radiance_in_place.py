"""PT_RGB with the path's radiance accumulated in place (csrc/tirt_render.hip, k_shade): from bounce 0 on a path's radiance is fr / fg / fb[slot] -- the shading
kernel adds an emitter's or the environment's term there, k_trace's shadow write-back adds the light samples' -- and the path's perfect_spec flag rides in bit 31
of its stored slot word.  Every film here is held to the CPU oracle bit for bit, NaNs in the same places (tests/oracle_api.py), on the cases in which that
accumulator can go wrong: paths carried over many bounces with shadow contributions landing on paths that go on (sphere-light kernel), emitter hits with MIS at
a later bounce (mesh-light kernel), the flag carried across bounces and a lit environment (generic kernel), a ragged frame-major film rendered in two calls,
accumulators left behind by an earlier, larger film, a pixel set's batches (LIST kernels), and the sample moments, which read the same three arrays."""
import numpy as np
import pytest

import adaptive_expected as ax
import moments_expected as me
import oracle_api as oa
from common import same_bits
from test_gpu_aov import SEED, build, oracle_of
from ti_raytrace_amd import Camera, scenes
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu
DEPTH, STACK = 15, 64
# scenes.synthetic at 64 x 64 x 6 frames: of the (triangles, spread) pairs tried on the oracle -- (400, 0.2) 1.3 closest rays per path, (3000, 0.1) 1.6,
# (1000, 0.5) 1.96, (2000, 0.5) 2.05, (3000, 0.3) 2.17, (20000, 0.1) 2.7 -- the smallest scene above 2 (4 918 shadow rays for 24 576 paths)
NTRI, SPREAD, SW, SH, SFRAMES = 2000, 0.5, 64, 64, 6


def differing(got, want):
    return "pixels that differ: %d" % int((~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).any(axis=2).sum())


def lit(film):
    return (np.nan_to_num(film, nan=1.0) != 0).any(axis=2)


def plain_oracle(ex):
    o = oa.OracleScene(ex.scene, ex.cam)
    o.lbvh_build()
    return o


def rendered(ctx, W, H, frames, begin=0):
    ctx.pt_rgb_render(begin, frames, SEED, DEPTH, STACK, 0)
    return ctx.film_download(W, H)[0]


def same_counts(ctx, ost):
    st = ctx.stats()
    assert (st["rays_closest"], st["rays_shadow"], st["paths"], st["stack_overflow"]) == (ost["rays_closest"], ost["rays_shadow"], ost["paths"], 0), (st, ost)


@pytest.fixture(scope="module")
def soup(gpu_ctx_ok):
    """the scene of tests 1 and 6 on the device, its oracle film and the oracle's counts"""
    ex = scenes.synthetic(SW, SH, SFRAMES, ntri=NTRI, spread=SPREAD, device_id=0, seed=SEED)
    ex.build_scene()
    want, ost = plain_oracle(ex).render(SW, SH, 0, SFRAMES, seed=SEED)
    return ex, want, ost


# ---- 1. sphere-light instantiation, many bounces ----------------------------------------------------------------------------------------------------
def test_paths_carried_over_many_bounces_with_shadow_rays(soup):
    ex, want, ost = soup
    print("oracle: %.3f closest rays per path, %d shadow rays, %d paths, %d lit pixels" % (ost["rays_closest"] / ost["paths"], ost["rays_shadow"], ost["paths"], int(lit(want).sum())))
    assert ost["rays_closest"] > 2 * ost["paths"] and ost["rays_shadow"] > 0
    assert lit(want).sum() >= 64
    ctx = ex.scene.ctx
    ctx.film_clear(); ctx.stats_reset()
    got = rendered(ctx, SW, SH, SFRAMES)
    assert same_bits(got, want), differing(got, want)
    same_counts(ctx, ost)


# ---- 2. mesh-light instantiation: emitter hits with MIS at bounce >= 1 ------------------------------------------------------------------------------
def test_cornell_box_emitter_hits_after_the_first_bounce(gpu_ctx_ok):
    W, H, N = 64, 48, 8
    ex = build("cornell", W, H, N, aov=False)
    want, ost = oracle_of(ex, "cornell").render(W, H, 0, N, seed=SEED)
    assert ost["rays_closest"] > 2 * ost["paths"] and ost["rays_shadow"] > 0 and lit(want).mean() > 0.5
    ctx = ex.scene.ctx
    ctx.stats_reset()
    got = rendered(ctx, W, H, N)
    assert same_bits(got, want), differing(got, want)
    same_counts(ctx, ost)


# ---- 3. generic kernel: glass, a lit environment, the flag carried in the slot word ---------------------------------------------------------------
def test_teapot_glass_under_a_lit_environment(gpu_ctx_ok):
    W, H, N = 48, 40, 12
    ex = build("teapot", W, H, N, aov=False)
    want, ost = oracle_of(ex, "teapot").render(W, H, 0, N, seed=SEED)
    assert ex.scene.env_power > 0 and ost["rays_closest"] > 1.5 * ost["paths"] and lit(want).mean() > 0.9          # misses add a term that is not zero
    ctx = ex.scene.ctx
    ctx.stats_reset()
    got = rendered(ctx, W, H, N)
    assert same_bits(got, want), differing(got, want)
    same_counts(ctx, ost)


def glass_pane_box(W, H, device_id=None):
    """the Cornell box with a pane of glass (ior 1.5, 10 scene units thick) hung under its quad light and reaching towards the camera: a light sample taken from
    under the pane is stopped by it, so what lights the floor and the blocks came through the glass -- an emitter hit behind a glass vertex"""
    ex = scenes.cornell_box(W, H, 4, device_id=device_id, seed=SEED)
    m = SCD.Material()
    m.type = SCD.MAT_GLASS; m.setIor(1.5); m.setExtinciton(500.0); m.setColor([1.0, 1.0, 1.0, 1.0]); m.alebdoTex = -1
    ex.scene.add_mesh(scenes._box((150.0, 490.0, -400.0), (410.0, 500.0, -20.0)), m)
    return ex


def test_an_emitter_directly_behind_a_glass_vertex(gpu_ctx_ok):
    """camera, pane, pane, light and camera, surface, pane, pane, light: emitter hits at bounce >= 2 whose perfect_spec == 1 was set by a glass vertex and
    carried in the stored slot word from one launch to the next (with the flag lost they would be MIS-weighted against a light sample that was never taken)"""
    W, H, N = 64, 48, 8
    ex = glass_pane_box(W, H, device_id=0)
    ex.build_scene()
    o = plain_oracle(ex)
    want, ost = o.render(W, H, 0, N, seed=SEED)
    # the oracle alone: camera rays that meet the pane from below and, carried on in their own direction (a slab gives the direction back), meet the emitter
    rays = oa.camera_rays(ex.cam, W, H)
    rec, prim, _ = o.closest_hit(rays)
    mat = ex.scene.primitive_np[:, 2]
    on_glass = (prim >= 0) & (ex.scene.material_np[mat[np.maximum(prim, 0)], 0] == SCD.MAT_GLASS) & (rays[:, 4] > 0)
    d = rays[on_glass, 3:6]
    beyond = rays[on_glass, 0:3] + d * (rec[on_glass, 0:1] + 11.0 / d[:, 1:2])
    _, prim2, _ = o.closest_hit(np.concatenate([beyond, d], axis=1).astype(np.float32))
    to_light = (prim2 >= 0) & (ex.scene.material_np[mat[np.maximum(prim2, 0)], 0] == SCD.MAT_LIGHT)
    print("camera rays on the pane: %d, of them on towards the emitter: %d; lit pixels %d" % (int(on_glass.sum()), int(to_light.sum()), int(lit(want).sum())))
    assert to_light.sum() >= 16 and lit(want).mean() > 0.5
    ctx = ex.scene.ctx
    ctx.stats_reset()
    got = rendered(ctx, W, H, N)
    assert same_bits(got, want), differing(got, want)
    same_counts(ctx, ost)


# ---- 4. ragged, frame-major film in two calls ------------------------------------------------------------------------------------------------------
def test_ragged_frame_major_film_in_two_calls(gpu_ctx_ok):
    W, H = 50, 37                                                     # P = 1850: P % 64 = 58, so the paths are numbered frame-major (TileMap::F == 0)
    assert (W * H) % 64 != 0
    ex = build("cornell", W, H, 5, aov=False)
    want, ost = oracle_of(ex, "cornell").render(W, H, 0, 5, seed=SEED)
    ctx = ex.scene.ctx
    ctx.set_option("merge_paths", 0)                                  # every call its own batch
    ctx.stats_reset()
    rendered(ctx, W, H, 3)
    got = rendered(ctx, W, H, 2, begin=3)
    assert same_bits(got, want), differing(got, want)
    same_counts(ctx, ost)


# ---- 5. accumulators left behind by a larger film ---------------------------------------------------------------------------------------------------
def test_stale_accumulators_of_an_earlier_film(gpu_ctx_ok):
    def at(ex, o, W, H, frames):
        cam = Camera.Camera(W, H, frames)
        cam.scale = ex.cam.scale; cam.set_target(*ex.cam.target)
        ex.scene.ctx.film_create(W, H, 0, 1, 4096)
        cam.attach(ex.scene.ctx); o.set_camera(cam)
        return rendered(ex.scene.ctx, W, H, frames), o.render(W, H, 0, frames, seed=SEED)[0]

    used = build("cornell", 64, 64, 4, aov=False)
    o = oracle_of(used, "cornell")
    big, want_big = at(used, o, 64, 64, 4)
    assert same_bits(big, want_big), differing(big, want_big)
    small, want = at(used, o, 40, 24, 3)
    fresh = build("cornell", 64, 64, 4, aov=False)
    clean, _ = at(fresh, oracle_of(fresh, "cornell"), 40, 24, 3)
    assert lit(want).mean() > 0.5
    assert same_bits(small, clean, nan_payload=True), differing(small, clean)
    assert same_bits(small, want), differing(small, want)


# ---- 6. a pixel set's batches (LIST kernels) ---------------------------------------------------------------------------------------------------------
def test_a_pixel_sets_pass_over_part_of_the_first_scene(soup):
    ex, want, _ = soup
    ctx = ex.scene.ctx
    order = ax.local_order(SW, SH, 0, 1, ex.integrator.tile_size)
    # every third pixel of the first 1 900 and every lit one: 64 divides neither count, both kinds of pixel are in
    pick = np.zeros(SW * SH, bool)
    pick[order[5:1900:3]] = True
    pick |= lit(want).reshape(-1)
    pixels = order[pick[order]].astype(np.int32)
    inside = pick.reshape(SW, SH)
    assert len(pixels) % 64 != 0 and 0 < len(pixels) < SW * SH and (lit(want) & inside).sum() >= 64 and (~lit(want) & inside).sum() >= 64
    ctx.film_clear()
    ctx.pixel_set_upload(pixels)
    try:
        got = rendered(ctx, SW, SH, SFRAMES)
    finally:
        ctx.pixel_set_clear()
    assert same_bits(got[inside], want[inside]), "pixels of the set that differ: %d" % int((got[inside].view(np.uint32) != want[inside].view(np.uint32)).any(axis=1).sum())
    assert (got[~inside].view(np.uint32) == 0).all()


# ---- 7. the sample moments read the same arrays -----------------------------------------------------------------------------------------------------
def test_sample_moments_on_the_cornell_box(gpu_ctx_ok):
    W, H = 64, 48
    ex = build("cornell", W, H, 32, aov=False, moments=True)
    ctx, orc = ex.scene.ctx, oracle_of(ex, "cornell")
    xs = [me.oracle_sample(orc, W, H, fr, SEED) for fr in me.EXACT_FRAMES]          # the existing moments test's reference: Welford over the oracle's exact samples
    want_mom = me.expected(xs, W, H)
    want = np.zeros((W, H, 3), np.float32)
    for fr in me.EXACT_FRAMES:
        ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)
        orc.render(W, H, fr, 1, seed=SEED, hdr=want)
    got, mom = ctx.film_download(W, H)[0], ctx.moments_download(W, H)
    assert same_bits(got, want), differing(got, want)
    assert not np.isnan(mom).any() and (mom == want_mom).all(), "words that differ: %d" % int((mom != want_mom).sum())
    assert (mom[:, :, 0] == len(xs)).all()
    # one eight-frame batch: the film against the oracle, every sample counted
    ctx.film_clear()
    got = rendered(ctx, W, H, 8)
    want8, _ = orc.render(W, H, 0, 8, seed=SEED)
    assert same_bits(got, want8), differing(got, want8)
    assert (ctx.moments_download(W, H)[:, :, 0] == 8).all()
