"""PT_RGB's first step in one kernel (csrc/tirt_render.hip, k_pvb_cand_shade, option "primary_fused"): the camera ray's direction, the walk of its pixel's candidate
list and the first shading step without the direction and the hit record going through device memory.  The option only changes WHICH kernels do the work: every film
below must come out byte for byte the same, NaNs in place, with the same counters and the same list statistics, whether it is 1 or 0 -- and, where the suite has an
oracle scene, equal to the CPU oracle bit for bit.  Batches of 16 frames and more, so that the lists are used (option "primary_beams_min_frames")."""
import numpy as np
import pytest

import adaptive_expected as ax
import oracle_api as oa
from common import same_bits, tiny_scene
from test_gpu_aov import build, oracle_of
from ti_raytrace_amd import scenes

pytestmark = pytest.mark.gpu
SEED, DEPTH, STACK, FRAMES = 5, 15, 64, 16


def differing(got, want):
    return "pixels that differ: %d" % int((got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())


def run(ctx, W, H, fused, render=None, clear=True):
    """one job with the option set: (film, counters, camera rays through the lists, of them left to k_trace, shading launches)"""
    ctx.set_option("primary_fused", fused)
    if clear: ctx.film_clear()
    ctx.stats_reset()
    b0 = ctx.primary_beam_stats()
    (render or (lambda c: c.pt_rgb_render(0, FRAMES, SEED, DEPTH, STACK, 0)))(ctx)
    film = ctx.film_download(W, H)[0]
    st, b1 = ctx.stats(), ctx.primary_beam_stats()
    counts = (st["rays_closest"], st["rays_shadow"], st["paths"], st["shaded"], st["stack_overflow"])
    # (the list statistics count from the last list build: a build inside the job starts them at zero)
    built = b1["list_builds"] > 0
    rays = b1["rays"] - (0 if built else b0["rays"])
    left = b1["rays_to_k_trace"] - (0 if built else b0["rays_to_k_trace"])
    return film, counts, rays, left, st["launches_shade"]


def on_and_off(ctx, W, H, render=None, fused_taken=True, batches=1):
    """the job with the option on, then off, on one context; everything compared; returns the film and the statistics of the fused run"""
    on = run(ctx, W, H, 1, render)
    off = run(ctx, W, H, 0, render)
    assert same_bits(on[0], off[0], nan_payload=True), differing(on[0], off[0])
    assert on[1] == off[1] and on[1][4] == 0, (on[1], off[1])
    assert on[2:4] == off[2:4], (on[2:4], off[2:4])
    # the fused path shades bounce 0 in two launches (the rays of the lists, the rays k_trace was asked about) where the separate path has one
    assert on[4] - off[4] == (batches if fused_taken else 0), (on[4], off[4])
    return on


def synthetic(W, H, ntri=None):
    kw = {} if ntri is None else {"ntri": ntri}
    return scenes.synthetic(W, H, FRAMES, device_id=0, seed=SEED, **kw)


# ---- 1. against the separate launches and the oracle: mesh-light kernel (word 4), sphere-light kernel (word 32), the generic one -----------------------------
# 50 x 30: P = 1500 is no multiple of 64, the paths are numbered frame-major (TileMap::F == 0); 48 x 32: P = 24 x 64, pixel-block major, the wave's division by F
@pytest.mark.parametrize("size", [(50, 30), (48, 32)])
@pytest.mark.parametrize("name", ["cornell", "synthetic"])
def test_fused_film_equals_the_separate_launches_and_the_oracle(gpu_ctx_ok, name, size):
    W, H = size
    assert ((W * H) % 64 == 0) == (size == (48, 32))
    if name == "cornell":
        ex = build("cornell", W, H, FRAMES, aov=False)
        orc = oracle_of(ex, "cornell")
    else:
        ex = synthetic(W, H)
        ex.build_scene()
        orc = oa.OracleScene(ex.scene, ex.cam); orc.lbvh_build()
    film, counts, rays, left, _ = on_and_off(ex.scene.ctx, W, H)
    print(name, size, "rays", rays, "left to k_trace", left, counts)
    assert rays == FRAMES * W * H, "the camera rays did not go through the lists"
    want, ost = orc.render(W, H, 0, FRAMES, seed=SEED)
    assert same_bits(film, want), differing(film, want)
    assert counts[:3] == (ost["rays_closest"], ost["rays_shadow"], ost["paths"])


def test_teapot_glass_under_the_environment_map(gpu_ctx_ok):
    """the generic instantiation: glass at the first vertex, misses under a lit environment that read-modify-write the accumulator at later bounces, NaN pixels"""
    W, H = 48, 40
    ex = build("teapot", W, H, FRAMES, aov=False)
    assert ex.scene.env_power > 0
    film, counts, rays, left, _ = on_and_off(ex.scene.ctx, W, H)
    assert rays == FRAMES * W * H
    want, ost = oracle_of(ex, "teapot").render(W, H, 0, FRAMES, seed=SEED)
    print("teapot: NaN words %d, left to k_trace %d" % (int(np.isnan(want).sum()), left))
    assert same_bits(film, want), differing(film, want)
    assert counts[:3] == (ost["rays_closest"], ost["rays_shadow"], ost["paths"])


# ---- 2. both branches in one batch; no lists at all ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [DEPTH, 1])
def test_rays_of_the_lists_and_rays_left_to_k_trace_in_one_batch(gpu_ctx_ok, depth):
    """20 000 triangles behind 1 500 pixels: many pixels see more leaves than a list holds and keep a short one, or none -- their rays are k_trace's and are shaded
    by the second launch, behind the others in the same queues.  depth 1: bounce 0 is also the last, the leftover scratch (st[0], hit) is all there is"""
    W, H = 50, 30
    ex = synthetic(W, H, ntri=20000)
    ex.build_scene()
    film, counts, rays, left, _ = on_and_off(ex.scene.ctx, W, H, render=lambda c: c.pt_rgb_render(0, FRAMES, SEED, depth, STACK, 0))
    print("depth", depth, "rays", rays, "left to k_trace", left, counts)
    assert rays == FRAMES * W * H
    assert 0 < left < rays, "the test needs rays on both sides"
    assert np.nan_to_num(film, nan=1.0).any()


@pytest.mark.parametrize("depth", [DEPTH, 1])
def test_cornell_box_with_one_bounce_and_many(gpu_ctx_ok, depth):
    W, H = 50, 30
    ex = build("cornell", W, H, FRAMES, aov=False)
    film, counts, rays, left, _ = on_and_off(ex.scene.ctx, W, H, render=lambda c: c.pt_rgb_render(0, FRAMES, SEED, depth, STACK, 0))
    assert rays == FRAMES * W * H and counts[2] == rays
    if depth == 1: assert counts[0] == rays          # one closest-hit ray per path, nothing after it


def test_far_camera_every_ray_is_k_traces(gpu_ctx_ok):
    """further than eight scene extents away no pixel gets a list (tirt_pvb.hip): a camera ray that misses the root's box is a miss all the same and is shaded at
    once, every other one is left to k_trace and shaded by the second launch"""
    W = H = 64
    ex = tiny_scene(400, seed=3, W=W, H=H, spread=0.25, device_id=0)
    ex.build_scene()
    ex.frame_camera(40.0)
    ctx = ex.scene.ctx
    film, counts, rays, left, _ = on_and_off(ctx, W, H)
    assert ctx.primary_beam_stats()["pixels_with_list"] == 0
    assert rays == FRAMES * W * H and 0 < left < rays
    ctx.set_option("primary_beams", 0)               # and without the list pass at all: the ordinary launch, whatever the option says
    plain = run(ctx, W, H, 1)
    assert same_bits(plain[0], film, nan_payload=True) and plain[1] == counts and plain[2] == 0


# ---- 3. tiles, films of two sizes on one context, a camera move between two calls -----------------------------------------------------------------------------
def test_tiles_of_several_ranks(gpu_ctx_ok):
    W = H = 64
    for tile in (100, 512):                          # ragged tiles in linear order; whole 8-pixel columns in 8 x 8 blocks
        ex = synthetic(W, H, ntri=5000)
        ex.build_scene()
        ctx = ex.scene.ctx
        ctx.film_create(W, H, 1, 3, tile)
        film, counts, rays, left, _ = on_and_off(ctx, W, H)
        assert 0 < rays < FRAMES * W * H and counts[2] == rays, (tile, rays)


def test_a_large_film_before_a_small_one_on_the_same_context(gpu_ctx_ok):
    """the lane's buffers keep what the 96 x 64 job left in them: the 48 x 32 job must not read it (leftover list, hit records, accumulators)"""
    def small_after_big(fused, big_first):
        ex = synthetic(96, 64, ntri=20000)
        ex.build_scene()
        ctx = ex.scene.ctx
        ctx.set_option("primary_fused", fused)
        if big_first:
            ctx.pt_rgb_render(0, FRAMES, SEED, DEPTH, STACK, 0)
        ctx.film_create(48, 32, 0, 1, 4096)
        return run(ctx, 48, 32, fused)

    on, off, fresh = small_after_big(1, True), small_after_big(0, True), small_after_big(1, False)
    assert 0 < on[3] < on[2] == FRAMES * 48 * 32
    for other in (off, fresh):
        assert same_bits(on[0], other[0], nan_payload=True), differing(on[0], other[0])
        assert on[1:4] == other[1:4]


def test_two_calls_with_a_camera_move_between_them_and_no_sync(gpu_ctx_ok):
    W, H = 96, 64
    films = []
    for fused in (1, 0):
        ex = synthetic(W, H, ntri=20000)
        ex.build_scene()
        ctx = ex.scene.ctx
        ctx.set_option("primary_fused", fused)
        ctx.stats_reset()
        ctx.pt_rgb_render(0, FRAMES, SEED, DEPTH, STACK, 0)
        ex.cam.yaw += 0.15; ex.cam.update()          # submits what is pending and does not wait; new lists for the second call
        ctx.pt_rgb_render(FRAMES, FRAMES, SEED, DEPTH, STACK, 0)
        st = ctx.stats()
        films.append((ctx.film_download(W, H)[0], (st["rays_closest"], st["rays_shadow"], st["paths"], st["shaded"], st["stack_overflow"]), st["launches_shade"]))
    assert same_bits(films[0][0], films[1][0], nan_payload=True), differing(films[0][0], films[1][0])
    assert films[0][1] == films[1][1]
    assert films[0][2] - films[1][2] == 2            # both calls took the fused path


# ---- 4. what keeps the separate launches: feature buffers, a pixel set, PT_Spec; the sample moments read the accumulators -------------------------------------
def test_feature_buffers_keep_the_separate_launches(gpu_ctx_ok):
    W, H = 50, 30
    ex = build("cornell", W, H, FRAMES, aov=True)
    ctx = ex.scene.ctx
    ctx.aov_enable(True)
    recs = []
    for fused in (1, 0):
        res = run(ctx, W, H, fused)                  # (film_clear zeroes the records too)
        recs.append((res, ctx.aov_download(W, H)))
    assert recs[0][0][4] == recs[1][0][4], "feature buffers read the camera rays' hit records: the fused path must not be taken"
    assert same_bits(recs[0][0][0], recs[1][0][0], nan_payload=True) and recs[0][0][1:4] == recs[1][0][1:4]
    assert same_bits(recs[0][1], recs[1][1], nan_payload=True)
    ctx.aov_enable(False)                            # and the film is the film of the fused path without them
    plain = on_and_off(ctx, W, H)
    assert same_bits(plain[0], recs[0][0][0], nan_payload=True)


def test_a_pixel_set_keeps_the_separate_launches(gpu_ctx_ok):
    W = H = 64
    ex = synthetic(W, H, ntri=2000)
    ex.build_scene()
    ctx = ex.scene.ctx
    order = ax.local_order(W, H, 0, 1, ex.integrator.tile_size)
    pixels = order[5:1900:3].astype(np.int32)
    ctx.pixel_set_upload(pixels)
    try:
        on_and_off(ctx, W, H, fused_taken=False)
    finally:
        ctx.pixel_set_clear()


def test_pt_spec_keeps_the_separate_launches(gpu_ctx_ok):
    W = H = 48
    ex = scenes.spectral_box(W, H, FRAMES, device_id=0)
    ex.build_scene()
    on = on_and_off(ex.scene.ctx, W, H, render=lambda c: c.pt_spec_render(0, FRAMES, 3, 10, STACK, 0), fused_taken=False)
    assert on[2] == FRAMES * W * H


def test_sample_moments_read_the_first_radiance(gpu_ctx_ok):
    W, H = 50, 30
    ex = build("cornell", W, H, FRAMES, aov=False, moments=True)
    ctx = ex.scene.ctx
    moms = []
    for fused in (1, 0):
        res = run(ctx, W, H, fused)
        moms.append((res, ctx.moments_download(W, H)))
    assert moms[0][0][4] - moms[1][0][4] == 1
    assert same_bits(moms[0][0][0], moms[1][0][0], nan_payload=True) and moms[0][0][1:4] == moms[1][0][1:4]
    assert same_bits(moms[0][1], moms[1][1], nan_payload=True)
    assert (moms[0][1][:, :, 0] == FRAMES).all()
