"""The sample moments of the path tracer on the device (csrc/tirt_moments.hip through tirt_moments_* and PathTrace(moments=True)): bit for bit against
Welford's update restated in numpy (tests/moments_expected.py) over the CPU oracle's exact pixel-samples, on the Cornell box and the glass Teapot with its
samples that are not finite; independent of how the frames are cut into calls, batches, lanes and tiles and of the route of the camera rays; the film
untouched; the other integrators leaving the records alone; the counts of tirt_moments_converged; lifecycle and refusals."""
import numpy as np
import pytest

import moments_expected as me
from test_gpu_aov import SEED, build, check, oracle_of, rewind
from ti_raytrace_amd import Debug, _native, scenes

pytestmark = pytest.mark.gpu
WORDS = _native.MOM_WORDS
DEPTH, STACK = 15, 64


def equal_records(got, want, what):
    """bit for bit but for the sign of a zero; a record holds no NaN"""
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(got).any(), (what, "NaN in a record")
    ne = got != want
    assert not ne.any(), (what, "words that differ: %d of %d, first at %s" % (int(ne.sum()), ne.size, np.argwhere(ne)[:4].tolist()))


# ---- 1. against the oracle, exactly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,H", [("cornell", 24, 20), ("cornell", 13, 7), ("cornell", 1, 1), ("teapot", 24, 20)],
                         ids=["cornell-24x20", "cornell-13x7", "cornell-1x1", "teapot-24x20"])
def test_records_equal_welford_over_the_oracles_samples(gpu_ctx_ok, kind, W, H):
    ex = build(kind, W, H, 32, aov=False, moments=True)
    ctx, orc = ex.scene.ctx, oracle_of(ex, kind)
    # six one-frame calls at the frames whose oracle samples are exact
    xs = [me.oracle_sample(orc, W, H, fr, SEED) for fr in me.EXACT_FRAMES]
    want = me.expected(xs, W, H)
    bad_px = int((want[:, :, _native.MOM_BAD] > 0).sum())
    print("%s %d x %d: oracle samples that are not finite: %d pixels; n in [%g, %g]" % (kind, W, H, bad_px, want[:, :, 0].min(), want[:, :, 0].max()))
    if kind == "teapot":
        assert bad_px >= 1          # the oracle alone: frame 31 of this film and seed has a pixel-sample that is not finite
        assert (want[:, :, 0] + want[:, :, _native.MOM_BAD] == len(xs)).all()
    for fr in me.EXACT_FRAMES:
        ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)
    got = ctx.moments_download(W, H)
    equal_records(got, want, (kind, "six one-frame calls"))
    assert (got[:, :, 0] + got[:, :, _native.MOM_BAD] == len(xs)).all()
    # the fields are views of the same record
    it = ex.integrator
    assert it.samples.to_numpy().shape == (W, H) and it.variance.to_numpy().shape == (W, H, 3)
    check(it.samples.to_numpy(), got[:, :, 0], "samples", True); check(it.mean.to_numpy(), got[:, :, 1:4], "mean", True)
    check(it.bad.to_numpy(), got[:, :, 7], "bad", True)
    var = it.variance.to_numpy()
    n = got[:, :, 0:1]
    assert not np.isnan(var).any() and (var[(n < 2)[:, :, 0]] == 0).all()
    with np.errstate(all="ignore"):
        assert np.array_equal(var[(n >= 2)[:, :, 0]], (got[:, :, 4:7] / (n - np.float32(1)))[(n >= 2)[:, :, 0]])
    # frame 0 at eight seeds, eight calls
    ctx.film_clear()
    assert (ctx.moments_download(W, H).view(np.uint32) == 0).all()
    seeds = range(1, 9)
    for seed in seeds:
        ctx.pt_rgb_render(0, 1, seed, DEPTH, STACK, 0)
    equal_records(ctx.moments_download(W, H), me.expected([me.oracle_sample(orc, W, H, 0, seed) for seed in seeds], W, H), (kind, "frame 0 at eight seeds"))
    # frames {0, 1} as one call, merge_paths at its default
    ctx.film_clear()
    ctx.pt_rgb_render(0, 2, SEED, DEPTH, STACK, 0)
    equal_records(ctx.moments_download(W, H), me.expected(xs[:2], W, H), (kind, "a two-frame batch"))


# ---- 2. the cut into calls, batches, lanes, routes and tiles does not matter -------------------------------------------------------------------
@pytest.mark.parametrize("W,H,ts", [(24, 20, 100), (32, 24, 8 * 24)], ids=["24x20-ragged-tiles", "32x24-blocked-tiles"])
def test_split_invariance(gpu_ctx_ok, W, H, ts):
    """(32 x 24: P % 64 == 0, the pixel-block-major path numbering, and tiles the device walks in 8 x 8 blocks; 24 x 20: neither)"""
    N = 8
    ex = build("cornell", W, H, N, aov=False, moments=True)
    ctx = ex.scene.ctx
    ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
    whole, hdr = ctx.moments_download(W, H), ctx.film_download(W, H)[0]
    assert (whole[:, :, 0] == N).all() and (whole[:, :, 4:7] > 0).any() and not np.isnan(whole).any()

    def again(what, render):
        ctx.film_clear()
        render()
        check(ctx.moments_download(W, H), whole, what, True)
        check(ctx.film_download(W, H)[0], hdr, ("hdr", what), True)

    def frame_by_frame():
        for fr in range(N):
            ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)
    ctx.set_option("merge_paths", 0)
    again("eight calls, merge_paths 0", frame_by_frame)
    ctx.set_option("merge_paths", 32 << 20)
    again("eight calls, merged", frame_by_frame)
    ctx.set_option("batch_paths", 2 * W * H)                # four batches of two frames on four lanes
    ctx.stats_reset()
    again("one call, four batches", lambda: ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0))
    assert ctx.stats()["launches_trace_closest"] // DEPTH == 4
    ctx.set_option("overlap_lanes", 1)
    again("one call, four batches, one lane", lambda: ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0))
    ctx.set_option("overlap_lanes", 4)
    ctx.set_option("batch_paths", 32 << 20)
    ctx.set_option("primary_beams_min_frames", 1)
    for beams in (0, 1):
        ctx.set_option("primary_beams", beams)
        again(("primary_beams", beams), lambda: ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0))
        if beams:
            assert ctx.primary_beam_stats()["rays"] >= N * W * H
    # three ranks: zero outside their own pixels, and together the single context's records
    ranks = 3
    p = np.arange(W * H).reshape(W, H)
    merged = np.zeros_like(whole)
    for rank in range(ranks):
        ctx.film_create(W, H, rank, ranks, ts)
        ctx.moments_enable(True)
        ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
        part = ctx.moments_download(W, H)
        mine = (p // ts) % ranks == rank
        assert mine.any() and (part[~mine].view(np.uint32) == 0).all(), rank
        assert ctx.moments_converged(0.05)[0] == int(mine.sum())
        merged[mine] = part[mine]
    check(merged, whole, "three ranks merged", True)


# ---- 3. the film is untouched; the other integrators leave the records alone ----------------------------------------------------------------------
def test_film_untouched_and_other_integrators_leave_the_records_alone(gpu_ctx_ok):
    W, H, N = 24, 20, 6
    ex = build("cornell", W, H, N, aov=False, moments=True)
    ctx = ex.scene.ctx
    ex.integrator.render_frames(N)
    rec, hdr = ex.integrator.moments_to_numpy(), ex.integrator.hdr.to_numpy()
    assert (rec[:, :, 0] == N).all()
    plain = build("cornell", W, H, N, aov=False)
    plain.integrator.render_frames(N)
    check(plain.integrator.hdr.to_numpy(), hdr, "hdr with and without the moments", True)
    with pytest.raises(_native.TirtError, match="not enabled"):
        plain.integrator.moments_to_numpy()
    d = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode="normal", seed=SEED)
    ex.cam.frame = 3; ex.cam.frame_cpu[0] = 3
    d.render()
    assert (d.hdr.to_numpy() != 0).any()
    check(ctx.moments_download(W, H), rec, "after Debug", True)
    ctx.bdpt_rgb_render(0, 2, SEED)
    assert np.isfinite(ctx.film_download(W, H)[0]).all()
    check(ctx.moments_download(W, H), rec, "after BDPT_RGB", True)
    # PT_Spec: its samples are hero-wavelength radiances, not RGB
    sp = scenes.spectral_box(16, 8, 2, device_id=0, seed=SEED)
    sp.build_scene()
    sp.scene.ctx.moments_enable(True)
    sp.integrator.render_frames(2)
    assert (sp.integrator.hdr.to_numpy() != 0).any()
    assert (sp.scene.ctx.moments_download(16, 8).view(np.uint32) == 0).all()


# ---- 4. tirt_moments_converged ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "teapot"])
def test_converged_counts_equal_numpy(gpu_ctx_ok, kind):
    import torch
    W, H = 24, 20
    ex = build(kind, W, H, 32, aov=False, moments=True)
    ctx, it = ex.scene.ctx, ex.integrator
    assert it.converged(0.1) == (0, 0, 0)                   # nothing rendered: nothing measured
    ctx.pt_rgb_render(0, 1, SEED, DEPTH, STACK, 0)
    assert it.converged(0.1) == (0, 0, 0)                   # one sample: still nothing
    for fr in (1, 3, 7, 15, 31):
        ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)
    rec = it.moments_to_numpy()
    n = rec[:, :, 0]
    with np.errstate(all="ignore"):
        nn = n * (n - 1)
        ratio = np.sqrt((rec[:, :, 4:7].astype(np.float64) / nn[:, :, None]).sum(axis=2)) / np.abs(rec[:, :, 1:4].astype(np.float64).sum(axis=2) / 3)
    ratio = ratio[np.isfinite(ratio) & (ratio > 0)]
    middle = float(np.median(ratio))
    seen = {}
    for name, thr in (("separates", middle), ("above all", float(ratio.max()) * 4.0), ("below all", float(ratio.min()) / 4.0)):
        got, want = it.converged(thr), me.converged(rec, thr)
        print(kind, name, thr, got)
        assert got == want, (name, thr)
        seen[name] = got
    measured = seen["separates"][0]
    assert measured == int((n >= 2).sum()) and 0 < seen["separates"][1] < measured
    assert seen["above all"][1] == 0 and seen["below all"][1] == len(ratio)
    if kind == "teapot":
        assert seen["separates"][2] >= 1
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(_native.TirtError, match="threshold"):
            it.converged(bad)
    t = it.moments_to_torch()
    assert t.shape == (W, H, WORDS) and t.dtype == torch.float32 and t.device == torch.device("cuda", ctx.device_id)
    check(t.cpu().numpy(), rec, "moments_to_torch", True)


# ---- 5. lifecycle and refusals ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(gpu_ctx_ok):
    W, H, N = 24, 20, 4
    ex = build("cornell", W, H, N, aov=False)
    ctx, it = ex.scene.ctx, ex.integrator
    for call in (lambda: ctx.moments_download(W, H), lambda: ctx.moments_export_device(1 << 20), lambda: ctx.moments_converged(0.1)):
        with pytest.raises(_native.TirtError, match="not enabled"):
            call()
    it.render_frames(N)
    ctx.moments_enable(True)
    with pytest.raises(_native.TirtError, match="null"):
        ctx.moments_export_device(0)
    assert (ctx.moments_download(W, H).view(np.uint32) == 0).all()          # enabled: zeros until a frame is rendered
    rewind(ex)
    it.render_frames(N)
    rec = ctx.moments_download(W, H)
    assert (rec[:, :, 0] == N).all()
    ctx.film_clear()
    assert (ctx.moments_download(W, H).view(np.uint32) == 0).all()          # film_clear zeroes them
    it.render_frames(N)
    check(ctx.moments_download(W, H), rec, "after film_clear", True)
    it.render_frames(N)                                                     # without a clear the same frames count again
    assert (ctx.moments_download(W, H)[:, :, 0] == 2 * N).all()
    ctx.moments_enable(False)
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.moments_download(W, H)
    ctx.film_clear()
    it.render_frames(N)
    ctx.moments_enable(True)
    assert (ctx.moments_download(W, H).view(np.uint32) == 0).all()          # enable, disable, enable starts from zero
    ctx.film_create(13, 7, 0, 1, 4096)                                      # a new film starts disabled
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.moments_download(13, 7)
    fresh = _native.Context(0)
    try:
        for call in (lambda: fresh.moments_enable(True), lambda: fresh.moments_download(W, H), lambda: fresh.moments_converged(0.1)):
            with pytest.raises(_native.TirtError, match="film not created"):
                call()
    finally:
        fresh.close()
