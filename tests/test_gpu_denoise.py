"""The denoiser on the device (csrc/tirt_denoise.hip through tirt_denoise* and PathTrace.denoise): bit for bit against the numpy restatement of
the definition (tests/denoise_expected.py) on the Cornell box, a soup with silhouettes, the Teapot with its NaN words and films so small or ragged
that taps leave them at every level; the device-memory variant on torch tensors; the inputs untouched; the refusals."""
import numpy as np
import pytest

import denoise_expected as de
import ti_raytrace_amd
from test_film_shapes import make as make_row, tile_size, Row
from test_gpu_aov import SEED, build, check
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
FRAMES = 4
TEAPOT_FRAMES = 16          # the oracle's Teapot film at 48 x 40 and this seed gets its first NaN pixel in frames 12..15: none before
OTHER = dict(levels=3, sigma_c=0.5, sigma_n=0.6, sigma_z=0.05)
_cache = {}


def rendered(kind, W, H):
    """(example, hdr, records) of a 4-frame render (Teapot: 16) with feature buffers, made once per module"""
    key = (kind, W, H)
    if key not in _cache:
        frames = TEAPOT_FRAMES if kind == "teapot" else FRAMES
        ex = build(kind, W, H, frames)
        ex.integrator.render_frames(frames)
        _cache[key] = (ex, ex.integrator.hdr.to_numpy(), ex.integrator.aov_to_numpy())
    return _cache[key]


@pytest.mark.parametrize("kind,W,H,params", [
    ("cornell", 64, 48, {}), ("cornell", 64, 48, dict(levels=1)), ("cornell", 64, 48, OTHER),
    ("soup", 32, 32, {}), ("soup", 32, 32, OTHER), ("teapot", 48, 40, {}), ("teapot", 48, 40, dict(levels=1))],
    ids=["cornell", "cornell-1-level", "cornell-other", "soup", "soup-other", "teapot", "teapot-1-level"])
def test_bits_equal_the_definition(gpu_ctx_ok, kind, W, H, params):
    ex, hdr, aov = rendered(kind, W, H)
    it = ex.integrator
    rgb = it.rgb_film.to_numpy()
    it.denoise(**params)
    got = it.denoised.to_numpy()
    want = de.denoise_expected(hdr, aov, **params)
    nan_in = int(np.isnan(aov).sum() + np.isnan(hdr).sum())
    print("%s %d x %d %s: NaN words in %d, out %d; changed words %d of %d" % (kind, W, H, params, nan_in, int(np.isnan(want).sum()),
                                                                               int((want.view(np.uint32) != hdr.view(np.uint32)).sum()), want.size))
    assert got.shape == (W, H, 3) and got.dtype == np.float32
    if kind == "soup":
        alpha = aov[:, :, _native.AOV_ALPHA]
        assert (alpha == 0).any() and (alpha == 1).any()          # hits and misses: silhouettes
    if kind == "teapot":
        assert nan_in > 0
    assert np.isfinite(want).mean() > 0.9 and not np.array_equal(want, hdr)
    check(got, want, (kind, params))
    # the inputs are only read
    check(it.hdr.to_numpy(), hdr, "hdr", True); check(it.rgb_film.to_numpy(), rgb, "rgb_film", True); check(it.aov_to_numpy(), aov, "records", True)


@pytest.mark.parametrize("W,H,scale", [(1, 1, 0.4), (3, 5, 0.4), (65, 63, 0.8)], ids=["1x1", "3x5", "65x63"])
def test_bits_on_films_the_taps_leave(gpu_ctx_ok, W, H, scale):
    ex = make_row("cornell", W, H, scale, device_id=0)
    ctx = ex.scene.ctx
    ctx.film_create(W, H, 0, 1, tile_size(Row(W, H, None, (1,), scale, "")))
    ctx.aov_enable(True)
    ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, 0)
    hdr, aov = ctx.film_download(W, H)[0], ctx.aov_download(W, H)
    assert (aov[:, :, _native.AOV_ALPHA] > 0).any()
    for params in ({}, dict(levels=1), dict(levels=8)):
        ctx.denoise(**params)
        check(ctx.denoise_download(W, H), de.denoise_expected(hdr, aov, **params), (W, H, params))
    check(ctx.film_download(W, H)[0], hdr, "hdr", True); check(ctx.aov_download(W, H), aov, "records", True)


def test_device_variant_on_torch_tensors(gpu_ctx_ok):
    import torch
    W, H = 64, 48
    ex, hdr, aov = rendered("cornell", W, H)
    it, ctx = ex.integrator, ex.scene.ctx
    dev = torch.device("cuda", ctx.device_id)
    it.denoise()
    want = it.denoised.to_numpy()
    t = it.denoised_to_torch()
    assert t.shape == (W, H, 3) and t.dtype == torch.float32 and t.device == dev
    check(t.cpu().numpy(), want, "denoised_to_torch", True)
    hdr_t, aov_t = torch.from_numpy(hdr).to(dev), it.aov_to_torch()
    keep_h, keep_a = hdr_t.clone(), aov_t.clone()
    out = ti_raytrace_amd.denoise(hdr_t, aov_t, ctx=ctx)
    assert out.shape == (W, H, 3) and out.dtype == torch.float32 and out.device == dev
    check(out.cpu().numpy(), want, "tirt_denoise_device on the scene's context", True)
    check(ti_raytrace_amd.denoise(hdr_t, aov_t).cpu().numpy(), want, "on a context of its own (no film)", True)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        h2, a2 = hdr_t * 1.0, aov_t * 1.0                     # made on the side stream just before: the filter must be ordered after them
        out2 = ti_raytrace_amd.denoise(h2, a2, ctx=ctx, **OTHER)
        back = out2.cpu()                                     # and this copy after the filter
    side.synchronize()
    it.denoise(**OTHER)
    check(back.numpy(), it.denoised.to_numpy(), "on a non-default stream", True)
    assert torch.equal(hdr_t, keep_h) and torch.equal(aov_t.view(torch.int32), keep_a.view(torch.int32))
    for bad, exc in ((hdr, TypeError), (hdr_t.double(), TypeError), (hdr_t.cpu(), TypeError), (hdr_t[:, :, :2], ValueError), (hdr_t[:32], ValueError)):
        with pytest.raises(exc):
            ti_raytrace_amd.denoise(bad, aov_t, ctx=ctx)


def test_nan_normals_infinite_radiance_and_misses_on_a_made_up_film(gpu_ctx_ok):
    """what the rendered scenes do not hold: NaN normals (their pixels drop out of every sum, their own included), an infinite and a NaN film pixel, a
    column of misses, depths from 1e-7 (z*z below the 1e-12 floor) to 1e3, colour distances that put exp() among the denormals"""
    import torch
    W, H = 37, 29
    r = np.random.RandomState(11)
    hdr = (r.uniform(0.0, 1.0, (W, H, 3)) ** 4 * 8.0).astype(np.float32)
    aov = np.zeros((W, H, 8), np.float32)
    aov[:, :, 0:3] = r.uniform(0.0, 1.0, (W, H, 3)); aov[:, :, 7] = r.choice([0.25, 0.5, 1.0], (W, H))
    n = r.normal(size=(W, H, 3)); aov[:, :, 3:6] = n / np.linalg.norm(n, axis=2, keepdims=True) * (r.uniform(0, 1, (W, H, 1)) < 0.5)
    aov[:, :, 6] = np.exp(r.uniform(np.log(1e-7), np.log(1e3), (W, H)))
    aov[:, 10:12] = 0.0                                        # misses
    aov[5, 5, 3:6] = np.nan; aov[20, 3, 4] = np.nan; aov[36, 28, 3] = np.nan
    hdr[8, 20, 0] = np.inf; hdr[9, 20] = np.nan; hdr[0, 0, 2] = -np.inf
    dev = torch.device("cuda", 0)
    hdr_t, aov_t = torch.from_numpy(hdr).to(dev), torch.from_numpy(aov).to(dev)
    for params in ({}, dict(levels=2, sigma_c=0.05, sigma_n=2.0, sigma_z=10.0), dict(levels=8, sigma_c=1e3)):
        got = ti_raytrace_amd.denoise(hdr_t, aov_t, **params).cpu().numpy()
        want = de.denoise_expected(hdr, aov, **params)
        assert np.isnan(want[5, 5]).all() and np.isnan(want[9, 20]).all() and np.isposinf(want[8, 20, 0]) and np.isfinite(want).mean() > 0.95
        check(got, want, params)


def test_refusals_and_lifecycle(gpu_ctx_ok):
    import torch
    W, H = 64, 48
    ex = build("cornell", W, H, FRAMES, aov=False)
    it, ctx = ex.integrator, ex.scene.ctx
    it.render_frames(FRAMES)
    with pytest.raises(_native.TirtError, match="not enabled"):
        it.denoise()
    ctx.aov_enable(True)
    with pytest.raises(_native.TirtError, match="nothing filtered"):
        ctx.denoise_download(W, H)
    with pytest.raises(_native.TirtError, match="nothing filtered"):
        ctx.denoise_export_device(1 << 20)
    ctx.film_clear()
    it.render_frames(FRAMES)
    for bad in (dict(levels=0), dict(levels=9), dict(levels=-1)):
        with pytest.raises(_native.TirtError, match="levels"):
            it.denoise(**bad)
    for name in ("sigma_c", "sigma_n", "sigma_z"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(_native.TirtError, match="sigma"):
                it.denoise(**{name: v})
    with pytest.raises(_native.TirtError, match="nothing filtered"):          # a refused call filtered nothing
        ctx.denoise_download(W, H)
    it.denoise()
    first = it.denoised.to_numpy()
    assert np.isfinite(first).all()
    with pytest.raises(_native.TirtError, match="null"):
        ctx.denoise_export_device(0)
    # the device variant: host memory, an output that is an input, bad parameters
    dev = torch.device("cuda", ctx.device_id)
    hdr_t, aov_t, out_t = it.denoised_to_torch(), it.aov_to_torch(), torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    host = np.zeros((W, H, 8), np.float32)
    for args in ((host.ctypes.data, aov_t.data_ptr(), out_t.data_ptr()), (hdr_t.data_ptr(), host.ctypes.data, out_t.data_ptr()),
                 (hdr_t.data_ptr(), aov_t.data_ptr(), host.ctypes.data)):
        with pytest.raises(_native.TirtError, match="not device memory"):
            ctx.denoise_device(*args, W, H)
    for out in (hdr_t.data_ptr(), aov_t.data_ptr(), aov_t.data_ptr() + 4 * W * H, hdr_t.data_ptr() + 16):
        with pytest.raises(_native.TirtError, match="overlaps"):
            ctx.denoise_device(hdr_t.data_ptr(), aov_t.data_ptr(), out, W, H)
    with pytest.raises(_native.TirtError, match="null"):
        ctx.denoise_device(hdr_t.data_ptr(), aov_t.data_ptr(), 0, W, H)
    with pytest.raises(_native.TirtError, match="levels"):
        ctx.denoise_device(hdr_t.data_ptr(), aov_t.data_ptr(), out_t.data_ptr(), W, H, levels=9)
    with pytest.raises(_native.TirtError, match="bad size"):
        ctx.denoise_device(hdr_t.data_ptr(), aov_t.data_ptr(), out_t.data_ptr(), 0, H)
    # tirt_film_clear leaves the filtered film alone; a new film drops it; a rank's partial film is refused
    ctx.film_clear()
    check(ctx.denoise_download(W, H), first, "after film_clear", True)
    ctx.film_create(W, H, 0, 2, 8 * H)
    with pytest.raises(_native.TirtError, match="nothing filtered"):
        ctx.denoise_download(W, H)
    ctx.aov_enable(True)
    ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, 0)
    with pytest.raises(_native.TirtError, match="tile_count"):
        ctx.denoise()
    fresh = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.denoise()
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.denoise_download(W, H)
    finally:
        fresh.close()
