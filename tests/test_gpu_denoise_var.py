"""The variance-guided mode of the denoiser on the device (csrc/tirt_denoise.hip through tirt_denoise_var*, PathTrace.denoise_var() and
ti_raytrace_amd.denoise_var(hdr, aov, moments)): bit for bit against the numpy restatement of its definition (tests/denoise_var_expected.py) on made-up
films with everything a record can hold; the context's route against the device-memory route on a rendered film; tirt_denoise unchanged; refusals."""
import numpy as np
import pytest

import denoise_expected as de
import denoise_var_expected as dv
import ti_raytrace_amd
from test_gpu_aov import SEED, build, check
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
OTHER = dict(levels=3, sigma_c=0.7, sigma_n=0.6, sigma_z=0.05)


def made_up(W, H, seed):
    """random hdr, feature records and moment records: pixels with n = 0 and n = 1, zero variance, a variance so large that the sum over channels
    overflows, a negative and a NaN M2 (no variance either), NaN and infinite film pixels, a NaN normal, misses, depths over ten decades"""
    r = np.random.RandomState(seed)
    hdr = (r.uniform(0.0, 1.0, (W, H, 3)) ** 4 * 8.0).astype(np.float32)
    aov = np.zeros((W, H, 8), np.float32)
    aov[:, :, 0:3] = r.uniform(0.0, 1.0, (W, H, 3)); aov[:, :, 7] = r.choice([0.25, 0.5, 1.0], (W, H))
    n = r.normal(size=(W, H, 3)); aov[:, :, 3:6] = n / np.linalg.norm(n, axis=2, keepdims=True) * (r.uniform(0, 1, (W, H, 1)) < 0.5)
    aov[:, :, 6] = np.exp(r.uniform(np.log(1e-7), np.log(1e3), (W, H)))
    mom = np.zeros((W, H, 8), np.float32)
    mom[:, :, 0] = r.choice([0, 1, 2, 4, 4, 4, 16, 100], (W, H))
    mom[:, :, 1:4] = hdr
    mom[:, :, 4:7] = (hdr * r.uniform(0.0, 2.0, (W, H, 3))) ** 2 * mom[:, :, 0:1] * (r.uniform(0, 1, (W, H, 1)) < 0.85)      # 15 %: no variance at all
    mom[:, :, 7] = r.choice([0, 0, 0, 1], (W, H))
    flat = lambda a: a.reshape(W * H, -1)
    P = W * H
    if P > 1:
        aov[:, H // 2] = 0.0                                   # a row of misses
        k = r.permutation(P)
        flat(mom)[k[0 % P], 4:7] = 3.0e38; flat(mom)[k[0 % P], 0] = 2          # v.r + v.g overflows: not a known variance
        flat(mom)[k[1 % P], 5] = -1.0e3; flat(mom)[k[1 % P], 0] = 4           # a negative sum
        flat(mom)[k[2 % P], 6] = np.nan; flat(mom)[k[2 % P], 0] = 4
        flat(hdr)[k[3 % P], 0] = np.inf
        flat(hdr)[k[4 % P]] = np.nan
        flat(aov)[k[5 % P], 3:6] = np.nan
        flat(aov)[k[6 % P], 4] = np.nan
    return hdr, aov, mom


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (33, 17)], ids=["1x1", "5x3", "33x17"])
def test_bits_equal_the_definition_on_made_up_films(gpu_ctx_ok, W, H):
    import torch
    hdr, aov, mom = made_up(W, H, 100 * W + H)
    if W * H > 1:
        assert (mom[:, :, 0] == 0).any() and (mom[:, :, 0] == 1).any() and np.isnan(hdr).any() and np.isnan(aov).any()
    dev = torch.device("cuda", 0)
    hdr_t, aov_t, mom_t = (torch.from_numpy(a).to(dev) for a in (hdr, aov, mom))
    keep = [t.clone() for t in (hdr_t, aov_t, mom_t)]
    for levels in (1, 3, 8):
        for extra in ({}, dict(sigma_c=0.7, sigma_n=0.6, sigma_z=0.05)):
            params = dict(levels=levels, **extra)
            want, s = dv.denoise_var_expected(hdr, aov, mom, want_s=True, **params)
            assert not np.isnan(s).any()                       # the propagated variance never turns NaN
            got = ti_raytrace_amd.denoise_var(hdr_t, aov_t, mom_t, **params).cpu().numpy()
            assert got.shape == (W, H, 3) and got.dtype == np.float32
            check(got, want, (W, H, params))
            if W * H > 100:
                assert np.isfinite(want).mean() > 0.9 and not np.array_equal(want, de.denoise_expected(hdr, aov, levels=levels))
    for t, k in zip((hdr_t, aov_t, mom_t), keep):              # the inputs are only read
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))


def test_context_route_equals_device_route_and_tirt_denoise_is_unchanged(gpu_ctx_ok):
    import torch
    W, H, N = 24, 20, 4
    ex = build("cornell", W, H, N, aov=True, moments=True)
    it, ctx = ex.integrator, ex.scene.ctx
    it.render_frames(N)
    hdr, aov, mom = it.hdr.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy()
    assert (mom[:, :, 0] == N).all()
    it.denoise()
    before = it.denoised.to_numpy()
    check(before, de.denoise_expected(hdr, aov), "tirt_denoise before")
    dev = torch.device("cuda", ctx.device_id)
    hdr_t, aov_t, mom_t = torch.from_numpy(hdr).to(dev), it.aov_to_torch(), it.moments_to_torch()
    for params in ({}, OTHER):
        it.denoise_var(**params)
        got = it.denoised.to_numpy()
        check(got, dv.denoise_var_expected(hdr, aov, mom, **params), ("tirt_denoise_var", params))
        check(ti_raytrace_amd.denoise_var(hdr_t, aov_t, mom_t, ctx=ctx, **params).cpu().numpy(), got, ("device route, the scene's context", params), True)
        check(ti_raytrace_amd.denoise_var(hdr_t, aov_t, mom_t, **params).cpu().numpy(), got, ("device route, a context of its own", params), True)
        assert not np.array_equal(got, before) and np.isfinite(got).all()
    check(it.hdr.to_numpy(), hdr, "hdr", True); check(it.aov_to_numpy(), aov, "feature records", True); check(it.moments_to_numpy(), mom, "moment records", True)
    it.denoise()
    check(it.denoised.to_numpy(), before, "tirt_denoise after", True)
    check(ti_raytrace_amd.denoise(hdr_t, aov_t, ctx=ctx).cpu().numpy(), before, "tirt_denoise_device after", True)


def test_refusals(gpu_ctx_ok):
    import torch
    W, H, N = 24, 20, 2
    ex = build("cornell", W, H, N, aov=True, moments=False)
    it, ctx = ex.integrator, ex.scene.ctx
    it.render_frames(N)
    with pytest.raises(ValueError, match="moments=True"):
        it.denoise_var()
    with pytest.raises(_native.TirtError, match="moment buffers not enabled"):
        ctx.denoise_var()
    ctx.moments_enable(True)
    ctx.aov_enable(False)
    with pytest.raises(_native.TirtError, match="feature buffers not enabled"):
        ctx.denoise_var()
    ctx.aov_enable(True)
    for bad in (dict(levels=0), dict(levels=9)):
        with pytest.raises(_native.TirtError, match="levels"):
            ctx.denoise_var(**bad)
    for name in ("sigma_c", "sigma_n", "sigma_z"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(_native.TirtError, match="sigma"):
                ctx.denoise_var(**{name: v})
    ctx.denoise_var()                                          # nothing rendered since the records were enabled: n = 0 everywhere, guides alone
    assert ctx.denoise_download(W, H).shape == (W, H, 3)
    dev = torch.device("cuda", ctx.device_id)
    hdr_t = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    aov_t, mom_t = torch.zeros((W, H, 8), dtype=torch.float32, device=dev), torch.zeros((W, H, 8), dtype=torch.float32, device=dev)
    out_t = torch.empty_like(hdr_t)
    host = np.zeros((W, H, 8), np.float32)
    ptrs = [hdr_t.data_ptr(), aov_t.data_ptr(), mom_t.data_ptr(), out_t.data_ptr()]
    for k in range(4):
        args = list(ptrs); args[k] = host.ctypes.data
        with pytest.raises(_native.TirtError, match="not device memory"):
            ctx.denoise_var_device(*args, W, H)
        args[k] = 0
        with pytest.raises(_native.TirtError, match="null"):
            ctx.denoise_var_device(*args, W, H)
    for out in (hdr_t.data_ptr(), aov_t.data_ptr(), mom_t.data_ptr(), mom_t.data_ptr() + 4 * W * H):
        with pytest.raises(_native.TirtError, match="overlaps"):
            ctx.denoise_var_device(ptrs[0], ptrs[1], ptrs[2], out, W, H)
    with pytest.raises(_native.TirtError, match="aligned"):
        ctx.denoise_var_device(ptrs[0], ptrs[1], ptrs[2] + 4, ptrs[3], W, H - 1)
    with pytest.raises(_native.TirtError, match="bad size"):
        ctx.denoise_var_device(*ptrs, 0, H)
    with pytest.raises(_native.TirtError, match="levels"):
        ctx.denoise_var_device(*ptrs, W, H, levels=9)
    for bad, exc in ((host, TypeError), (mom_t.double(), TypeError), (mom_t.cpu(), TypeError), (mom_t[:, :, :4], ValueError), (mom_t[:12], ValueError)):
        with pytest.raises(exc):
            ti_raytrace_amd.denoise_var(hdr_t, aov_t, bad, ctx=ctx)
    ctx.film_create(W, H, 0, 2, 100)                           # a rank's partial film is refused
    ctx.aov_enable(True); ctx.moments_enable(True)
    with pytest.raises(_native.TirtError, match="tile_count"):
        ctx.denoise_var()
    fresh = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.denoise_var()
    finally:
        fresh.close()


@pytest.mark.parametrize("W,H", [(5, 3), (33, 17)], ids=["5x3", "33x17"])
def test_the_two_modes_in_turn_on_one_context_leave_nothing_behind_for_each_other(gpu_ctx_ok, W, H):
    """Both modes are one set of kernels over one scratch and one launch path; they pack the fourth words of its records differently, and the
    variance-guided mode starts its ping-pong from the other half of A: on one context tirt_denoise, tirt_denoise_var, tirt_denoise again, at levels 1 and 3.  The first and the third
    give the same bits, those of denoise_expected; the second those of denoise_var_expected.  5 x 3 is the smallest film where a level-1 tap leaves
    the film on every side; 33 x 17 crosses a wave boundary along j and every step of level 3 lands inside and outside.
    The device-memory entry points take a made-up film (`made_up`: NaN pixels, unknown variances).  The context's own route has no way to take made-up
    records -- there is no import of feature or moment records -- so it runs the same sequence on a rendered Cornell box of the same size."""
    import torch
    dev = torch.device("cuda", 0)
    hdr, aov, mom = made_up(W, H, 100 * W + H)
    hdr_t, aov_t, mom_t = (torch.from_numpy(a).to(dev) for a in (hdr, aov, mom))
    ctx = _native.Context(0)
    try:
        for levels in (1, 3):
            first = ti_raytrace_amd.denoise(hdr_t, aov_t, levels=levels, ctx=ctx).cpu().numpy()
            second = ti_raytrace_amd.denoise_var(hdr_t, aov_t, mom_t, levels=levels, ctx=ctx).cpu().numpy()
            third = ti_raytrace_amd.denoise(hdr_t, aov_t, levels=levels, ctx=ctx).cpu().numpy()
            check(first, de.denoise_expected(hdr, aov, levels=levels), ("tirt_denoise_device first", W, H, levels))
            check(second, dv.denoise_var_expected(hdr, aov, mom, levels=levels), ("tirt_denoise_var_device between", W, H, levels))
            check(third, first, ("tirt_denoise_device again", W, H, levels), True)
    finally:
        ctx.close()
    N = 2
    ex = build("cornell", W, H, N, aov=True, moments=True)
    it = ex.integrator
    it.render_frames(N)
    hdr, aov, mom = it.hdr.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy()
    assert (mom[:, :, 0] == N).all()
    for levels in (1, 3):
        it.denoise(levels=levels); first = it.denoised.to_numpy()
        it.denoise_var(levels=levels); second = it.denoised.to_numpy()
        it.denoise(levels=levels); third = it.denoised.to_numpy()
        check(first, de.denoise_expected(hdr, aov, levels=levels), ("tirt_denoise first", W, H, levels))
        check(second, dv.denoise_var_expected(hdr, aov, mom, levels=levels), ("tirt_denoise_var between", W, H, levels))
        check(third, first, ("tirt_denoise again", W, H, levels), True)
