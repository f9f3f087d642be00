"""The temporal accumulation on the device (csrc/tirt_temporal.hip through tirt_temporal_*, PathTrace(temporal=True) and
ti_raytrace_amd.temporal_accumulate): bit for bit, NaNs in the same places, against the numpy restatement of its definition (tests/temporal_expected.py)
applied to the records the device itself rendered -- same camera, a yaw step that reprojects, rejects and leaves the film, the cap, a film pixel that is
not finite, ragged shapes, the device-memory route, the filter over the accumulated film, an adaptively sampled view; nothing else moved; lifecycle; refusals.
Films are 24 x 20 with 2 frames per view at seeds SEED, SEED + 1, ... unless a case says otherwise."""
import numpy as np
import pytest

import denoise_var_expected as dv
import temporal_expected as te
import ti_raytrace_amd
from test_gpu_aov import SEED, build, check, rewind
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
W, H = 24, 20
YAW_STEP = 0.2          # Cornell 24 x 20 from yaw 0: the oracle's films reproject 386 of 480 pixels, reject 47 and send 3 off the film
DEPTH, STACK = 15, 64
WIDE = dict(sigma_n=4.0, sigma_z=10.0)          # guides that reject nothing: dn <= 4 for mean normals, |d - z| <= 10 d


def tbuild(kind, w, h, temporal=True, **kw):
    return build(kind, w, h, 2, aov=True, moments=True, temporal=temporal, **kw)


def render_view(ex, view, yaw=None, frames=2, first_frame=0, seed=None):
    """move the camera, clear the film, render `frames` frames at the view's own seed; the film and its records as the device holds them, and the camera"""
    if yaw is not None:
        ex.cam.set_view_point(yaw, 0.0, 0.0, ex.cam.scale)
    rewind(ex)
    it = ex.integrator
    it.seed = SEED + view if seed is None else seed
    ex.scene.ctx.pt_rgb_render(first_frame, frames, it.seed, DEPTH, STACK, 0)
    return it.hdr.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy(), te.Cam(ex.cam)


def accumulate_views(ex, yaws, what, **params):
    """render and accumulate the views in turn; after each the device's history must equal the restatement chained over the device's own records.
    Returns the views, the accumulated (hdr, mom) and the restatement's info per step."""
    it = ex.integrator
    views, infos, acc = [], [], None
    for k, yaw in enumerate(yaws):
        views.append(render_view(ex, k, yaw))
        hdr, aov, mom, cam = views[-1]
        it.temporal_accumulate(**params)
        if acc is None:
            acc = te.first(hdr, aov, mom)
        else:
            h, m, info = te.accumulate(hdr, aov, mom, acc[0], views[-2][1], acc[1], cam, views[-2][3], want_info=True, **params)
            acc = (h, m); infos.append(info)
        got_h, got_m = it.temporal_to_numpy()
        check(got_h, acc[0], (what, "hdr after view", k)); check(got_m, acc[1], (what, "moments after view", k))
    return views, acc, infos


def test_first_accumulate_copies_the_film_and_its_records(gpu_ctx_ok):
    ex = tbuild("cornell", W, H)
    it = ex.integrator
    hdr, aov, mom, _ = render_view(ex, 0, 0.0)
    assert (mom[:, :, 0] == 2).all() and 0.5 < (aov[:, :, 7] > 0).mean() < 1.0
    it.temporal_accumulate()
    got_h, got_m = it.temporal_to_numpy()
    check(got_h, hdr, "hdr", True); check(got_m, mom, "moments", True)
    check(it.accumulated.to_numpy(), hdr, "accumulated", True); check(it.accumulated_samples.to_numpy(), mom[:, :, 0], "accumulated_samples", True)


def test_same_camera_two_views_merge(gpu_ctx_ok):
    """With guides that reject nothing every pixel whose camera rays hit something in both views must take the merge, n_o = n_1 + n_2: a pixel's own
    history pixel carries a bilinear weight of 1 - O(1e-6).  (At the default guides an edge pixel whose two jittered samples met two surfaces has another
    mean normal in each view and is rejected: there the case is held to the restatement alone.)"""
    for params in (WIDE, {}):
        ex = tbuild("cornell", W, H)
        views, (acc_h, acc_m), infos = accumulate_views(ex, [0.0, 0.0], ("same camera", params), **params)
        both = (views[0][1][:, :, 7] > 0) & (views[1][1][:, :, 7] > 0)
        n_sum = views[0][2][:, :, 0] + views[1][2][:, :, 0]
        merged = infos[0]["history"] & (acc_m[:, :, 0] == n_sum)
        print("same camera", params, "pixels hit in both views", int(both.sum()), "merged with n_1 + n_2", int(merged.sum()))
        assert both.sum() > W * H // 2 and (n_sum == 4).all() and not np.array_equal(views[0][0], views[1][0])
        if params:
            assert merged[both].all()
        else:
            assert merged.sum() > W * H // 2


def test_yaw_step_reprojects_rejects_and_leaves_the_film(gpu_ctx_ok):
    ex = tbuild("cornell", W, H)
    views, acc, infos = accumulate_views(ex, [0.0, YAW_STEP], "yaw step")
    info = infos[0]
    print("yaw step %.2f: history %d of %d, rejected on depth or normal %d, off the film %d" % (YAW_STEP, info["history"].sum(), W * H, info["rejected"].sum(), info["off_film"].sum()))
    assert info["history"].sum() >= W * H // 2 and info["rejected"].sum() >= 1 and info["off_film"].sum() >= 1


def test_four_views_with_a_cap_of_three(gpu_ctx_ok):
    ex = tbuild("cornell", W, H)
    views, (acc_h, acc_m), infos = accumulate_views(ex, [0.0, 0.03, 0.06, 0.09], "cap", max_history=3.0)
    capped = [int(i["capped"].sum()) for i in infos]
    print("pixels that took the cap branch per step:", capped, "largest n", float(acc_m[:, :, 0].max()))
    assert capped[0] == 0 and capped[1] >= W * H // 4 and capped[2] >= W * H // 4          # n_h is 2, then 4, then 5
    assert acc_m[:, :, 0].max() == 5.0


def test_a_film_pixel_that_is_not_finite_stays_and_poisons_no_neighbour(gpu_ctx_ok):
    """The glass Teapot at 13 x 7: from the example's own camera (yaw 0), frame 6 at seed 10 has a pixel-sample that is not finite (the oracle's film says so
    too).  View 1, a small yaw step away, is clean; view 2 is frames 0 .. 7 at that seed from yaw 0 (eight frames, so that the film is a film) -- its film
    pixel is NaN, stays NaN, and its moment record (seven finite samples, one bad) still merges; view 3 reprojects a history with that NaN pixel in it, and
    comes out finite everywhere."""
    w, h = 13, 7
    ex = tbuild("teapot", w, h)
    it = ex.integrator
    v1 = render_view(ex, 0, 0.01)
    it.temporal_accumulate()
    v2 = render_view(ex, 1, 0.0, frames=8, seed=10)
    nan_px = ~np.isfinite(v2[0]).all(axis=2)
    assert np.isfinite(v1[0]).all() and nan_px.sum() >= 1 and (v2[2][:, :, 7][nan_px] >= 1).all() and not np.isnan(v2[2]).any()
    it.temporal_accumulate()
    want_h, want_m, info = te.accumulate(v2[0], v2[1], v2[2], v1[0], v1[1], v1[2], v2[3], v1[3], want_info=True)
    got_h, got_m = it.temporal_to_numpy()
    check(got_h, want_h, "hdr, view 2"); check(got_m, want_m, "moments, view 2")
    assert np.array_equal(~np.isfinite(got_h).all(axis=2), nan_px) and not np.isnan(got_m).any()
    assert (info["history"] & nan_px).any(), "the pixel that is not finite took no history: the case does not show that its moments merge"
    assert (got_m[:, :, 0][info["history"] & nan_px] > v2[2][:, :, 0][info["history"] & nan_px]).all()
    v3 = render_view(ex, 2, 0.02)
    it.temporal_accumulate()
    want_h3, want_m3, info3 = te.accumulate(v3[0], v3[1], v3[2], want_h, v2[1], want_m, v3[3], v2[3], want_info=True)
    got_h3, got_m3 = it.temporal_to_numpy()
    check(got_h3, want_h3, "hdr, view 3"); check(got_m3, want_m3, "moments, view 3")
    assert np.isfinite(v3[0]).all() and np.isfinite(got_h3).all() and np.isfinite(got_m3).all() and info3["history"].sum() >= 10


@pytest.mark.parametrize("kind,w,h", [("cornell", 1, 1), ("cornell", 13, 7), ("cornell", 65, 63)], ids=["1x1", "13x7", "65x63"])
def test_shapes(gpu_ctx_ok, kind, w, h):
    ex = tbuild(kind, w, h)
    views, acc, infos = accumulate_views(ex, [0.0, 0.1, 0.2], "%d x %d" % (w, h))
    print("%d x %d: history %s of %d" % (w, h, [int(i["history"].sum()) for i in infos], w * h))
    if w * h > 1:
        assert all(i["history"].sum() >= w * h // 2 for i in infos)


def test_device_route_equals_the_context_route(gpu_ctx_ok):
    import torch
    ex = tbuild("cornell", W, H)
    it, ctx = ex.integrator, ex.scene.ctx
    dev = torch.device("cuda", ctx.device_id)
    render_view(ex, 0, 0.0)
    it.temporal_accumulate()
    hist_h, hist_m = it.temporal_to_torch()
    hist_a, cam_prev = it.aov_to_torch(), te.Cam(ex.cam)
    got_h, got_m = it.temporal_to_numpy()
    check(hist_h.cpu().numpy(), got_h, "temporal_to_torch hdr", True); check(hist_m.cpu().numpy(), got_m, "temporal_to_torch moments", True)
    hdr, aov, mom, cam = render_view(ex, 1, YAW_STEP)
    cur = [torch.from_numpy(hdr).to(dev), it.aov_to_torch(), it.moments_to_torch()]
    keep = [t.clone() for t in cur + [hist_h, hist_a, hist_m]]
    for params in ({}, dict(max_history=3.0, sigma_n=0.6, sigma_z=0.05)):
        it.temporal_reset()                                    # back to the history of view 1: accumulate it again from the tensors' twin on the context
        render_view(ex, 0, 0.0)
        it.temporal_accumulate()
        render_view(ex, 1, YAW_STEP)
        it.temporal_accumulate(**params)
        ctx_h, ctx_m = it.temporal_to_numpy()
        for c in (ctx, None):
            for cams in ((ex.cam, cam_prev), ((cam.view_np[0], cam.view_inv_np[0], cam.eye_np[0], cam.fx, cam.fy, cam.cx, cam.cy), cam_prev)):
                out_h, out_m = ti_raytrace_amd.temporal_accumulate(*cur, hist_h, hist_a, hist_m, *cams, ctx=c, **params)
                check(out_h.cpu().numpy(), ctx_h, ("device route hdr", params), True); check(out_m.cpu().numpy(), ctx_m, ("device route moments", params), True)
        want_h, want_m = te.accumulate(hdr, aov, mom, got_h, hist_a.cpu().numpy(), got_m, cam, cam_prev, **params)
        check(ctx_h, want_h, ("hdr", params)); check(ctx_m, want_m, ("moments", params))
    for t, k in zip(cur + [hist_h, hist_a, hist_m], keep):     # the inputs are only read
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    th, tm = it.temporal_to_torch()
    nh, nm = it.temporal_to_numpy()
    check(th.cpu().numpy(), nh, "temporal_to_torch hdr", True); check(tm.cpu().numpy(), nm, "temporal_to_torch moments", True)


def test_denoise_temporal_is_denoise_var_over_the_accumulated_film(gpu_ctx_ok):
    ex = tbuild("cornell", W, H)
    it = ex.integrator
    views, (acc_h, acc_m), _ = accumulate_views(ex, [0.0, 0.05, 0.1], "denoise")
    aov = views[-1][1]
    for params in ({}, dict(levels=3, sigma_c=0.7, sigma_n=0.6, sigma_z=0.05)):
        it.denoise_temporal(**params)
        got = it.denoised.to_numpy()
        check(got, dv.denoise_var_expected(acc_h, aov, acc_m, **params), ("tirt_temporal_denoise_var", params))
        check(it.denoised_to_torch().cpu().numpy(), got, "denoised_to_torch", True)
    it.denoise_var()                                           # the film's own filter writes the same buffer from the film's own records
    check(it.denoised.to_numpy(), dv.denoise_var_expected(*views[-1][:3]), "tirt_denoise_var afterwards")
    assert not np.array_equal(it.denoised.to_numpy(), got)


def test_nothing_else_moves_and_the_history_lives_as_stated(gpu_ctx_ok):
    on, off = tbuild("cornell", W, H), tbuild("cornell", W, H, temporal=False)
    it, ctx = on.integrator, on.scene.ctx
    for k, yaw in enumerate((0.0, 0.05)):
        a, b = render_view(on, k, yaw), render_view(off, k, yaw)
        it.temporal_accumulate()
        it.denoise_temporal()
        it.denoise_var(); off.integrator.denoise_var()
        for x, y, what in zip(a[:3], b[:3], ("hdr", "aov", "moments")):
            check(x, y, (what, "rendered beside the history, view", k), True)
        check(it.hdr.to_numpy(), b[0], "hdr after the accumulate", True); check(it.aov_to_numpy(), b[1], "aov after the accumulate", True)
        check(it.moments_to_numpy(), b[2], "moments after the accumulate", True)
        check(it.denoised.to_numpy(), off.integrator.denoised.to_numpy(), "denoise_var", True)
    with pytest.raises(_native.TirtError, match="not enabled"):
        off.integrator.scene.ctx.temporal_accumulate()
    # tirt_film_clear keeps the history
    before = it.temporal_to_numpy()
    ctx.film_clear()
    after = it.temporal_to_numpy()
    check(after[0], before[0], "hdr history over a film_clear", True); check(after[1], before[1], "moment history over a film_clear", True)
    assert (it.moments_to_numpy().view(np.uint32) == 0).all()
    # temporal_reset and a geometry update empty it: nothing to download, and the next accumulate is a first one
    for how in ("reset", "update_vertices"):
        if how == "reset":
            it.temporal_reset()
        else:
            on.scene.update_vertices(np.ascontiguousarray(on.scene.vertex_np[:, 0:3], np.float32))      # the same positions: the world stood still, the library cannot know
        with pytest.raises(_native.TirtError, match="nothing accumulated"):
            it.temporal_to_numpy()
        with pytest.raises(_native.TirtError, match="nothing accumulated"):
            it.denoise_temporal()
        hdr, aov, mom, _ = render_view(on, 7, 0.1)
        it.temporal_accumulate()
        got_h, got_m = it.temporal_to_numpy()
        check(got_h, hdr, ("first accumulate after", how), True); check(got_m, mom, ("first accumulate after", how), True)
    # tirt_film_create disables it
    ctx.film_create(W, H)
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.temporal_accumulate()
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.temporal_download(W, H)


def test_refusals(gpu_ctx_ok):
    import torch
    fresh = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.temporal_enable(True)
        fresh.film_create(W, H)
        with pytest.raises(_native.TirtError, match="feature buffers not enabled"):
            fresh.temporal_enable(True)
        fresh.aov_enable(True)
        with pytest.raises(_native.TirtError, match="moment buffers not enabled"):
            fresh.temporal_enable(True)
        fresh.film_create(W, H, 0, 2, 100)                     # a rank's partial film
        fresh.aov_enable(True); fresh.moments_enable(True)
        with pytest.raises(_native.TirtError, match="tile_count"):
            fresh.temporal_enable(True)
        with pytest.raises(_native.TirtError, match="not enabled"):
            fresh.temporal_reset()
    finally:
        fresh.close()
    ex = tbuild("cornell", W, H)
    it, ctx = ex.integrator, ex.scene.ctx
    for call in (lambda: ctx.temporal_download(W, H), lambda: ctx.temporal_denoise_var(), lambda: it.temporal_to_torch()):
        with pytest.raises(_native.TirtError, match="nothing accumulated"):
            call()
    for off in (ctx.aov_enable, ctx.moments_enable):
        with pytest.raises(_native.TirtError, match="temporal accumulation is on"):
            off(False)
    render_view(ex, 0, 0.0)
    for name in ("max_history", "sigma_n", "sigma_z"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(_native.TirtError, match="finite and > 0"):
                ctx.temporal_accumulate(**{name: v})
    with pytest.raises(_native.TirtError, match="nothing accumulated"):          # a refused accumulate accumulated nothing
        ctx.temporal_download(W, H)
    ctx.temporal_accumulate()
    with pytest.raises(_native.TirtError, match="levels"):
        ctx.temporal_denoise_var(levels=9)
    ctx.temporal_enable(False)                                 # off: the records may go again
    ctx.aov_enable(False); ctx.aov_enable(True)
    # the device-memory entry
    dev = torch.device("cuda", ctx.device_id)
    z3 = lambda: torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    z8 = lambda: torch.zeros((W, H, 8), dtype=torch.float32, device=dev)
    t = [z3(), z8(), z8(), z3(), z8(), z8(), z3(), z8()]      # hdr_c aov_c mom_c hdr_h aov_h mom_h | hdr_o mom_o
    ptrs = [x.data_ptr() for x in t]
    cam = te.Cam(ex.cam)
    run = lambda p, w=W, h=H, **kw: ctx.temporal_device(*p[:6], cam, cam, p[6], p[7], w, h, **kw)
    run(ptrs)
    host = np.zeros((W, H, 8), np.float32)
    for k in range(8):
        args = list(ptrs); args[k] = host.ctypes.data
        with pytest.raises(_native.TirtError, match="not device memory"):
            run(args)
        args[k] = 0
        with pytest.raises(_native.TirtError, match="null"):
            run(args)
    for k in range(6):                                         # an output on an input, hdr_o on mom_o, an output that begins inside an input
        for o in (6, 7):
            args = list(ptrs); args[o] = ptrs[k]
            with pytest.raises(_native.TirtError, match="overlaps"):
                run(args)
    for args in (ptrs[:6] + [ptrs[7], ptrs[7]], ptrs[:6] + [ptrs[6], ptrs[2] + 16 * W * H]):
        with pytest.raises(_native.TirtError, match="overlaps"):
            run(args)
    for k in (1, 2, 4, 5, 7):
        args = list(ptrs); args[k] = ptrs[k] + 4
        with pytest.raises(_native.TirtError, match="aligned"):
            run(args, h=H - 1)
    with pytest.raises(_native.TirtError, match="bad size"):
        run(ptrs, w=0)
    for name in ("max_history", "sigma_n", "sigma_z"):
        with pytest.raises(_native.TirtError, match="finite and > 0"):
            run(ptrs, **{name: float("nan")})
    for bad, exc in ((host, TypeError), (t[2].double(), TypeError), (t[2].cpu(), TypeError), (t[2][:, :, :4], ValueError), (t[2][:12], ValueError)):
        with pytest.raises(exc):
            ti_raytrace_amd.temporal_accumulate(t[0], t[1], bad, t[3], t[4], t[5], cam, cam, ctx=ctx)


def test_an_adaptively_sampled_view_merges_with_each_pixels_own_count(gpu_ctx_ok):
    ex = tbuild("cornell", W, H)
    it, ctx = ex.integrator, ex.scene.ctx
    v1 = render_view(ex, 0, 0.0)
    it.temporal_accumulate()
    render_view(ex, 1, 0.05)
    ex.cam.frame = 2; ex.cam.frame_cpu[0] = 2
    res = it.render_adaptive(0.02, 8, min_samples=2, pass_frames=2)
    hdr, aov, mom, cam = it.hdr.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy(), te.Cam(ex.cam)
    counts = np.unique(mom[:, :, 0] + mom[:, :, 7])
    print("adaptive view:", res, "sample counts", counts.tolist())
    assert len(counts) >= 2 and counts.min() == 2 and counts.max() == 8
    n_listed = ctx.pixel_set_from_moments(0.02, 2, 16)         # an installed set is only read
    listed = ctx.pixel_set_download()
    it.temporal_accumulate()
    want_h, want_m, info = te.accumulate(hdr, aov, mom, v1[0], v1[1], v1[2], cam, v1[3], want_info=True)
    got_h, got_m = it.temporal_to_numpy()
    check(got_h, want_h, "hdr"); check(got_m, want_m, "moments")
    assert len(np.unique(got_m[:, :, 0][info["history"]])) >= 2 and info["history"].sum() >= W * H // 2
    assert n_listed == len(listed) and np.array_equal(ctx.pixel_set_download(), listed)
    it.pixel_set(None)
    check(it.hdr.to_numpy(), hdr, "hdr", True); check(it.moments_to_numpy(), mom, "moments", True)
