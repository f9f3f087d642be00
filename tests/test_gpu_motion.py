"""The motion records on the device (csrc/tirt_temporal.hip k_motion_resolve and k_temporal<true>, csrc/tirt_dynamic.hip's snapshot, through
tirt_motion_*, PathTrace(temporal=True, motion=True) and ti_raytrace_amd.temporal_accumulate(motion=)): bit for bit against the numpy restatement
(tests/motion_expected.py) on the centre-ray hits of the CPU oracle and the vertex rows the device itself holds before and after the update -- one box
of the Cornell box translated by about 1.5 pixels, the other turned about its vertical axis; without the records the history is gone; nothing moved
means nothing changed; two updates are one; the device-memory route; lifecycle.  Films are 24 x 20 with 2 frames per view unless a case says otherwise;
tests/test_motion_host.py holds the two moves to the conditions asserted here on the oracle's own films."""
import numpy as np
import pytest

import motion_expected as mx
import temporal_expected as te
import ti_raytrace_amd
from test_gpu_aov import build, check, oracle_of
from test_gpu_temporal import render_view
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
W, H = 24, 20


def mbuild(w, h, motion=True):
    return build("cornell", w, h, 2, aov=True, moments=True, temporal=True, motion=motion)


def rows_of(ex):
    return ex.scene.ctx.vertex_download(ex.scene.vertex_count)


def update(ex, tris, new):
    """Scene.update_vertices on the triangles `tris` (a run of consecutive triangles: a block of the Cornell box is one)"""
    assert np.array_equal(tris, np.arange(tris[0], tris[0] + len(tris)))
    ex.scene.update_vertices(np.ascontiguousarray(new, np.float32).reshape(-1, 3), first_vertex=3 * int(tris[0]))


def first_view(ex):
    """view 0 rendered and accumulated: (its records and camera, the accumulated (hdr, mom), the vertex rows it saw)"""
    v0 = render_view(ex, 0, 0.0)
    ex.integrator.temporal_accumulate()
    return v0, ex.integrator.temporal_to_numpy(), rows_of(ex)


def expected_record(ex, rows1, rows0, w, h):
    """the restatement on the oracle's centre-ray hits of the geometry as it stands (the host mirrors follow Scene.update_vertices)"""
    orc = oracle_of(ex, "cornell")
    return mx.record(*mx.centre_hits(orc, ex.cam, w, h), ex.scene.primitive_np, rows1, rows0, w, h)


def move_and_accumulate(case, w, h, motion):
    """One body for both settings: view 0, the move of `case`, view 1 from the same camera (render_view clears the film in between), the accumulate.
    With motion records the history survives the update and everything is held to the restatement; without them it is gone after the update."""
    ex = mbuild(w, h, motion)
    it = ex.integrator
    v0, acc0, rows0 = first_view(ex)
    tris, new = mx.move(case, rows0, ex.cam, w)
    update(ex, tris, new)
    rows1 = rows_of(ex)
    check(rows1, mx.moved_rows(rows0, tris, new), "vertex rows after the update")
    if not motion:
        with pytest.raises(_native.TirtError, match="nothing accumulated"):
            it.temporal_to_numpy()
        with pytest.raises(ValueError, match="motion=True"):
            it.motion_to_numpy()
        return None
    check(it.temporal_to_numpy()[0], acc0[0], "the history over the update", True)
    v1 = render_view(ex, 1)
    it.temporal_accumulate()
    rec = it.motion_to_numpy()
    check(rec, expected_record(ex, rows1, rows0, w, h), (case, "motion records"))
    check(it.motion.to_numpy(), rec, "the field", True); check(it.motion_to_torch().cpu().numpy(), rec, "motion_to_torch", True)
    want_h, want_m, info = mx.accumulate_mv(*v1[:3], acc0[0], v0[1], acc0[1], v1[3], v0[3], rec, want_info=True)
    got_h, got_m = it.temporal_to_numpy()
    check(got_h, want_h, (case, "hdr")); check(got_m, want_m, (case, "moments"))
    static = mx.accumulate_mv(*v1[:3], acc0[0], v0[1], acc0[1], v1[3], v0[3], np.zeros_like(rec), want_info=True)
    return ex, rec, info, static, (got_h, got_m)


# ---- 1. records and accumulation against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["translate", "rotate"])
def test_a_moved_box_keeps_its_history(gpu_ctx_ok, case):
    ex, rec, info, static, got = move_and_accumulate(case, W, H, True)
    taps_differ = (info["tap_i0"] != static[2]["tap_i0"]) | (info["tap_j0"] != static[2]["tap_j0"])
    print("%s: history %d of %d (static reprojection %d), rejected %d, pixels whose first tap differs %d, records that are not zero %d"
          % (case, info["history"].sum(), W * H, static[2]["history"].sum(), info["rejected"].sum(), taps_differ.sum(), (rec[:, :, 0:3] != 0).any(axis=2).sum()))
    assert info["history"].sum() >= W * H // 2 and info["rejected"].sum() >= 1 and taps_differ.sum() >= 1
    assert not np.array_equal(got[1], static[1])
    if case == "rotate":
        assert (rec[:, :, 4:7] != 0).any()
    st = ex.scene.ctx.stats()
    assert st["stack_overflow"] == 0 and st["rays_closest"] >= W * H


@pytest.mark.parametrize("w,h", [(1, 1), (13, 7), (65, 63)], ids=["1x1", "13x7", "65x63"])
def test_shapes(gpu_ctx_ok, w, h):
    ex, rec, info, static, got = move_and_accumulate("translate", w, h, True)
    print("%d x %d: history %d of %d, records that are not zero %d" % (w, h, info["history"].sum(), w * h, (rec[:, :, 0:3] != 0).any(axis=2).sum()))
    if w * h > 1:
        assert info["history"].sum() >= w * h // 2 and (rec[:, :, 0:3] != 0).any()


# ---- 2. without the feature the history is gone ---------------------------------------------------------------------------------------------------
def test_without_motion_records_the_update_empties_the_history(gpu_ctx_ok):
    assert move_and_accumulate("translate", W, H, False) is None


# ---- 3. nothing moved means nothing changed -------------------------------------------------------------------------------------------------------
def test_nothing_moved_means_nothing_changed(gpu_ctx_ok):
    on, off = mbuild(W, H, True), mbuild(W, H, False)
    for k, yaw in enumerate((0.0, 0.05, 0.1)):
        a, b = render_view(on, k, yaw), render_view(off, k, yaw)
        for x, y, what in zip(a[:3], b[:3], ("hdr", "aov", "moments")):
            check(x, y, (what, "rendered with motion records enabled, view", k), True)
        on.integrator.temporal_accumulate(); off.integrator.temporal_accumulate()
        for x, y, what in zip(on.integrator.temporal_to_numpy(), off.integrator.temporal_to_numpy(), ("hdr", "moments")):
            check(x, y, (what, "accumulated, view", k), True)
        assert (on.integrator.motion_to_numpy().view(np.uint32) == 0).all()
    # an update that writes the same positions back marks the geometry as moved: the records come from the rays, and they say that nothing moved
    it = on.integrator
    acc, prev = it.temporal_to_numpy(), a
    rows0 = rows_of(on)
    on.scene.update_vertices(np.ascontiguousarray(rows0[:, 0:3]))
    rows1 = rows_of(on)
    check(np.ascontiguousarray(rows1[:, 0:3]), np.ascontiguousarray(rows0[:, 0:3]), "positions written back", True)      # (the face normals are made again, from the f32 positions: a last bit may differ)
    v = render_view(on, 3, 0.15)
    it.temporal_accumulate()
    rec = it.motion_to_numpy()
    check(rec, expected_record(on, rows1, rows0, W, H), "records of an update that moved nothing")
    assert (rec[:, :, 3] == 1).sum() > W * H // 2 and (rec[:, :, [0, 1, 2, 7]] == 0).all() and np.abs(rec[:, :, 4:7]).max() <= 1e-6
    want_h, want_m, info = mx.accumulate_mv(*v[:3], acc[0], prev[1], acc[1], v[3], prev[3], rec, want_info=True)
    st_h, st_m, st_info = te.accumulate(*v[:3], acc[0], prev[1], acc[1], v[3], prev[3], want_info=True)
    got_h, got_m = it.temporal_to_numpy()
    check(got_h, want_h, "hdr"); check(got_m, want_m, "moments")
    assert np.array_equal(info["history"], st_info["history"]) and info["history"].sum() >= W * H // 2


# ---- 4. two updates between accumulates are one update to the final positions ---------------------------------------------------------------------
def test_two_updates_between_accumulates_equal_one(gpu_ctx_ok):
    results = []
    for steps in (2, 1):
        ex = mbuild(W, H, True)
        it = ex.integrator
        v0, acc0, rows0 = first_view(ex)
        tris, new = mx.move("translate", rows0, ex.cam, W)
        if steps == 2:
            old = rows0[:, 0:3].reshape(-1, 3, 3)[tris]
            update(ex, tris, (old + (new - old) * np.float32(0.5)).astype(np.float32))
        update(ex, tris, new)
        render_view(ex, 1)
        it.temporal_accumulate()
        results.append((rows_of(ex), it.motion_to_numpy()) + it.temporal_to_numpy())
    for x, y, what in zip(results[0], results[1], ("vertex rows", "motion records", "hdr", "moments")):
        check(x, y, what, True)
    assert (results[0][1][:, :, 0:3] != 0).any()


# ---- 5. the torch route -----------------------------------------------------------------------------------------------------------------------------
def test_device_route_equals_the_context_route(gpu_ctx_ok):
    import torch
    ex = mbuild(W, H, True)
    it, ctx = ex.integrator, ex.scene.ctx
    dev = torch.device("cuda", ctx.device_id)
    v0, acc0, rows0 = first_view(ex)
    hist_h, hist_m = it.temporal_to_torch()
    hist_a, cam_prev = it.aov_to_torch(), v0[3]
    tris, new = mx.move("translate", rows0, ex.cam, W)
    update(ex, tris, new)
    hdr, aov, mom, cam = render_view(ex, 1)
    cur = [torch.from_numpy(hdr).to(dev), it.aov_to_torch(), it.moments_to_torch()]
    it.temporal_accumulate()
    motion = it.motion_to_torch()
    ctx_h, ctx_m = it.temporal_to_numpy()
    keep = [t.clone() for t in cur + [hist_h, hist_a, hist_m, motion]]
    for c in (ctx, None):
        out_h, out_m = ti_raytrace_amd.temporal_accumulate(*cur, hist_h, hist_a, hist_m, cam, cam_prev, ctx=c, motion=motion)
        check(out_h.cpu().numpy(), ctx_h, "device route hdr", True); check(out_m.cpu().numpy(), ctx_m, "device route moments", True)
    plain_h, plain_m = ti_raytrace_amd.temporal_accumulate(*cur, hist_h, hist_a, hist_m, cam, cam_prev, ctx=ctx)
    assert not np.array_equal(plain_m.cpu().numpy(), ctx_m)          # without the records it is another accumulation
    for t, k in zip(cur + [hist_h, hist_a, hist_m, motion], keep):   # the inputs are only read
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    # the refusals of tirt_temporal_device hold for the new argument
    z3 = lambda: torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    z8 = lambda: torch.zeros((W, H, 8), dtype=torch.float32, device=dev)
    t = [z3(), z8(), z8(), z3(), z8(), z8(), z3(), z8(), z8()]      # hdr_c aov_c mom_c hdr_h aov_h mom_h | hdr_o mom_o | motion
    ptrs = [x.data_ptr() for x in t]
    run = lambda p, w=W, h=H: ctx.motion_temporal_device(*p[:6], cam, cam, p[6], p[7], w, h, p[8])
    run(ptrs)
    host = np.zeros((W, H, 8), np.float32)
    with pytest.raises(_native.TirtError, match="not device memory"):
        run(ptrs[:8] + [host.ctypes.data])
    with pytest.raises(_native.TirtError, match="null"):
        run(ptrs[:8] + [0])
    with pytest.raises(_native.TirtError, match="aligned"):
        run(ptrs[:8] + [ptrs[8] + 4], h=H - 1)
    for o in (6, 7):
        args = list(ptrs); args[o] = ptrs[8]
        with pytest.raises(_native.TirtError, match="overlaps"):
            run(args)
    with pytest.raises(_native.TirtError, match="overlaps"):
        run(ptrs[:7] + [ptrs[8] + 16 * W * H, ptrs[8]])              # an output that begins inside the records
    for bad, exc in ((host, TypeError), (t[8].double(), TypeError), (t[8].cpu(), TypeError), (t[8][:, :, :4], ValueError), (t[8][:12], ValueError)):
        with pytest.raises(exc):
            ti_raytrace_amd.temporal_accumulate(*t[:6], cam, cam, ctx=ctx, motion=bad)


# ---- 6. lifecycle -------------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle(gpu_ctx_ok):
    fresh = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.motion_enable(True)
        fresh.film_create(W, H)
        with pytest.raises(_native.TirtError, match="temporal accumulation not enabled"):
            fresh.motion_enable(True)
        with pytest.raises(_native.TirtError, match="motion records not enabled"):
            fresh.motion_download(W, H)
    finally:
        fresh.close()
    ex = mbuild(W, H, True)
    it, ctx, sc = ex.integrator, ex.scene.ctx, ex.scene
    with pytest.raises(_native.TirtError, match="motion records are on"):
        ctx.temporal_enable(False)
    with pytest.raises(_native.TirtError, match="nothing accumulated"):
        ctx.motion_download(W, H)
    v0, acc0, rows0 = first_view(ex)
    assert (ctx.motion_download(W, H).view(np.uint32) == 0).all()      # a first accumulate: zeros
    tris, new = mx.move("translate", rows0, ex.cam, W)
    pos = np.ascontiguousarray(new, np.float32).reshape(-1, 3)
    # a refused update changes nothing: the next accumulate is a static one
    bad = pos.copy(); bad[4, 1] = np.nan
    with pytest.raises(_native.TirtError, match="NaN or infinite"):
        ctx.vertex_update(3 * int(tris[0]), len(pos), bad.ctypes.data, 3, 0, 3)
    it.temporal_accumulate()
    assert (ctx.motion_download(W, H).view(np.uint32) == 0).all()
    acc0 = it.temporal_to_numpy()
    # between an update and the rebuild the accumulate is refused, and it has changed nothing; after the rebuild it runs
    ctx.vertex_update(3 * int(tris[0]), len(pos), pos.ctypes.data, 3, 0, 3)
    with pytest.raises(_native.TirtError, match="tirt_lbvh_build must follow the vertex update"):
        ctx.temporal_accumulate()
    check(it.temporal_to_numpy()[1], acc0[1], "the history over a refused accumulate", True)
    ctx.lbvh_build()
    # tirt_film_clear keeps both the history and the mark: the accumulate further down still goes through the records
    ctx.film_clear()
    check(it.temporal_to_numpy()[0], acc0[0], "hdr history over a film_clear after an update", True)
    check(it.temporal_to_numpy()[1], acc0[1], "moment history over a film_clear after an update", True)
    assert (it.moments_to_numpy().view(np.uint32) == 0).all()
    ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
    it.seed = 11
    ctx.pt_rgb_render(0, 2, it.seed, 15, 64, 0)
    # what the accumulate reads it only reads: the film, the records, the denoised film, an installed pixel set
    it.denoise_var()
    n_listed = ctx.pixel_set_from_moments(0.02, 2, 16)
    listed = ctx.pixel_set_download()
    before = (it.hdr.to_numpy(), it.rgb_film.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy(), it.denoised.to_numpy())
    ctx.temporal_accumulate()
    rec = ctx.motion_download(W, H)
    assert (rec[:, :, 0:3] != 0).any()
    after = (it.hdr.to_numpy(), it.rgb_film.to_numpy(), it.aov_to_numpy(), it.moments_to_numpy(), it.denoised.to_numpy())
    for x, y, what in zip(before, after, ("hdr", "rgb_film", "aov", "moments", "denoised")):
        check(x, y, (what, "over an accumulate with motion records"), True)
    assert n_listed == len(listed) and np.array_equal(ctx.pixel_set_download(), listed)
    it.pixel_set(None)
    # temporal_reset and scene_upload clear the mark and the history: the next accumulate is a first one, its records zeros
    back = np.ascontiguousarray(rows0[3 * int(tris[0]):3 * int(tris[0]) + len(pos), 0:3])
    for how in ("reset", "scene_upload"):
        ctx.vertex_update(3 * int(tris[0]), len(pos), (back if how == "reset" else pos).ctypes.data, 3, 0, 3)      # marks the geometry as moved
        if how == "reset":
            it.temporal_reset()
        else:
            ctx.scene_upload(rows0, sc.primitive_np, sc.material_np, sc.shape_np, sc.light_np, sc.light_count, sc.minboundarynp, sc.maxboundarynp)
        for call in (it.temporal_to_numpy, it.motion_to_numpy):
            with pytest.raises(_native.TirtError, match="nothing accumulated"):
                call()
        ctx.lbvh_build()
        hdr, aov, mom, _ = render_view(ex, 5, 0.0)
        it.temporal_accumulate()
        got_h, got_m = it.temporal_to_numpy()
        check(got_h, hdr, ("first accumulate after", how), True); check(got_m, mom, ("first accumulate after", how), True)
        assert (it.motion_to_numpy().view(np.uint32) == 0).all()
    # motion off: the records are gone, the history may go too; tirt_film_create disables both
    ctx.motion_enable(False)
    with pytest.raises(_native.TirtError, match="motion records not enabled"):
        ctx.motion_download(W, H)
    it.temporal_to_numpy()                                          # nothing had moved since the last accumulate: the history stays
    ctx.motion_enable(True)
    ctx.film_create(W, H)
    with pytest.raises(_native.TirtError, match="motion records not enabled"):
        ctx.motion_download(W, H)
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.temporal_accumulate()
