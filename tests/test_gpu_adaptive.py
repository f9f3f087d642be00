"""Adaptive sampling of the path tracer on the device (csrc/tirt_adaptive.hip through tirt_pixel_set_* / tirt_pt_rgb_render_adaptive, PathTrace.pixel_set and
PathTrace.render_adaptive): every pixel's film bit for bit the oracle's film of that pixel's own sample count; stop counts, moment and feature records
against the dense device path and the numpy restatement (tests/adaptive_expected.py); the list tirt_pixel_set_from_moments makes, order included, on ragged,
blocked two-rank and 1 x 1 films; a caller's own set; the split across ranks; the dense path unmoved; lifecycle and refusals.

Cornell 24 x 20, seed 5, threshold 0.3, at least 4 and at most 32 samples in passes of 4 (tests/test_adaptive_host.py recomputes on the CPU that this
spreads the stop counts)."""
import collections
import ctypes as C

import numpy as np
import pytest

import adaptive_expected as ax
import aov_expected as ae
import moments_expected as me
from common import same_bits
from test_gpu_aov import SEED, build, check, oracle_of, rewind
from ti_raytrace_amd import Debug, _native, scenes

pytestmark = pytest.mark.gpu
W, H = 24, 20
THR, MIN, MAX, PASS = 0.3, 4, 32, 4
DEPTH, STACK = 15, 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state(ctx, w, h, aov=True):
    """(hdr, moments, feature buffers) of a context, downloaded"""
    return ctx.film_download(w, h)[0], ctx.moments_download(w, h), ctx.aov_download(w, h) if aov else None


def dense_boundaries(ctx, w, h, aov=True):
    """{m: (hdr, moments, feature buffers) after m dense frames} for m = 0, 4, .. 32, rendered in 4-frame calls"""
    out = {0: state(ctx, w, h, aov)}
    for m in range(PASS, MAX + 1, PASS):
        ctx.pt_rgb_render(m - PASS, PASS, SEED, DEPTH, STACK, 0)
        out[m] = state(ctx, w, h, aov)
    return out


@pytest.fixture(scope="module")
def run(gpu_ctx_ok):
    """one adaptive render and one dense render in 4-frame calls of the same scene, shared by tests 1 to 3"""
    ex = build("cornell", W, H, MAX, aov=True, moments=True)
    result = ex.integrator.render_adaptive(THR, MAX, MIN, PASS)
    hdr, mom, aov = state(ex.scene.ctx, W, H)
    count = ex.integrator.sample_count.to_numpy()
    assert ex.scene.ctx.pixel_set_download() is None and ex.cam.frame == 0          # the driver leaves no set behind and advances nothing
    dense_ex = build("cornell", W, H, MAX, aov=True, moments=True)
    dense = dense_boundaries(dense_ex.scene.ctx, W, H)
    n_p, info = ax.simulate({m: d[1] for m, d in dense.items()}, THR, MIN, MAX, PASS)
    hist = dict(sorted(collections.Counter(count.reshape(-1).astype(int).tolist()).items()))
    print("stop counts on the device:", hist, result)
    return dict(ex=ex, result=result, hdr=hdr, mom=mom, aov=aov, count=count, dense=dense, n_p=n_p, info=info, hist=hist)


# ---- 1. the film, bit for bit, against the oracle ------------------------------------------------------------------------------------------------
def test_film_equals_the_oracles_film_of_each_pixels_own_sample_count(run):
    orc = oracle_of(run["ex"], "cornell")
    count = run["count"]
    assert count.dtype == np.float32 and (count == np.round(count)).all()
    for n in sorted(set(count.reshape(-1).astype(int).tolist())):
        assert 1 <= n <= MAX
        want, _ = orc.render(W, H, 0, n, seed=SEED)
        at = count == n
        assert same_bits(run["hdr"][at], want[at]), (n, int(at.sum()), int((run["hdr"][at] != want[at]).any(axis=1).sum()))


# ---- 2. records and stop counts against the dense device path and numpy ---------------------------------------------------------------------------
def test_stop_counts_and_records_equal_the_dense_path_at_each_pixels_count(run):
    n_p, dense = run["n_p"], run["dense"]
    assert np.array_equal(run["count"].astype(np.int64), n_p), "pixels whose stop count differs: %d" % int((run["count"] != n_p).sum())
    for m in sorted(set(n_p.reshape(-1).tolist())):
        at = n_p == m
        d_hdr, d_mom, d_aov = dense[m]
        assert np.array_equal(bits(run["mom"][at]), bits(d_mom[at])), ("moments", m)
        assert np.array_equal(bits(run["aov"][at]), bits(d_aov[at])), ("feature buffers", m)
        assert np.array_equal(bits(run["hdr"][at]), bits(d_hdr[at])), ("hdr", m)
    assert run["result"] == run["info"]
    assert run["result"]["pixel_samples"] == int(n_p.sum()) and run["result"]["pixels_at_max"] == int((n_p == MAX).sum())
    assert run["result"]["passes"] == MAX // PASS and run["result"]["frames"] == MAX


# ---- 3. the test shows something ----------------------------------------------------------------------------------------------------------------
def test_the_stop_counts_are_spread(run):
    hist, P = run["hist"], W * H
    print(hist)
    at_min, at_max = hist.get(MIN, 0), hist.get(MAX, 0)
    assert len(hist) >= 5
    assert at_min >= 0.1 * P and at_max >= 0.1 * P and P - at_min - at_max >= 0.1 * P
    assert run["result"]["pixel_samples"] < MAX * P


# ---- 4. tirt_pixel_set_from_moments alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ranks,ts", [(24, 20, 1, 4096), (32, 24, 2, 8 * 24), (1, 1, 1, 4096)], ids=["24x20", "32x24-two-blocked-ranks", "1x1"])
def test_the_list_from_the_moments_equals_numpy_element_for_element(gpu_ctx_ok, w, h, ranks, ts):
    ex = build("cornell", w, h, MAX, aov=False, moments=True)
    ctx = ex.scene.ctx
    for rank in range(ranks):
        ctx.film_create(w, h, rank, ranks, ts)
        ctx.moments_enable(True)
        order = ax.local_order(w, h, rank, ranks, ts)
        if ranks > 1:
            assert (np.diff(order) < 0).any()                     # blocked tiles: local order is not pixel order
        assert ctx.pixel_set_from_moments(THR, MIN, MAX) == len(order)          # nothing rendered: every own pixel, in local order
        assert np.array_equal(ctx.pixel_set_download(), order)
        ctx.pixel_set_clear()
        begin = 0
        for frames in (4, 12):
            ctx.pt_rgb_render(begin, frames - begin, SEED, DEPTH, STACK, 0)
            begin = frames
            rec = ctx.moments_download(w, h)
            for thr in (THR, 0.05, 0.0):
                want = ax.select(rec, thr, MIN, MAX, order=order)
                count = ctx.pixel_set_from_moments(thr, MIN, MAX)
                got = ctx.pixel_set_download()
                print(w, h, "rank", rank, "after", frames, "frames, threshold", thr, ":", count, "of", len(order))
                assert got.dtype == np.int32 and count == len(got) == len(want)
                assert np.array_equal(got, want), "first difference at %s" % np.flatnonzero(got != want)[:4].tolist()
                ctx.pixel_set_clear()
            if w * h > 1:
                assert 0 < len(ax.select(rec, THR, MIN, MAX, order=order)) < len(order)
            # the bounds: everything is listed below min_samples, nothing at max_samples
            assert np.array_equal(ax.select(rec, THR, frames + 1, MAX, order=order), order) and ctx.pixel_set_from_moments(THR, frames + 1, MAX) == len(order)
            assert np.array_equal(ctx.pixel_set_download(), order)
            assert ctx.pixel_set_from_moments(THR, 1, frames) == 0 and len(ctx.pixel_set_download()) == 0
            ctx.pixel_set_clear()


# ---- 5. a caller's set ------------------------------------------------------------------------------------------------------------------------------
def patch_list():
    """a 5 x 5 patch and three scattered pixels; a 24 x 20 film is one linear tile, so local order is ascending p"""
    px = [i * H + j for i in range(3, 8) for j in range(4, 9)] + [0, 12 * H + 19, 23 * H + 19]
    return np.array(sorted(px), np.int32)


@pytest.mark.parametrize("name,pixels", [("patch", patch_list()), ("64", np.arange(100, 164, dtype=np.int32)), ("one", np.array([237], np.int32))])
def test_a_callers_set_renders_its_pixels_and_touches_no_other(gpu_ctx_ok, name, pixels):
    N = 8
    ex = build("cornell", W, H, N, aov=True, moments=True)
    ctx, it = ex.scene.ctx, ex.integrator
    orc = oracle_of(ex, "cornell")
    want, _ = orc.render(W, H, 0, N, seed=SEED)
    dense = build("cornell", W, H, N, aov=True, moments=True)
    dense.scene.ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
    d_hdr, d_mom, d_aov = state(dense.scene.ctx, W, H)
    inside = np.zeros(W * H, bool); inside[pixels] = True
    inside = inside.reshape(W, H)
    it.pixel_set(pixels)
    assert np.array_equal(ctx.pixel_set_download(), pixels)

    def one_call():
        ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)

    def frame_by_frame():
        for fr in range(N):
            ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)

    for lanes in (1, 4):
        ctx.set_option("overlap_lanes", lanes)
        for merge in (32 << 20, 0):
            ctx.set_option("merge_paths", merge)
            for what, render in (("one call", one_call), ("eight calls", frame_by_frame)):
                ctx.film_clear()
                assert np.array_equal(ctx.pixel_set_download(), pixels)          # film_clear leaves the set alone
                render()
                hdr, mom, aov = state(ctx, W, H)
                tag = (name, what, lanes, merge)
                assert same_bits(hdr[inside], want[inside]), tag
                assert np.array_equal(bits(hdr[inside]), bits(d_hdr[inside])) and np.array_equal(bits(mom[inside]), bits(d_mom[inside])), tag
                assert np.array_equal(bits(aov[inside]), bits(d_aov[inside])), tag
                assert (mom[inside][:, 0] + mom[inside][:, 7] == N).all()
                assert (bits(hdr[~inside]) == 0).all() and (bits(mom[~inside]) == 0).all() and (bits(aov[~inside]) == 0).all(), tag
    assert (want[inside] != 0).any()
    # the empty set: a call that does nothing
    ctx.film_clear()
    ctx.pixel_set_upload([])
    assert len(ctx.pixel_set_download()) == 0
    one_call()
    assert all((bits(x) == 0).all() for x in state(ctx, W, H))
    it.pixel_set(None)
    assert ctx.pixel_set_download() is None


# ---- 6. split across ranks --------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_sum_to_the_single_contexts_adaptive_result(gpu_ctx_ok):
    w, h, ts = 32, 24, 8 * 24
    ex = build("cornell", w, h, MAX, aov=True, moments=True)
    ctx, it = ex.scene.ctx, ex.integrator
    whole_result = it.render_adaptive(THR, MAX, MIN, PASS)
    whole = state(ctx, w, h)
    n_whole = whole[1][:, :, 0] + whole[1][:, :, 7]
    assert len(set(n_whole.reshape(-1).tolist())) >= 3
    p = np.arange(w * h).reshape(w, h)
    merged = [np.zeros_like(x) for x in whole]
    samples = 0
    for rank in range(2):
        ctx.film_create(w, h, rank, 2, ts)
        ctx.aov_enable(True); ctx.moments_enable(True)
        res = it.render_adaptive(THR, MAX, MIN, PASS)
        part = state(ctx, w, h)
        mine = (p // ts) % 2 == rank
        assert mine.sum() == w * h // 2
        for x, m in zip(part, merged):
            assert (bits(x[~mine]) == 0).all(), rank
            m[mine] = x[mine]
        samples += res["pixel_samples"]
        assert res["pixel_samples"] == int(n_whole[mine].sum())
    for got, want, what in zip(merged, whole, ("hdr", "moments", "feature buffers")):
        assert np.array_equal(bits(got), bits(want)), what
    assert samples == whole_result["pixel_samples"]


# ---- 7. nothing existing moves ---------------------------------------------------------------------------------------------------------------------
def test_the_dense_path_is_unmoved_before_and_after_a_set(gpu_ctx_ok):
    N = 12
    ex = build("cornell", W, H, N, aov=True, moments=True)
    ctx = ex.scene.ctx
    orc = oracle_of(ex, "cornell")
    film, _ = orc.render(W, H, 0, N, seed=SEED)
    feat, hits, _ = ae.expected(ex, orc, W, H, range(N), SEED)
    xs = [me.oracle_sample(orc, W, H, fr, SEED) for fr in me.EXACT_FRAMES]
    moments = me.expected(xs, W, H)
    assert hits > 0

    def dense(what):
        ctx.film_clear()
        ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
        assert same_bits(ctx.film_download(W, H)[0], film), what
        check(ctx.aov_download(W, H), feat, what)
        assert (ctx.moments_download(W, H)[:, :, 0] == N).all()
        ctx.film_clear()
        for fr in me.EXACT_FRAMES:
            ctx.pt_rgb_render(fr, 1, SEED, DEPTH, STACK, 0)
        got = ctx.moments_download(W, H)
        assert not np.isnan(got).any() and (got == moments).all(), what

    dense("no set yet")
    ctx.film_clear()
    ctx.pixel_set_upload(patch_list())
    ctx.pt_rgb_render(0, 2, SEED, DEPTH, STACK, 0)
    ctx.pixel_set_clear()
    dense("after a set was installed and cleared")
    # ... and the camera rays' candidate lists are back in use
    ctx.set_option("primary_beams_min_frames", 1)
    ctx.stats_reset()
    dense("candidate lists")
    assert ctx.primary_beam_stats()["rays"] >= N * W * H
    # a list pass does not use them
    ctx.film_clear()
    ctx.pixel_set_upload(patch_list())
    before = ctx.primary_beam_stats()["rays"]
    ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
    assert ctx.primary_beam_stats()["rays"] == before
    inside = np.zeros(W * H, bool); inside[patch_list()] = True
    assert same_bits(ctx.film_download(W, H)[0][inside.reshape(W, H)], film[inside.reshape(W, H)])


# ---- 8. lifecycle and refusals ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(gpu_ctx_ok):
    N = 4
    ex = build("cornell", W, H, N, aov=True, moments=True)
    ctx, it = ex.scene.ctx, ex.integrator
    lib = _native.lib()
    ctx.pt_rgb_render(0, N, SEED, DEPTH, STACK, 0)
    keep = patch_list()
    ctx.pixel_set_upload(keep)
    before = state(ctx, W, H)

    def unchanged(what):
        assert np.array_equal(ctx.pixel_set_download(), keep), what
        for a, b in zip(state(ctx, W, H), before):
            assert np.array_equal(bits(a), bits(b)), what

    for what, px in (("below the film", [-1, 5]), ("beyond the film", [5, W * H]), ("a duplicate", [5, 5]), ("unordered", [7, 5])):
        with pytest.raises(_native.TirtError, match="tirt_pixel_set_upload"):
            ctx.pixel_set_upload(px)
        unchanged(what)
    one = np.array([5], np.int32)
    assert lib.tirt_pixel_set_upload(ctx.handle, one.ctypes.data_as(C.c_void_p), 0) == lib.tirt_pixel_set_upload(ctx.handle, None, 3) != 0
    assert lib.tirt_pixel_set_upload(ctx.handle, one.ctypes.data_as(C.c_void_p), -1) != 0
    unchanged("n and the list disagree")
    for what, args in (("min_samples 0", (THR, 0, MAX)), ("max below min", (THR, 8, 7)), ("negative", (-0.1, MIN, MAX)), ("NaN", (float("nan"), MIN, MAX)),
                       ("infinite", (float("inf"), MIN, MAX))):
        with pytest.raises(_native.TirtError, match="tirt_pixel_set_from_moments"):
            ctx.pixel_set_from_moments(*args)
        unchanged(what)
    n = C.c_int64(0)
    small = np.zeros(4, np.int32)
    assert lib.tirt_pixel_set_download(ctx.handle, small.ctypes.data_as(C.c_void_p), 4, C.byref(n)) != 0 and (small == 0).all()
    assert lib.tirt_pixel_set_download(ctx.handle, None, 0, None) != 0
    # the adaptive driver owns the set: it refuses one that is installed
    with pytest.raises(_native.TirtError, match="tirt_pixel_set_clear"):
        it.render_adaptive(THR, MAX, MIN, PASS)
    unchanged("render_adaptive with a set installed")
    # the other integrators refuse while a set is installed, and work again after the clear
    dbg = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode="normal", seed=SEED)
    for call in (dbg.render, lambda: ctx.bdpt_rgb_render(0, 1, SEED)):
        with pytest.raises(_native.TirtError, match="tirt_pixel_set_clear"):
            call()
        unchanged("another integrator")
    ctx.pixel_set_clear()
    ctx.pixel_set_clear()                                    # no set: nothing to do
    assert ctx.pixel_set_download() is None
    ctx.bdpt_rgb_render(0, 1, SEED)
    dbg.render()
    assert (ctx.film_download(W, H)[0] != 0).any()
    # a film whose pixels disagree in their sample count is no dense prefix
    ctx.film_clear()
    ctx.pixel_set_upload(keep[:3])
    ctx.pt_rgb_render(0, 1, SEED, DEPTH, STACK, 0)
    ctx.pixel_set_clear()
    ragged = state(ctx, W, H)
    for frame in (0, 1):
        ex.cam.frame = frame; ex.cam.frame_cpu[0] = frame
        with pytest.raises(_native.TirtError, match="dense prefix"):
            it.render_adaptive(THR, MAX, MIN, PASS)
        assert ctx.pixel_set_download() is None              # the refusal came from inside the loop, after the first selection: no set stays behind
        for a, b in zip(state(ctx, W, H), ragged):
            assert np.array_equal(bits(a), bits(b))
    # a dense prefix the caller rendered itself is accepted, and counts
    rewind(ex)
    it.render_frames(N)
    ex.cam.frame = N; ex.cam.frame_cpu[0] = N
    res = it.render_adaptive(THR, MAX, MIN, PASS)
    count = it.sample_count.to_numpy()
    assert count.min() >= N and count.max() == MAX and res["frames"] == MAX - N and res["pixel_samples"] == int(count.sum()) - N * W * H
    for what, kw in (("pass_frames", dict(pass_frames=0)), ("min_samples", dict(min_samples=0)), ("max_samples", dict(min_samples=8, max_samples=4))):
        with pytest.raises(_native.TirtError, match=what):
            it.render_adaptive(**dict(dict(threshold=THR, max_samples=MAX), **kw))
        assert ctx.pixel_set_download() is None
    # a context without moment records
    plain = build("cornell", W, H, N, aov=False)
    with pytest.raises(_native.TirtError, match="not enabled"):
        plain.scene.ctx.pixel_set_from_moments(THR, MIN, MAX)
    with pytest.raises(_native.TirtError, match="not enabled"):
        plain.scene.ctx.pt_rgb_render_adaptive(0, SEED, THR, MAX)
    with pytest.raises(ValueError, match="moments=True"):
        plain.integrator.render_adaptive(THR, MAX)
    # another rank's pixel; tirt_film_create drops the set
    ctx.film_create(W, H, 0, 2, 100)
    with pytest.raises(_native.TirtError, match="another rank"):
        ctx.pixel_set_upload([5, 105])
    ctx.pixel_set_upload([5, 205])
    ctx.film_create(W, H, 0, 1, 4096)
    assert ctx.pixel_set_download() is None
    # blocked tiles: the list is in local order, which is not pixel order
    ctx.film_create(32, 24, 0, 1, 8 * 24)
    order = ax.local_order(32, 24, 0, 1, 8 * 24)
    mine = order[[0, 9, 70, 200, 767]]
    assert (np.diff(mine) < 0).any()
    ctx.pixel_set_upload(mine)
    assert np.array_equal(ctx.pixel_set_download(), mine)
    with pytest.raises(_native.TirtError, match="local order"):
        ctx.pixel_set_upload(np.sort(mine))
    assert np.array_equal(ctx.pixel_set_download(), mine)
    # PT_Spec refuses too
    sp = scenes.spectral_box(16, 8, 2, device_id=0, seed=SEED)
    sp.build_scene()
    sp.scene.ctx.pixel_set_upload([3, 4])
    with pytest.raises(_native.TirtError, match="tirt_pixel_set_clear"):
        sp.integrator.render_frames(1)
    sp.scene.ctx.pixel_set_clear()
    sp.integrator.render_frames(1)
    assert (sp.integrator.hdr.to_numpy() != 0).any()
    fresh = _native.Context(0)
    try:
        for call in (lambda: fresh.pixel_set_upload([0]), lambda: fresh.pixel_set_from_moments(THR, MIN, MAX), lambda: fresh.pt_rgb_render_adaptive(0, SEED, THR, MAX)):
            with pytest.raises(_native.TirtError, match="film not created"):
                call()
        assert fresh.pixel_set_download() is None
    finally:
        fresh.close()
