"""The feature buffers of the path tracer on the device (csrc/tirt_aov.hip through tirt_aov_* and PathTrace(aov=True)): bit for bit against the records
the CPU oracle's hits give (tests/aov_expected.py) on the Cornell box, a triangle soup with misses, the Teapot with its sphere light and smooth normals, and
the ragged films of tests/test_film_shapes.py; independent of how the frames are cut into calls, batches and lanes and of the route the camera rays take;
the film untouched; tiles; lifecycle; PT_Spec."""
import numpy as np
import pytest

import aov_expected as ae
import oracle_api as oa
from common import same_bits, tiny_scene
from test_film_shapes import ROW_IDS, ROWS, make as make_row, oracle as oracle_row, tile_size
from ti_raytrace_amd import Debug, _native, scenes

pytestmark = pytest.mark.gpu
EXH = _native.TRAVERSE_EXHAUSTIVE
SEED = 5
WORDS = _native.AOV_WORDS


def differing(got, want, nan_payload=False):
    eq = got.view(np.uint32) == want.view(np.uint32)
    if not nan_payload:
        eq |= np.isnan(got) & np.isnan(want)
    return "words that differ: %d of %d, first at %s" % (int((~eq).sum()), eq.size, np.argwhere(~eq)[:4].tolist())


def check(got, want, what, nan_payload=False):
    assert same_bits(got, want, nan_payload=nan_payload), (what, differing(got, want, nan_payload))


def build(kind, W, H, frames, aov=True, **kw):
    """an example on device 0 with its path tracer's feature buffers on (or off), and what its oracle scene needs"""
    if kind == "cornell":
        ex = scenes.cornell_box(W, H, frames, device_id=0, seed=SEED, aov=aov, **kw)
    elif kind == "soup":
        ex = tiny_scene(200, W=W, H=H, device_id=0)
        ex.sample_count = frames; ex.integrator.seed = SEED; ex.integrator.aov = aov
    elif kind == "teapot":
        ex = scenes.single_model(W, H, frames, device_id=0, seed=SEED, aov=aov, **kw)
    else:
        raise ValueError(kind)
    ex.build_scene()
    return ex


def oracle_of(ex, kind):
    orc = oa.OracleScene(ex.scene, ex.cam)
    orc.lbvh_build()
    if kind == "teapot":
        orc.process_normal(ex.scene.vertex_index_np)
    return orc


def rewind(ex):
    ex.scene.ctx.film_clear()
    ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,H,frames", [("cornell", 64, 48, 12), ("soup", 32, 32, 12), ("teapot", 48, 40, 12)])
def test_records_equal_the_oracle(gpu_ctx_ok, kind, W, H, frames):
    ex = build(kind, W, H, frames)
    ex.integrator.render_frames(frames)
    got = ex.integrator.aov_to_numpy()
    hdr = ex.integrator.hdr.to_numpy()
    want, hits, misses = ae.expected(ex, oracle_of(ex, kind), W, H, range(frames), SEED)
    nans = bool(np.isnan(want).any())
    print("%s %d x %d x %d: oracle hits %d, misses %d, NaN words %d" % (kind, W, H, frames, hits, misses, int(np.isnan(want).sum())))
    if kind == "soup":
        assert hits > W * H and misses > W * H          # both, and plenty of each
    if nans:
        print("strict NaN payloads:", same_bits(got, want, nan_payload=True), differing(got, want, True))
    check(got, want, kind, nan_payload=nans)
    assert (got[:, :, _native.AOV_ALPHA] > 0).mean() > 0.1
    # the fields are slices of the same download
    it = ex.integrator
    check(it.albedo.to_numpy(), got[:, :, 0:3], "albedo", True); check(it.normal.to_numpy(), got[:, :, 3:6], "normal", True)
    check(it.depth.to_numpy(), got[:, :, 6], "depth", True); check(it.alpha.to_numpy(), got[:, :, 7], "alpha", True)
    assert it.normal.to_numpy().shape == (W, H, 3) and it.depth.to_numpy().shape == (W, H)
    # 4. the film is the film of the same job without feature buffers
    plain = build(kind, W, H, frames, aov=False)
    plain.integrator.render_frames(frames)
    check(plain.integrator.hdr.to_numpy(), hdr, "hdr of " + kind, True)
    with pytest.raises(_native.TirtError):
        plain.integrator.aov_to_numpy()


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_records_equal_the_oracle_on_ragged_films(gpu_ctx_ok, row):
    W, H, frames = row.W, row.H, 4
    ex = make_row("cornell", W, H, row.scale, device_id=0)
    orc = oracle_row(ex, "cornell")
    ctx = ex.scene.ctx
    ctx.film_create(W, H, 0, 1, tile_size(row))
    ctx.pt_rgb_render(0, frames, SEED, 15, 64, 0)
    hdr = ctx.film_download(W, H)[0]
    ctx.film_clear()
    ctx.aov_enable(True)
    ctx.pt_rgb_render(0, frames, SEED, 15, 64, 0)
    got = ctx.aov_download(W, H)
    want, hits, _ = ae.expected(ex, orc, W, H, range(frames), SEED)
    assert hits > 0
    check(got, want, (W, H))
    check(ctx.film_download(W, H)[0], hdr, ("hdr", W, H), True)


# ---- 2. the call pattern does not matter ----------------------------------------------------------------------------------------------------
def test_calls_of_any_size_give_the_same_records(gpu_ctx_ok):
    W, H, N = 64, 48, 12
    ex = build("cornell", W, H, N)
    ex.integrator.render_frames(N)
    want = ex.integrator.aov_to_numpy()
    assert np.isfinite(want).all() and (want[:, :, _native.AOV_ALPHA] == 1).mean() > 0.5
    for merge in (None, 0):                              # deferred submission merges the calls (default), or every call is its own batch
        ex = build("cornell", W, H, N)
        if merge is not None:
            ex.scene.ctx.set_option("merge_paths", merge)
        for _ in range(N):
            ex.integrator.render(); ex.cam.update_frame()
        check(ex.integrator.aov_to_numpy(), want, ("frame by frame", merge), True)
        rewind(ex)
        ex.integrator.render_frames(5); ex.cam.update_frame(5)
        ex.integrator.render_frames(7); ex.cam.update_frame(7)
        check(ex.integrator.aov_to_numpy(), want, ("5 + 7", merge), True)


def big_job(lanes, aov=True):
    """512 x 512 x 40 frames in batches of about 3 Mi paths: (records, film, batches)"""
    W = H = 512
    ex = build("cornell", W, H, 40, aov=aov)
    ctx = ex.scene.ctx
    ctx.set_option("batch_paths", 3 << 20)
    if lanes:
        ctx.set_option("overlap_lanes", lanes)
    ctx.stats_reset()
    ex.integrator.render_frames(40)
    rec = ex.integrator.aov_to_numpy() if aov else None
    hdr = ex.integrator.hdr.to_numpy()
    st = ctx.stats()
    return rec, hdr, st["launches_trace_closest"] // 15       # one closest-hit launch per bounce and batch (MAX_DEPTH 15)


def test_batches_on_several_lanes_apply_their_frames_in_order(gpu_ctx_ok):
    rec, hdr, nb = big_job(0)
    assert nb >= 3, nb
    rec1, hdr1, nb1 = big_job(1)
    assert nb1 == nb
    check(rec, rec1, "records, 4 lanes against 1", True)
    check(hdr, hdr1, "film, 4 lanes against 1", True)
    assert (rec[:, :, _native.AOV_ALPHA] == 1).mean() > 0.5 and np.isfinite(rec).all()
    # 4. the film of the same job without feature buffers
    _, hdr0, nb0 = big_job(0, aov=False)
    assert nb0 == nb
    check(hdr, hdr0, "film with and without feature buffers", True)


# ---- 3. both routes of the camera rays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,H", [("cornell", 64, 48), ("soup", 32, 32)])
def test_candidate_lists_and_exhaustive_traversal_give_the_same_records(gpu_ctx_ok, kind, W, H):
    N = 12
    ex = build(kind, W, H, N)
    ctx = ex.scene.ctx
    ctx.set_option("primary_beams_min_frames", 1)
    recs = {}
    for beams, flags in ((0, 0), (1, 0), (1, EXH)):
        ctx.set_option("primary_beams", beams)
        ctx.film_clear()
        ctx.pt_rgb_render(0, N, SEED, 15, 64, flags)
        recs[beams, flags] = ctx.aov_download(W, H)
        if beams and not flags:
            assert ctx.primary_beam_stats()["rays"] == N * W * H          # the camera rays went through the lists
    want, _, _ = ae.expected(ex, oracle_of(ex, kind), W, H, range(N), SEED)
    for key, got in recs.items():
        check(got, want, (kind, key))
        check(got, recs[0, 0], (kind, key, "against lists off"), True)


# ---- 4. Debug and BDPT leave the records alone ----------------------------------------------------------------------------------------------
def test_debug_and_bdpt_renders_leave_the_records_alone(gpu_ctx_ok):
    W, H, N = 64, 48, 6
    ex = build("cornell", W, H, N)
    ctx = ex.scene.ctx
    ex.integrator.render_frames(N)
    want = ex.integrator.aov_to_numpy()
    assert (want[:, :, _native.AOV_ALPHA] == 1).mean() > 0.5
    d = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode="normal", seed=SEED)
    ex.cam.frame = 3; ex.cam.frame_cpu[0] = 3
    d.render()
    assert (d.hdr.to_numpy() != 0).any()
    check(ex.integrator.aov_to_numpy(), want, "after Debug", True)
    ctx.bdpt_rgb_render(0, 2, SEED)
    assert np.isfinite(ctx.film_download(W, H)[0]).all()
    check(ex.integrator.aov_to_numpy(), want, "after BDPT_RGB", True)


# ---- 5. tiles -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [8 * 48, 100], ids=["blocked", "ragged"])
def test_three_ranks_sum_to_the_whole(gpu_ctx_ok, ts):
    W, H, N, ranks = 64, 48, 6, 3
    ex = build("cornell", W, H, N)
    ctx = ex.scene.ctx
    orc = oracle_of(ex, "cornell")
    ex.integrator.render_frames(N)
    whole = ex.integrator.aov_to_numpy()
    check(whole, ae.expected(ex, orc, W, H, range(N), SEED)[0], "one rank")
    p = np.arange(W * H).reshape(W, H)
    acc = np.zeros_like(whole)
    for rank in range(ranks):
        ctx.film_create(W, H, rank, ranks, ts)
        ctx.aov_enable(True)
        ctx.pt_rgb_render(0, N, SEED, 15, 64, 0)
        part = ctx.aov_download(W, H)
        mine = (p // ts) % ranks == rank
        assert mine.any() and (part[~mine].view(np.uint32) == 0).all(), rank
        check(part[mine], whole[mine], ("own tiles", rank), True)
        check(part, ae.expected(ex, orc, W, H, range(N), SEED, mine=mine)[0], ("oracle", rank))
        acc += part
    check(acc, whole, "sum", True)


# ---- 6. lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_lifecycle(gpu_ctx_ok):
    import torch
    W, H, N = 64, 48, 4
    ex = build("cornell", W, H, N, aov=False)
    ctx, it = ex.scene.ctx, ex.integrator
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.aov_download(W, H)
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.aov_export_device(1 << 20)
    it.render_frames(N)                                   # renders as ever
    assert (it.hdr.to_numpy() != 0).any()
    ctx.aov_enable(True)
    with pytest.raises(_native.TirtError, match="null"):
        ctx.aov_export_device(0)
    assert (ctx.aov_download(W, H).view(np.uint32) == 0).all()          # enabled: zeros until a frame is rendered
    rewind(ex)
    it.render_frames(N)
    rec = ctx.aov_download(W, H)
    assert (rec[:, :, _native.AOV_ALPHA] == 1).mean() > 0.5
    t = it.aov_to_torch()
    assert t.shape == (W, H, WORDS) and t.dtype == torch.float32 and t.device == torch.device("cuda", ctx.device_id)
    check(t.cpu().numpy(), rec, "aov_to_torch", True)
    ctx.film_clear()
    assert (ctx.aov_download(W, H).view(np.uint32) == 0).all()          # film_clear zeroes them
    it.render_frames(N)
    check(ctx.aov_download(W, H), rec, "after film_clear", True)
    ctx.aov_enable(False)
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.aov_download(W, H)
    ctx.film_clear()
    it.render_frames(N)                                   # disabled: no records, the same film
    ctx.aov_enable(True)
    assert (ctx.aov_download(W, H).view(np.uint32) == 0).all()          # enable, disable, enable starts from zero
    ctx.film_clear()
    it.render_frames(N)
    check(ctx.aov_download(W, H), rec, "after enable, disable, enable", True)
    ctx.film_create(32, 24, 0, 1, 4096)                   # a new film starts disabled
    with pytest.raises(_native.TirtError, match="not enabled"):
        ctx.aov_download(32, 24)
    fresh = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="film not created"):
            fresh.aov_enable(True)
    finally:
        fresh.close()


# ---- 7. PT_Spec -----------------------------------------------------------------------------------------------------------------------------
def test_pt_spec_records_equal_pt_rgb(gpu_ctx_ok):
    W = H = 32
    N = 4
    sp = scenes.spectral_box(W, H, N, device_id=0, seed=SEED, aov=True)
    sp.build_scene()
    sp.integrator.render_frames(N)
    got = sp.integrator.aov_to_numpy()
    # the same box, camera and seed through PT_RGB (example/spectral_box.py smooths its normals; its materials keep their colours)
    ex = scenes.cornell_box(W, H, N, device_id=0, seed=SEED, aov=True)
    ex.build_scene()
    ex.scene.process_normal()
    ex.integrator.render_frames(N)
    want = ex.integrator.aov_to_numpy()
    assert (want[:, :, _native.AOV_ALPHA] == 1).mean() > 0.5
    check(got, want, "PT_Spec against PT_RGB", True)
    orc = oa.OracleScene(ex.scene, ex.cam)
    orc.lbvh_build(); orc.process_normal(ex.scene.vertex_index_np)
    check(want, ae.expected(ex, orc, W, H, range(N), SEED)[0], "against the oracle")
