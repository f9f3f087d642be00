"""The device held to the CPU oracle on films that are not square and on films whose pixel count fits none of the device's block sizes (the table, the
scenes and what each row is there for: tests/test_film_shapes.py).  PT_RGB, PT_Spec and Debug bit for bit, BDPT_RGB / BDPT_SPEC at the tolerance of the
square tests (tests/test_gpu_bdpt.py, tests/test_gpu_bdpt_spec.py: float-atomic splat order, rel-L2 <= 1e-3) plus the exact set of pixels that got anything;
the parts of several ranks against the oracle's parts; tone map, export / import; one context taken through a sequence of film sizes; and the film the
reference's own source text makes at 60 x 44 (tests/golden/refkat_nonsquare.npz)."""
import numpy as np
import pytest

import debug_views as dv
import oracle_api as oa
from common import rel_l2, same_bits
from test_film_shapes import BLOCKED, FRAMES, PT_SCENES, ROW_IDS, ROWS, SEED, Row, can_fail, lit, make, oracle, tile_size
from ti_raytrace_amd import Camera, Debug, _native

pytestmark = pytest.mark.gpu
EXH = _native.TRAVERSE_EXHAUSTIVE


def differing(got, want):
    return int((~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).any(axis=2).sum())


def twin_of(kind, row, render, tables=None):
    """the oracle's film of the transposed shape, same pose (CPU only)"""
    ex = make(kind, row.H, row.W, row.scale, tables=False)
    return render(oracle(ex, kind, tables), ex, row.H, row.W)


def owned(row, rank, ranks):
    return (np.arange(row.W * row.H).reshape(row.W, row.H) // tile_size(row)) % ranks == rank


def path_traced(row, kind, dev_render, orc_render, tables_of=None):
    """film, ray counts and overflow of every rank of every tiling of the row, lists off / on and exhaustive, against the oracle's; the parts sum to the
    one-rank film.  dev_render(ctx, flags), orc_render(o, ex, W, H, **tiles) -> (film, stats)."""
    W, H, ts = row.W, row.H, tile_size(row)
    ex = make(kind, W, H, row.scale, device_id=0)
    ctx = ex.scene.ctx
    tables = ex.integrator.tables() if tables_of else None
    o = oracle(ex, kind, tables)
    whole, _ = orc_render(o, ex, W, H)
    can_fail(whole, twin_of(kind, row, lambda oo, e, w, h: orc_render(oo, e, w, h)[0], tables))
    ctx.set_option("primary_beams_min_frames", 1)
    for ranks in sorted(set(row.ranks) | {1}):
        acc = np.zeros_like(whole)
        for rank in range(ranks):
            ctx.film_create(W, H, rank, ranks, ts)
            want, ost = orc_render(o, ex, W, H, tile_rank=rank, tile_count=ranks, tile_size=ts)
            mine = owned(row, rank, ranks)
            assert (want[~mine] == 0).all() and same_bits(want[mine], whole[mine])
            for beams, flags in ((0, 0), (1, 0), (1, EXH)):
                ctx.set_option("primary_beams", beams)
                ctx.film_clear(); ctx.stats_reset()
                dev_render(ctx, flags)
                got = ctx.film_download(W, H)[0]
                st, bst = ctx.stats(), ctx.primary_beam_stats()
                what = (kind, W, H, ranks, rank, beams, flags)
                assert same_bits(got, want), (what, "pixels that differ: %d" % differing(got, want))
                assert (got[~mine] == 0).all(), what
                for k in ("rays_closest", "rays_shadow", "paths"):
                    assert st[k] == ost[k], (what, k, st[k], ost[k])
                assert st["stack_overflow"] == 0, what
                if beams and not flags and mine.any():
                    assert bst["rays"] == FRAMES * int(mine.sum()), (what, bst)          # the camera rays went through the lists
            acc += got
        assert same_bits(acc, whole), (kind, W, H, ranks)
    return ex, o, whole


@pytest.mark.parametrize("kind", PT_SCENES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_pt_rgb_film_equals_the_oracle(gpu_ctx_ok, row, kind):
    ex, o, whole = path_traced(row, kind, lambda ctx, flags: ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, flags),
                               lambda o, ex, W, H, **t: o.render(W, H, 0, FRAMES, seed=SEED, **t))
    # tone map, export -> import into a fresh context of the same shape
    import torch
    W, H = row.W, row.H
    ctx = ex.scene.ctx
    ctx.film_create(W, H, 0, 1, tile_size(row))
    ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, 0)
    ctx.tone_map(0.5)
    hdr, rgb = ctx.film_download(W, H, want_rgb=True)
    assert same_bits(hdr, whole)
    want_rgb = o.tone_map(0.5, whole)
    assert same_bits(rgb, want_rgb), "tone map: %d pixels differ" % differing(rgb, want_rgb)
    t = torch.full((W, H, 3), -1.0, dtype=torch.float32, device=torch.device("cuda", 0))
    ctx.film_export_device(t.data_ptr()); torch.cuda.synchronize()
    assert same_bits(t.cpu().numpy(), whole)
    fresh = _native.Context(0)
    try:
        fresh.film_create(W, H, 0, 1, tile_size(row))
        fresh.film_import_device(t.data_ptr())
        assert same_bits(fresh.film_download(W, H)[0], whole)
    finally:
        fresh.close()


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_pt_spec_film_equals_the_oracle(gpu_ctx_ok, row):
    path_traced(row, "spectral", lambda ctx, flags: ctx.pt_spec_render(0, FRAMES, SEED, 10, 64, flags),
                lambda o, ex, W, H, **t: o.spec_render(W, H, 0, FRAMES, seed=SEED, **t), tables_of=True)


@pytest.mark.parametrize("row", BLOCKED, ids=["%dx%d" % (r.W, r.H) for r in BLOCKED])
def test_the_blocked_rows_walk_their_tiles_in_blocks(gpu_ctx_ok, row):
    """a row that silently fell back to the linear order would test nothing.  The film cannot tell (the maps are bijections); the list pass's diagnostics can:
    `diag_lane_slots` adds up, per WAVE, 64 x the leaf steps of its slowest camera ray, so it depends on which 64 pixels share a wave -- an 8 x 8 block or a
    strip of 1.6 (2.7) columns -- while `diag_leaf_steps`, the sum over the rays, does not.  Against the same film with one tile of W * H + 1 pixels, which is
    no whole number of columns and so forces the linear order: same film, same ray steps, other wave maxima."""
    W, H = row.W, row.H
    res = []
    for ts in (row.tile_size, W * H + 1):                       # (one tile that is not a whole number of columns: linear)
        ex = make("soup", W, H, row.scale, device_id=0)
        ctx = ex.scene.ctx
        ctx.film_create(W, H, 0, 1, ts)
        ctx.set_option("primary_beams_min_frames", 1); ctx.set_option("primary_beams_diag", 1)
        ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, 0)
        res.append((ctx.film_download(W, H)[0], ctx.primary_beam_stats()))
    (a, sa), (b, sb) = res
    print(row, sa, sb)
    assert same_bits(a, b) and sa["rays"] == sb["rays"] == FRAMES * W * H
    assert sa["diag_leaf_steps"] == sb["diag_leaf_steps"] > 0
    assert sa["diag_lane_slots"] != sb["diag_lane_slots"], "the tiles of %d pixels were not walked in 8 x 8 blocks" % row.tile_size


@pytest.mark.parametrize("kind", PT_SCENES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_debug_views_equal_the_oracle(gpu_ctx_ok, row, kind):
    import torch
    from ti_raytrace_amd import RayQuery
    W, H = row.W, row.H
    ex = make(kind, W, H, row.scale, device_id=0, integrator="debug")
    o = oracle(ex, kind)
    ctx = ex.scene.ctx
    films = {}
    for frame in (0, 3):
        want = dv.views(ex, o, W, H, frame, SEED)
        for mode in dv.MODES:
            ctx.debug_render(frame, SEED, Debug.MODES[mode], 64, 0)
            got = ctx.film_download(W, H)[0]
            assert same_bits(got, want[mode]), (kind, W, H, mode, frame, differing(got, want[mode]))
            films[mode, frame] = got
    if kind == "cornell":
        assert lit(films["albedo", 0]).mean() > 0.1
    # the host's camera rays through the query kernel: the same primitives, and the views composed from ITS hit records are the device's frame 0
    rays = oa.camera_rays(ex.cam, W, H)
    h = RayQuery(ex.scene, 64, 0).closest(torch.from_numpy(rays).to(torch.device("cuda", 0)), attributes=True)
    torch.cuda.synchronize()
    prim, rec = h.prim.cpu().numpy(), h.record.cpu().numpy()
    _, oprim, _ = o.closest_hit(rays)
    assert np.array_equal(prim, oprim)
    for mode in dv.MODES:
        assert same_bits(dv.compose(ex.scene, rays, rec, prim, mode, W, H), films[mode, 0]), (kind, W, H, mode)


def bdpt(row, kind, frames, spec=False):
    W, H = row.W, row.H
    ex = make(kind, W, H, row.scale, device_id=0, integrator="bdpt")
    o = oracle(ex, kind)
    ctx = ex.scene.ctx
    ctx.set_option("bdpt_state_fill", 2)
    ctx.stats_reset()
    for f in range(frames):                       # frame by frame on the device, one call on the oracle, as the square tests do
        (ctx.bdpt_spec_render if spec else ctx.bdpt_rgb_render)(f, 1, SEED)
    got = ctx.film_download(W, H)[0]
    st = ctx.stats()
    if spec:
        want, ost, _ = o.bdpt_spec_render(ex.cam, W, H, 0, frames, seed=SEED, stack_size=1024)
    else:
        want, ost, _ = o.bdpt_render(ex.cam, W, H, 0, frames, seed=SEED)
    assert lit(want).mean() > 0.1
    gf, wf = np.isfinite(got).all(axis=2), np.isfinite(want).all(axis=2)
    assert (gf == wf).all() and wf.mean() > 0.98
    r = rel_l2(got[wf], want[wf])
    print("%s BDPT%s %d x %d x %d: rel-L2 %.3e" % (kind, "_SPEC" if spec else "", W, H, frames, r))
    assert r <= 1e-3
    assert st["rays_closest"] == ost["rays_closest"] and st["rays_shadow"] == ost["rays_shadow"]
    # which pixels got anything at all -- exact: an exchanged bound of the light-tracing splat moves or drops splats along one edge only
    assert np.array_equal(lit(got), lit(want)), np.argwhere(lit(got) != lit(want))[:8]
    return ex, o, got, want


@pytest.mark.parametrize("kind,frames", [("cornell", 3), ("veach", 2)])
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_bdpt_rgb_film_equals_the_oracle(gpu_ctx_ok, row, kind, frames):
    bdpt(row, kind, frames)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_bdpt_spec_film_equals_the_oracle(gpu_ctx_ok, row):
    bdpt(row, "prism", 2, spec=True)


def test_one_context_through_a_sequence_of_films(gpu_ctx_ok):
    """buffers sized by an earlier W * H (path state, candidate lists, BDPT vertex arrays, the film) are used again after tirt_film_create"""
    ex = make("cornell", 64, 64, 0.8, device_id=0, integrator="bdpt")
    ctx = ex.scene.ctx
    ctx.set_option("primary_beams_min_frames", 1)
    o = oracle(ex, "cornell")
    first = None
    for W, H in ((64, 64), (50, 30), (200, 3), (96, 40), (1, 1), (64, 64)):
        cam = Camera.Camera(W, H, FRAMES)
        cam.scale = ex.cam.scale; cam.set_target(*ex.cam.target)
        ctx.film_create(W, H, 0, 1, tile_size(Row(W, H, None, (1,), 0.8, "")))
        cam.attach(ctx); o.set_camera(cam)
        ctx.stats_reset()
        ctx.pt_rgb_render(0, FRAMES, SEED, 15, 64, 0)
        pt = ctx.film_download(W, H)[0]
        st = ctx.stats()
        want, ost = o.render(W, H, 0, FRAMES, seed=SEED)
        assert same_bits(pt, want), (W, H, differing(pt, want))
        assert (st["rays_closest"], st["rays_shadow"], st["paths"], st["stack_overflow"]) == (ost["rays_closest"], ost["rays_shadow"], ost["paths"], 0)
        assert ctx.primary_beam_stats()["rays"] == FRAMES * W * H
        ctx.film_clear(); ctx.set_option("bdpt_state_fill", 2)
        ctx.bdpt_rgb_render(0, 2, SEED)
        bd = ctx.film_download(W, H)[0]
        bwant, _, _ = o.bdpt_render(cam, W, H, 0, 2, seed=SEED)
        assert np.isfinite(bd).all() and rel_l2(bd, bwant) <= 1e-3 and np.array_equal(lit(bd), lit(bwant)), (W, H)
        views = {}
        ex.cam = cam
        for frame in (0, 2):
            wv = dv.views(ex, o, W, H, frame, SEED)
            for mode in dv.MODES:
                ctx.debug_render(frame, SEED, Debug.MODES[mode], 64, 0)
                views[mode, frame] = ctx.film_download(W, H)[0]
                assert same_bits(views[mode, frame], wv[mode]), (W, H, mode, frame)
        ctx.film_clear()
        if first is None:
            first = (pt, bd, views)
    assert same_bits(pt, first[0]) and rel_l2(bd, first[1]) <= 1e-3
    assert all(same_bits(views[k], first[2][k]) for k in views)


@pytest.mark.parametrize("bdpt_", [False, True], ids=["pt_rgb", "bdpt_rgb"])
def test_device_film_equals_the_reference_text_film_at_a_non_square_size(gpu_ctx_ok, bdpt_):
    from test_film_shapes import GN, nonsquare_scene
    from test_refkat import film_close
    ex, W, H, frames, seed = nonsquare_scene(device_id=0, bdpt=bdpt_)
    ex.integrator.seed = seed
    ex.build_scene()
    ex.integrator.render_frames(frames)
    got = ex.integrator.hdr.to_numpy()
    rel, per = film_close(got, GN["bdpt_film" if bdpt_ else "pt_film"])
    print("%d x %d: device vs reference text rel-L2 %.2e, worst value %.2e" % (W, H, rel, per))
    assert rel <= 1e-5 and per <= 1e-4, (rel, per)
