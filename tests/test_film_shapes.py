"""Films that are not square, and films whose pixel count fits none of the device's block sizes: the shape table, the scenes and the
conditions under which a comparison on them can fail at all (CPU side, the oracle alone) -- and the oracle itself held to a non-square film made by
the reference's own source text (tests/golden/refkat_nonsquare.npz, tools/refkat/make_refkat.py --nonsquare-only).

tests/test_gpu_film_shapes.py holds the device to the oracle on the same table.  Every other oracle comparison of the suite uses a square film whose
side is a multiple of 8, where W and H can be exchanged anywhere (the film index i * H + j, cx / cy, the bounds of the light-tracing splat) and the
fall-back branches of the pixel maps (tiles that are not blocked, paths that are not pixel-block major, a last partial wave) are never taken."""
import os
from collections import namedtuple

import numpy as np
import pytest

import oracle_api as oa
from common import host_only, same_bits
from ti_raytrace_amd import scenes
from ti_raytrace_amd.PT_RGB import default_tile_size

Row = namedtuple("Row", "W H tile_size ranks scale what")
# scale: the camera's distance in scene diagonals (Example.frame_camera).  fy = fx = focal * W / FULL_HGT: with a tiny W the rows of a film fan out over
# almost a half-space, and from outside (0.8) a 1 x 64 or 3 x 200 film looks past the scene with all but 1.5 % of its pixels; those rows put the eye INSIDE
# the scene's bounds, where every direction meets something.
ROWS = [
    Row(50, 30, None, (1,), 0.8, "neither blocked tiles nor pixel-block-major paths (P = 1500: 23 waves and a last one of 28 pixels)"),
    Row(32, 30, None, (1,), 0.8, "P % 64 == 0 with H % 8 != 0: pixel-block-major paths over a linear tile"),
    Row(24, 40, 320, (1, 3), 0.8, "blocked tiles (8 whole columns) on a film taller than wide"),
    Row(40, 24, 192, (1, 3), 0.8, "blocked tiles on a film wider than tall"),
    Row(37, 29, 100, (1, 3), 0.8, "primes: a ragged last tile (73 pixels), a ragged last wave, tiles that start in the middle of a column"),
    Row(1, 64, None, (1,), 0.1, "one column: cx = 0.5, exactly one wave"),
    Row(64, 1, None, (1,), 0.8, "one row: cy = 0.5, H = 1 in every i * H + j"),
    Row(1, 1, None, (1,), 0.4, "one pixel: 63 idle lanes in every kernel (0.4: a pose whose one ray meets something in all three scenes)"),
    Row(3, 200, None, (1,), 0.1, "three long columns (P = 600)"),
    Row(200, 3, None, (1,), 0.8, "two hundred columns of three pixels"),
    Row(65, 63, 4096, (2,), 0.8, "one past / one short of 64: P = 4095, a tile of 4095 pixels and an empty second rank"),
]
ROW_IDS = ["%dx%d" % (r.W, r.H) for r in ROWS]
BLOCKED = [r for r in ROWS if r.tile_size is not None and r.H % 8 == 0 and r.tile_size % (8 * r.H) == 0 and (r.W * r.H) % r.tile_size == 0]
assert [(r.W, r.H) for r in BLOCKED] == [(24, 40), (40, 24)]
FRAMES = 9                      # with primary_beams_min_frames = 1 both the ordinary launch and the list path run (tests/test_gpu_beams.py uses 9 to 12)
SEED = 5
PT_SCENES = ("cornell", "teapot", "soup")
SMOOTH = ("teapot", "veach", "spectral")          # the examples that call Scene.process_normal


def tile_size(row):
    return row.tile_size or default_tile_size(row.H)


def make(kind, W, H, scale, device_id=None, integrator="pt", tables=True):
    """One of the scenes at W x H with the camera `scale` diagonals from the scene's centre; packed on the host (device_id None) or built on a device.
    cornell / teapot (example/single_model.py: env map, smooth normals, glass) / soup (3 000 random triangles) / spectral (example/spectral_box.py) /
    veach (example/veach_bdpt.py) / prism (example/prism_rainbow.py).  integrator: pt, bdpt (cornell; veach and prism have their own), debug."""
    from ti_raytrace_amd import BDPT_RGB, Debug
    if kind == "cornell":
        ex = scenes.cornell_box(W, H, FRAMES, device_id=device_id)
    elif kind == "teapot":
        ex = scenes.single_model(W, H, FRAMES, device_id=device_id)
    elif kind == "soup":
        ex = scenes.synthetic(W, H, FRAMES, ntri=3000, device_id=device_id)
    elif kind == "spectral":
        ex = scenes.spectral_box(W, H, FRAMES, device_id=device_id)
    elif kind == "veach":
        ex = scenes.veach_bdpt(W, H, FRAMES, device_id=device_id)
    elif kind == "prism":
        ex = scenes.prism_rainbow(W, H, FRAMES, device_id=device_id)
    else:
        raise ValueError(kind)
    if integrator == "bdpt" and kind == "cornell":
        ex.integrator = BDPT_RGB.BDPT(W, H, ex.cam, ex.scene, 64)
    elif integrator == "debug":
        ex.integrator = Debug.Debug(W, H, ex.cam, ex.scene, 64, seed=SEED)
    if device_id is None:
        ex.scene.setup_data_cpu()
        ex.integrator.setup_data_cpu()
        if tables and hasattr(ex.integrator, "setup_tables"):      # the spectral integrators: the Rgb2Spec table from the oracle instead of the device (13 s)
            ex.integrator.setup_tables(lambda res, xyz, d65: oa.spec_table_build(res, xyz, d65))
    else:
        ex.build_scene()
    if kind == "prism":                       # the example's own camera (scenes.prism_rainbow.build_scene), nearer for the rows that look from inside
        ex.cam.scale = 10.0 * scale / 0.8; ex.cam.set_target(0.0, 0.0, 0.0); ex.cam.update()
    else:
        ex.frame_camera(scale if kind != "veach" else scale * 0.5 / 0.8)         # (example/veach_bdpt.py looks from 0.5 diagonals)
    return ex


def oracle(ex, kind, tables=None):
    """(tables: PT_Spec.PathTrace.tables() of another example of the same kind -- they do not depend on the film)"""
    o = oa.OracleScene(ex.scene, ex.cam)
    o.lbvh_build()
    if kind in SMOOTH:
        o.process_normal(ex.scene.vertex_index_np)
    if kind in ("spectral", "prism"):
        o.set_spectral(tables or ex.integrator.tables())
    return o


def lit(film):
    """pixels with anything in them (a NaN counts)"""
    return (np.nan_to_num(film, nan=1.0) != 0).any(axis=2)


def can_fail(film, twin):
    """what a film must be for a comparison on it to notice an exchange of W and H: more than a tenth of its pixels lit, and not the transpose of the
    transposed shape's film (a 1 x 1 film is its own transpose)"""
    W, H = film.shape[:2]
    assert lit(film).mean() > 0.1, "%d x %d: only %.1f %% of the pixels are lit" % (W, H, 100 * lit(film).mean())
    if (W, H) != (1, 1):
        assert not same_bits(film, np.ascontiguousarray(twin.transpose(1, 0, 2))), "%d x %d: the film is the transposed film's transpose" % (W, H)


def pt_films(kind, row, frames=FRAMES):
    """the oracle's PT_RGB film of a row and of its transposed twin (W <-> H, same pose)"""
    out = []
    for W, H in ((row.W, row.H), (row.H, row.W)):
        ex = make(kind, W, H, row.scale)
        out.append(oracle(ex, kind).render(W, H, 0, frames, seed=SEED)[0])
    return out


@pytest.mark.parametrize("kind", PT_SCENES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_every_row_can_fail(row, kind):
    film, twin = pt_films(kind, row)
    can_fail(film, twin)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_oracle_pt_rgb_is_deterministic_and_tile_independent(row):
    """what test_oracle_golden.py::test_render_is_deterministic_and_tile_independent asserts at 32 x 32: the device is only as right as the oracle it is held to"""
    W, H, ts = row.W, row.H, tile_size(row)
    ex = make("cornell", W, H, row.scale)
    o = oracle(ex, "cornell")
    full, st = o.render(W, H, 0, 3, seed=SEED, nthreads=3)
    again, st1 = o.render(W, H, 0, 3, seed=SEED, nthreads=1)
    assert same_bits(full, again) and st == st1 and st["paths"] == 3 * W * H
    p = np.arange(W * H).reshape(W, H)
    for ranks, size in ((3, ts), (3, 100), (2, 7)):
        acc = np.zeros_like(full)
        for r in range(ranks):
            part, _ = o.render(W, H, 0, 3, seed=SEED, tile_rank=r, tile_count=ranks, tile_size=size)
            mine = (p // size) % ranks == r
            assert (part[~mine] == 0).all() and same_bits(part[mine], full[mine]), (ranks, size, r)
            acc += part
        assert same_bits(acc, full), (ranks, size)
    h2, _ = o.render(W, H, 0, 2, seed=SEED)
    h3, _ = o.render(W, H, 2, 1, seed=SEED, hdr=h2.copy())
    assert same_bits(h3, full)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_oracle_bdpt_is_deterministic_and_stateful(row):
    """(the BDPT restatement has neither threads nor tiles: every pixel's light sub-path may land on any other pixel)"""
    W, H = row.W, row.H
    ex = make("cornell", W, H, row.scale, integrator="bdpt")
    o = oracle(ex, "cornell")
    a, st, _ = o.bdpt_render(ex.cam, W, H, 0, 3, seed=SEED)
    b, st1, _ = o.bdpt_render(ex.cam, W, H, 0, 3, seed=SEED)
    assert same_bits(a, b) and st == st1 and np.isfinite(a).all()
    h2, _, state = o.bdpt_render(ex.cam, W, H, 0, 2, seed=SEED)
    h3, _, _ = o.bdpt_render(ex.cam, W, H, 2, 1, seed=SEED, hdr=h2, state=state)
    assert same_bits(h3, a)
    twin_ex = make("cornell", H, W, row.scale, integrator="bdpt")
    twin, _, _ = oracle(twin_ex, "cornell").bdpt_render(twin_ex.cam, H, W, 0, 3, seed=SEED)
    can_fail(a, twin)


# ---- a non-square film from the reference's own source text ---------------------------------------------------------------------------------------------
# tools/refkat/make_refkat.py --nonsquare-only: integrator/PT_RGB.py's and integrator/BDPT_RGB.py's render() executed as plain Python on the Cornell box at
# W != H with W * H % 64 != 0, frames 0 (no jitter) and 1.  The 16 x 16 fixtures of tests/test_refkat.py cannot tell `hdr[i, j]` from `hdr[j, i]`, `cx` from
# `cy` or Camera.get_image_point's `u >= W` from `u >= H`, in the oracle or anywhere else: this one decides whether the ORACLE has W and H the right way
# round, at the tolerances test_refkat.py asserts for the square films.
GN = np.load(os.path.join(os.path.dirname(__file__), "golden", "refkat_nonsquare.npz"))


def nonsquare_scene(device_id=None, bdpt=False):
    W, H, frames, seed = [int(x) for x in GN["cfg"][:4]]
    from ti_raytrace_amd import BDPT_RGB
    ex = scenes.cornell_box(W, H, 4, device_id=device_id)
    if bdpt:
        ex.integrator = BDPT_RGB.BDPT(W, H, ex.cam, ex.scene, 64)
    if device_id is None:
        host_only(ex, 0.8)
    return ex, W, H, frames, seed


def test_the_fixture_is_not_square():
    W, H, frames, seed = [int(x) for x in GN["cfg"][:4]]
    assert W != H and W >= 12 and H >= 8 and (W * H) % 64 != 0 and frames == 2
    for key in ("pt_film", "bdpt_film"):
        film = GN[key]
        assert film.shape == (W, H, 3) and np.isfinite(film).all() and lit(film).mean() > 0.1


@pytest.mark.parametrize("bdpt", [False, True], ids=["pt_rgb", "bdpt_rgb"])
def test_oracle_film_equals_the_reference_text_film_at_a_non_square_size(bdpt):
    from test_refkat import film_close
    ex, W, H, frames, seed = nonsquare_scene(bdpt=bdpt)
    o = oracle(ex, "cornell")
    got = o.bdpt_render(ex.cam, W, H, 0, frames, seed=seed)[0] if bdpt else o.render(W, H, 0, frames, seed=seed)[0]
    rel, per = film_close(got, GN["bdpt_film" if bdpt else "pt_film"])
    print("%d x %d x %d frames: oracle vs reference text rel-L2 %.2e, worst value %.2e" % (W, H, frames, rel, per))
    assert rel <= 1e-5 and per <= 1e-4, (rel, per)
