"""Option "primary_beams_edges" (csrc/tirt_pvb.h, pvb_beam_triangle_off): k_pvb_beam drops a triangle that one of its own edge planes through the eye separates
from the pixel's pyramid.  The lists with the option on against the lists with it off -- the parent's --, the films and counters of both, and the leaf steps the
camera rays take.  tests/test_gpu_beam_lists.py holds the lists themselves (with the option at its default, on) to their definition; tests/test_beam_edges_host.py
the function to geometry.

What "the codes at 1 are a subset of those at 0" means where a list overflows.  A list holds the PVB_CMAX leaves of least `nr` among those that pass, and the
pixel's bound comes in to just below the nearest leaf that had to go.  With fewer leaves passing, fewer have to go: the bound at 1 is not below the bound at 0, and
between the two bounds the list at 1 may hold leaves that the list at 0 had no room for.  So: wherever the pixel's bound did not move the codes at 1 are a subset of
those at 0, as stated; where it moved, every code at 1 whose nr lies within the bound at 0 is on the list at 0 -- what the list at 0 covered, the list at 1 covers
with a subset -- and the codes at 1 beyond that bound are counted and printed."""
import numpy as np
import pytest

import beam_lists_expected as bl
from beam_lists_cases import CASES
from common import same_bits
from test_gpu_beam_lists import on_device
from test_gpu_primary_fused import differing, run
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
NAMES = ["cornell_16x12", "soup_0.8", "slivers", "one_triangle", "teapot_window"]
SEED, DEPTH, STACK = 5, 15, 64
W, H, FRAMES = 45, 27, 17


def lists_at(ctx, edges):
    ctx.set_option("primary_beams_edges", edges)
    return ctx.primary_beam_lists_download()


def steps_at(ctx, edges):
    """leaf steps of the camera rays of one 17-frame job (k_pvb_cand under "primary_beams_diag"; depth 1: the camera rays are all there is)"""
    ctx.set_option("primary_beams_edges", edges)
    ctx.set_option("primary_beams_diag", 1)
    ctx.film_clear()
    ctx.pt_rgb_render(0, FRAMES, SEED, 1, STACK, 0)
    st = ctx.primary_beam_stats()
    ctx.set_option("primary_beams_diag", 0)
    return st


@pytest.fixture(scope="module")
def downloaded(gpu_ctx_ok):
    """per case: the lists at 1 and at 0, the diagnostics of a job at each, the context"""
    out = {}

    def get(name):
        if name not in out:
            spec, ex = on_device(name)
            ctx = ex.scene.ctx
            builds = ctx.primary_beam_stats()["list_builds"]
            on, off = lists_at(ctx, 1), lists_at(ctx, 0)
            assert ctx.primary_beam_stats()["list_builds"] == builds + 2, "setting the option did not make the lists again"
            again = lists_at(ctx, 0)
            assert ctx.primary_beam_stats()["list_builds"] == builds + 2 and again["count"].tobytes() == off["count"].tobytes(), "setting the option to what it was made the lists again"
            out[name] = (spec, ex, on, off, steps_at(ctx, 1), steps_at(ctx, 0))
        return out[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_lists_on_against_off(downloaded, name):
    spec, ex, on, off, s_on, s_off = downloaded(name)
    P = on["P"]
    assert P == off["P"] == spec.order().shape[0] and on["lists"] and off["lists"]
    c1, c0 = on["count"], off["count"]
    assert np.array_equal(c1 >= 0, c0 >= 0), "pixels with a list: %d at 1, %d at 0" % (int((c1 >= 0).sum()), int((c0 >= 0).sum()))
    b1, b0 = on["bound"], off["bound"]
    bad = np.flatnonzero((c1 >= 0) & (b1 < b0))
    assert bad.size == 0, "local pixel %d: bound %r at 1 below %r at 0" % (int(bad[0]), float(b1[bad[0]]), float(b0[bad[0]]))
    moved = beyond = dropped = 0
    for k in np.flatnonzero(c1 >= 0):
        l1 = {int(c): on["nr"][a, k] for a, c in enumerate(on["code"][:c1[k], k])}
        l0 = {int(c): off["nr"][a, k] for a, c in enumerate(off["code"][:c0[k], k])}
        assert len(l1) == c1[k] and len(l0) == c0[k], "local pixel %d: a code twice on a list" % k
        same_bound = b1[k].tobytes() == b0[k].tobytes()
        moved += not same_bound
        for c, nr in l1.items():
            if same_bound or nr <= b0[k]:
                assert c in l0, "local pixel %d: leaf code %#x (nr %r) is listed at 1 and not at 0 (bounds %r, %r)" % (k, c & 0xffffffff, float(nr), float(b1[k]), float(b0[k]))
            else:
                beyond += 1
            if same_bound:
                assert nr.tobytes() == l0[c].tobytes(), "local pixel %d: leaf code %#x has nr %r at 1 and %r at 0" % (k, c & 0xffffffff, float(nr), float(l0[c]))
        dropped += len(set(l0) - set(l1))
    assert c1[c1 >= 0].sum() <= c0[c0 >= 0].sum()
    print("beam edges %-14s pixels with a list %4d, leaves listed %6d at 0, %6d at 1 (dropped from their pixel's list %d), bounds that moved %d, entries at 1 beyond the bound at 0 %d"
          % (name, int((c1 >= 0).sum()), int(c0[c0 >= 0].sum()), int(c1[c1 >= 0].sum()), dropped, moved, beyond))


@pytest.mark.parametrize("name", NAMES)
def test_leaf_steps_on_against_off(downloaded, name):
    spec, ex, on, off, s_on, s_off = downloaded(name)
    rays = FRAMES * on["P"]
    assert s_on["rays"] == s_off["rays"] == rays, "the camera rays did not go through the lists"
    print("beam edges %-14s leaf steps per ray %.3f at 0, %.3f at 1; lane slots per ray %.3f, %.3f; rays to k_trace %d, %d"
          % (name, s_off["diag_leaf_steps"] / rays, s_on["diag_leaf_steps"] / rays, s_off["diag_lane_slots"] / rays, s_on["diag_lane_slots"] / rays,
             s_off["rays_to_k_trace"], s_on["rays_to_k_trace"]))
    assert s_on["diag_leaf_steps"] <= s_off["diag_leaf_steps"]
    assert s_on["rays_to_k_trace"] <= s_off["rays_to_k_trace"]
    if name == "soup_0.8":
        assert s_on["diag_leaf_steps"] < s_off["diag_leaf_steps"]


def test_one_triangle_pixels_off_the_triangle_have_empty_lists(downloaded):
    """a pixel whose square at 1.5 pixels is disjoint from the triangle on the film (float64, separating axes) has count 0 at 1; at 0 the lone leaf is on every list"""
    spec, ex, on, off, _, _ = downloaded("one_triangle")
    c64 = bl.Cam64(ex.cam)
    q = c64.to_camera(ex.scene.vertex_np[:3, :3].astype(np.float64))
    assert (q[:, 2] < 0).all(), "the triangle is not in front of the camera"
    tri = c64.film(q)
    order = spec.order()
    i, j = (order // spec.H).astype(np.float64), (order % spec.H).astype(np.float64)
    sq = np.stack([np.stack([i + a, j + b], axis=1) for a, b in ((-1.5, -1.5), (1.5, -1.5), (1.5, 1.5), (-1.5, 1.5))], axis=1)      # [P, 4, 2]
    edges = np.roll(tri, -1, axis=0) - tri
    axes = np.concatenate([np.eye(2), np.stack([-edges[:, 1], edges[:, 0]], axis=1)], axis=0)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    ps, pt = sq @ axes.T, tri @ axes.T                                                                                           # [P, 4, axes], [3, axes]
    gap = np.maximum(ps.min(axis=1) - pt.max(axis=0), pt.min(axis=0) - ps.max(axis=1)).max(axis=1)
    away = gap > 1e-9
    assert away.any() and (~away).any(), "the film has no pixel off the triangle, or none on it"
    assert (off["count"][away] == 1).any(), "no pixel off the triangle lists it with the option off: the test finds nothing"
    assert (on["count"][away] == 0).all(), "local pixels %s lie 1.5 pixels off the triangle and list it" % np.flatnonzero(away & (on["count"] != 0))[:8].tolist()
    print("one_triangle: %d of %d pixels are 1.5 pixels off the triangle; lists of one leaf: %d at 0, %d at 1" % (int(away.sum()), away.size, int((off["count"] == 1).sum()), int((on["count"] == 1).sum())))


@pytest.mark.parametrize("name", NAMES)
def test_films_and_counters_on_against_off(gpu_ctx_ok, name):
    """45 x 27 x 17 frames of the case's scene from the case's camera: the film, the ray counters and the camera rays through the lists bit for bit with the option 1
    and 0, through the fused first step and through the separate launches; the rays left to k_trace not above the value at 0"""
    spec = CASES[name]
    ex = spec.make(W, H)
    ex.build_scene()
    spec.aim(ex)
    ctx = ex.scene.ctx
    ctx.film_create(W, H, 0, 1, 4096)
    render = lambda c: c.pt_rgb_render(0, FRAMES, SEED, DEPTH, STACK, 0)
    res = {}
    for edges in (1, 0):
        ctx.set_option("primary_beams_edges", edges)
        for fused in (1, 0):
            res[edges, fused] = run(ctx, W, H, fused, render)
    ref = res[0, 0]
    assert ref[2] == FRAMES * W * H and ref[1][4] == 0
    for key, r in res.items():
        assert same_bits(r[0], ref[0], nan_payload=True), "%s: %s" % (key, differing(r[0], ref[0]))
        assert r[1] == ref[1] and r[2] == ref[2], (key, r[1:3], ref[1:3])
    for fused in (1, 0):
        assert res[1, fused][3] <= res[0, fused][3], "rays left to k_trace: %d at 1, %d at 0" % (res[1, fused][3], res[0, fused][3])
        assert res[1, fused][3] == res[1, 1][3] and res[0, fused][3] == res[0, 1][3]
    print("beam edges %-14s film %d x %d x %d: rays %d, left to k_trace %d at 0, %d at 1" % (name, W, H, FRAMES, ref[2], res[0, 1][3], res[1, 1][3]))


def test_the_option_is_checked(gpu_ctx_ok):
    ctx = _native.Context(0)
    with pytest.raises(_native.TirtError, match="primary_beams_edges"):
        ctx.set_option("primary_beams_edges", 2)
