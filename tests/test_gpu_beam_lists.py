"""The camera rays' candidate lists downloaded (tirt_primary_beam_lists_download) and held to the sentence the header of csrc/tirt_pvb.hip rests on -- every leaf
that could hold a verified hit within the bound is on the list, with all the leaves in front of it -- and pvb_walk_list, the walk k_pvb_cand and
k_pvb_cand_shade share, asked row by row (tirt_kat_primary_list_walk) on sample rays AIMED at where k_pvb_beam can be wrong: triangle vertices and edge crossings
in and around each pixel's square, sphere silhouettes, the pixel's corners (tests/beam_lists_expected.py).  The films of tests/test_gpu_beams.py see a missing
leaf only if a random jitter lands on it, it is the closest hit and another listed leaf still yields a hit within the bound.

Every case: (1) download, check_lists; (2) all sample rows through the walk, twice -- every wave holding the rows of one pixel, and the rows shuffled, so that a
wave's ballots see rays of many pixels -- row for row the same, and equal to expected_walk: the direction bit for bit, the verdict, the hit and the leaf steps of
walking the list as given on EVERY row, H's first element on the resolved ones; (3) the same rays through trace_closest: H's first element on every row, hence
the walk's answer bit for bit on the resolved ones.  The cases: tests/beam_lists_cases.py.

Each case prints (pytest -s) the mean list length against the mean number of leaves with a non-empty H over the sample rows, and the share of unresolved rows;
docs/HISTORY.md has the table."""
import numpy as np
import pytest

import beam_lists_expected as bl
from beam_lists_cases import CASES, make_cases
from ti_raytrace_amd import _native

pytestmark = pytest.mark.gpu
f = np.float32


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def walk_rows(ctx, k, jx, jy, at):
    """the rows through tirt_kat_primary_list_walk twice: the rows of one tested pixel (`at`, ascending) filling whole waves (padded with copies of the pixel's
    first row), and all rows shuffled by a fixed seed.  Both must agree row for row; returns the [n, 9] rows."""
    n = k.shape[0]
    idx = []
    start = np.searchsorted(at, np.arange(at.max() + 2)) if n else np.zeros(1, np.int64)
    for a in range(start.shape[0] - 1):
        r = np.arange(start[a], start[a + 1])
        if r.size:
            idx.append(np.concatenate([r, np.full(-r.size % 64, r[0])]))
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    real = np.ones(idx.shape[0], bool)
    pos = 0
    for a in range(start.shape[0] - 1):
        m = start[a + 1] - start[a]
        if m:
            real[pos + m:pos + m + (-m % 64)] = False
            pos += m + (-m % 64)
    out = ctx.kat_primary_list_walk(k[idx], jx[idx], jy[idx])
    by_pixel = out[real]
    assert np.array_equal(idx[real], np.arange(n))
    perm = np.random.default_rng(99).permutation(n)
    shuffled = np.zeros_like(by_pixel)
    shuffled[perm] = ctx.kat_primary_list_walk(k[perm], jx[perm], jy[perm])
    bad = np.flatnonzero((bits(by_pixel) != bits(shuffled)).any(axis=1))
    assert bad.size == 0, "row %d (local pixel %d): the walk answers %s with its pixel's rows in one wave and %s among other pixels' rows" % (
        int(bad[0]), int(k[bad[0]]), by_pixel[bad[0]].tolist(), shuffled[bad[0]].tolist())
    return by_pixel


def check_state(spec, ex, label):
    """the three steps of the module's docstring for the context's current (build, camera, film); returns the downloaded lists"""
    sc, ctx = ex.scene, ex.scene.ctx
    n = sc.primitive_count
    lists = ctx.primary_beam_lists_download()
    P = spec.order().shape[0]
    assert lists["P"] == P and lists["cmax"] == bl.PVB_CMAX and lists["count"].shape == (P,)
    dl = ctx.wide_tree_download(n)
    compact = ctx.lbvh_download(n, want_morton=False, want_bvh=False)[2]
    geo = bl.from_download(dl, sc.primitive_np, ex.cam)
    assert lists["lists"] == (spec.lists and (lists["count"] >= 0).any()) and lists["pixels_with_list"] == int((lists["count"] >= 0).sum())
    if not spec.lists:
        assert geo.far and (lists["count"] == -1).all(), "a camera %.1f extents away got lists" % spec.scale
    tot = {"listed": 0, "with_hits": 0, "full": 0, "cut": 0, "pixels": 0, "rows": 0, "unresolved": 0, "dropped": 0}
    for case in make_cases(spec, sc, ex.cam, compact, geo):
        st = bl.check_lists(case, lists)
        want = bl.expected_walk(case, lists)
        rows = case.rows
        got = walk_rows(ctx, case.ks[rows["at"]].astype(np.int32), rows["jx"], rows["jy"], rows["at"])
        who = lambda r: "%s, %s row %d (jx %r, jy %r)" % (case.name(int(rows["at"][r])), bl.KIND_NAMES[int(rows["kind"][r])], r, float(rows["jx"][r]), float(rows["jy"][r]))
        bad = np.flatnonzero((bits(got[:, 0:3]) != bits(case.rays[:, 3:6])).any(axis=1))
        assert bad.size == 0, "%s: direction %s, restated %s" % (who(bad[0]), got[bad[0], 0:3].tolist(), case.rays[bad[0], 3:6].tolist())
        res = got[:, 3] != 0.0
        bad = np.flatnonzero(res != want["resolved"])
        assert bad.size == 0, "%s: resolved %s, expected %s (count %d, bound %r, H's first t %r)" % (
            who(bad[0]), bool(res[bad[0]]), bool(want["resolved"][bad[0]]), int(lists["count"][case.ks[rows["at"][bad[0]]]]),
            float(lists["bound"][case.ks[rows["at"][bad[0]]]]), float(want["first"][0][bad[0]]))
        got_hit = np.stack([bits(got[:, 4]), bits(got[:, 5]), bits(got[:, 6]), bits(got[:, 7])], axis=1)
        for what, (t, u, v, p), rows_checked in (("walking its list as given", want["walk"], np.ones(res.shape[0], bool)), ("H's first element", want["first"], want["resolved"])):
            exp = np.stack([bits(t), bits(u), bits(v), np.asarray(p, np.int32).view(np.uint32)], axis=1)
            bad = np.flatnonzero((got_hit != exp).any(axis=1) & rows_checked)
            assert bad.size == 0, "%s: the walk reports (t, u, v, prim) = %s, %s gives %s" % (
                who(bad[0]), (got[bad[0], 4:7].tolist(), int(got_hit[bad[0], 3].view(np.int32))), what, ([float(t[bad[0]]), float(u[bad[0]]), float(v[bad[0]])], int(p[bad[0]])))
        bad = np.flatnonzero(got[:, 8].astype(np.int64) != want["steps"])
        assert bad.size == 0, "%s: %d leaf steps, the list as given takes %d" % (who(bad[0]), int(got[bad[0], 8]), int(want["steps"][bad[0]]))
        # k_trace on the same rays: H's first element on every row (so: the walk's answer on the resolved ones, bit for bit)
        out, prim, _ = ctx.trace_closest(case.rays)
        ft, _, _, fp = want["first"]
        bad = np.flatnonzero((bits(out[:, 0]) != bits(ft)) | (prim != fp))
        assert bad.size == 0, "%s: trace_closest gives (t, prim) = (%r, %d), H's first element is (%r, %d)" % (
            who(bad[0]), float(out[bad[0], 0]), int(prim[bad[0]]), float(ft[bad[0]]), int(fp[bad[0]]))
        for key in ("listed", "with_hits", "full", "cut", "pixels"):
            tot[key] += st[key]
        tot["rows"] += res.shape[0]; tot["unresolved"] += int((~res).sum()); tot["dropped"] += case.dropped
    px = max(tot["pixels"], 1)
    print("beam lists %-22s pixels with a list %4d, mean list length %6.2f, mean leaves with hits %6.2f, full lists %3d, bounds that came in %3d, rows %6d, unresolved %5.1f %%, aimed rows dropped by the cap %d"
          % (label, tot["pixels"], tot["listed"] / px, tot["with_hits"] / px, tot["full"], tot["cut"], tot["rows"], 100.0 * tot["unresolved"] / max(tot["rows"], 1), tot["dropped"]))
    return lists, tot


def on_device(name):
    spec = CASES[name]
    ex = spec.make(spec.W, spec.H)
    ex.build_scene()
    spec.aim(ex)
    ex.scene.ctx.film_create(spec.W, spec.H, *spec.tiles)
    return spec, ex


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_and_walk(gpu_ctx_ok, name):
    spec, ex = on_device(name)
    lists, tot = check_state(spec, ex, name)
    if name == "slivers":
        assert tot["cut"] >= 1 and tot["full"] >= 1, "no list of the slivers overflowed: the case does not reach the overflow rule"
    if name == "cornell_inside":
        k = np.flatnonzero(lists["count"] > 0)
        assert (lists["nr"][0, k] == 0.0).any(), "no entry with nr == 0 although the eye is inside the scene"
    if name == "soup_far":
        assert tot["unresolved"] > 0


def test_lists_follow_the_camera_and_the_vertices(gpu_ctx_ok):
    """a second download after `cam.yaw += 0.4`, and a third after Scene.update_vertices, differs from the one before and passes the checks for the new state;
    each counts as one list build, a download of lists that stand as none"""
    spec, ex = on_device("cornell_16x12")
    ctx = ex.scene.ctx
    ctx.stats_reset()
    key = lambda l: (l["count"].tobytes(), l["bound"].tobytes(), np.where(np.arange(bl.PVB_CMAX)[:, None] < l["count"][None, :], l["code"], 0).tobytes())
    a, _ = check_state(spec, ex, "cornell, first pose")
    assert ctx.primary_beam_stats()["list_builds"] == 1
    ex.cam.yaw += 0.4; ex.cam.update()
    b, _ = check_state(spec, ex, "cornell, yaw + 0.4")
    assert key(a) != key(b) and ctx.primary_beam_stats()["list_builds"] == 2
    pos = ex.scene.vertex_np[:, :3].reshape(-1, 3, 3)
    centre = pos.mean(axis=1, keepdims=True)
    moved = (centre + (pos - centre) * f(0.7) + f(3.0)).astype(f)
    ex.scene.update_vertices(moved)
    assert np.array_equal(bits(ctx.vertex_download(ex.scene.vertex_count)[:, :3]), bits(moved.reshape(-1, 3)))
    c, _ = check_state(spec, ex, "cornell, moved vertices")
    assert key(b) != key(c) and ctx.primary_beam_stats()["list_builds"] == 3


def test_refusals_and_switches(gpu_ctx_ok):
    """no scene / no film: the argument error and nothing written; the option off: no lists, every count -1, and the walk refuses"""
    L = _native.lib()
    info = np.full(4, 7, np.int32)
    ctx = _native.Context(0)
    assert L.tirt_primary_beam_lists_download(ctx.handle, None, None, None, info.ctypes.data) == -2 and (info == 7).all()
    spec, ex = on_device("cornell_13x7")
    ctx = ex.scene.ctx
    P = spec.W * spec.H
    count = np.full(P, 7, np.int32)
    assert L.tirt_primary_beam_lists_download(ctx.handle, count.ctypes.data, None, None, info.ctypes.data) == -2 and (info == 7).all() and (count == 7).all()
    assert L.tirt_primary_beam_lists_download(ctx.handle, None, None, None, None) == -2
    assert ctx.primary_beam_lists_info() == {"P": P, "cmax": bl.PVB_CMAX, "lists": True, "pixels_with_list": P}
    z = np.zeros(1, f)
    with pytest.raises(_native.TirtError, match="local pixel outside"):
        ctx.kat_primary_list_walk(np.array([P], np.int32), z, z)
    with pytest.raises(_native.TirtError, match="stride too small"):
        ctx.kat_primary_list_walk(np.zeros(1, np.int32), z, z, out_stride=8)
    ctx.set_option("primary_beams", 0)
    off = ctx.primary_beam_lists_download()
    assert not off["lists"] and off["pixels_with_list"] == 0 and (off["count"] == -1).all()
    with pytest.raises(_native.TirtError, match="no candidate lists"):
        ctx.kat_primary_list_walk(np.zeros(1, np.int32), z, z)
    ctx.set_option("primary_beams", 1)
    assert ctx.primary_beam_lists_info()["lists"]
