"""The winding number on the device (csrc/tirt_winding.hip, the terms in csrc/tirt_winding.h, through tirt_query_winding_number / tirt_winding_number /
tirt_winding_prepare / _table_download / tirt_kat_winding and ti_raytrace_amd.PointQuery) against the definition of include/tirt.h as
tests/winding_expected.py restates it over the DOWNLOADED tree: the moment table and every answer are compared on bits, the approximation at the default
beta against float64."""
import numpy as np
import pytest
import torch

import closest_point_expected as E
import signed_distance_scenes as S
import winding_expected as W
from common import custom_scene
from test_winding_host import hole_points, kat_rows, kat_expected, assert_kat
from ti_raytrace_amd import PointQuery, _native, scenes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
D = np.float64
SCAN = _native.TRAVERSE_EXHAUSTIVE
COUNT = _native.COUNT_NODES
INF = float("inf")
BETAS = (1.0, 2.0, 3.5, INF)
NAMES = ("one", "two", "fan", "cube", "cube_open", "torus", "torus_open", "cornell", "cube_sphere", "cube_sphere_lbvh", "torus_far", "cube_degenerate")
FAR_CENTRE = (28000.0, -28000.0, 28000.0)          # 10^4 extents of the torus (2.8) from the origin
# max |w - float64| at beta = 2 over accuracy_queries, as tools/winding_accuracy.py measured it on the device (profiles/winding_accuracy.txt); the test allows twice that
MEASURED_MAX_ERROR = {"torus": 2.1083e-2, "torus_open": 2.1473e-2}
_SCENES = {}


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mesh(name):
    """(triangles [T, 3, 3] float64, spheres ((x, y, z, r), ...), traversal_tree)"""
    cube = S.cube_triangles()
    if name == "one":
        return np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], D), (), 1
    if name == "two":
        return S.mesh_triangles("quad"), (), 1
    if name == "fan":                                             # five triangles about the origin: one full node and one more level
        a = 2 * np.pi * np.arange(6) / 5
        return np.array([[[0, 0, 0.3], [np.cos(a[k]), np.sin(a[k]), 0], [np.cos(a[k + 1]), np.sin(a[k + 1]), 0]] for k in range(5)]).astype(F).astype(D), (), 1
    if name == "cube":
        return cube, (), 1
    if name == "cube_open":
        return cube[2:], (), 1
    if name == "torus":
        return W.torus_triangles(), (), 1
    if name == "torus_open":
        return W.torus_triangles()[W.torus_hole()], (), 1
    if name == "torus_far":
        return W.torus_triangles(centre=FAR_CENTRE), (), 1
    if name == "cube_sphere":
        return cube, ((2.5, 0.5, 0.5, 0.75),), 1
    if name == "cube_sphere_lbvh":
        return cube, ((2.5, 0.5, 0.5, 0.75),), 0
    if name == "cube_degenerate":
        return S.mesh_triangles("cube_degenerate"), (), 1
    raise KeyError(name)


def build(name, tris=None):
    if name == "cornell":
        ex = scenes.cornell_box(32, 32, 4, device_id=0)
    else:
        t, spheres, tree = mesh(name)
        ex = custom_scene(t if tris is None else tris, spheres=spheres)
        ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    return ex


def queries(geom, cell, seed):
    """about 2 000 points: uniform in the scene box scaled by 1.5, within a cell of the surface, exactly on vertices and face centroids, at sphere centres and
    on their surfaces, 5 .. 10^4 extents away and at 10^20, then a NaN row and an infinite one"""
    r = np.random.RandomState(seed)
    lo, hi = S.scene_box(geom)
    ext = float((hi - lo).max())
    mid = 0.5 * (lo + hi)
    t = geom.tris.astype(D)
    parts = [mid + 0.75 * (hi - lo) * r.uniform(-1, 1, (1200, 3))]
    k = r.randint(0, t.shape[0], 300)
    bc = r.dirichlet((1, 1, 1), 300)
    on = (t[k] * bc[:, :, None]).sum(axis=1)
    nrm = np.cross(t[k, 1] - t[k, 0], t[k, 2] - t[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    parts.append(on + nrm * (cell * r.uniform(-1, 1, (300, 1))))
    parts.append(t[r.randint(0, t.shape[0], 100), r.randint(0, 3, 100)])
    cen = t[r.randint(0, t.shape[0], 100)].astype(F)
    parts.append(((cen[:, 0] + cen[:, 1]) + cen[:, 2]) * F(1.0 / 3.0))
    for s in geom.spheres.astype(D):
        d = r.normal(size=(20, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        parts += [s[None, :3], s[:3] + s[3] * d, s[:3] + s[3] * d * r.uniform(0, 1.2, (20, 1))]
    d = r.normal(size=(100, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    parts.append(mid + d * ext * 10.0 ** r.uniform(0.7, 4, (100, 1)))
    parts.append(np.array([[1e20, 0, 0], [0, -1e20, 1e20]]))
    parts.append(np.array([[np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]]]))
    return np.concatenate(parts, axis=0).astype(F)


def case(name):
    """the scene on the device, its downloaded tree and table, its queries"""
    if name not in _SCENES:
        ex = build(name)
        ctx = ex.scene.ctx
        geom = E.scene_geometry(ex.scene)
        d = ctx.wide_tree_download(ex.scene.primitive_count)
        tree = W.Tree(d)
        table, sums, e = ctx.winding_table()
        _SCENES[name] = dict(ex=ex, ctx=ctx, geom=geom, info=d, tree=tree, table=table, sums=sums, e=e,
                             pts=queries(geom, float(tree.cell.max()), 100 + NAMES.index(name)))
    return _SCENES[name]


def wn(ex, pts, beta=2.0, flags=0, stack_size=64):
    """(w, counts or None) as numpy"""
    q = PointQuery(ex.scene, stack_size, flags & SCAN)
    p = on_dev(pts)
    w, c = q.winding_counts(p, beta) if flags & COUNT else (q.winding_number(p, beta), None)
    torch.cuda.synchronize(DEV)
    return w.cpu().numpy(), None if c is None else c.cpu().numpy()


def same(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def first_bad(a, b):
    bad = np.nonzero(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))[0]
    return bad[:6], a[bad[:6]], b[bad[:6]]


# ---- 1. the moment table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_table_is_the_restatements(gpu_ctx_ok, name):
    c = case(name)
    tree = c["tree"]
    assert c["e"] == tree.e and c["table"].shape == (tree.nodes, 4, 16) and c["sums"].shape == (tree.nodes, 16)
    if name == "one":
        assert tree.nodes == 0 and tree.root_code < 0
    if name.startswith("cube_sphere"):
        assert c["info"]["shapes_boxed"] == (0 if name.endswith("lbvh") else 1)
    want_table, want_sums = W.moment_table(tree)
    for node in range(tree.nodes):                               # per node, through the tree's own child codes
        assert np.array_equal(c["sums"][node], want_sums[node]), (name, node, tree.codes[node], c["sums"][node], want_sums[node])
        for slot in range(4):
            got, want = c["table"][node, slot], want_table[node, slot]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, node, slot, int(tree.codes[node, slot]), got, want)
    t2, s2, _ = c["ctx"].winding_table()                         # asked again: the same table
    assert np.array_equal(t2.view(np.uint32), c["table"].view(np.uint32)) and np.array_equal(s2, c["sums"])


# ---- 2. the walk is the restated walk, 3. without approximation it is the scan, the exact sum and the host route -------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_walk_is_the_restated_walk(gpu_ctx_ok, name):
    c = case(name)
    pts, tree, table = c["pts"], c["tree"], c["table"]
    big = tree.tri.shape[0] > 500
    for beta in BETAS:
        sub = pts[::8] if (big and beta == INF) else pts           # (the restatement of 2 000 x 2 000 exact terms: every eighth query)
        S_want, counts_want = W.walk(tree, table, sub, beta)
        want = W.answer(sub, S_want)
        got, counts = wn(c["ex"], sub, beta, COUNT)
        assert same(got, want), (name, beta, first_bad(got, want))
        assert np.array_equal(counts, counts_want.astype(np.int32)), (name, beta)
        plain, _ = wn(c["ex"], sub, beta)
        assert same(plain, got), (name, beta, "COUNT_NODES changes the answer")
    fin = W.finite_rows(pts)
    assert np.isnan(got[~W.finite_rows(sub)]).all() and np.isfinite(got[W.finite_rows(sub)]).all() and (~fin).sum() == 2


@pytest.mark.parametrize("name", NAMES)
def test_exact_walk_is_the_scan_the_sum_and_the_host_route(gpu_ctx_ok, name):
    c = case(name)
    pts, geom = c["pts"], c["geom"]
    walk, _ = wn(c["ex"], pts, INF)
    scan, scan_counts = wn(c["ex"], pts, INF, SCAN | COUNT)
    assert same(walk, scan), (name, first_bad(walk, scan))
    fin = W.finite_rows(pts)
    assert (scan_counts[fin] == (0, c["ex"].scene.primitive_count)).all() and (scan_counts[~fin] == 0).all()
    host = c["ctx"].winding_number(pts, INF)
    assert same(host, walk)
    host2, host_counts = c["ctx"].winding_number(pts, 2.0, flags=COUNT)
    dev2, dev_counts = wn(c["ex"], pts, 2.0, COUNT)
    assert same(host2, dev2) and np.array_equal(host_counts, dev_counts)
    sub = pts[::8] if geom.tris.shape[0] > 500 else pts
    want = W.answer(sub, W.exact_sum(sub, geom.tris, geom.spheres))
    got = walk[::8] if geom.tris.shape[0] > 500 else walk
    assert same(got, want), (name, first_bad(got, want))
    if name == "cube":
        k = np.nonzero(fin)[0][:1200]
        assert np.array_equal(walk[k] > 0.5, S.inside_box(pts[k].astype(D), S.CUBE_LO, S.CUBE_HI))
        assert set(np.unique(np.round(walk[k] * 2)).tolist()) == {0.0, 2.0}
    if name == "cube_open":
        w = wn(c["ex"], np.array([[0.5, 0.5, 0.5]], F), INF)[0][0]
        assert abs(float(w) - 5.0 / 6.0) < 1e-5
    if name.startswith("cube_sphere"):
        k = np.arange(1200)                                      # (the uniform ones: none of them ON a surface)
        assert np.array_equal(walk[k] > 0.5, S.inside_box(pts[k].astype(D), S.CUBE_LO, S.CUBE_HI) | S.inside_sphere(pts[k].astype(D), (2.5, 0.5, 0.5, 0.75)))
        assert (walk[k] > 0.5).sum() > 50
        for beta in (1.0, 2.0):                                  # a sphere beneath an approximated child owes nothing
            assert np.array_equal(wn(c["ex"], pts[k], beta)[0] > 0.5, walk[k] > 0.5)


# ---- 4. the plumbing -------------------------------------------------------------------------------------------------------------------------------
def test_chunks_side_stream_and_strides(gpu_ctx_ok):
    c = case("torus")
    ex, ctx, pts = c["ex"], c["ctx"], c["pts"]
    q = PointQuery(ex.scene)
    p = on_dev(pts)
    want, want_counts = q.winding_counts(p, 2.0)
    ctx.set_option("query_chunk_rays", 256)                      # eight chunks
    try:
        got, counts = q.winding_counts(p, 2.0)
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(counts, want_counts)
    wide = torch.zeros((pts.shape[0], 8), device=DEV)
    wide[:, 2:5] = p
    view = wide[:, 2:5]
    assert view.stride() == (8, 1)
    assert torch.equal(q.winding_number(view, 2.0).view(torch.int32), want.view(torch.int32))
    s = torch.cuda.Stream(DEV)
    big = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(4):                                       # keep the side stream busy before the points exist
            big = torch.tanh(big @ big)
        late = torch.where(big[0, 0] > 2.0, p * 0.0, p)          # (tanh <= 1: an exact copy of p, made after the products)
        w = q.winding_number(late, 2.0)
        consumer = w * 2.0
    torch.cuda.synchronize(DEV)
    assert torch.equal(consumer.view(torch.int32), (want * 2.0).view(torch.int32))


def test_stack_of_one_entry(gpu_ctx_ok):
    """the one-triangle scene needs no stack at all; on the torus a one-entry stack loses subtrees: those rows are NaN, tirt_stats says TIRT_ERR_STACK, and
    nothing is written outside the output"""
    c = case("one")
    assert same(wn(c["ex"], c["pts"], 2.0, stack_size=1)[0], wn(c["ex"], c["pts"], 2.0)[0])
    c = case("torus")
    ctx, pts = c["ctx"], c["pts"]
    n = pts.shape[0]
    p = on_dev(pts)
    guard = torch.full((n + 256,), 7.0, device=DEV)
    cguard = torch.full((n + 256, 2), 7, dtype=torch.int32, device=DEV)
    ctx.stats_reset()
    ctx.query_winding_number(p.data_ptr(), n, 3, guard[128:].data_ptr(), beta=INF, stack_size=1, flags=COUNT, counts=cguard[128:].data_ptr())
    torch.cuda.synchronize(DEV)
    with pytest.raises(_native.TirtStackOverflow) as err:
        ctx.stats()
    fin = W.finite_rows(pts)
    assert err.value.stats["stack_overflow"] == int(fin.sum())
    out = guard.cpu().numpy()
    assert np.isnan(out[128:128 + n]).all() and (out[:128] == 7.0).all() and (out[128 + n:] == 7.0).all()
    cout = cguard.cpu().numpy()
    assert (cout[:128] == 7).all() and (cout[128 + n:] == 7).all()
    ctx.stats_reset()
    assert same(wn(c["ex"], pts, 2.0)[0], W.answer(pts, W.walk(c["tree"], c["table"], pts, 2.0)[0]))      # the next call is right again
    assert ctx.stats()["stack_overflow"] == 0


def test_argument_errors(gpu_ctx_ok):
    c = case("cube")
    ctx = c["ctx"]
    p = on_dev(c["pts"][:64])
    out = torch.zeros(64, device=DEV)
    for beta in (0.5, -1.0, float("nan"), float("-inf")):
        with pytest.raises(_native.TirtError, match=r"error -2:.*beta must be >= 1"):
            ctx.query_winding_number(p.data_ptr(), 64, 3, out.data_ptr(), beta=beta)
        with pytest.raises(_native.TirtError, match=r"error -2:.*beta must be >= 1"):
            ctx.winding_number(c["pts"][:64], beta)
        with pytest.raises(ValueError, match="beta must be >= 1"):
            PointQuery(c["ex"].scene).winding_number(p, beta)
    with pytest.raises(_native.TirtError, match=r"error -2:.*point_stride < 3"):
        ctx.query_winding_number(p.data_ptr(), 64, 2, out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"error -2:.*null out_w"):
        ctx.query_winding_number(p.data_ptr(), 64, 3, 0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*out_w: not device memory"):
        ctx.query_winding_number(p.data_ptr(), 64, 3, np.zeros(64, F).ctypes.data)
    with pytest.raises(ValueError, match='method is "pseudonormal" or "winding"'):
        PointQuery(c["ex"].scene).inside(p, method="parity")
    assert PointQuery(c["ex"].scene).winding_number(p[:0]).shape == (0,)


# ---- 5. moving geometry ----------------------------------------------------------------------------------------------------------------------------
def test_table_follows_update_vertices(gpu_ctx_ok):
    tris = W.torus_triangles(20, 12)
    ex = build("torus", tris)
    ctx = ex.scene.ctx
    pts = queries(E.scene_geometry(ex.scene), 1e-4, 7)[::4]
    before = wn(ex, pts, 2.0)[0]
    moved = (tris * np.array([1.25, 0.8, 1.5]) + np.array([0.3, -0.2, 0.1])).astype(F)
    ex.scene.update_vertices(moved.reshape(-1, 3))
    after, counts = wn(ex, pts, 2.0, COUNT)
    fresh = build("torus", moved.astype(D))
    want, want_counts = wn(fresh, pts, 2.0, COUNT)
    assert same(after, want) and np.array_equal(counts, want_counts) and not same(after, before)
    ta, sa, _ = ctx.winding_table()
    tb, sb, _ = fresh.scene.ctx.winding_table()
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)) and np.array_equal(sa, sb)


# ---- 6. inside ---------------------------------------------------------------------------------------------------------------------------------------
def test_inside_by_winding_number(gpu_ctx_ok):
    c = case("torus")
    q = PointQuery(c["ex"].scene)
    fin = W.finite_rows(c["pts"])
    p = on_dev(c["pts"][fin])
    cell = float(c["tree"].cell.max())
    by_w, by_n = q.inside(p, method="winding"), q.inside(p)
    far = q.closest(p).dist2.sqrt() > cell
    torch.cuda.synchronize(DEV)
    assert by_w.dtype == torch.bool and int(far.sum()) > 1200 and bool(by_w[far].any()) and bool((~by_w[far]).any())
    assert torch.equal(by_w[far], by_n[far])
    assert torch.equal(q.inside(p, method="pseudonormal"), by_n)
    # the open torus, in front of its window: the points the pseudo-normal sign gets wrong (tests/test_winding_host.py)
    c = case("torus_open")
    q = PointQuery(c["ex"].scene)
    pts, truth, pseudo = hole_points()
    p = on_dev(pts)
    by_w, by_n = q.inside(p, method="winding").cpu().numpy(), q.inside(p).cpu().numpy()
    assert pts.shape[0] >= 20 and np.array_equal(by_w, truth)
    assert np.array_equal(by_n, pseudo) and (by_n != truth).all()


# ---- 7. the term code --------------------------------------------------------------------------------------------------------------------------------
def test_kat_device_is_host_is_numpy(gpu_ctx_ok):
    ctx = case("cube")["ctx"]
    rows, sph = kat_rows()
    for data, is_sphere in ((rows, False), (sph, True)):
        dev, host = ctx.kat_winding(data, is_sphere), _native.kat_winding_host(data, is_sphere)
        assert np.array_equal(dev[2], host[2]) and same(dev[0], host[0]) and same(dev[1], host[1])
        assert_kat(dev, kat_expected(data, is_sphere), "device")


# ---- the default beta against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["torus", "torus_open"])
def test_accuracy_of_the_default_beta(gpu_ctx_ok, name):
    """beta = 2 on the 2 000-triangle tori against the float64 exact sum: the maximum error stays within twice what tools/winding_accuracy.py measured (the
    seeds are fixed: only a lost or doubled term trips this, and a node-sized term is of the order of 0.1 .. 1), and no query farther than 2 % of the extent
    from the surface (the open torus: that includes the window's rim) is on the wrong side of 0.5"""
    c = case(name)
    pts = W.accuracy_queries(c["geom"].tris)
    w64 = W.exact_float64(pts, c["geom"].tris)
    q = PointQuery(c["ex"].scene)
    p = on_dev(pts)
    w = q.winding_number(p).cpu().numpy()
    dist = q.closest(p).dist2.sqrt().cpu().numpy()
    err = np.abs(w.astype(D) - w64)
    lo, hi = S.scene_box(c["geom"])
    far = dist > 0.02 * float((hi - lo).max())
    wrong = far & ((w > 0.5) != (w64 > 0.5))
    print("%s: beta 2: max error %.4e, mean %.4e; %d of %d queries farther than 2 %% of the extent, %d of them misclassified"
          % (name, err.max(), err.mean(), int(far.sum()), pts.shape[0], int(wrong.sum())))
    assert err.max() <= 2.0 * MEASURED_MAX_ERROR[name]
    assert int(far.sum()) > pts.shape[0] // 2 and int(wrong.sum()) == 0, (pts[wrong][:8], w[wrong][:8], w64[wrong][:8])
