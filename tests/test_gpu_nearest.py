"""K nearest primitives on the device (csrc/tirt_nearest.hip through tirt_query_nearest / tirt_nearest and ti_raytrace_amd.PointQuery.nearest / .count_within)
against the definition of include/tirt.h as tests/nearest_expected.py restates it.  Every comparison is on bits: the culled walk against the scan over
all primitives (both on the device) and both against numpy; then the relation to closest(), ties at the cut-off, the bound and the count, the plumbing,
moving geometry and the stack."""
import numpy as np
import pytest
import torch

import closest_point_expected as E
import nearest_expected as NE
from common import custom_scene, duplicate_code_scene, long_chain_scene, same_bits as same
from ti_raytrace_amd import Example, PointQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN, COUNT = _native.TRAVERSE_EXHAUSTIVE, _native.COUNT_NODES
KS = (1, 2, 5, 64)
_SCENES, _TABLES = {}, {}
TIE_COPIES = range(2, 10)                                     # the primitive ids of the eight identical triangles of the tie scene


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    """PointNearest (or any tuple of tensors / None) -> numpy"""
    torch.cuda.synchronize(DEV)
    return tuple(None if x is None else x.cpu().numpy() for x in h)


def tie_triangles():
    """8 identical copies of one triangle (ids 2 .. 9) beside 4 others (ids 0, 1, 10, 11)"""
    t = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.25]])
    others = [t + np.array(s) for s in ((1.5, 0.2, 0.1), (-1.2, 0.4, -0.3), (0.3, 1.6, 0.5), (0.1, -1.4, 0.2))]
    return np.stack(others[:2] + [t] * 8 + others[2:])


def scene(name):
    """(built example, its Geometry), built once per module"""
    if name not in _SCENES:
        r = np.random.RandomState(3)
        if name == "one":                                    # a one-primitive scene: the root's code is a leaf code
            ex = custom_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]]], spheres=())
        elif name == "two":
            ex = custom_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]], spheres=())
        elif name == "cornell":
            ex = scenes.cornell_box(16, 16, 1, device_id=0)
        elif name == "mesh_spheres":                         # a triangle mesh plus analytic spheres, one of them among the triangles
            tris = r.uniform(-1, 1, (300, 1, 3)) + r.uniform(-0.15, 0.15, (300, 3, 3))
            ex = custom_scene(tris, spheres=((0.0, 3.0, 0.0, 0.75), (0.2, -0.1, 0.3, 0.4), (-2.5, 0.5, 0.0, 0.1)))
        elif name == "dup":
            ex = duplicate_code_scene(16, 16, device_id=0)
        elif name == "chain":
            ex = long_chain_scene(16, 16)
        elif name == "ties":
            ex = custom_scene(tie_triangles(), spheres=())
        elif name == "teapot":
            ex = scenes.single_model(16, 16, 1, device_id=0)
        else:
            raise KeyError(name)
        ex.build_scene()
        _SCENES[name] = (ex, E.scene_geometry(ex.scene))
    return _SCENES[name]


def query_points(geom, n, seed):
    """n float32 points of the kinds the culling can get wrong: uniform in 1.5 x the box, on the surface, the vertices themselves (every incident triangle
    ties at 0), edge midpoints, 10 / 1e3 / 1e6 extents away, and rows with NaN, +inf, -inf (the mix of test_gpu_closest_point.py)"""
    r = np.random.RandomState(seed)
    t = geom.tris.astype(np.float64)
    lo, hi = t.reshape(-1, 3).min(axis=0), t.reshape(-1, 3).max(axis=0)
    if geom.spheres.shape[0]:
        s = geom.spheres.astype(np.float64)
        lo, hi = np.minimum(lo, (s[:, :3] - s[:, 3:]).min(axis=0)), np.maximum(hi, (s[:, :3] + s[:, 3:]).max(axis=0))
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    n_far, n_bad = 8, 9
    n_vert = min(max(n // 5, 1), 3 * t.shape[0]) if t.shape[0] <= 4000 else n // 5
    n_surf = n_edge = n // 6
    n_uni = n - (n_vert + n_surf + n_edge + 3 * n_far + n_bad)
    parts = [mid + 0.75 * (hi - lo) * r.uniform(-1, 1, (n_uni, 3))]
    k = r.randint(0, t.shape[0], n_surf)
    b = r.dirichlet((1, 1, 1), n_surf)
    parts.append((t[k] * b[:, :, None]).sum(axis=1))
    verts = t.reshape(-1, 3)
    parts.append(verts if n_vert == verts.shape[0] else verts[r.choice(verts.shape[0], n_vert, replace=False)])
    k, e = r.randint(0, t.shape[0], n_edge), r.randint(0, 3, n_edge)
    parts.append(0.5 * (t[k, e] + t[k, (e + 1) % 3]))
    for far in (10.0, 1.0e3, 1.0e6):
        d = r.normal(size=(n_far, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        parts.append(mid + d * far * ext)
    bad = np.tile(mid, (n_bad, 1))
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * j + a, a] = v
    parts.append(bad)
    p = np.concatenate(parts, axis=0).astype(F)
    assert p.shape == (n, 3)
    return p


def table(name, n=1024):
    """points of scene `name` and the restatement's per-primitive terms for them, made once and left unchanged"""
    if name not in _TABLES:
        ex, geom = scene(name)
        pts = query_points(geom, n, seed=11)
        _TABLES[name] = (pts, NE.Table(pts, geom))
    return _TABLES[name]


def prefix(want64, k):
    """the definition's answer for k from its answer for 64: the list of k is the list of 64 cut short, the count is the count"""
    return tuple(w[:, :k] for w in want64[:4]) + (want64[4],)


def device_answer(ex, pts, k, flags=0, max_distance=None, count=True, stack_size=64):
    return cpu(PointQuery(ex.scene, stack_size, flags).nearest(pts if isinstance(pts, torch.Tensor) else on_dev(pts), k, max_distance, attributes=True, count=count))


def assert_same(got, want, what):
    d2, prim, q, uv, count = got
    bad = np.nonzero((prim != want[1]).any(axis=1))[0]
    assert bad.size == 0, (what, "prim", bad[:8], prim[bad[:4]], want[1][bad[:4]], d2[bad[:4]], want[0][bad[:4]])
    assert same(d2, want[0]), (what, "d2")
    assert same(q, want[2]), (what, "point")
    assert same(uv, want[3]), (what, "uv")
    if count is not None:
        bad = np.nonzero(count != want[4])[0]
        assert bad.size == 0, (what, "count", bad[:8], count[bad[:8]], want[4][bad[:8]])
    assert_lists_valid(got, what)


def assert_lists_valid(got, what):
    """sorted by D2, no primitive twice, the padding (inf, -1, 0, 0) behind the entries and nowhere else"""
    d2, prim, q, uv, count = got
    held = (prim >= 0).sum(axis=1)
    k = prim.shape[1]
    cols = np.arange(k)[None, :]
    assert ((prim >= 0) == (cols < held[:, None])).all(), (what, "padding inside a list")
    pad = prim < 0
    assert np.isposinf(d2[pad]).all() and np.isfinite(d2[~pad]).all(), (what, "d2 of the padding")
    assert (q[pad] == 0).all() and (uv[pad] == 0).all(), (what, "attributes of the padding")
    with np.errstate(invalid="ignore"):
        assert not (np.diff(d2, axis=1) < 0).any(), (what, "not sorted")
    s = np.sort(np.where(pad, -1 - cols, prim), axis=1)
    assert not (np.diff(s, axis=1) == 0).any(), (what, "a primitive appears twice")
    if count is not None:
        assert np.array_equal(held, np.minimum(count, k)), (what, "entries held against the count")


def bounds_of(tab, n, seed):
    """a scalar bound and a per-query bound tensor chosen from the restatement: the scalar is the median distance of element 4 (or the last there is),
    the tensor mixes the distance of a random element, the float above it, half of it, 0, -1, NaN and +inf"""
    want = tab.nearest(64, None)
    r = np.random.RandomState(seed)
    held = np.maximum((want[1] >= 0).sum(axis=1), 1)
    with np.errstate(all="ignore"):
        t = np.sqrt(want[0][np.arange(n), r.randint(0, 1 << 30, n) % held]).astype(F)
        col = np.sqrt(want[0][:, min(4, want[0].shape[1] - 1)])
        scalar = float(np.median(col[np.isfinite(col)])) if np.isfinite(col).any() else float(np.median(np.sqrt(want[0][:, 0][np.isfinite(want[0][:, 0])])))
        kinds = np.stack([t, np.nextafter(t, F(np.inf)), t * F(0.5), t * F(1.5), np.zeros(n, F), np.full(n, -1.0, F), np.full(n, np.nan, F), np.full(n, np.inf, F)], axis=1)
    return scalar, kinds[np.arange(n), r.randint(0, kinds.shape[1], n)].astype(F)


# ---- 1. walk == scan == numpy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "cornell", "mesh_spheres", "dup", "chain", "ties"])
def test_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, tab = table(name)
    n = pts.shape[0]
    pt = on_dev(pts)
    scalar, per_query = bounds_of(tab, n, seed=5)
    strided = torch.zeros((n, 3), device=DEV)
    strided[:, 1] = on_dev(per_query)
    assert strided[:, 1].stride() == (3,)
    cases = 0
    for kind, dmax, dev_dmax in (("none", None, None), ("scalar", scalar, scalar), ("tensor", per_query, strided[:, 1])):
        want64 = tab.nearest(64, dmax)
        for k in KS:
            want = prefix(want64, k)
            for count in (True, False):                      # (the two differ in the cull)
                for flags in (0, SCAN):
                    got = device_answer(ex, pt, k, flags, dev_dmax, count, stack_size=2048 if name == "chain" else 64)
                    assert (got[4] is not None) == count
                    assert_same(got, want, (name, kind, k, count, "scan" if flags else "walk"))
                    cases += 1
    assert cases == 3 * 4 * 2 * 2
    finite = np.isfinite(pts).all(axis=1)
    want = tab.nearest(64, None)
    n_surf = geom.tris.shape[0] + geom.spheres.shape[0]
    assert (want[4][finite] == n_surf).all() and (want[4][~finite] == 0).all() and (want[1][~finite] == -1).all()
    assert ex.scene.ctx.stats()["stack_overflow"] == 0


def test_teapot_walk_equals_scan(gpu_ctx_ok):
    ex, geom = scene("teapot")
    assert geom.tris.shape[0] > 12000
    pt = on_dev(query_points(geom, 1024, seed=13))
    first = device_answer(ex, pt, 5, SCAN)
    with np.errstate(all="ignore"):
        col = np.sqrt(first[0][:, 4])
    scalar = float(np.median(col[np.isfinite(col)]))
    r = np.random.RandomState(7)
    with np.errstate(invalid="ignore"):
        per_query = on_dev((col * r.choice(np.array([0.0, 0.5, 1.0, 2.0, np.inf, -1.0], F), 1024)).astype(F))
    for dmax in (None, scalar, per_query):
        for k in (1, 5, 64):
            for count in (True, False):
                scan = device_answer(ex, pt, k, SCAN, dmax, count)
                walk = device_answer(ex, pt, k, 0, dmax, count)
                assert_same(walk, scan, ("teapot", k, count))
    cnt = cpu((PointQuery(ex.scene).count_within(pt, scalar),))[0]
    assert (cnt >= 5).sum() > 100 and (cnt == 0).sum() > 10


# ---- 2. relation to closest() ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mesh_spheres", "ties", "one"])
def test_first_element_is_closest(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, tab = table(name)
    pt = on_dev(pts)
    scalar, per_query = bounds_of(tab, pts.shape[0], seed=9)
    for flags in (0, SCAN):
        q = PointQuery(ex.scene, 64, flags)
        for dmax in (None, scalar, on_dev(per_query)):
            cp = cpu(q.closest(pt, dmax, attributes=True))
            for k in (1, 5, 64):
                for count in (False, True):
                    nn = cpu(q.nearest(pt, k, dmax, attributes=True, count=count))
                    assert nn[0].shape == (pts.shape[0], k) and nn[2].shape == (pts.shape[0], k, 3) and nn[3].shape == (pts.shape[0], k, 2)
                    assert np.array_equal(nn[1][:, 0], cp[1]), (name, flags, k)
                    assert same(nn[0][:, 0], cp[0]) and same(nn[2][:, 0], cp[2]) and same(nn[3][:, 0], cp[3]), (name, flags, k)


# ---- 3. ties at the cut-off -------------------------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut_off(gpu_ctx_ok):
    ex, geom = scene("ties")
    assert geom.tris.shape[0] == 12 and geom.spheres.shape[0] == 0 and list(geom.tri_prim) == list(range(12))
    assert all(np.array_equal(geom.tris[i], geom.tris[2]) for i in TIE_COPIES)
    r = np.random.RandomState(1)
    b = r.dirichlet((1, 1, 1), 64)
    t = geom.tris[2].astype(np.float64)
    near = (t * b[:, :, None]).sum(axis=1) + r.uniform(-0.05, 0.05, (64, 1)) * np.array([0.0, -0.25, 1.0])      # on and just off the copies: nearer to them than to the others
    pts = np.concatenate([near, t, query_points(geom, 192, seed=3)]).astype(F)
    tab = NE.Table(pts, geom)
    for flags in (0, SCAN):
        got = device_answer(ex, pts, 3, flags)
        assert_same(got, tab.nearest(3, None), ("ties", flags))
        assert (got[1][:67] == np.array([2, 3, 4])).all(), got[1][:67]      # the three smallest ids of the eight copies
        assert (got[0][:67, 0:1] == got[0][:67]).all()
        # k = 8 + 1: all copies in id order, then the nearest other
        got = device_answer(ex, pts[:67], 9, flags)
        assert (got[1][:, :8] == np.arange(2, 10)).all() and np.isin(got[1][:, 8], (0, 1, 10, 11)).all()
        # a bound that is exactly the tied distance keeps all eight; the float below it none of them
        d = got[0][:, 0]
        for kk in (3, 64):
            at = device_answer(ex, pts[:67], kk, flags, on_dev(np.sqrt(d.astype(np.float64)).astype(F)))
            want = tab_rows(tab, 67).nearest(kk, np.sqrt(d.astype(np.float64)).astype(F))
            assert_same(at, want, ("ties at the bound", flags, kk))
            assert np.isin(at[4], (0, 8)).all()              # dmax * dmax rounds to D2 or just below it: all eight or none, never some
        # k larger than the primitive count pads with (inf, -1, 0, 0)
        full = device_answer(ex, pts, 64, flags)
        finite = np.isfinite(pts).all(axis=1)
        assert (full[4][finite] == 12).all() and (full[1][finite, :12] >= 0).all() and (full[1][:, 12:] == -1).all()
        assert np.isposinf(full[0][:, 12:]).all() and (full[2][:, 12:] == 0).all() and (full[3][:, 12:] == 0).all()
        assert (np.sort(full[1][finite, :12], axis=1) == np.arange(12)).all()      # every primitive once


def tab_rows(tab, n):
    """the first n rows of a restatement table"""
    t = NE.Table.__new__(NE.Table)
    t.n, t.d2, t.q, t.u, t.v, t.prim = n, tab.d2[:n], tab.q[:n], tab.u[:n], tab.v[:n], tab.prim
    return t


# ---- 4. bounds and counts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mesh_spheres"])
def test_bounds_and_counts(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, tab = table(name)
    n, k = pts.shape[0], 5
    free = tab.nearest(64, None)
    assert tab.prim.size >= k + 2
    cls = np.random.RandomState(21).randint(0, 3, n)
    with np.errstate(all="ignore"):
        d = np.sqrt(free[0].astype(np.float64))
        dmax = np.select([cls == 0, cls == 1], [0.5 * d[:, 0], 0.5 * (d[:, 1] + d[:, 2])], 1.01 * d[:, k + 1]).astype(F)
    dmax[~np.isfinite(dmax)] = F(1.0)                        # (the non-finite queries: any bound, nothing is found)
    want = tab.nearest(k, dmax)
    cnt = want[4]
    sizes = ((cnt == 0).sum(), ((cnt > 0) & (cnt < k)).sum(), (cnt > k).sum())
    assert min(sizes) >= n // 10, sizes                      # each class holds at least a tenth of the queries
    pt, dm = on_dev(pts), on_dev(dmax)
    for flags in (0, SCAN):
        q = PointQuery(ex.scene, 64, flags)
        for count in (True, False):
            assert_same(device_answer(ex, pt, k, flags, dm, count), want, (name, flags, count))
        cw = cpu((q.count_within(pt, dm),))[0]
        assert cw.dtype == np.int32 and np.array_equal(cw, cnt)
        alone = q.nearest(pt, 0, dm, attributes=True, count=True)      # k = 0 with the count: the count alone
        assert alone.dist2.shape == (n, 0) and alone.prim.shape == (n, 0) and alone.point.shape == (n, 0, 3) and alone.uv.shape == (n, 0, 2)
        assert np.array_equal(cpu((alone.count,))[0], cnt)
        # a scalar bound, and the count without a bound (every surface primitive of the scene, for every finite query)
        s = float(np.median(dmax))
        assert np.array_equal(cpu((q.count_within(pt, s),))[0], tab.nearest(0, s)[4])
        assert np.array_equal(cpu((q.count_within(pt, float("inf")),))[0], free[4])
        for bad in (-1.0, float("nan")):
            assert (cpu((q.count_within(pt, bad),))[0] == 0).all()


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------------------------------
def equal_answers(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_layouts_empty_and_single(gpu_ctx_ok):
    ex, geom = scene("cornell")
    pts, tab = table("cornell")
    pt = on_dev(pts)
    n = pt.shape[0]
    q = PointQuery(ex.scene)
    _, per_query = bounds_of(tab, n, seed=5)
    dm = on_dev(per_query)
    base = q.nearest(pt, 4, dm, attributes=True, count=True)
    wide = torch.full((n, 8), 7.0, device=DEV)
    wide[:, :3] = pt
    assert wide[:, :3].stride() == (8, 1)
    assert equal_answers(q.nearest(wide[:, :3], 4, dm, attributes=True, count=True), base)
    rows = torch.full((2 * n, 3), -5.0, device=DEV)
    rows[::2] = pt
    assert equal_answers(q.nearest(rows[::2], 4, dm, attributes=True, count=True), base)
    sd = torch.full((n, 5), -3.0, device=DEV)
    sd[:, 2] = dm
    assert sd[:, 2].stride() == (5,)
    assert equal_answers(q.nearest(pt, 4, sd[:, 2], attributes=True, count=True), base)
    plain = q.nearest(pt, 4, dm)
    assert plain.point is None and plain.uv is None and plain.count is None and equal_answers(plain[:2], base[:2])
    e = q.nearest(pt[:0], 4, attributes=True, count=True)
    assert e.dist2.shape == (0, 4) and e.prim.shape == (0, 4) and e.point.shape == (0, 4, 3) and e.uv.shape == (0, 4, 2) and e.count.shape == (0,)
    assert q.count_within(pt[:0], 1.0).shape == (0,)
    one = cpu(q.nearest(pt[5:6], 4, 1.0e9, attributes=True, count=True))
    assert_same(one, tuple(w[5:6] for w in tab.nearest(4, 1.0e9)), "n == 1")
    with pytest.raises(ValueError):
        q.nearest(pt, 4, dm[:-1])
    with pytest.raises(TypeError):
        q.nearest(pt, 4, dm.double())


def test_chunking(gpu_ctx_ok):
    ex, geom = scene("mesh_spheres")
    ctx = ex.scene.ctx
    pt = on_dev(query_points(geom, 1000, seed=17))
    q = PointQuery(ex.scene)
    dm = q.nearest(pt, 4).dist2[:, 3].sqrt() * 1.5
    a = [q.nearest(pt, 4, dm, attributes=True, count=c) for c in (True, False)]
    ctx.set_option("query_chunk_rays", 256)                  # max(256, 256 / 4) = 256 queries: four chunks
    try:
        b = [q.nearest(pt, 4, dm, attributes=True, count=c) for c in (True, False)]
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert equal_answers(a[0], b[0]) and equal_answers(a[1], b[1])
    assert (a[0].count > 4).any() and (a[0].prim[:, 3] >= 0).any()


def test_ordered_on_the_callers_stream(gpu_ctx_ok):
    ex, geom = scene("mesh_spheres")
    src = on_dev(query_points(geom, 2048, seed=19))
    q = PointQuery(ex.scene)
    want = q.nearest(src, 8, 0.5, attributes=True, count=True)
    want_sum = want.dist2.nan_to_num(posinf=3.0).sum(dim=1) * 2.0 + want.prim.float().sum(dim=1) + want.point.sum(dim=(1, 2)) + want.count.float()
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(8):                                 # keep the side stream busy before the points exist
            big = torch.tanh(big @ big)
        pt = torch.where(big[0, 0] > 2.0, src * 0.0, src)   # (tanh <= 1: an exact copy of src, made after the products)
        h = q.nearest(pt, 8, 0.5, attributes=True, count=True)
        consumer = h.dist2.nan_to_num(posinf=3.0).sum(dim=1) * 2.0 + h.prim.float().sum(dim=1) + h.point.sum(dim=(1, 2)) + h.count.float()
    torch.cuda.synchronize(DEV)
    assert torch.equal(h.prim, want.prim) and torch.equal(consumer.view(torch.int32), want_sum.view(torch.int32))


def test_host_route_equals_torch_route(gpu_ctx_ok):
    ex, geom = scene("mesh_spheres")
    ctx = ex.scene.ctx
    pts, tab = table("mesh_spheres")
    _, per_query = bounds_of(tab, pts.shape[0], seed=5)
    for k in (1, 5):
        got = ctx.nearest(pts, k)
        assert got[5] is None
        assert_same(got[:5], tab.nearest(k, None), ("host route", k))
        for flags in (0, SCAN, COUNT):
            got = ctx.nearest(pts, k, per_query, 64, flags)
            assert_same(got[:5], device_answer(ex, pts, k, flags & SCAN, on_dev(per_query)), ("host route, bound", k, flags))
            if flags & COUNT:
                counts = torch.empty((pts.shape[0], 2), dtype=torch.int32, device=DEV)
                d2 = torch.empty((pts.shape[0], k), device=DEV)
                cnt = torch.empty(pts.shape[0], dtype=torch.int32, device=DEV)
                pt, dm = on_dev(pts), on_dev(per_query)
                ctx.query_nearest(pt.data_ptr(), pts.shape[0], 3, k, 64, COUNT, dmax=dm.data_ptr(), out_d2=d2.data_ptr(), out_count=cnt.data_ptr(),
                                  counts=counts.data_ptr(), stream=torch.cuda.current_stream(DEV).cuda_stream)
                assert np.array_equal(got[5], cpu((counts,))[0])
                finite = np.isfinite(pts).all(axis=1) & (per_query >= 0)
                assert (got[5][~finite] == 0).all() and (got[5][finite, 0] > 0).all()
    d2, prim, q, uv, cnt, _ = ctx.nearest(pts[:10], 3, 0.5, attributes=False, count=False)
    assert q is None and uv is None and cnt is None and same(d2, device_answer(ex, pts[:10], 3, 0, 0.5)[0])
    d2, prim, q, uv, cnt, _ = ctx.nearest(pts, 0, 0.5)
    assert d2.shape == (pts.shape[0], 0) and np.array_equal(cnt, tab.nearest(0, 0.5)[4])
    assert ctx.nearest(np.zeros((0, 3), F), 3)[0].shape == (0, 3)
    scan_counts = ctx.nearest(pts[:64], 2, None, 64, SCAN | COUNT)[5]
    assert (scan_counts[:, 0] == 0).all() and (scan_counts[:, 1] == ex.scene.primitive_count).all()


def test_refusals_queue_nothing(gpu_ctx_ok):
    ex, geom = scene("cornell")
    ctx = ex.scene.ctx
    pts, _ = table("cornell")
    pt = on_dev(pts[:100])
    host = np.ascontiguousarray(pts[:100])
    out = torch.full((100, 4), -7.0, device=DEV)
    out3 = torch.full((100, 4, 3), -7.0, device=DEV)
    outc = torch.full((100,), -7, dtype=torch.int32, device=DEV)
    lib = _native.lib()
    P = dict(points=pt.data_ptr(), n=100, point_stride=3, k=4)
    cases = [
        (r"error -2:.*k outside 0..TIRT_NEAREST_MAX", dict(P, k=65, out_d2=out.data_ptr())),
        (r"error -2:.*k outside 0..TIRT_NEAREST_MAX", dict(P, k=-1, out_d2=out.data_ptr())),
        (r"error -2:.*k == 0 without out_count", dict(P, k=0, out_d2=out.data_ptr())),
        (r"error -2:.*no output at all", dict(P)),
        (r"error -2:.*points: not device memory", dict(P, points=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*dmax: not device memory", dict(P, dmax=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*out_point: not device memory", dict(P, out_d2=out.data_ptr(), out_point=host.ctypes.data)),
        (r"error -2:.*out_count: not device memory", dict(P, out_d2=out.data_ptr(), out_count=host.ctypes.data)),
        (r"error -2:.*point_stride < 3", dict(P, point_stride=2, out_d2=out.data_ptr())),
        (r"error -2:.*point_out_stride < 3", dict(P, out_d2=out.data_ptr(), out_point=out3.data_ptr(), point_out_stride=2)),
        (r"error -2:.*uv_stride < 2", dict(P, out_d2=out.data_ptr(), out_uv=out3.data_ptr(), uv_stride=1)),
        (r"error -2:.*dmax_stride < 1", dict(P, dmax=outc.data_ptr(), dmax_stride=0, out_d2=out.data_ptr())),
        (r"error -2:.*unknown flags", dict(P, flags=4, out_d2=out.data_ptr())),
        (r"error -2:.*stack_size", dict(P, stack_size=0, out_d2=out.data_ptr())),
        (r"error -2:.*counts must be 8-byte aligned", dict(P, flags=COUNT, out_d2=out.data_ptr(), counts=outc.data_ptr() + 4)),
    ]
    for pattern, kw in cases:
        with pytest.raises(_native.TirtError, match=pattern):
            ctx.query_nearest(**kw)
        assert lib.tirt_last_error()                         # the message is there for a C caller too
    unbuilt = _native.Context(0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*LBVH not built"):
        unbuilt.query_nearest(pt.data_ptr(), 100, 3, 4, out_d2=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.nearest(host, 4)
    torch.cuda.synchronize(DEV)
    assert (out == -7.0).all() and (out3 == -7.0).all() and (outc == -7).all()      # nothing ran
    s = torch.cuda.Stream(DEV)
    x = torch.zeros(16, device=DEV)
    with torch.cuda.stream(s):
        x.add_(1.0)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_native.TirtError, match="capturing"):
        with torch.cuda.graph(g, stream=s):
            x.add_(1.0)
            PointQuery(ex.scene).nearest(pt, 4)


def sphere_obj_triangles():
    ex = Example.example(8, 8, 1, 0)
    ex.scene.add_obj(scenes.asset("model", "sphere.obj"))
    ex.scene.setup_data_cpu()
    return E.scene_geometry(ex.scene).tris.astype(np.float64)


def test_after_update_vertices(gpu_ctx_ok):
    tris = sphere_obj_triangles()
    ext = (tris.reshape(-1, 3).max(axis=0) - tris.reshape(-1, 3).min(axis=0)).max()
    half = tris.shape[0] // 2
    moved = tris.copy()
    moved[:half] += np.array([0.3 * ext, 0.0, 0.0])
    ex = custom_scene(tris)
    ex.build_scene()
    pts = query_points(E.scene_geometry(ex.scene), 1024, seed=31)
    before = device_answer(ex, pts, 5, 0, 0.2 * ext)
    ex.scene.update_vertices(moved[:half].astype(F), first_vertex=0)
    fresh = custom_scene(moved)
    fresh.build_scene()
    a, b = device_answer(ex, pts, 5, 0, 0.2 * ext), device_answer(fresh, pts, 5, 0, 0.2 * ext)
    assert_same(a, b, "updated against fresh")
    assert_same(a, device_answer(ex, pts, 5, SCAN, 0.2 * ext), "updated walk against scan")
    assert_same(device_answer(ex, pts, 5, 0, None, count=False), device_answer(ex, pts, 5, SCAN, None, count=False), "updated walk against scan, no bound")
    assert not np.array_equal(a[1], before[1]) and not np.array_equal(a[4], before[4])      # the answers did move


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    W = H = 32
    films, rays = [], []
    for with_queries in (False, True):
        ex = scenes.cornell_box(W, H, 8, device_id=0)
        ex.build_scene()
        pt = on_dev(query_points(E.scene_geometry(ex.scene), 2048, seed=23))
        q = PointQuery(ex.scene)
        ex.scene.ctx.stats_reset()
        for f in (0, 2, 4):
            ex.cam.frame = f; ex.cam.frame_cpu[0] = f
            ex.integrator.render_frames(2)
            if with_queries:
                q.nearest(pt, 8, attributes=True)
                q.nearest(pt, 3, 100.0, count=True)
                q.count_within(pt, 50.0)
            else:
                ex.scene.ctx.sync()
        films.append(ex.integrator.hdr.to_numpy())
        st = ex.scene.ctx.stats()
        rays.append((st["rays_closest"], st["rays_shadow"]))
    assert np.array_equal(films[0].view(np.int32), films[1].view(np.int32))
    assert (films[0] != 0).any()
    assert rays[0] == rays[1] and rays[0][0] > 0             # the queries are not rays: no ray counter moved


# ---- 6. the stack --------------------------------------------------------------------------------------------------------------------------------------
def test_long_chain_and_stack_overflow(gpu_ctx_ok):
    """the 600-deep duplicate-Morton chain: a 2048-entry stack (16 in LDS, the rest in global memory) gives the scan's answers, a 4-entry stack drops
    entries and tirt_stats says so (nothing faults), and the next call is right again"""
    ex, geom = scene("chain")
    ctx = ex.scene.ctx
    pts, tab = table("chain")
    scan = device_answer(ex, pts, 5, SCAN)
    ctx.stats_reset()
    assert_same(device_answer(ex, pts, 5, 0, stack_size=2048), scan, "stack 2048")
    assert ctx.stats()["stack_overflow"] == 0
    small = device_answer(ex, pts, 5, 0, stack_size=4)
    with pytest.raises(_native.TirtStackOverflow) as err:
        ctx.stats()
    assert 0 < err.value.stats["stack_overflow"] <= pts.shape[0]
    assert_lists_valid(small, "stack 4")                     # fewer primitives were met, but what was met is a list
    assert (small[4] <= scan[4]).all()
    ctx.stats_reset()
    assert_same(device_answer(ex, pts, 5, 0, stack_size=2048), scan, "stack 2048 again")
    assert ctx.stats()["stack_overflow"] == 0


def test_stack_sizes_around_the_lds_part(gpu_ctx_ok):
    """stacks that end just below, at and just beyond the 16 entries a lane has in LDS (at 16 there is no tail and the spill pointer is null, at 17 the
    tail is one entry per thread), and 64, on the Teapot: the culled walk of k = 5 (shallow stacks), the count within a bound, and the count of everything
    without a bound, which visits every leaf and is the deepest the stack gets.  A query can only differ from the scan if it dropped an entry, a query
    that fits a stack fits every larger one, answers are equal where nothing overflows, and 64 entries hold the Teapot's tree."""
    ex, geom = scene("teapot")
    ctx = ex.scene.ctx
    pts = query_points(geom, 1024, seed=29)
    pt = on_dev(pts)
    with np.errstate(all="ignore"):
        col = np.sqrt(device_answer(ex, pt, 5, SCAN)[0][:, 4])
    bound = float(np.median(col[np.isfinite(col)]))
    sizes = (15, 16, 17, 64)
    reached = False
    for k, count, dmax in ((5, False, None), (5, True, bound), (64, True, None)):
        scan = device_answer(ex, pt, k, SCAN, dmax, count)
        over, miss, answers = [], [], []
        for s in sizes:
            ctx.stats_reset()
            got = device_answer(ex, pt, k, 0, dmax, count, stack_size=s)
            try:
                over.append(ctx.stats()["stack_overflow"])
            except _native.TirtStackOverflow as err:
                over.append(err.stats["stack_overflow"])
            differs = (got[0].view(np.uint32) != scan[0].view(np.uint32)).any(axis=1) | (got[1] != scan[1]).any(axis=1)
            if count:
                differs |= got[4] != scan[4]
            miss.append(int(differs.sum()))
            answers.append(got)
        ctx.stats_reset()
        print("k %d, count %s, bound %s, stack sizes %s: queries that dropped an entry %s, queries that differ from the scan %s" % (k, count, dmax, sizes, over, miss))
        assert all(m <= o for m, o in zip(miss, over)), (sizes, over, miss)
        assert all(a >= b for a, b in zip(over, over[1:])), (sizes, over)
        assert over[-1] == 0 and miss[-1] == 0
        for s, o, got in zip(sizes, over, answers):
            if o == 0:
                assert_same(got, scan, ("stack", s, k, count))      # equal answers where nothing overflows
        reached = reached or over[0] > 0
    assert reached, "no lane needed more than 15 entries: the sizes around the 16 in LDS test nothing"
