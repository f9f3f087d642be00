"""Pair lists on the device (csrc/tirt_pairs.hip through tirt_query_point_pairs / tirt_query_mesh_pairs / tirt_point_pairs / tirt_mesh_pairs and
PointQuery.within / TriangleQuery.pairs / .count_within) against the definitions "Point pairs" and "Triangle pairs" of include/tirt.h as
tests/pairs_expected.py restates them.  Every comparison is on bits: the culled walk against the scan over all primitives (both on the device) and both
against numpy; then the links to closest(), nearest(), count_within() and collides(), the row-length regimes of the order pass, the scan over more than
one block, the capacity rule, the modes and flags, chunking, the plumbing, moving geometry and the stack."""
import numpy as np
import pytest
import torch

import closest_point_expected as CE
import pairs_expected as PE
from common import custom_scene, duplicate_code_scene, long_chain_scene, same_bits as same
from test_gpu_nearest import query_points, sphere_obj_triangles
from test_gpu_triangle_query import box_mesh, query_triangles
from ti_raytrace_amd import PointQuery, TriangleQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN, COUNT, UNORDERED = _native.TRAVERSE_EXHAUSTIVE, _native.COUNT_NODES, _native.PAIRS_UNORDERED
N = 200                                                      # queries per scene: not a multiple of 64
NAMES = ["one", "two", "cornell", "dup", "chain", "tied"]
TWO = [[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]]
_SCENES, _TABLES = {}, {}


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    torch.cuda.synchronize(DEV)
    return tuple(None if x is None else x.cpu().numpy() for x in h)


def scene(name):
    """(built example, its Geometry), built once per module: the tiny scenes of the triangle-query tests, the Cornell box and the Teapot"""
    if name not in _SCENES:
        r = np.random.RandomState(3)
        if name == "one":                                    # a one-primitive scene: the root's code is a leaf code
            ex = custom_scene(TWO[:1], spheres=())
        elif name == "two":                                  # two triangles and an analytic sphere: in a point's rows, in no triangle's
            ex = custom_scene(TWO, spheres=((0.3, 0.4, 1.5, 0.5),))
        elif name == "cornell":
            ex = scenes.cornell_box(16, 16, 1, device_id=0)
        elif name == "dup":
            ex = duplicate_code_scene(16, 16, device_id=0)
        elif name == "chain":
            ex = long_chain_scene(16, 16)
        elif name == "tied":                                 # 6 triangles, 8 coincident copies of each, interleaved: every distance ties 8 ways across ids
            ex = custom_scene(np.tile(r.uniform(-1, 1, (6, 3, 3)), (8, 1, 1)), spheres=())
        elif name == "teapot":
            ex = scenes.single_model(16, 16, 1, device_id=0)
        else:
            raise KeyError(name)
        ex.build_scene()
        _SCENES[name] = (ex, CE.scene_geometry(ex.scene))
    return _SCENES[name]


def tables(name):
    """the queries of scene `name` (points and triangles, some with NaN or Inf coordinates) and the restatement's tables, made once and left unchanged"""
    if name not in _TABLES:
        ex, geom = scene(name)
        pts, tris = query_points(geom, N, seed=11), query_triangles(geom, N, seed=11)
        assert not np.isfinite(pts).all() and not np.isfinite(tris).all()
        _TABLES[name] = (pts, PE.PointTable(pts, geom), tris, PE.TriangleTable(tris, geom))
    return _TABLES[name]


def bounds_of(d2, seed):
    """from a table of D2 [n, P]: a scalar bound (the median distance of the third element) and a per-query tensor that mixes the distance of a random
    element, the float above it, half of it, 0, -1, NaN and +inf"""
    n = d2.shape[0]
    r = np.random.RandomState(seed)
    with np.errstate(all="ignore"):
        s = np.sort(np.where(np.isfinite(d2), d2, F(np.inf)), axis=1)
        col = np.sqrt(s[:, min(2, s.shape[1] - 1)])
        scalar = float(np.median(col[np.isfinite(col)]))
        t = np.sqrt(s[np.arange(n), r.randint(0, min(s.shape[1], 12), n)]).astype(F)
        t = np.where(np.isfinite(t), t, F(1.0)).astype(F)
        kinds = np.stack([t, np.nextafter(t, F(np.inf)), t * F(0.5), t * F(1.5), np.zeros(n, F), np.full(n, -1.0, F), np.full(n, np.nan, F), np.full(n, np.inf, F)], axis=1)
    return scalar, kinds[np.arange(n), r.randint(0, kinds.shape[1], n)].astype(F)


def within(ex, pt, dmax, flags=0, stack_size=64, **kw):
    return cpu(PointQuery(ex.scene, stack_size, flags).within(pt if isinstance(pt, torch.Tensor) else on_dev(pt), dmax, attributes=True, **kw))


def pairs(ex, tris, dmax, flags=0, stack_size=64, **kw):
    return cpu(TriangleQuery(ex.scene, stack_size, flags).pairs(tris if isinstance(tris, torch.Tensor) else on_dev(tris), dmax, points=True, **kw))


def assert_same(got, want, what):
    """row_start and the ids first (they say where), then every other output bit for bit"""
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), (what, "row_start", np.nonzero(np.diff(got[0]) != np.diff(want[0]))[0][:8])
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, (what, "prim", bad[:8], got[1][bad[:8]], want[1][bad[:8]])
    assert same(got[2], want[2]), (what, "d2")
    for k in range(3, len(want)):
        if got[k].dtype == np.int32:
            assert np.array_equal(got[k], want[k]), (what, "code", np.nonzero(got[k] != want[k])[0][:8])
        else:
            assert same(got[k], want[k]), (what, "output %d" % k)


def assert_rows_valid(got, what):
    """every row in the definition's order, no primitive twice"""
    rs, prim, d2 = got[0], got[1], got[2]
    q = PE.query_of(rs)
    assert np.array_equal(np.lexsort((prim, d2.view(np.uint32), q)), np.arange(q.size)), (what, "not ordered")
    assert np.unique(q.astype(np.int64) << 32 | prim).size == q.size, (what, "a primitive appears twice in a row")


def host_sorted(got):
    """an unordered result with every row put into the definition's order on the host"""
    q = PE.query_of(got[0])
    order = np.lexsort((got[1], got[2].view(np.uint32), q))
    return (got[0],) + tuple(x[order] for x in got[1:])


def equal_tensors(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y))
               for x, y in zip(a, b))


# ---- 1. walk == scan == numpy, every output ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_points_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, tab, _, _ = tables(name)
    pt = on_dev(pts)
    scalar, per_query = bounds_of(tab.d2, seed=5)
    stack = 2048 if name == "chain" else 64
    for kind, dmax, dev in (("none", None, None), ("scalar", scalar, scalar), ("tensor", per_query, on_dev(per_query)), ("zero", 0.0, 0.0), ("negative", -1.0, -1.0),
                            ("nan", np.nan, float("nan"))):
        want = tab.within(dmax)
        for flags in (SCAN, 0):
            assert_same(within(ex, pt, dev, flags, stack), want, (name, kind, "scan" if flags else "walk"))
        if kind in ("negative", "nan"):
            assert want[0][-1] == 0
    finite = np.isfinite(pts).all(axis=1)
    free = np.diff(tab.within(None)[0])
    assert (free[finite] == geom.tris.shape[0] + geom.spheres.shape[0]).all() and (free[~finite] == 0).all() and (~finite).sum() == 9
    assert ex.scene.ctx.stats()["stack_overflow"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_triangles_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom = scene(name)
    _, _, tris, tab = tables(name)
    tq = on_dev(tris)
    scalar, per_query = bounds_of(tab.d2, seed=6)
    stack = 2048 if name == "chain" else 64
    for kind, dmax, dev in (("none", None, None), ("scalar", scalar, scalar), ("tensor", per_query, on_dev(per_query)), ("zero", 0.0, 0.0), ("negative", -1.0, -1.0),
                            ("nan", np.nan, float("nan"))):
        want = tab.pairs(dmax)
        for flags in (SCAN, 0):
            assert_same(pairs(ex, tq, dev, flags, stack), want, (name, kind, "scan" if flags else "walk"))
        if kind in ("negative", "nan"):
            assert want[0][-1] == 0
    finite = np.isfinite(tris).all(axis=(1, 2))
    free = tab.pairs(None)
    assert (np.diff(free[0])[finite] == geom.tris.shape[0]).all() and (np.diff(free[0])[~finite] == 0).all() and (~finite).sum() == 9
    assert np.isin(free[1], geom.tri_prim).all()             # an analytic sphere is in nobody's row
    if name in ("cornell", "dup", "chain"):
        assert tab.pairs(0.0)[0][-1] > 50                    # the contact list is not empty
    assert ex.scene.ctx.stats()["stack_overflow"] == 0


# ---- 2. the links to the sibling queries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "two", "tied"])
def test_point_rows_link_to_closest_nearest_and_count(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, tab, _, _ = tables(name)
    pt = on_dev(pts)
    scalar, per_query = bounds_of(tab.d2, seed=9)
    for flags in (0, SCAN):
        q = PointQuery(ex.scene, 64, flags)
        for dmax in (None, scalar, on_dev(per_query)):
            rs, prim, d2, point, uv = cpu(q.within(pt, dmax, attributes=True))
            cp = cpu(q.closest(pt, dmax, attributes=True))
            nn = cpu(q.nearest(pt, 5, dmax, attributes=True, count=True))
            n = np.diff(rs)
            assert np.array_equal(n, nn[4]) and np.array_equal(n > 0, cp[1] >= 0)
            if dmax is not None:
                assert np.array_equal(n, cpu((q.count_within(pt, dmax),))[0])
            first = rs[:-1][n > 0]
            assert np.array_equal(prim[first], cp[1][n > 0]) and same(d2[first], cp[0][n > 0]) and same(point[first], cp[2][n > 0]) and same(uv[first], cp[3][n > 0])
            for j in range(5):                               # element j of every row that has one against column j of nearest(5)
                has = n > j
                at = rs[:-1][has] + j
                assert np.array_equal(prim[at], nn[1][has, j]) and same(d2[at], nn[0][has, j]) and same(point[at], nn[2][has, j]) and same(uv[at], nn[3][has, j])
                assert (nn[1][~has, j] == -1).all()
            assert (n > 1).any() and (n == 0).any()


@pytest.mark.parametrize("name", ["cornell", "dup"])
def test_triangle_rows_link_to_closest_count_and_collides(gpu_ctx_ok, name):
    ex, geom = scene(name)
    _, _, tris, tab = tables(name)
    tq = on_dev(tris)
    scalar, per_query = bounds_of(tab.d2, seed=10)
    for flags in (0, SCAN):
        q = TriangleQuery(ex.scene, 64, flags)
        for dmax in (0.0, None, scalar, on_dev(per_query)):
            rs, prim, d2, code, P, Q = cpu(q.pairs(tq, dmax, points=True))
            cp = cpu(q.closest(tq, dmax, points=True))
            n = np.diff(rs)
            assert np.array_equal(n > 0, cp[1] >= 0)
            first = rs[:-1][n > 0]
            assert np.array_equal(prim[first], cp[1][n > 0]) and same(d2[first], cp[0][n > 0]) and np.array_equal(code[first], cp[2][n > 0])
            assert same(P[first], cp[3][n > 0]) and same(Q[first], cp[4][n > 0])
            if dmax is not None:
                cw = cpu((q.count_within(tq, dmax),))[0]
                assert cw.dtype == np.int32 and np.array_equal(cw, n)
        contact = cpu(q.pairs(tq))                           # the default bound is 0: the contact pair list
        hit = cpu((q.collides(tq),))[0]
        assert np.array_equal(np.diff(contact[0]) > 0, hit) and hit.any() and not hit.all() and (contact[2] == 0).all()
        assert contact[4] is None and contact[5] is None
    v, f = box_mesh((155.0, 130.0, -200.0), (215.0, 190.0, -140.0))      # a box pushed into the top of the Cornell box's short block
    if name == "cornell":
        mesh = TriangleQuery(ex.scene).pairs((on_dev(v), on_dev(f)))
        got = cpu(mesh)
        assert (np.diff(got[0]) > 0).tolist() == [True] * 4 + [False] * 4 + [True] * 4
        assert np.array_equal(cpu((mesh.query(),))[0], PE.query_of(got[0]))
        assert_same(got[:4], PE.TriangleTable(v[f], geom).pairs(0.0)[:4], "box mesh")


# ---- 3. the row-length regimes of the order pass -------------------------------------------------------------------------------------------------------
def test_teapot_row_lengths_on_both_sides_of_64_and_1024(gpu_ctx_ok):
    ex, geom = scene("teapot")
    n_prim = geom.tris.shape[0] + geom.spheres.shape[0]
    assert n_prim > 4096
    r = np.random.RandomState(4)
    t = geom.tris.astype(np.float64)
    ext = (t.reshape(-1, 3).max(axis=0) - t.reshape(-1, 3).min(axis=0)).max()
    # one query with no bound: a single row of all primitives, which is ordered in place in global memory
    one = t[r.randint(0, t.shape[0], 1)].mean(axis=1).astype(F)
    tab1 = PE.PointTable(one, geom)
    for flags in (SCAN, 0):
        got = within(ex, one, None, flags)
        assert got[0].tolist() == [0, n_prim]
        assert_same(got, tab1.within(None), ("one row of all", flags))
    # 64 queries on the surface with a ladder of bounds: rows from a handful of pairs to all of them
    pts = t[r.randint(0, t.shape[0], 64)].mean(axis=1).astype(F)
    dmax = (ext * 10.0 ** np.linspace(-2.3, 0.3, 64)).astype(F)
    want = PE.PointTable(pts, geom).within(dmax)
    n = np.diff(want[0])
    sides = ((n < 64).sum(), ((n > 64) & (n < 1024)).sum(), (n > 1024).sum())
    assert min(sides) >= 5, sides                            # both sides of a wave and of the longest row that is ordered in LDS
    for flags in (SCAN, 0):
        got = within(ex, pts, on_dev(dmax), flags)
        assert_same(got, want, ("ladder", flags))
        assert_rows_valid(got, ("ladder", flags))
    assert np.array_equal(cpu((PointQuery(ex.scene).count_within(on_dev(pts), on_dev(dmax)),))[0], n)
    # triangles: the code travels with its pair through both paths of the order pass
    tris = (t[r.randint(0, t.shape[0], 12)] + r.uniform(-0.01, 0.01, (12, 3, 3)) * ext).astype(F)
    tmax = (ext * 10.0 ** np.linspace(-2.0, 0.3, 12)).astype(F)
    want = PE.TriangleTable(tris, geom).pairs(tmax)
    n = np.diff(want[0])
    assert (n < 64).any() and ((n > 64) & (n < 1024)).any() and (n > 1024).any(), n
    for flags in (SCAN, 0):
        assert_same(pairs(ex, tris, on_dev(tmax), flags), want, ("triangle ladder", flags))


# ---- 4. the scan over more than one block --------------------------------------------------------------------------------------------------------------
def test_row_start_of_70000_queries(gpu_ctx_ok):
    ex, geom = scene("cornell")
    t = geom.tris.astype(np.float64).reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    pt = on_dev((lo + (hi - lo) * np.random.RandomState(8).uniform(-0.1, 1.1, (70000, 3))).astype(F))      # 69 blocks of the scan: the block sums are themselves scanned
    bound = 0.08 * float((hi - lo).max())
    q = PointQuery(ex.scene)
    h = q.within(pt, bound)
    cnt = q.count_within(pt, bound)
    torch.cuda.synchronize(DEV)
    want = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(cnt.long(), 0)])
    assert h.row_start.dtype == torch.int64 and torch.equal(h.row_start, want)
    assert h.prim.shape[0] == int(want[-1]) and (cnt == 0).any() and (cnt > 2).any()
    assert_rows_valid(cpu(h[:3]), "70000 queries")
    idx = h.query()
    assert idx.shape == h.prim.shape and torch.equal(torch.bincount(idx, minlength=70000), cnt.long())
    assert (h.prim >= 0).all() and (h.prim < ex.scene.primitive_count).all()


# ---- 5. the capacity rule, the modes and the flags -----------------------------------------------------------------------------------------------------
def raw_call(ex, tri, query, dmax, mode, capacity, flags=0, stack_size=64, row_start=None, size=None, fill=-7):
    """tirt_query_point_pairs / tirt_query_mesh_pairs on arrays the test pre-fills: (row_start, prim, d2, code) as tensors of `size` pairs"""
    ctx = ex.scene.ctx
    n = query.shape[0]
    size = capacity if size is None else size
    rs = torch.full((n + 1,), fill, dtype=torch.int64, device=DEV) if row_start is None else row_start.clone()
    prim = torch.full((size,), fill, dtype=torch.int32, device=DEV)
    d2 = torch.full((size,), float(fill), dtype=torch.float32, device=DEV)
    code = torch.full((size,), fill, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if tri:
        ctx.query_mesh_pairs(query.data_ptr(), n, 9, mode, rs.data_ptr(), capacity=capacity, stack_size=stack_size, flags=flags, dmax_all=dmax, out_d2=d2.data_ptr(),
                             out_prim=prim.data_ptr(), out_code=code.data_ptr(), stream=stream)
    else:
        ctx.query_point_pairs(query.data_ptr(), n, 3, mode, rs.data_ptr(), capacity=capacity, stack_size=stack_size, flags=flags, dmax_all=dmax, out_d2=d2.data_ptr(),
                              out_prim=prim.data_ptr(), stream=stream)
    torch.cuda.synchronize(DEV)
    return rs, prim, d2, code


@pytest.mark.parametrize("tri", [False, True])
def test_capacity_whole_rows_only(gpu_ctx_ok, tri):
    ex, geom = scene("cornell")
    pts, ptab, tris, ttab = tables("cornell")
    query = on_dev(tris if tri else pts)
    dmax = bounds_of((ttab if tri else ptab).d2, seed=12)[0]
    want = (ttab.pairs(dmax) if tri else ptab.within(dmax))
    rs = want[0]
    total = int(rs[-1])
    k = int(np.nonzero(np.diff(rs) > 1)[0][N // 2])          # a row of at least two pairs in the middle
    end = int(rs[k + 1])
    for capacity in (end, end - 1, 0, total):
        got = raw_call(ex, tri, query, dmax, _native.PAIRS_BOTH, capacity, size=total + 64)
        rows, written = PE.rows_that_fit(rs, capacity)
        assert np.array_equal(got[0].cpu().numpy(), rs), capacity      # row_start is complete in every case
        assert np.array_equal(got[1][:written].cpu().numpy(), want[1][:written]) and same(got[2][:written].cpu().numpy(), want[2][:written]), capacity
        if tri:
            assert np.array_equal(got[3][:written].cpu().numpy(), want[3][:written]), capacity
        assert (got[1][written:] == -7).all() and (got[2][written:] == -7.0).all() and (got[3][written if tri else 0:] == -7).all(), capacity      # the sentinel stands
    # (row k is the last one written at `end` but for empty rows behind it, and is cut whole one pair short of it)
    assert PE.rows_that_fit(rs, end)[0] >= k + 1 and PE.rows_that_fit(rs, end)[1] == end and PE.rows_that_fit(rs, end - 1) == (k, int(rs[k])) and PE.rows_that_fit(rs, 0)[1] == 0
    # the torch front end with a capacity: no host wait, the rows that fit, query() of those rows alone
    front = (TriangleQuery(ex.scene).pairs(query, dmax, capacity=end - 1) if tri else PointQuery(ex.scene).within(query, dmax, capacity=end - 1))
    rows, written = PE.rows_that_fit(rs, end - 1)
    assert front.prim.shape[0] == end - 1 and int(front.row_start[-1]) == total > end - 1
    assert np.array_equal(front.prim[:written].cpu().numpy(), want[1][:written]) and np.array_equal(front.query().cpu().numpy(), PE.query_of(rs[:rows + 1]))


@pytest.mark.parametrize("tri", [False, True])
def test_modes_and_flags(gpu_ctx_ok, tri):
    ex, geom = scene("dup")
    pts, ptab, tris, ttab = tables("dup")
    query = on_dev(tris if tri else pts)
    dmax = bounds_of((ttab if tri else ptab).d2, seed=13)[0]
    want = (ttab.pairs(dmax) if tri else ptab.within(dmax))
    total = int(want[0][-1])
    count = raw_call(ex, tri, query, dmax, _native.PAIRS_COUNT, 0, size=16)
    assert np.array_equal(count[0].cpu().numpy(), want[0])
    assert (count[1] == -7).all() and (count[2] == -7.0).all() and (count[3] == -7).all()      # the sizing call writes row_start and nothing else
    both = raw_call(ex, tri, query, dmax, _native.PAIRS_BOTH, total)
    fill = raw_call(ex, tri, query, dmax, _native.PAIRS_FILL, total, row_start=count[0])
    assert equal_tensors(fill, both)
    assert np.array_equal(both[1].cpu().numpy(), want[1]) and same(both[2].cpu().numpy(), want[2])
    for flags in (0, SCAN):                                  # ordered=False: the same rows as sets; a host sort of each row gives the ordered result
        f = pairs if tri else within
        loose = f(ex, query, dmax, flags, ordered=False)
        assert np.array_equal(loose[0], want[0])
        assert_same(host_sorted(loose), want, ("unordered", flags))
    # N_box / N_leaf per query: the scan tests every primitive of every query that is walked at all, the walk fewer
    counts = torch.zeros((N, 2), dtype=torch.int32, device=DEV)
    rs = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    run = ex.scene.ctx.query_mesh_pairs if tri else ex.scene.ctx.query_point_pairs
    for flags in (COUNT, COUNT | SCAN):
        run(query.data_ptr(), N, 9 if tri else 3, _native.PAIRS_COUNT, rs.data_ptr(), flags=flags, dmax_all=dmax, counts=counts.data_ptr(),
            stream=torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize(DEV)
        assert np.array_equal(rs.cpu().numpy(), want[0])
        c = counts.cpu().numpy()
        if flags & SCAN:
            assert (c[:, 0] == 0).all() and (c[:, 1] == ex.scene.primitive_count).all()
        else:
            finite = np.isfinite(tris).all(axis=(1, 2)) if tri else np.isfinite(pts).all(axis=1)
            assert (c[~finite] == 0).all() and (c[finite, 0] > 0).all() and (c[:, 1] >= np.diff(want[0])).all() and c[:, 1].sum() < N * ex.scene.primitive_count


def test_empty_and_single(gpu_ctx_ok):
    ex, geom = scene("cornell")
    pts, ptab, tris, ttab = tables("cornell")
    e = PointQuery(ex.scene).within(on_dev(pts[:0]), 1.0, attributes=True)
    torch.cuda.synchronize(DEV)
    assert e.row_start.tolist() == [0] and e.prim.shape == (0,) and e.dist2.shape == (0,) and e.point.shape == (0, 3) and e.uv.shape == (0, 2) and e.query().shape == (0,)
    e = TriangleQuery(ex.scene).pairs(on_dev(tris[:0]), 1.0, points=True, capacity=4)
    torch.cuda.synchronize(DEV)
    assert e.row_start.tolist() == [0] and e.prim.shape == (4,) and e.point_query.shape == (4, 3)
    assert TriangleQuery(ex.scene).count_within(on_dev(tris[:0]), 1.0).shape == (0,)
    one = within(ex, pts[5:6], None)
    assert one[0].tolist() == [0, geom.tris.shape[0] + geom.spheres.shape[0]]


# ---- 6. chunking ---------------------------------------------------------------------------------------------------------------------------------------
def test_chunking(gpu_ctx_ok):
    ex, geom = scene("dup")
    ctx = ex.scene.ctx
    pt, tq = on_dev(query_points(geom, 1000, seed=17)), on_dev(query_triangles(geom, 1000, seed=17))
    pq, tqq = PointQuery(ex.scene), TriangleQuery(ex.scene)
    bound = float(pq.nearest(pt, 4).dist2[:, 3].sqrt().nan_to_num(posinf=0.0).median())
    a = (pq.within(pt, bound, attributes=True), tqq.pairs(tq, bound, points=True), pq.within(pt, bound, capacity=500))
    ctx.set_option("query_chunk_rays", 256)                  # four chunks: rows at the chunk borders have to land at their global offsets
    try:
        b = (pq.within(pt, bound, attributes=True), tqq.pairs(tq, bound, points=True), pq.within(pt, bound, capacity=500))
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert equal_tensors(a[0], b[0]) and equal_tensors(a[1], b[1])
    assert torch.equal(a[2].row_start, b[2].row_start) and torch.equal(a[2].row_start, a[0].row_start)
    written = PE.rows_that_fit(a[2].row_start.cpu().numpy(), 500)[1]
    assert 0 < written <= 500 and torch.equal(a[2].prim[:written], b[2].prim[:written]) and torch.equal(a[2].prim[:written], a[0].prim[:written])
    rs = a[0].row_start.cpu().numpy()
    assert all(0 < rs[k] < rs[-1] for k in (256, 512, 768)) and int(a[1].row_start[-1]) > 1000      # there are pairs on both sides of every border


# ---- 7. plumbing ---------------------------------------------------------------------------------------------------------------------------------------
def test_host_route_equals_torch_route(gpu_ctx_ok):
    ex, geom = scene("two")
    ctx = ex.scene.ctx
    pts, ptab, tris, ttab = tables("two")
    _, per_query = bounds_of(ptab.d2, seed=5)
    for flags in (0, SCAN):
        got = ctx.point_pairs(pts, per_query, flags=flags)
        assert_same(got[:5], within(ex, pts, on_dev(per_query), flags), ("host points", flags))
        assert_same(got[:5], ptab.within(per_query), ("host points, numpy", flags))
        got = ctx.mesh_pairs(tris, per_query, flags=flags)
        want = pairs(ex, tris, on_dev(per_query), flags)
        assert_same(got[:4] + (got[4][:, 0], got[4][:, 1]), want, ("host triangles", flags))
    full = ctx.point_pairs(pts, 1.0)
    total = int(full[0][-1])
    cut = ctx.point_pairs(pts, 1.0, capacity=total - 1)      # BOTH on the host route: the rows that fit, nothing behind them
    rows, written = PE.rows_that_fit(full[0], total - 1)
    assert np.array_equal(cut[0], full[0]) and np.array_equal(cut[1][:written], full[1][:written]) and (cut[1][written:] == -1).all() and np.isnan(cut[2][written:]).all()
    assert ctx.point_pairs(np.zeros((0, 3), F))[0].tolist() == [0]
    counts = ctx.mesh_pairs(tris[:64], 0.5, flags=SCAN | COUNT)[5]
    assert (counts[:, 0] == 0).all() and (counts[:, 1] == ex.scene.primitive_count).all()


def test_strided_input_and_side_stream(gpu_ctx_ok):
    ex, geom = scene("cornell")
    pts, ptab, tris, ttab = tables("cornell")
    scalar = bounds_of(ptab.d2, seed=5)[0]
    q = PointQuery(ex.scene)
    src = on_dev(pts)
    base = q.within(src, scalar, attributes=True)
    wide = torch.full((N, 8), 7.0, device=DEV)
    wide[:, :3] = src
    assert wide[:, :3].stride() == (8, 1)
    assert equal_tensors(q.within(wide[:, :3], scalar, attributes=True), base)
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(8):                                 # keep the side stream busy before the points exist
            big = torch.tanh(big @ big)
        pt = torch.where(big[0, 0] > 2.0, src * 0.0, src)   # (tanh <= 1: an exact copy of src, made after the products)
        h = q.within(pt, scalar, attributes=True)           # (its host wait is on this stream's work)
        g = q.within(pt, scalar, capacity=int(base.row_start[-1]))
        consumer = h.dist2.sum() * 2.0 + h.prim.float().sum() + g.prim.float().sum()
    torch.cuda.synchronize(DEV)
    assert equal_tensors(h, base) and torch.equal(g.prim, base.prim)
    assert torch.equal(consumer, base.dist2.sum() * 2.0 + base.prim.float().sum() + base.prim.float().sum())


def test_after_update_vertices(gpu_ctx_ok):
    tris = sphere_obj_triangles()
    ext = (tris.reshape(-1, 3).max(axis=0) - tris.reshape(-1, 3).min(axis=0)).max()
    half = tris.shape[0] // 2
    moved = tris.copy()
    moved[:half] += np.array([0.3 * ext, 0.0, 0.0])
    ex = custom_scene(tris)
    ex.build_scene()
    geom = CE.scene_geometry(ex.scene)
    pts, qt = query_points(geom, N, seed=31), query_triangles(geom, N, seed=31)
    before = within(ex, pts, 0.2 * ext)
    ex.scene.update_vertices(moved[:half].astype(F), first_vertex=0)
    fresh = custom_scene(moved)
    fresh.build_scene()
    a = within(ex, pts, 0.2 * ext)
    assert_same(a, within(fresh, pts, 0.2 * ext), "updated against fresh")
    assert_same(a, within(ex, pts, 0.2 * ext, SCAN), "updated walk against scan")
    assert not np.array_equal(a[0], before[0])               # the rows did move
    b = pairs(ex, qt, 0.05 * ext)
    assert_same(b, pairs(fresh, qt, 0.05 * ext), "triangles, updated against fresh")
    assert_same(b, pairs(ex, qt, 0.05 * ext, SCAN), "triangles, updated walk against scan")


def test_stack_of_one_entry_writes_inside_its_rows(gpu_ctx_ok):
    """a stack of one entry drops subtrees: tirt_stats says so, every row holds a subset of the full row in the definition's order, row_start is the
    prefix sum of what was met, and nothing is written behind the last row (the sentinel stands) -- nothing faults, and the next call is right again"""
    ex, geom = scene("cornell")
    ctx = ex.scene.ctx
    pts, ptab, tris, ttab = tables("cornell")
    for tri in (False, True):
        query = on_dev(tris if tri else pts)
        dmax = bounds_of((ttab if tri else ptab).d2, seed=12)[0] * 2.0
        want = (ttab.pairs(dmax) if tri else ptab.within(dmax))
        total = int(want[0][-1])
        ctx.stats_reset()
        got = raw_call(ex, tri, query, dmax, _native.PAIRS_BOTH, total + 100, stack_size=1)
        with pytest.raises(_native.TirtStackOverflow) as err:
            ctx.stats()
        assert 0 < err.value.stats["stack_overflow"] <= 2 * N      # (once per walk that dropped an entry: the counting walk and the filling walk)
        ctx.stats_reset()
        rs, prim, d2 = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
        met = int(rs[-1])
        assert rs[0] == 0 and (np.diff(rs) >= 0).all() and (np.diff(rs) <= np.diff(want[0])).all() and 0 < met < total
        assert (prim[met:] == -7).all() and (d2[met:] == -7.0).all()
        assert_rows_valid((rs, prim[:met], d2[:met]), ("stack 1", tri))
        full = set(zip(PE.query_of(want[0]).tolist(), want[1].tolist()))
        assert set(zip(PE.query_of(rs).tolist(), prim[:met].tolist())) <= full
        again = raw_call(ex, tri, query, dmax, _native.PAIRS_BOTH, total)
        assert np.array_equal(again[1].cpu().numpy(), want[1]) and ctx.stats()["stack_overflow"] == 0


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    W = H = 32
    films, rays = [], []
    for with_queries in (False, True):
        ex = scenes.cornell_box(W, H, 8, device_id=0)
        ex.build_scene()
        geom = CE.scene_geometry(ex.scene)
        pt, tq = on_dev(query_points(geom, 512, seed=23)), on_dev(query_triangles(geom, 512, seed=23))
        p, t = PointQuery(ex.scene), TriangleQuery(ex.scene)
        ex.scene.ctx.stats_reset()
        for f in (0, 2, 4):
            ex.cam.frame = f; ex.cam.frame_cpu[0] = f
            ex.integrator.render_frames(2)
            if with_queries:
                p.within(pt, 50.0, attributes=True)
                t.pairs(tq, 0.0, points=True, capacity=4096)
                t.count_within(tq, 10.0)
            else:
                ex.scene.ctx.sync()
        films.append(ex.integrator.hdr.to_numpy())
        st = ex.scene.ctx.stats()
        rays.append((st["rays_closest"], st["rays_shadow"]))
    assert np.array_equal(films[0].view(np.int32), films[1].view(np.int32))
    assert (films[0] != 0).any()
    assert rays[0] == rays[1] and rays[0][0] > 0             # the queries are not rays: no ray counter moved
