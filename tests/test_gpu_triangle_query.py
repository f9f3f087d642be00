"""Triangle-distance queries on the device (csrc/tirt_triangle_query.hip through tirt_query_mesh_distance / tirt_mesh_distance / tirt_kat_tri_tri and
ti_raytrace_amd.TriangleQuery) against the definition of include/tirt.h, "Triangle distance", as tests/triangle_query_expected.py restates it.  Every
comparison is on bits: the device functions against the host twin and numpy row by row, the culled walk against the scan over all primitives (both on
the device) and both against numpy's brute force; then the link to PointQuery, the contact test, the bound, the plumbing and the stack."""
import numpy as np
import pytest
import torch

import closest_point_expected as CE
import triangle_query_cases as cases
import triangle_query_expected as E
from common import custom_scene, duplicate_code_scene, long_chain_scene, same_bits as same
from ti_raytrace_amd import PointQuery, TriangleQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN, COUNT = _native.TRAVERSE_EXHAUSTIVE, _native.COUNT_NODES
_SCENES, _WANT = {}, {}
TWO = [[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]]


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    torch.cuda.synchronize(DEV)
    return tuple(None if x is None else x.cpu().numpy() for x in h)


def scene(name):
    """(built example, its Geometry), built once per module"""
    if name not in _SCENES:
        r = np.random.RandomState(3)
        if name == "one":                                    # a one-primitive scene: the root's code is a leaf code
            ex = custom_scene(TWO[:1], spheres=())
        elif name == "two":                                  # two triangles and an analytic sphere, which takes no part
            ex = custom_scene(TWO, spheres=((0.3, 0.4, 1.5, 0.5),))
        elif name == "cornell":
            ex = scenes.cornell_box(16, 16, 1, device_id=0)
        elif name == "dup":
            ex = duplicate_code_scene(16, 16, device_id=0)
        elif name == "chain":
            ex = long_chain_scene(16, 16)
        elif name == "tied":                                 # 6 triangles, 8 coincident copies of each, interleaved: every answer ties 8 ways across ids
            ex = custom_scene(np.tile(r.uniform(-1, 1, (6, 3, 3)), (8, 1, 1)), spheres=())
        elif name == "far":                                  # 60 triangles of extent ~2 moved 1e4 extents from the origin: fp32 neighbours there are ~1e-3 apart
            ex = custom_scene(r.uniform(-1, 1, (60, 1, 3)) + r.uniform(-0.3, 0.3, (60, 3, 3)) + np.array([2.0e4, -1.0e4, 1.5e4]), spheres=())
        elif name == "teapot":
            ex = scenes.single_model(16, 16, 1, device_id=0)
        else:
            raise KeyError(name)
        ex.build_scene()
        _SCENES[name] = (ex, CE.scene_geometry(ex.scene))
    return _SCENES[name]


def query_triangles(geom, n, seed):
    """n float32 query triangles [n, 3, 3] of the kinds the candidates and the culling can get wrong"""
    r = np.random.RandomState(seed)
    t = geom.tris.astype(np.float64)
    nt = t.shape[0]
    lo, hi = t.reshape(-1, 3).min(axis=0), t.reshape(-1, 3).max(axis=0)
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    k = max(n // 12, 1)
    small = lambda m, s: r.uniform(-1, 1, (m, 3, 3)) * s * ext
    pick = lambda m: t[r.randint(0, nt, m)]
    parts = []
    parts.append((mid + 0.75 * (hi - lo) * r.uniform(-1, 1, (2 * k, 1, 3))) + small(2 * k, 0.03))      # small, inside and outside the box
    parts.append(mid + small(k, 3.0))                                                                    # larger than the scene
    s = pick(k); w = r.dirichlet((1, 1, 1), k)
    parts.append((s * w[:, :, None]).sum(axis=1)[:, None, :] + small(k, 0.05))                          # around a surface point: most pierce it
    s = pick(k); w = r.uniform(-0.5, 1.5, (k, 3, 3)); w /= w.sum(axis=2, keepdims=True)
    parts.append(np.einsum("nij,njk->nik", w, s))                                                       # coplanar with a scene triangle, overlapping it
    parts.append(pick(k)); parts.append(pick(k)[:, [2, 0, 1]])                                          # copied from the scene
    s = pick(k); q = s[:, :1] + small(k, 0.1); q[np.arange(k), r.randint(0, 3, k)] = s[np.arange(k), r.randint(0, 3, k)]
    parts.append(q)                                                                                      # one shared vertex
    s = pick(k); q = s[:, :1] + small(k, 0.1); e = r.randint(0, 3, k); f = r.randint(0, 3, k)
    q[np.arange(k), e] = s[np.arange(k), f]; q[np.arange(k), (e + 1) % 3] = s[np.arange(k), (f + 2) % 3]
    parts.append(q)                                                                                      # one shared edge
    q = mid + 0.6 * (hi - lo) * r.uniform(-1, 1, (k, 1, 3)) + small(k, 0.2); q[: k // 2, 2] = q[: k // 2, 1]; q[k // 2:, 1:] = q[k // 2:, :1]
    q[-1] = pick(1)[0][:1]                                                                               # degenerate: segments, points, a scene vertex as a point
    parts.append(q)
    n_far = 4
    for far in (10.0, 1.0e3, 1.0e6):                                                                     # many extents away
        d = r.normal(size=(n_far, 1, 3)); d /= np.linalg.norm(d, axis=2, keepdims=True)
        parts.append(mid + d * far * ext + small(n_far, 0.05))
    bad = np.tile(pick(1)[0] + 0.01 * ext, (9, 1, 1))                                                    # NaN, +inf, -inf in one coordinate of a triangle that touches otherwise
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * j + a, a, (a + j) % 3] = v
    parts.append(bad)
    have = sum(p.shape[0] for p in parts)
    parts.append((mid + 0.6 * (hi - lo) * r.uniform(-1, 1, (n - have, 1, 3))) + small(n - have, 0.15))  # the rest: middling triangles in the box
    q = np.concatenate(parts, axis=0).astype(F)
    assert q.shape == (n, 3, 3)
    return q


def device_answer(ex, tris, flags=0, max_distance=None, stack_size=64):
    """(d2, prim, code, P, Q) as numpy"""
    return cpu(TriangleQuery(ex.scene, stack_size, flags).closest(on_dev(tris), max_distance, points=True))


def assert_same(got, want, what):
    d2, prim, code, P, Q = got
    bad = np.nonzero(prim != want[1])[0]
    assert bad.size == 0, (what, "prim", bad[:8], prim[bad[:8]], want[1][bad[:8]], d2[bad[:8]], want[0][bad[:8]])
    assert same(d2, want[0]), (what, "d2")
    assert np.array_equal(code, want[2]), (what, "code", np.nonzero(code != want[2])[0][:8])
    assert same(P, want[3]), (what, "point on the query triangle")
    assert same(Q, want[4]), (what, "point on the scene")


def numpy_answer(name, n=512):
    """query triangles of scene `name` and the definition's answer for them (brute force in numpy), made once and left alone"""
    if name not in _WANT:
        ex, geom = scene(name)
        tris = query_triangles(geom, n, seed=11)
        _WANT[name] = (tris, E.brute_force(tris, geom))
    return _WANT[name]


# ---- 1. the device functions, row by row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [0, 1, 2])
def test_known_answer_rows_device_equals_host_equals_numpy(gpu_ctx_ok, what):
    ctx = scene("two")[0].scene.ctx
    rows = cases.ROWS[what]()
    got = ctx.kat_tri_tri(rows, what)
    assert same(got, _native.kat_tri_tri_host(rows, what)), np.nonzero((got.view(np.uint32) != _native.kat_tri_tri_host(rows, what).view(np.uint32)).any(axis=1))[0][:8]
    assert same(got, E.kat_rows(rows, what))
    assert ctx.kat_tri_tri(rows[:0], what).shape == (0, _native.KAT_TRI_TRI_ROWS[what][1])


# ---- 2. walk == scan == numpy on all five outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "two", "cornell", "dup", "chain", "tied", "far"])
def test_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom = scene(name)
    tris, want = numpy_answer(name, 256 if name == "chain" else 512)
    assert_same(device_answer(ex, tris, SCAN, stack_size=2048), want, (name, "scan"))
    assert_same(device_answer(ex, tris, 0, stack_size=2048), want, (name, "walk"))
    finite = np.isfinite(tris).all(axis=(1, 2))
    assert (~finite).sum() == 9 and (want[1][finite] >= 0).all() and (want[1][~finite] == -1).all()
    assert np.isposinf(want[0][~finite]).all() and (want[2][~finite] == -1).all() and not want[3][~finite].any() and not want[4][~finite].any()
    assert np.isin(want[1][want[1] >= 0], geom.tri_prim).all()      # an analytic sphere is nobody's answer
    if name in ("cornell", "dup", "chain"):
        classes = [(want[2] >= a) & (want[2] <= b) for a, b in ((0, 2), (3, 5), (6, 14), (15, 17), (18, 20))]
        assert all(c.any() for c in classes), [int(c.sum()) for c in classes]      # every class of candidate answers somewhere
    if name == "tied":
        assert (want[1][finite] < 6).all()                   # eight ids tie on every answer: the smallest, i.e. the first copy


def test_teapot_walk_equals_scan(gpu_ctx_ok):
    ex, geom = scene("teapot")
    tris = query_triangles(geom, 256, seed=13)
    q = on_dev(tris)
    scan = device_answer(ex, tris, SCAN)
    assert_same(device_answer(ex, tris, 0), scan, "teapot")
    walk, cnt = TriangleQuery(ex.scene, 64, 0).closest_counts(q)
    scan_c, cnt_scan = TriangleQuery(ex.scene, 64, SCAN).closest_counts(q)
    walk, scan_c, cnt, cnt_scan = cpu(walk[:3]), cpu(scan_c[:3]), cpu((cnt,))[0], cpu((cnt_scan,))[0]
    for h in (walk, scan_c):                                 # the counting instantiations answer the same
        assert np.array_equal(h[1], scan[1]) and same(h[0], scan[0]) and np.array_equal(h[2], scan[2])
    finite = np.isfinite(tris).all(axis=(1, 2))
    assert (cnt_scan[:, 1] == ex.scene.primitive_count).all() and (cnt_scan[:, 0] == 0).all() and (cnt[~finite] == 0).all()
    print("teapot: N_leaf walk / scan = %.5f, mean N_box %.1f, mean N_leaf %.1f" % (cnt[:, 1].sum() / cnt_scan[:, 1].sum(), cnt[:, 0].mean(), cnt[:, 1].mean()))
    assert cnt[:, 1].sum() < cnt_scan[:, 1].sum()


# ---- 3. the link to the point query ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "dup"])
def test_link_to_point_query(gpu_ctx_ok, name):
    """a triangle is never further than any of its vertices, and where a vertex answers (code 0..2) the distance is that vertex's closest-point distance,
    bit for bit.  ('dup' has an analytic sphere light, which takes no part in the triangle query: the comparisons are made where the point query's
    winner is a triangle too.)"""
    ex, geom = scene(name)
    tris, want = numpy_answer(name)
    d2, prim, code, _, _ = device_answer(ex, tris)
    pq = PointQuery(ex.scene)
    vd2 = np.stack([cpu(pq.closest(on_dev(tris[:, j])))[0] for j in range(3)], axis=1)
    vprim = np.stack([cpu(pq.closest(on_dev(tris[:, j])))[1] for j in range(3)], axis=1)
    finite = np.isfinite(tris).all(axis=(1, 2))
    tri_won = np.isin(vprim, geom.tri_prim)
    assert tri_won[finite].mean() > 0.9
    assert (d2[finite, None] <= np.where(tri_won, vd2, np.inf)[finite]).all()
    by_vertex = finite & (code >= 0) & (code <= 2)
    assert by_vertex.sum() > 30
    j = code[by_vertex]
    own, own_tri = vd2[by_vertex, j], tri_won[by_vertex, j]
    assert own_tri.sum() > 30 and same(d2[by_vertex][own_tri], own[own_tri])
    assert (own[~own_tri] <= d2[by_vertex][~own_tri]).all()  # (the point query's winner is the analytic sphere: it was nearer than any triangle)
    # what the triangle query is for: some triangles are strictly closer than all their vertices (edge against edge, or crossing)
    assert (d2[finite] < vd2[finite].min(axis=1)).sum() > 30


# ---- 4. contact ------------------------------------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """the 12 triangles of an axis-aligned box as (vertices [8, 3], faces [12, 3])"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], F)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int64)
    return v, f


def test_collides(gpu_ctx_ok):
    """a 60-unit box pushed 35 units into the top (y = 165) of the Cornell box's short block, and the same box 140 units above it"""
    ex, geom = scene("cornell")
    q = TriangleQuery(ex.scene)
    for y0, any_contact in ((130.0, True), (305.0, False)):
        v, f = box_mesh((155.0, y0, -200.0), (215.0, y0 + 60.0, -140.0))
        got = cpu((q.collides((on_dev(v), on_dev(f))), q.collides((on_dev(v), on_dev(f.astype(np.int32)))), q.collides(on_dev(v[f]))))
        want = E.brute_force(v[f], geom, 0.0)[1] >= 0
        assert got[0].dtype == np.bool_ and all(np.array_equal(g, want) for g in got), (y0, got, want)
        assert want.any() == any_contact
        if any_contact:
            # the four sides cross the block's top; the box's top is above it and its bottom inside the block, touching no surface
            assert want.tolist() == [True] * 4 + [False] * 4 + [True] * 4      # (box_mesh's faces: z = lo, z = hi, y = lo, y = hi, x = lo, x = hi)
            h = cpu(q.closest(on_dev(v[f]), 0.0, points=True))
            assert (h[0][want] == 0).all() and (h[2][want] >= 15).all() and (h[1][want] >= 10).all() and (h[1][want] <= 11).all()      # edges through the top face's two triangles
            assert np.array_equal(h[3][want], h[4][want]) and np.allclose(h[3][want][:, 1], 165.0, atol=1e-3)


# ---- 5. the bound ----------------------------------------------------------------------------------------------------------------------------------------
def test_max_distance(gpu_ctx_ok):
    ex, geom = scene("cornell")
    tris, want = numpy_answer("cornell")
    n = tris.shape[0]
    with np.errstate(all="ignore"):
        t = np.sqrt(want[0]).astype(F)
        kinds = {"half": (t * F(0.5)).astype(F), "t": t.copy(), "next": np.nextafter(t, F(np.inf)).astype(F), "twice": (t * F(2)).astype(F),
                 "inf": np.full(n, np.inf, F), "zero": np.zeros(n, F), "minus1": np.full(n, -1.0, F), "nan": np.full(n, np.nan, F)}
    pick = np.random.RandomState(5).randint(0, len(kinds), size=n)
    kinds["mixed"] = np.stack(list(kinds.values()), axis=1)[np.arange(n), pick]

    def expected(dmax):
        """the definition's rule on the unbounded answer: it stands iff its D2 <= dmax * dmax (any other primitive's D2 is no smaller)"""
        with np.errstate(invalid="ignore"):
            keep = (want[0] <= CE.limit2(np.broadcast_to(np.asarray(dmax, F), (n,)))) & (want[1] >= 0)
        return (np.where(keep, want[0], F(np.inf)), np.where(keep, want[1], -1), np.where(keep, want[2], -1), np.where(keep[:, None], want[3], F(0)),
                np.where(keep[:, None], want[4], F(0)))

    assert_same(E.brute_force(tris, geom, kinds["mixed"]), expected(kinds["mixed"]), "the rule against the restatement's own bound")
    for flags in (0, SCAN):
        for kind in ("mixed", "zero", "next"):
            assert_same(device_answer(ex, tris, flags, on_dev(kinds[kind])), expected(kinds[kind]), (flags, kind))
        for scalar in (float("inf"), 0.0, -1.0, float("nan"), float(np.median(t[np.isfinite(t)]))):
            assert_same(device_answer(ex, tris, flags, scalar), expected(scalar), (flags, scalar))
    found = want[1] >= 0
    touching = found & (want[0] == 0)
    z = expected(0.0)
    assert touching.sum() > 50 and (z[1][touching] >= 0).all() and (z[1][~touching] == -1).all() and (z[2][~touching] == -1).all() and np.isposinf(z[0][~touching]).all()
    assert (expected(kinds["next"])[1][found] >= 0).all() and (expected(-1.0)[1] == -1).all() and (expected(float("nan"))[1] == -1).all()
    strided = torch.zeros((n, 3), device=DEV)
    strided[:, 1] = on_dev(kinds["mixed"])
    assert_same(device_answer(ex, tris, 0, strided[:, 1]), expected(kinds["mixed"]), "strided bound")
    assert np.array_equal(cpu((TriangleQuery(ex.scene).collides(on_dev(tris)),))[0], touching)


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------------------------------------------
def equal_hits(a, b):
    return all((x is None and y is None) or torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def test_layouts_and_sizes(gpu_ctx_ok):
    ex, geom = scene("cornell")
    tris, want = numpy_answer("cornell")
    t = on_dev(tris)
    n = t.shape[0]
    q = TriangleQuery(ex.scene)
    base = q.closest(t, points=True)
    wide = torch.full((n, 5, 3), 7.0, device=DEV)            # rows of 15 floats, the triangle in the first 9: handed over as it is
    wide[:, :3] = t
    assert wide[:, :3].stride() == (15, 3, 1)
    assert equal_hits(q.closest(wide[:, :3], points=True), base)
    rows = torch.full((2 * n, 3, 3), -5.0, device=DEV)
    rows[::2] = t
    assert rows[::2].stride() == (18, 3, 1) and equal_hits(q.closest(rows[::2], points=True), base)
    assert equal_hits(q.closest(t.permute(1, 2, 0).contiguous().permute(2, 0, 1), points=True), base)      # any other layout: copied once
    # an indexed mesh (vertices, faces) of the finite query triangles, made on the host (rows are merged on their bits) and gathered in torch
    fin = np.nonzero(np.isfinite(tris).all(axis=(1, 2)))[0]
    vbits, inv = np.unique(tris[fin].reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    faces = inv.reshape(-1, 3).astype(np.int64)
    assert vbits.shape[0] < 3 * fin.size and faces.min() == 0 and faces.max() == vbits.shape[0] - 1
    verts = on_dev(vbits.view(F))
    sub = tuple(x[on_dev(fin)] for x in base)
    assert equal_hits(q.closest((verts, on_dev(faces)), points=True), sub)
    assert equal_hits(q.closest((verts, on_dev(faces.astype(np.int32))), points=True), sub)
    h = q.closest(t)
    assert equal_hits(h[:3], base[:3]) and h.point_query is None and h.point_scene is None
    # outputs of the C entry in a caller's layout: points in rows of 8 floats, every output optional
    out = torch.full((n, 8), -7.0, device=DEV)
    ex.scene.ctx.query_mesh_distance(t.data_ptr(), n, 9, out_points=out.data_ptr(), points_stride=8, stream=torch.cuda.current_stream(DEV).cuda_stream)
    assert torch.equal(out[:, 0:3].contiguous().view(torch.int32), base.point_query.contiguous().view(torch.int32))
    assert torch.equal(out[:, 3:6].contiguous().view(torch.int32), base.point_scene.contiguous().view(torch.int32)) and (out[:, 6:] == -7.0).all()
    for m in (0, 1, 63, 64, 65):
        e = q.closest(t[:m], points=True)
        assert e.d2.shape == (m,) and e.prim.shape == (m,) and e.code.shape == (m,) and e.point_query.shape == (m, 3) and e.point_scene.shape == (m, 3)
        assert_same(cpu(e), tuple(w[:m] for w in want), ("n", m))
        assert_same(cpu(q.closest(t[7:7 + m], 1.0e9, points=True)), tuple(w[7:7 + m] for w in want), ("n, offset", m))
    assert q.collides(t[:0]).shape == (0,)
    with pytest.raises(ValueError):
        q.closest(t, base.d2[:-1])
    with pytest.raises(TypeError):
        q.closest(t, base.d2.double())

    class OtherDevice:
        _ctx = None
        _device_id = 1
    with pytest.raises(ValueError):
        TriangleQuery(OtherDevice()).closest(t)


def test_chunking(gpu_ctx_ok):
    """(the smallest query_chunk_rays is 256, so three chunks take more than 512 queries: 600, the one test above that size)"""
    ex, geom = scene("dup")
    ctx = ex.scene.ctx
    tris = query_triangles(geom, 600, seed=17)
    t = on_dev(tris)
    q = TriangleQuery(ex.scene)
    dm = q.closest(t).d2.sqrt() * 1.5
    a = q.closest(t, dm, points=True)
    ha, ca = q.closest_counts(t, dm)
    ctx.set_option("query_chunk_rays", 256)                  # three chunks: 256, 256, 88
    try:
        b = q.closest(t, dm, points=True)
        hb, cb = q.closest_counts(t, dm)
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert equal_hits(a, b) and torch.equal(ca, cb) and equal_hits(ha, hb) and equal_hits(ha[:3], a[:3])
    assert_same(cpu(b), E.brute_force(tris, geom, cpu((dm,))[0]), "three chunks")


def test_ordered_on_the_callers_stream(gpu_ctx_ok):
    ex, geom = scene("cornell")
    tris, _ = numpy_answer("cornell")
    src = on_dev(tris)
    q = TriangleQuery(ex.scene)
    want = q.closest(src, points=True)
    want_sum = want.d2 * 2.0 + want.prim.float() + want.code.float() + want.point_query.sum(dim=1) + want.point_scene.sum(dim=1)
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(8):                                 # keep the side stream busy before the triangles exist
            big = torch.tanh(big @ big)
        t = torch.where(big[0, 0] > 2.0, src * 0.0, src)    # (tanh <= 1: an exact copy of src, made after the products)
        h = q.closest(t, points=True)
        consumer = h.d2 * 2.0 + h.prim.float() + h.code.float() + h.point_query.sum(dim=1) + h.point_scene.sum(dim=1)
    torch.cuda.synchronize(DEV)
    assert torch.equal(h.prim, want.prim) and torch.equal(consumer.view(torch.int32), want_sum.view(torch.int32))


def test_host_route_equals_torch_route(gpu_ctx_ok):
    ex, geom = scene("cornell")
    ctx = ex.scene.ctx
    tris, want = numpy_answer("cornell")
    d2, prim, code, pq, counts = ctx.mesh_distance(tris)
    assert counts is None
    assert_same((d2, prim, code, pq[:, 0], pq[:, 1]), want, "host route")
    dm = (np.sqrt(want[0]) * F(0.9)).astype(F)
    dm[::2] = np.inf
    for flags in (0, SCAN, COUNT):
        got = ctx.mesh_distance(tris, dm, 64, flags)
        assert_same((got[0], got[1], got[2], got[3][:, 0], got[3][:, 1]), device_answer(ex, tris, flags & SCAN, on_dev(dm)), ("host route, bound", flags))
        if flags & COUNT:
            _, cnt = TriangleQuery(ex.scene, 64, 0).closest_counts(on_dev(tris), on_dev(dm))
            assert np.array_equal(got[4], cpu((cnt,))[0])
    d2, prim, code, pq, _ = ctx.mesh_distance(tris[:10], 0.5, points=False)
    assert pq is None and same(d2, device_answer(ex, tris[:10], 0, 0.5)[0])
    assert ctx.mesh_distance(np.zeros((0, 3, 3), F))[0].shape == (0,)


def test_refusals_queue_nothing(gpu_ctx_ok):
    ex, geom = scene("cornell")
    ctx = ex.scene.ctx
    tris, _ = numpy_answer("cornell")
    t = on_dev(tris[:100])
    host = np.ascontiguousarray(tris[:100])
    out = torch.full((100,), -7.0, device=DEV)
    outi = torch.full((100,), -7, device=DEV, dtype=torch.int32)
    out6 = torch.full((100, 6), -7.0, device=DEV)
    lib = _native.lib()
    ok = dict(tris=t.data_ptr(), n=100, tri_stride=9)
    cases_ = [
        (r"error -2:.*tris: not device memory", dict(ok, tris=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*dmax: not device memory", dict(ok, dmax=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*out_d2: not device memory", dict(ok, out_d2=host.ctypes.data)),
        (r"error -2:.*out_code: not device memory", dict(ok, out_code=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*out_points: not device memory", dict(ok, out_points=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*tri_stride < 9", dict(ok, tri_stride=8, out_d2=out.data_ptr())),
        (r"error -2:.*points_stride < 6", dict(ok, out_points=out6.data_ptr(), points_stride=5, out_d2=out.data_ptr())),
        (r"error -2:.*dmax_stride < 1", dict(ok, dmax=out.data_ptr(), dmax_stride=0, out_d2=out.data_ptr())),
        (r"error -2:.*unknown flags", dict(ok, flags=4, out_d2=out.data_ptr())),
        (r"error -2:.*stack_size", dict(ok, stack_size=0, out_d2=out.data_ptr())),
        (r"error -2:.*stack_size", dict(ok, stack_size=4097, out_d2=out.data_ptr())),
        (r"error -2:.*counts must be 8-byte aligned", dict(ok, flags=COUNT, counts=out.data_ptr() + 4, out_prim=outi.data_ptr())),
    ]
    for pattern, kw in cases_:
        with pytest.raises(_native.TirtError, match=pattern):
            ctx.query_mesh_distance(**kw)
        assert lib.tirt_last_error()                         # the message is there for a C caller too
    unbuilt = _native.Context(0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*LBVH not built"):
        unbuilt.query_mesh_distance(t.data_ptr(), 100, 9, out_d2=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.mesh_distance(host)
    with pytest.raises(_native.TirtError, match=r"error -2:.*what is 0"):
        _native.check(lib.tirt_kat_tri_tri(ctx.handle, np.zeros(18, F), 1, 3, np.zeros(8, F)))
    torch.cuda.synchronize(DEV)
    assert (out == -7.0).all() and (out6 == -7.0).all() and (outi == -7).all()      # nothing ran
    s = torch.cuda.Stream(DEV)
    x = torch.zeros(16, device=DEV)
    with torch.cuda.stream(s):
        x.add_(1.0)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_native.TirtError, match="capturing"):
        with torch.cuda.graph(g, stream=s):
            x.add_(1.0)
            TriangleQuery(ex.scene).closest(t)


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    W = H = 32
    films, rays = [], []
    for with_queries in (False, True):
        ex = scenes.cornell_box(W, H, 8, device_id=0)
        ex.build_scene()
        t = on_dev(numpy_answer("cornell")[0])
        q = TriangleQuery(ex.scene)
        ex.scene.ctx.stats_reset()
        for f in (0, 2, 4):
            ex.cam.frame = f; ex.cam.frame_cpu[0] = f
            ex.integrator.render_frames(2)
            if with_queries:
                q.closest(t, points=True)
                q.collides(t)
            else:
                ex.scene.ctx.sync()
        films.append(ex.integrator.hdr.to_numpy())
        st = ex.scene.ctx.stats()
        rays.append((st["rays_closest"], st["rays_shadow"]))
    assert np.array_equal(films[0].view(np.int32), films[1].view(np.int32))
    assert (films[0] != 0).any()
    assert rays[0] == rays[1] and rays[0][0] > 0             # the queries are not rays: no ray counter moved


def test_after_update_vertices(gpu_ctx_ok):
    r = np.random.RandomState(8)
    tris = r.uniform(-1, 1, (200, 1, 3)) + r.uniform(-0.15, 0.15, (200, 3, 3))
    moved = tris.copy()
    moved[:100] += np.array([0.6, 0.0, 0.0])
    ex = custom_scene(tris)
    ex.build_scene()
    before = device_answer(ex, query_triangles(CE.scene_geometry(ex.scene), 256, seed=31))
    ex.scene.update_vertices(moved[:100].astype(F), first_vertex=0)
    fresh = custom_scene(moved)
    fresh.build_scene()
    q = query_triangles(CE.scene_geometry(fresh.scene), 256, seed=31)
    a, b = device_answer(ex, q), device_answer(fresh, q)
    assert_same(a, b, "updated against fresh")
    assert_same(a, device_answer(ex, q, SCAN), "updated walk against scan")
    assert_same(a, E.brute_force(q, CE.scene_geometry(fresh.scene)), "updated against numpy")
    assert not np.array_equal(a[1], before[1])               # the answers did move


# ---- 7. the stack ------------------------------------------------------------------------------------------------------------------------------------------
def test_stack_sizes_and_overflow(gpu_ctx_ok):
    """the 600-deep duplicate-Morton chain with stacks that end just below, at and just beyond the 16 entries a lane has in LDS (at 16 there is no tail and
    the spill pointer is null, at 17 the tail is one entry per thread), a tiny one and a large one: a query can only differ from the scan if it dropped an
    entry, a query that fits a stack fits every larger one, dropped entries are counted in stack_overflow, and the next call is right again"""
    ex, geom = scene("chain")
    ctx = ex.scene.ctx
    tris, want = numpy_answer("chain", 256)
    sizes = (4, 15, 16, 17, 2048)
    over, miss = [], []
    for s in sizes:
        ctx.stats_reset()
        d2, prim, _, _, _ = device_answer(ex, tris, 0, stack_size=s)
        try:
            over.append(ctx.stats()["stack_overflow"])
        except _native.TirtStackOverflow as err:
            over.append(err.stats["stack_overflow"])
        miss.append(int(((d2.view(np.uint32) != want[0].view(np.uint32)) | (prim != want[1])).sum()))
    print("stack sizes %s: queries that dropped an entry %s, queries that differ from the scan %s" % (sizes, over, miss))
    assert all(m <= o for m, o in zip(miss, over)), (sizes, over, miss)
    assert all(a >= b for a, b in zip(over, over[1:])), (sizes, over)
    assert over[-1] == 0 and miss[-1] == 0
    assert 0 < over[0] <= 256, "the tiny stack dropped nothing"
    assert over[2] > 0, "no lane filled the 16 entries in LDS: the sizes around them test nothing"
    ctx.stats_reset()
    device_answer(ex, tris, 0, stack_size=4)
    with pytest.raises(_native.TirtStackOverflow):
        ctx.stats()
    assert_same(device_answer(ex, tris, 0, stack_size=2048), want, "stack 2048 again")
    assert ctx.stats()["stack_overflow"] == 0
