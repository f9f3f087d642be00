"""Closest-point queries on the device (csrc/tirt_closest_point.hip through tirt_query_closest_point / tirt_closest_point /
tirt_kat_closest_point and ti_raytrace_amd.PointQuery) against the definition of include/tirt.h as tests/closest_point_expected.py restates it.
Every comparison is on bits: the device function against numpy row by row, the culled walk against the scan over all primitives (both on the
device) and, where numpy can afford the brute force, both against numpy; then the bound, the plumbing, the counts and the stack, moving geometry."""
import numpy as np
import pytest
import torch

import closest_point_expected as E
from common import custom_scene, duplicate_code_scene, hostile_triangles, long_chain_scene, same_bits as same
from ti_raytrace_amd import Example, PointQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN, COUNT = _native.TRAVERSE_EXHAUSTIVE, _native.COUNT_NODES
FAR_SHIFT = np.array([3.0e4, -2.0e4, 5.0e4])
_SCENES, _WANT = {}, {}


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    """PointHits (or any tuple of tensors / None) -> numpy"""
    torch.cuda.synchronize(DEV)
    return tuple(None if x is None else x.cpu().numpy() for x in h)


def sphere_obj_triangles():
    ex = Example.example(8, 8, 1, 0)
    ex.scene.add_obj(scenes.asset("model", "sphere.obj"))
    ex.scene.setup_data_cpu()
    tris = E.scene_geometry(ex.scene).tris.astype(np.float64)
    assert tris.shape == (2280, 3, 3)
    return tris


def scene(name):
    """(built example, its Geometry), built once per module"""
    if name not in _SCENES:
        r = np.random.RandomState(3)
        if name == "two":
            ex = custom_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]], spheres=((0.3, 0.4, 1.5, 0.5),))
        elif name == "one":                                  # a one-primitive scene: the root's code is a leaf code
            ex = custom_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]]], spheres=())
        elif name == "spheres10":                            # more than eight analytic spheres: their slots span the whole grid
            ex = custom_scene([[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]],
                              spheres=tuple((r.uniform(-2, 2), r.uniform(-2, 2), r.uniform(-2, 2), r.uniform(0.05, 0.6)) for _ in range(10)))
        elif name == "dup_lbvh":                             # the reference's own LBVH as the traversal tree: the sphere's slot spans the whole grid
            ex = duplicate_code_scene(16, 16, device_id=0)
            ex.scene.ctx.set_option("traversal_tree", 0)
        elif name == "cornell":
            ex = scenes.cornell_box(16, 16, 1, device_id=0)
        elif name == "sphere":
            ex = custom_scene(sphere_obj_triangles())
        elif name == "sphere_far":
            ex = custom_scene(sphere_obj_triangles() + FAR_SHIFT, spheres=((FAR_SHIFT[0], FAR_SHIFT[1] + 3.0, FAR_SHIFT[2], 0.75),))
        elif name == "dup":
            ex = duplicate_code_scene(16, 16, device_id=0)
        elif name == "teapot":
            ex = scenes.single_model(16, 16, 1, device_id=0)
        elif name == "synthetic":
            ex = scenes.synthetic(16, 16, 1, device_id=0)
        elif name == "identical":
            ex = custom_scene(hostile_triangles(name, r), spheres=())      # nothing but the 3000 copies: every finite query ties 3000 ways
        elif name == "clusters":
            ex = custom_scene(hostile_triangles(name, r))
        else:
            raise KeyError(name)
        ex.build_scene()
        _SCENES[name] = (ex, E.scene_geometry(ex.scene))
    return _SCENES[name]


def query_points(geom, n, seed):
    """n float32 points of the kinds the culling can get wrong: uniform in 1.5 x the box, on the surface, the vertices themselves (every incident triangle
    ties at 0), edge midpoints, 10 / 1e3 / 1e6 extents away, and rows with NaN, +inf, -inf"""
    r = np.random.RandomState(seed)
    t = geom.tris.astype(np.float64)
    lo, hi = t.reshape(-1, 3).min(axis=0), t.reshape(-1, 3).max(axis=0)
    if geom.spheres.shape[0]:
        s = geom.spheres.astype(np.float64)
        lo, hi = np.minimum(lo, (s[:, :3] - s[:, 3:]).min(axis=0)), np.maximum(hi, (s[:, :3] + s[:, 3:]).max(axis=0))
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    n_far, n_bad = 16, 9
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


def device_answer(ex, pts, flags=0, max_distance=None, stack_size=64):
    return cpu(PointQuery(ex.scene, stack_size, flags).closest(on_dev(pts), max_distance, attributes=True))


def assert_same(got, want, what):
    d2, prim, q, uv = got
    bad = np.nonzero(prim != want[1])[0]
    assert bad.size == 0, (what, "prim", bad[:8], prim[bad[:8]], want[1][bad[:8]], d2[bad[:8]], want[0][bad[:8]])
    assert same(d2, want[0]), (what, "d2")
    assert same(q, want[2]), (what, "point")
    assert same(uv, want[3]), (what, "uv")


def numpy_answer(name, n=2048):
    """points of scene `name` and the definition's answer for them (brute force in numpy), made once"""
    if name not in _WANT:
        ex, geom = scene(name)
        pts = query_points(geom, n, seed=11)
        _WANT[name] = (pts, E.brute_force(pts, geom))
    return _WANT[name]


# ---- 1. known answers -----------------------------------------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx_ok):
    ex, _ = scene("two")
    ctx = ex.scene.ctx
    r = np.random.RandomState(1)
    rows = r.uniform(-1.0, 1.0, (4096, 12)).astype(F)
    rows[:512] *= F(1000.0)
    rows[512:1024, 0:3] *= F(50.0)                           # far points, small triangles
    hand, hand_want = E.hand_rows()
    zero_area = np.array([[0.3, 0.2, 0.1, 1, 1, 1, 1, 1, 1, 1, 1, 1],            # a point
                          [0.3, 0.2, 0.1, 0, 0, 0, 1, 1, 1, 2, 2, 2],            # collinear
                          [0.5, 0.5, 0.5, 0, 0, 0, 1, 1, 1, 1, 1, 1],            # b == c, p on the segment
                          [0.3, 0.2, 0.1, 0, 0, 0, 0, 0, 0, 1, 0, 0]], F)        # a == b
    on_tri = np.array([[0.25, 0.25, 0.0, 0, 0, 0, 1, 0, 0, 0, 1, 0], [0.5, 0.0, 0.0, 0, 0, 0, 1, 0, 0, 0, 1, 0]], F)
    allrows = np.concatenate([rows, hand, zero_area, on_tri], axis=0)
    got = ctx.kat_closest_point(allrows)
    d2, q, u, v = E.tri_point(allrows[:, 0:3], allrows[:, 3:6], allrows[:, 6:9], allrows[:, 9:12])
    want = np.concatenate([d2[:, None], q, u[:, None], v[:, None]], axis=1)
    assert same(got, want), np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][:10]
    assert np.array_equal(got[4096:4103].view(np.uint32), hand_want.view(np.uint32))
    assert np.bincount(E.region(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12]), minlength=7).min() > 50
    assert (got[-2:, 0] == 0).all()                          # on the triangle: distance zero
    # spheres: random, the centre, inside, on the surface
    srows = r.uniform(-1.0, 1.0, (4096, 7)).astype(F)
    srows[:, 6] = np.abs(srows[:, 6]) + F(0.01)
    special = np.array([[1, 2, 3, 1, 2, 3, 0.5], [1.1, 2, 3, 1, 2, 3, 0.5], [1, 2.5, 3, 1, 2, 3, 0.5], [4, 2, 3, 1, 2, 3, 0.5]], F)
    srows = np.concatenate([srows, special], axis=0)
    got = ctx.kat_closest_point(srows, is_sphere=True)
    d2, q, u, v = E.sphere_point(srows[:, 0:3], srows[:, 3:6], srows[:, 6])
    want = np.concatenate([d2[:, None], q, u[:, None], v[:, None]], axis=1)
    assert same(got, want)
    assert got[-4, 0] == 0.25 and 0.15 < got[-3, 0] < 0.17 and got[-2, 0] == 0.0 and got[-1, 0] == 6.25      # centre, inside, on the sphere, outside
    assert np.array_equal(got[-4, 1:4], np.array([1.5, 2, 3], F)) and np.array_equal(got[-2, 1:4], np.array([1, 2.5, 3], F))
    assert np.array_equal(got[-1, 1:4], np.array([1.5, 2, 3], F))


# ---- 2. walk == scan == numpy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "cornell", "sphere", "dup", "one", "spheres10", "dup_lbvh"])
def test_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, want = numpy_answer(name)
    assert_same(device_answer(ex, pts, SCAN), want, (name, "scan"))
    assert_same(device_answer(ex, pts, 0), want, (name, "walk"))
    finite = np.isfinite(pts).all(axis=1)
    assert (want[1][finite] >= 0).all() and (want[1][~finite] == -1).all() and np.isposinf(want[0][~finite]).all()
    if geom.spheres.shape[0]:
        assert np.isin(geom.sphere_prim, want[1]).all()      # every analytic sphere is somebody's nearest surface


# ---- 3. walk == scan where numpy cannot follow; 6a. the walk tests fewer primitives ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["teapot", "synthetic", "identical", "clusters", "sphere_far"])
def test_walk_equals_scan(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts = query_points(geom, 4096, seed=13)
    scan = device_answer(ex, pts, SCAN)
    walk = device_answer(ex, pts, 0)
    assert_same(walk, scan, name)
    finite = np.isfinite(pts).all(axis=1)
    assert (scan[1][finite] >= 0).all() and (scan[1][~finite] == -1).all()
    if name == "identical":
        assert (scan[1][finite] == 0).all()                  # 3000 candidates at equal D2: the smallest id
    h, cnt = PointQuery(ex.scene, 64, 0).closest_counts(on_dev(pts))
    hs, cnt_scan = PointQuery(ex.scene, 64, SCAN).closest_counts(on_dev(pts))
    (prim, prim_s), cnt, cnt_scan = cpu((h.prim, hs.prim)), cpu((cnt,))[0], cpu((cnt_scan,))[0]
    assert np.array_equal(prim, scan[1]) and np.array_equal(prim_s, scan[1])
    n_prim = ex.scene.primitive_count
    assert (cnt_scan[:, 1] == n_prim).all() and (cnt_scan[:, 0] == 0).all()
    assert (cnt[~finite] == 0).all()
    print("%s: N_leaf walk / scan = %.5f, mean N_box %.1f, mean N_leaf %.1f" % (name, cnt[:, 1].sum() / cnt_scan[:, 1].sum(), cnt[:, 0].mean(), cnt[:, 1].mean()))
    if name != "identical":
        assert cnt[:, 1].sum() < cnt_scan[:, 1].sum()


# ---- 4. max_distance ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "sphere"])
def test_max_distance(gpu_ctx_ok, name):
    ex, geom = scene(name)
    pts, want = numpy_answer(name)
    n = pts.shape[0]
    with np.errstate(all="ignore"):
        t = np.sqrt(want[0]).astype(F)
        kinds = {"half": (t * F(0.5)).astype(F), "t": t.copy(), "next": np.nextafter(t, F(np.inf)).astype(F), "twice": (t * F(2)).astype(F),
                 "inf": np.full(n, np.inf, F), "zero": np.zeros(n, F), "minus1": np.full(n, -1.0, F), "nan": np.full(n, np.nan, F)}
    pick = np.random.RandomState(5).randint(0, len(kinds), size=n)
    kinds["mixed"] = np.stack(list(kinds.values()), axis=1)[np.arange(n), pick]

    def expected(dmax):
        """the definition's rule on the unbounded answer: it stands iff its D2 <= dmax * dmax (any other primitive's D2 is no smaller)"""
        with np.errstate(invalid="ignore"):
            keep = (want[0] <= E.limit2(np.broadcast_to(np.asarray(dmax, F), (n,)))) & (want[1] >= 0)
        return (np.where(keep, want[0], F(np.inf)), np.where(keep, want[1], -1), np.where(keep[:, None], want[2], F(0)), np.where(keep[:, None], want[3], F(0)))

    for flags in (0, SCAN):
        for kind, dm in kinds.items():
            assert_same(device_answer(ex, pts, flags, on_dev(dm)), expected(dm), (name, flags, kind))
        for scalar in (float("inf"), 0.0, -1.0, float("nan"), float(np.median(t[np.isfinite(t)]))):
            assert_same(device_answer(ex, pts, flags, scalar), expected(scalar), (name, flags, scalar))
        assert_same(device_answer(ex, pts, flags, None), want, (name, flags, None))
    found = want[1] >= 0
    assert (expected(kinds["next"])[1][found] >= 0).all() and (expected(kinds["minus1"])[1] == -1).all()
    on_surface = found & (want[0] == 0)
    assert on_surface.any() and (expected(kinds["zero"])[1][on_surface] >= 0).all() and (expected(kinds["zero"])[1][~on_surface] == -1).all()
    # t * t can round either way against D2: "t" keeps some and drops others, and the device agrees with the rule on every one (above)
    strided = torch.zeros((n, 3), device=DEV)
    strided[:, 1] = on_dev(kinds["mixed"])
    assert strided[:, 1].stride() == (3,)
    assert_same(device_answer(ex, pts, 0, strided[:, 1]), expected(kinds["mixed"]), (name, "strided"))


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------------------------------
def equal_hits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_layouts_empty_and_single(gpu_ctx_ok):
    ex, geom = scene("cornell")
    pts, want = numpy_answer("cornell")
    pt = on_dev(pts)
    n = pt.shape[0]
    q = PointQuery(ex.scene)
    base = q.closest(pt, attributes=True)
    wide = torch.full((n, 8), 7.0, device=DEV)
    wide[:, :3] = pt
    assert wide[:, :3].stride() == (8, 1)
    assert equal_hits(q.closest(wide[:, :3], attributes=True), base)
    rows = torch.full((2 * n, 3), -5.0, device=DEV)
    rows[::2] = pt
    assert rows[::2].stride() == (6, 1)
    assert equal_hits(q.closest(rows[::2], attributes=True), base)
    assert equal_hits(q.closest(pt)[:2], base[:2]) and q.closest(pt).point is None and q.closest(pt).uv is None
    e = q.closest(pt[:0], attributes=True)
    assert e.dist2.shape == (0,) and e.prim.shape == (0,) and e.point.shape == (0, 3) and e.uv.shape == (0, 2)
    one = cpu(q.closest(pt[5:6], 1.0e9, attributes=True))
    assert_same(one, tuple(w[5:6] for w in want), "n == 1")
    with pytest.raises(ValueError):
        q.closest(pt, base.dist2[:-1])
    with pytest.raises(TypeError):
        q.closest(pt, base.dist2.double())

    class OtherDevice:
        _ctx = None
        _device_id = 1
    with pytest.raises(ValueError):
        PointQuery(OtherDevice()).closest(pt)


def test_chunking(gpu_ctx_ok):
    ex, geom = scene("sphere")
    ctx = ex.scene.ctx
    pt = on_dev(query_points(geom, 1000, seed=17))
    q = PointQuery(ex.scene)
    dm = q.closest(pt).dist2.sqrt() * 1.5
    a = q.closest(pt, dm, attributes=True)
    ha, ca = q.closest_counts(pt, dm)
    ctx.set_option("query_chunk_rays", 256)                  # four chunks
    try:
        b = q.closest(pt, dm, attributes=True)
        hb, cb = q.closest_counts(pt, dm)
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert equal_hits(a, b) and torch.equal(ca, cb) and torch.equal(ha.prim, hb.prim)


def test_ordered_on_the_callers_stream(gpu_ctx_ok):
    ex, geom = scene("synthetic")
    src = on_dev(query_points(geom, 1 << 16, seed=19))
    q = PointQuery(ex.scene)
    want = q.closest(src, attributes=True)
    want_sum = want.dist2 * 2.0 + want.prim.float() + want.point.sum(dim=1)
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(8):                                 # keep the side stream busy before the points exist
            big = torch.tanh(big @ big)
        pt = torch.where(big[0, 0] > 2.0, src * 0.0, src)   # (tanh <= 1: an exact copy of src, made after the products)
        h = q.closest(pt, attributes=True)
        consumer = h.dist2 * 2.0 + h.prim.float() + h.point.sum(dim=1)
    torch.cuda.synchronize(DEV)
    assert torch.equal(h.prim, want.prim) and torch.equal(consumer.view(torch.int32), want_sum.view(torch.int32))


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    W = H = 32
    films, rays = [], []
    for with_queries in (False, True):
        ex = scenes.cornell_box(W, H, 8, device_id=0)
        ex.build_scene()
        pt = on_dev(query_points(E.scene_geometry(ex.scene), 20000, seed=23))
        q = PointQuery(ex.scene)
        ex.scene.ctx.stats_reset()
        for f in (0, 2, 4):
            ex.cam.frame = f; ex.cam.frame_cpu[0] = f
            ex.integrator.render_frames(2)
            if with_queries:
                q.closest(pt, attributes=True)
                q.closest(pt, 10.0)
            else:
                ex.scene.ctx.sync()
        films.append(ex.integrator.hdr.to_numpy())
        st = ex.scene.ctx.stats()
        rays.append((st["rays_closest"], st["rays_shadow"]))
    assert np.array_equal(films[0].view(np.int32), films[1].view(np.int32))
    assert (films[0] != 0).any()
    assert rays[0] == rays[1] and rays[0][0] > 0             # the queries are not rays: no ray counter moved


def test_refusals_queue_nothing(gpu_ctx_ok):
    ex, geom = scene("cornell")
    ctx = ex.scene.ctx
    pts, _ = numpy_answer("cornell")
    pt = on_dev(pts[:100])
    host = np.ascontiguousarray(pts[:100])
    out = torch.full((100,), -7.0, device=DEV)
    out3 = torch.full((100, 3), -7.0, device=DEV)
    lib = _native.lib()
    cases = [
        (r"error -2:.*points: not device memory", dict(points=host.ctypes.data, n=100, point_stride=3, out_d2=out.data_ptr())),
        (r"error -2:.*dmax: not device memory", dict(points=pt.data_ptr(), n=100, point_stride=3, dmax=host.ctypes.data, out_d2=out.data_ptr())),
        (r"error -2:.*out_point: not device memory", dict(points=pt.data_ptr(), n=100, point_stride=3, out_point=host.ctypes.data)),
        (r"error -2:.*point_stride < 3", dict(points=pt.data_ptr(), n=100, point_stride=2, out_d2=out.data_ptr())),
        (r"error -2:.*point_out_stride < 3", dict(points=pt.data_ptr(), n=100, point_stride=3, out_point=out3.data_ptr(), point_out_stride=2)),
        (r"error -2:.*uv_stride < 2", dict(points=pt.data_ptr(), n=100, point_stride=3, out_uv=out3.data_ptr(), uv_stride=1)),
        (r"error -2:.*dmax_stride < 1", dict(points=pt.data_ptr(), n=100, point_stride=3, dmax=out.data_ptr(), dmax_stride=0, out_d2=out.data_ptr())),
        (r"error -2:.*unknown flags", dict(points=pt.data_ptr(), n=100, point_stride=3, flags=4, out_d2=out.data_ptr())),
        (r"error -2:.*stack_size", dict(points=pt.data_ptr(), n=100, point_stride=3, stack_size=0, out_d2=out.data_ptr())),
        (r"error -2:.*counts must be 8-byte aligned", dict(points=pt.data_ptr(), n=100, point_stride=3, flags=COUNT, counts=out.data_ptr() + 4)),
    ]
    for pattern, kw in cases:
        with pytest.raises(_native.TirtError, match=pattern):
            ctx.query_closest_point(**kw)
        assert lib.tirt_last_error()                         # the message is there for a C caller too
    unbuilt = _native.Context(0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*LBVH not built"):
        unbuilt.query_closest_point(pt.data_ptr(), 100, 3, out_d2=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.closest_point(host)
    torch.cuda.synchronize(DEV)
    assert (out == -7.0).all() and (out3 == -7.0).all()      # nothing ran
    s = torch.cuda.Stream(DEV)
    x = torch.zeros(16, device=DEV)
    with torch.cuda.stream(s):
        x.add_(1.0)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_native.TirtError, match="capturing"):
        with torch.cuda.graph(g, stream=s):
            x.add_(1.0)
            PointQuery(ex.scene).closest(pt)


def test_host_route_equals_torch_route(gpu_ctx_ok):
    ex, geom = scene("sphere")
    ctx = ex.scene.ctx
    pts, want = numpy_answer("sphere")
    d2, prim, q, uv, counts = ctx.closest_point(pts)
    assert counts is None
    assert_same((d2, prim, q, uv), want, "host route")
    dm = (np.sqrt(want[0]) * F(0.9)).astype(F)
    dm[::2] = np.inf
    for flags in (0, SCAN, COUNT):
        got = ctx.closest_point(pts, dm, 64, flags)
        assert_same(got[:4], device_answer(ex, pts, flags & SCAN, on_dev(dm)), ("host route, bound", flags))
        if flags & COUNT:
            _, cnt = PointQuery(ex.scene, 64, 0).closest_counts(on_dev(pts), on_dev(dm))
            assert np.array_equal(got[4], cpu((cnt,))[0])
    d2, prim, q, uv, _ = ctx.closest_point(pts[:10], 0.5, attributes=False)
    assert q is None and uv is None and same(d2, device_answer(ex, pts[:10], 0, 0.5)[0])
    assert ctx.closest_point(np.zeros((0, 3), F))[0].shape == (0,)


# ---- 6b. the stack ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", [1, 0])
def test_long_chain_and_stack_overflow(gpu_ctx_ok, tree):
    """the 600-deep duplicate-Morton chain, in the SAH tree and in the reference's own LBVH (a ~200-level 4-wide tree): a 2048-entry stack (16 in LDS,
    the rest in global memory) gives the scan's answers, a 4-entry stack drops entries and tirt_stats says so, and the next call is right again"""
    ex = long_chain_scene(16, 16)
    ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    ctx = ex.scene.ctx
    pts = query_points(E.scene_geometry(ex.scene), 2048, seed=29)
    scan = device_answer(ex, pts, SCAN)
    ctx.stats_reset()
    assert_same(device_answer(ex, pts, 0, stack_size=2048), scan, "stack 2048")
    assert ctx.stats()["stack_overflow"] == 0
    device_answer(ex, pts, 0, stack_size=4)
    with pytest.raises(_native.TirtStackOverflow) as err:
        ctx.stats()
    assert 0 < err.value.stats["stack_overflow"] <= 2048
    assert_same(device_answer(ex, pts, 0, stack_size=2048), scan, "stack 2048 again")
    assert ctx.stats()["stack_overflow"] == 0


@pytest.mark.parametrize("tree", [1, 0])
def test_stack_sizes_around_the_lds_part(gpu_ctx_ok, tree):
    """the same chain and queries with stacks that end just below, at and just beyond the 16 entries a lane has in LDS (at 16 there is no tail and the
    spill pointer is null, at 17 the tail is one entry per thread): a query can only differ from the scan if it dropped an entry, a query that fits a
    stack fits every larger one, and a lane does fill all of LDS (dropped entries are counted, nothing else happens to them)"""
    ex = long_chain_scene(16, 16)
    ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    ctx = ex.scene.ctx
    pts = query_points(E.scene_geometry(ex.scene), 2048, seed=29)
    scan = device_answer(ex, pts, SCAN)
    sizes = (15, 16, 17, 18, 24, 2048)
    over, miss = [], []
    for s in sizes:
        ctx.stats_reset()
        d2, prim, _, _ = device_answer(ex, pts, 0, stack_size=s)
        try:
            over.append(ctx.stats()["stack_overflow"])
        except _native.TirtStackOverflow as err:
            over.append(err.stats["stack_overflow"])
        miss.append(int(((d2.view(np.uint32) != scan[0].view(np.uint32)) | (prim != scan[1])).sum()))
    print("tree %d: stack sizes %s: queries that dropped an entry %s, queries that differ from the scan %s" % (tree, sizes, over, miss))
    assert all(m <= o for m, o in zip(miss, over)), (sizes, over, miss)
    assert all(a >= b for a, b in zip(over, over[1:])), (sizes, over)
    assert over[-1] == 0 and miss[-1] == 0
    assert over[1] > 0, "no lane filled the 16 entries in LDS: the sizes around them test nothing"


# ---- 7. moving geometry ------------------------------------------------------------------------------------------------------------------------------
def test_after_update_vertices(gpu_ctx_ok):
    tris = sphere_obj_triangles()
    ext = (tris.reshape(-1, 3).max(axis=0) - tris.reshape(-1, 3).min(axis=0)).max()
    half = tris.shape[0] // 2
    moved = tris.copy()
    moved[:half] += np.array([0.3 * ext, 0.0, 0.0])
    ex = custom_scene(tris)
    ex.build_scene()
    ex.scene.update_vertices(moved[:half].astype(F), first_vertex=0)
    fresh = custom_scene(moved)
    fresh.build_scene()
    pts = query_points(E.scene_geometry(fresh.scene), 2048, seed=31)
    a, b = device_answer(ex, pts, 0), device_answer(fresh, pts, 0)
    assert_same(a, b, "updated against fresh")
    assert_same(a, device_answer(ex, pts, SCAN), "updated walk against scan")
    assert not np.array_equal(a[1], device_answer(scene("sphere")[0], pts, 0)[1])      # the answers did move
