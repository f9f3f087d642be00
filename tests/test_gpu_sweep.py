"""Sphere sweeps on the device (csrc/tirt_sweep.hip through tirt_query_sweep / tirt_sweep / tirt_kat_sweep and ti_raytrace_amd.SweepQuery) against the
definition of include/tirt.h as tests/sweep_expected.py restates it.  Every comparison is on bits: the device functions against the host text row by
row, the culled walk against the scan over all primitives (both on the device) and, on as many queries as numpy can afford, both against numpy; then
the ties to the point queries, the plumbing, the counts and the stack, moving geometry, and the queries around a cast."""
import numpy as np
import pytest
import torch

import closest_point_expected as CP
import sweep_expected as SE
from common import custom_scene, duplicate_code_scene, long_chain_scene, tiny_scene, same_bits as same
from ti_raytrace_amd import Example, PointQuery, RayQuery, SweepQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN, COUNT = _native.TRAVERSE_EXHAUSTIVE, _native.COUNT_NODES
SIZES = (1, 63, 64, 65, 4097)
RADII = (0.0, 0.001, 0.01, 0.2)                              # of the scene's extent
FIELDS = ("t", "prim", "code", "point", "uv", "normal")
_SCENES = {}


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    torch.cuda.synchronize(DEV)
    return {k: None if v is None else v.cpu().numpy() for k, v in h._asdict().items()}


def sphere_obj_triangles():
    ex = Example.example(8, 8, 1, 0)
    ex.scene.add_obj(scenes.asset("model", "sphere.obj"))
    ex.scene.setup_data_cpu()
    return CP.scene_geometry(ex.scene).tris.astype(np.float64)


def scene(name):
    """(built example, its Geometry, (grid_min, cell), box lo, box hi), built once per module"""
    if name not in _SCENES:
        r = np.random.RandomState(3)
        two = [[[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], [[1, 0, 0], [1, 1, -0.3], [0, 1, 0.2]]]
        if name == "one":                                    # a one-primitive scene: the root's code is a leaf code
            ex = custom_scene(two[:1], spheres=())
        elif name == "tiny":
            ex = tiny_scene(200, device_id=0)
        elif name == "chain":
            ex = long_chain_scene(16, 16)
        elif name == "dup":
            ex = duplicate_code_scene(16, 16, device_id=0)
        elif name == "cornell":
            ex = scenes.cornell_box(16, 16, 1, device_id=0)
        elif name == "spheres":                              # analytic spheres, more than eight: their slots span the whole grid
            ex = custom_scene(two, spheres=tuple((r.uniform(-2, 2), r.uniform(-2, 2), r.uniform(-2, 2), r.uniform(0.05, 0.6)) for _ in range(10)))
        elif name == "mesh":
            ex = custom_scene(sphere_obj_triangles())
        else:
            raise KeyError(name)
        ex.build_scene()
        geom = CP.scene_geometry(ex.scene)
        tree = ex.scene.ctx.wide_tree_download(ex.scene.primitive_count)
        pts = geom.tris.reshape(-1, 3).astype(np.float64)
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        if geom.spheres.shape[0]:
            s = geom.spheres.astype(np.float64)
            lo, hi = np.minimum(lo, (s[:, :3] - s[:, 3:]).min(axis=0)), np.maximum(hi, (s[:, :3] + s[:, 3:]).max(axis=0))
        _SCENES[name] = (ex, geom, (tree["grid_min"], tree["grid_cell"]), lo, hi)
    return _SCENES[name]


def sweep_rays(name, n, seed):
    """n float32 rows (o, d) of the kinds the culling can get wrong: origins inside the scene's box, 3 and 1000 extents away and aimed at it, starts
    in overlap (on the surface), directions with zero components, spheres that stand still, and rows with NaN and +-inf.  d is not normalised:
    mostly d = target - o, so that t = 1 is the target."""
    ex, geom, grid, lo, hi = scene(name)
    r = np.random.RandomState(seed)
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    target = mid + 0.5 * (hi - lo) * r.uniform(-1, 1, (n, 3))
    o = mid + 0.6 * (hi - lo) * r.uniform(-1, 1, (n, 3))
    kind = r.randint(0, 16, n)
    u = r.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[kind == 0] = (mid + 3.0 * ext * u)[kind == 0]
    o[kind == 1] = (mid + 1000.0 * ext * u)[kind == 1]
    t = geom.tris.astype(np.float64)
    k, b = r.randint(0, t.shape[0], n), r.dirichlet((1, 1, 1), n)
    surf = (t[k] * b[:, :, None]).sum(axis=1)
    o[kind == 2] = surf[kind == 2]                           # on the surface: overlap at the start for every radius
    o[kind == 3] = (surf + 0.005 * ext * u)[kind == 3]       # ... and just off it: overlap for the larger radii only
    if geom.spheres.shape[0]:                                # inside an analytic sphere: the contact from inside
        sp = geom.spheres.astype(np.float64)[r.randint(0, geom.spheres.shape[0], n)]
        o[kind == 9] = (sp[:, :3] + 0.3 * sp[:, 3:] * u)[kind == 9]
    d = target - o
    d[kind == 4] *= 3.0
    d[kind == 5, 0] = 0.0
    d[kind == 6, 1:] = 0.0                                   # along x
    d[kind == 7] = 0.0                                       # stands still
    d[kind == 8] = (u * ext * 1e-3)[kind == 8]               # a slow one: contacts at large t
    rays = np.concatenate([o, d], axis=1).astype(F)
    if n >= 63:
        for j, (col, val) in enumerate(((0, np.nan), (2, np.inf), (3, np.nan), (4, -np.inf), (5, np.inf))):
            rays[7 + 9 * j, col] = val
    return rays, F(ext)


def cast(name, rays, radius, tmax=None, flags=0, stack_size=64):
    ex = scene(name)[0]
    as_arg = lambda x: on_dev(x) if isinstance(x, np.ndarray) else x
    return cpu(SweepQuery(ex.scene, stack_size, flags).cast(on_dev(rays), as_arg(radius), as_arg(tmax), attributes=True))


def assert_same(got, want, what):
    bad = np.nonzero(got["prim"] != want["prim"])[0]
    assert bad.size == 0, (what, "prim", bad[:8], got["prim"][bad[:8]], want["prim"][bad[:8]], got["t"][bad[:8]], want["t"][bad[:8]])
    assert np.array_equal(got["code"], want["code"]), (what, "code")
    for k in ("t", "point", "uv", "normal"):
        assert same(got[k], want[k]), (what, k)


def variants(n, ext, i, seed):
    """the i-th way of giving radius and tmax for n queries: every radius of RADII as a scalar, then per query; tmax unbounded, a scalar, per query"""
    r = np.random.RandomState(seed)
    radius = float(F(RADII[i % 4]) * ext) if (i // 4) % 2 == 0 else (r.choice(np.array(RADII, F), n) * ext).astype(F)
    tmax = (None, 1.0, r.choice(np.array([np.inf, 2.0, 1.0, 0.5, 0.0], F), n).astype(F))[i % 3]
    return radius, tmax


# ---- 0. the device functions are the host text, row by row -----------------------------------------------------------------------------------------
def test_device_rows_equal_host_rows(gpu_ctx_ok):
    ctx = scene("one")[0].scene.ctx
    rs = np.random.RandomState(41)
    n = 4096
    o = rs.uniform(-0.5, 1.5, (n, 3)).astype(F); d = (rs.uniform(-0.5, 1.5, (n, 3)) - o).astype(F)
    r = rs.choice(np.array([0.0, 0.01, 0.05, 0.3], F), n); B = rs.choice(np.array([np.inf, 1.0, 0.5], F), n)
    a = rs.uniform(0, 1, (n, 3)).astype(F)
    b, c = (a + rs.uniform(-0.4, 0.4, (n, 3))).astype(F), (a + rs.uniform(-0.4, 0.4, (n, 3))).astype(F)
    c[::19] = (a + (b - a) * F(2.0))[::19]; d[::11] = 0.0; d[::13] = ((b - a) * F(0.75))[::13]
    rows = SE.tri_rows(o, d, r, F(2.0 ** -17), B, a, b, c)
    rows[5::97, 0] = np.nan; rows[6::97, 6] = -1.0; rows[7::97, 8] = np.nan
    got, want = ctx.kat_sweep(rows), _native.kat_sweep_host(rows)
    assert (np.bincount(got[:, 1].astype(int) + 1, minlength=9) > 0).all()
    assert same(got, want)
    assert same(got, SE.kat_expected(rows))
    rows = SE.sphere_rows(o, d, r, F(2.0 ** -17), B, a, rs.choice(np.array([0.02, 0.2, 0.7, 2.0], F), n))
    got = ctx.kat_sweep(rows, True)
    assert same(got, _native.kat_sweep_host(rows, True)) and same(got, SE.kat_expected(rows, True))
    assert set(np.unique(got[:, 1])) == {-1.0, 0.0, 8.0, 9.0}


# ---- 7. walk, scan and restatement agree on every bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "tiny", "chain", "dup", "cornell", "spheres", "mesh"])
def test_walk_equals_scan_equals_numpy(gpu_ctx_ok, name):
    ex, geom, grid, lo, hi = scene(name)
    stack = 2048 if name == "chain" else 64
    i = 0
    for n in SIZES:
        rays, ext = sweep_rays(name, n, seed=100 + n)
        for _ in RADII:
            radius, tmax = variants(n, ext, i, seed=i)
            walk = cast(name, rays, radius, tmax, 0, stack)
            scan = cast(name, rays, radius, tmax, SCAN, stack)
            assert_same(walk, scan, (name, n, i, "walk against scan"))
            # blocked is cast.t <= tmax, through the walk that stops at the first contact and through the scan
            B = np.broadcast_to(np.asarray(np.inf if tmax is None else tmax, F), (n,))
            want_b = (scan["t"] <= B) & np.isfinite(scan["t"])      # (a miss is t = +inf: an unbounded tmax does not make it a contact)
            assert np.array_equal(want_b, scan["prim"] >= 0)
            as_arg = lambda x: on_dev(x) if isinstance(x, np.ndarray) else x
            for flags in (0, SCAN):
                got_b = SweepQuery(ex.scene, stack, flags).blocked(on_dev(rays), as_arg(radius), as_arg(tmax))
                assert got_b.dtype == torch.bool and np.array_equal(got_b.cpu().numpy(), want_b), (name, n, i, flags, "blocked")
            i += 1
    assert ex.scene.ctx.stats()["stack_overflow"] == 0
    # the restatement, on as many queries as numpy can afford: every radius and every kind of bound among them
    n = 160 if name in ("mesh", "chain") else 257
    rays, ext = sweep_rays(name, n, seed=7)
    rs = np.random.RandomState(8)
    radius = (rs.choice(np.array(RADII, F), n) * ext).astype(F)
    tmax = rs.choice(np.array([np.inf, np.inf, 2.0, 1.0, 0.5], F), n).astype(F)
    want = SE.brute_force(rays, radius, tmax, geom, grid[0], grid[1])
    assert (want["prim"] >= 0).sum() > n // 16 and (want["prim"] < 0).sum() >= 5
    assert {-1, 0, 1} <= set(want["code"]), set(want["code"])              # a miss, an overlap and a face among them
    if name == "tiny":
        assert set(want["code"]) & {2, 3, 4} and set(want["code"]) & {5, 6, 7}, set(want["code"])      # ... and an edge and a corner
    if name == "spheres":
        assert {8, 9} <= set(want["code"]), set(want["code"])
    assert_same(cast(name, rays, radius, tmax, 0, stack), want, (name, "walk against numpy"))
    assert_same(cast(name, rays, radius, tmax, SCAN, stack), want, (name, "scan against numpy"))


def test_origins_far_away_and_invalid_queries(gpu_ctx_ok):
    """3 and 1000 extents away the margin grows with the origin and the walk still returns the scan's bits; invalid queries get the miss"""
    ex, geom, grid, lo, hi = scene("mesh")
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    r = np.random.RandomState(12)
    n = 600
    u = r.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    far = np.where(np.arange(n)[:, None] % 2 == 0, 3.0, 1000.0) * ext
    o = mid + far * u
    target = mid + 0.4 * (hi - lo) * r.uniform(-1, 1, (n, 3))
    rays = np.concatenate([o, target - o], axis=1).astype(F)
    for rad in (0.0, 0.01 * ext, 0.2 * ext):
        walk, scan = cast("mesh", rays, float(rad)), cast("mesh", rays, float(rad), None, SCAN)
        assert_same(walk, scan, ("far", rad))
        assert (walk["prim"] >= 0).mean() > 0.3
    on = geom.tris[0].astype(np.float64).mean(axis=0)        # a point of the mesh, approached from 3 extents above it
    bad = np.tile(np.array([[on[0], on[1], on[2] + 3 * ext, 0, 0, -ext]], F), (8, 1))
    radius = np.full(8, 0.01 * ext, F); tmax = np.full(8, np.inf, F)
    bad[0, 1] = np.nan; bad[1, 4] = np.inf; radius[2] = -1.0; radius[3] = np.nan; radius[4] = np.inf; tmax[5] = -1.0; tmax[6] = np.nan
    for flags in (0, SCAN):
        got = cast("mesh", bad, radius, tmax, flags)
        assert list(got["prim"][:7]) == [-1] * 7 and np.isinf(got["t"][:7]).all() and list(got["code"][:7]) == [-1] * 7
        assert not got["point"][:7].any() and not got["normal"][:7].any() and got["prim"][7] >= 0 and got["code"][7] >= 1


# ---- 8. ties to the point queries, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mesh", "spheres"])
def test_ties_to_the_point_queries(gpu_ctx_ok, name):
    ex, geom, grid, lo, hi = scene(name)
    n = 3000
    rays, ext = sweep_rays(name, n, seed=21)
    rays = rays[SE.valid(rays[:, 0:3], rays[:, 3:6], np.zeros(len(rays), F), np.zeros(len(rays), F))]
    n = rays.shape[0]
    radius = (np.random.RandomState(22).choice(np.array(RADII, F), n) * ext).astype(F)
    got = cast(name, rays, radius)
    pq = PointQuery(ex.scene)
    o, rad = on_dev(rays[:, 0:3]), on_dev(radius)
    # T == 0 exactly where some primitive is within r of o, and then prim is the smallest id among them
    cnt = pq.count_within(o, rad).cpu().numpy()
    assert np.array_equal(got["t"] == 0, cnt > 0) and (cnt > 0).sum() > 100
    assert np.array_equal(got["code"] == 0, cnt > 0)
    w = pq.within(o, rad)
    qi, wp = w.query().cpu().numpy(), w.prim.cpu().numpy()
    smallest = np.full(n, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(smallest, qi, wp)
    assert np.array_equal(got["prim"][cnt > 0], smallest[cnt > 0])
    # a contact in motion: point and uv are cp_triangle's / cp_sphere's answer on that primitive at c(T), and no primitive is nearer to c(T) than verified
    hit = np.nonzero(got["code"] >= 1)[0]
    assert hit.size > 200
    cT = (rays[hit, 0:3] + rays[hit, 3:6] * got["t"][hit][:, None]).astype(F)
    ctx = ex.scene.ctx
    is_sph = got["code"][hit] >= 8
    ver = np.zeros((hit.size, 6), F)
    tri_of = {int(p): k for k, p in enumerate(geom.tri_prim)}
    sph_of = {int(p): k for k, p in enumerate(geom.sphere_prim)}
    if (~is_sph).any():
        tk = np.array([tri_of[int(p)] for p in got["prim"][hit][~is_sph]])
        ver[~is_sph] = ctx.kat_closest_point(np.concatenate([cT[~is_sph], geom.tris[tk].reshape(-1, 9)], axis=1))
    if is_sph.any():
        sk = np.array([sph_of[int(p)] for p in got["prim"][hit][is_sph]])
        ver[is_sph] = ctx.kat_closest_point(np.concatenate([cT[is_sph], geom.spheres[sk]], axis=1), True)
    assert same(got["point"][hit], ver[:, 1:4]) and same(got["uv"][hit], ver[:, 4:6])
    m = SE.margin(grid[0], grid[1], rays[hit, 0:3], radius[hit])
    rh = radius[hit] + (radius[hit] * F(SE.TOL_REL) + m)
    assert (ver[:, 0] <= rh * rh).all()                                  # the certificate: within r + tol by the library's own distance
    near = pq.closest(on_dev(cT)).dist2.cpu().numpy()
    assert (near <= ver[:, 0]).all()


# ---- 9. the shape of the work ---------------------------------------------------------------------------------------------------------------------------
def equal_hits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def test_chunks_side_stream_strided_rays_and_empty(gpu_ctx_ok):
    ex, geom, grid, lo, hi = scene("mesh")
    ctx = ex.scene.ctx
    rays, ext = sweep_rays("mesh", 1000, seed=31)
    q = SweepQuery(ex.scene)
    rt, rad = on_dev(rays), on_dev(np.full(1000, 0.01 * ext, F))
    a = q.cast(rt, rad, 2.0, attributes=True)
    ha, ca = q.cast_counts(rt, rad, 2.0)
    ba = q.blocked(rt, rad, 2.0)
    ctx.set_option("query_chunk_rays", 256)                  # four chunks
    try:
        b = q.cast(rt, rad, 2.0, attributes=True)
        hb, cb = q.cast_counts(rt, rad, 2.0)
        bb = q.blocked(rt, rad, 2.0)
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert equal_hits(a, b) and torch.equal(ca, cb) and torch.equal(ha.prim, hb.prim) and torch.equal(ba, bb)
    # a strided [N, 8] view, a strided radius
    wide = torch.full((1000, 8), float("nan"), device=DEV); wide[:, :6] = rt
    rad2 = torch.zeros(2000, device=DEV); rad2[::2] = rad
    assert equal_hits(q.cast(wide[:, :6], rad2[::2], 2.0, attributes=True), a)
    # a side stream: the cast is ordered after the work that makes its rays and before the work that reads its answers
    s = torch.cuda.Stream(DEV)
    big = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(4):
            big = torch.tanh(big @ big)
        late = torch.where(big[0, 0] > 2.0, rt * 0.0, rt)
        h = q.cast(late, rad, 2.0, attributes=True)
        total = h.t.nan_to_num(posinf=0.0).sum() + h.prim.sum()
    torch.cuda.synchronize(DEV)
    assert equal_hits(h, a) and total == a.t.nan_to_num(posinf=0.0).sum() + a.prim.sum()
    # N = 0
    e = q.cast(torch.zeros((0, 6), device=DEV), 0.1, attributes=True)
    assert e.t.shape == (0,) and e.point.shape == (0, 3) and e.normal.shape == (0, 3) and q.blocked(torch.zeros((0, 6), device=DEV), 0.1).shape == (0,)
    assert q.cast_counts(torch.zeros((0, 6), device=DEV), torch.zeros(0, device=DEV))[1].shape == (0, 2)


def test_host_route_equals_torch_route(gpu_ctx_ok):
    ex, geom, grid, lo, hi = scene("spheres")
    rays, ext = sweep_rays("spheres", 500, seed=33)
    radius = (np.random.RandomState(34).choice(np.array(RADII, F), 500) * ext).astype(F)
    tmax = np.random.RandomState(35).choice(np.array([np.inf, 1.0], F), 500).astype(F)
    ctx = ex.scene.ctx
    for flags in (0, SCAN):
        want = cast("spheres", rays, radius, tmax, flags)
        got = ctx.sweep(rays, radius, tmax, 64, flags)
        assert_same(got, want, ("host route", flags))
        assert np.array_equal(got["blocked"], want["prim"] >= 0)
        assert np.array_equal(ctx.sweep(rays, radius, tmax, 64, flags, blocked_only=True)["blocked"], want["prim"] >= 0)
    got = ctx.sweep(rays, radius, tmax, 64, COUNT, attributes=False)
    assert "point" not in got and got["counts"].shape == (500, 2) and got["counts"][:, 1].max() <= ex.scene.primitive_count
    assert ctx.sweep(np.zeros((0, 6), F), 0.1)["t"].shape == (0,)


def test_refusals_queue_nothing(gpu_ctx_ok):
    ex = scene("cornell")[0]
    ctx = ex.scene.ctx
    rays, ext = sweep_rays("cornell", 100, seed=37)
    rt, host = on_dev(rays), np.ascontiguousarray(rays)
    out = torch.full((100,), -7.0, device=DEV)
    out3 = torch.full((100, 3), -7.0, device=DEV)
    base = dict(rays=rt.data_ptr(), n=100, ray_stride=6, radius_all=1.0)
    cases = [
        (r"error -2:.*rays: not device memory", dict(base, rays=host.ctypes.data, out_t=out.data_ptr())),
        (r"error -2:.*radius: not device memory", dict(base, radius=host.ctypes.data, out_t=out.data_ptr())),
        (r"error -2:.*tmax: not device memory", dict(base, tmax=host.ctypes.data, out_t=out.data_ptr())),
        (r"error -2:.*out_normal: not device memory", dict(base, out_normal=host.ctypes.data)),
        (r"error -2:.*ray_stride < 6", dict(base, ray_stride=5, out_t=out.data_ptr())),
        (r"error -2:.*radius_stride < 1", dict(base, radius=out.data_ptr(), radius_stride=0, out_t=out.data_ptr())),
        (r"error -2:.*tmax_stride < 1", dict(base, tmax=out.data_ptr(), tmax_stride=0, out_t=out.data_ptr())),
        (r"error -2:.*point_stride < 3", dict(base, out_point=out3.data_ptr(), point_stride=2)),
        (r"error -2:.*uv_stride < 2", dict(base, out_uv=out3.data_ptr(), uv_stride=1)),
        (r"error -2:.*normal_stride < 3", dict(base, out_normal=out3.data_ptr(), normal_stride=2)),
        (r"error -2:.*unknown flags", dict(base, flags=4, out_t=out.data_ptr())),
        (r"error -2:.*stack_size", dict(base, stack_size=0, out_t=out.data_ptr())),
        (r"error -2:.*counts must be 8-byte aligned", dict(base, flags=COUNT, counts=out.data_ptr() + 4)),
    ]
    for pattern, kw in cases:
        with pytest.raises(_native.TirtError, match=pattern):
            ctx.query_sweep(**kw)
    unbuilt = _native.Context(0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*LBVH not built"):
        unbuilt.query_sweep(rt.data_ptr(), 100, 6, radius_all=1.0, out_t=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.sweep(host, 1.0)
    torch.cuda.synchronize(DEV)
    assert (out == -7.0).all() and (out3 == -7.0).all()      # nothing ran


def test_a_stack_of_one_entry_and_the_long_chain(gpu_ctx_ok):
    """stack_size = 1: the same answers, or entries dropped and counted -- a query can only differ from the scan if it dropped one; the next call with
    room is right again.  On the 600-deep chain a 2048-entry stack (16 in LDS, the rest in the spill buffer) gives the scan's answers, 17 and 4 drop."""
    for name, sizes in (("mesh", (1, 64)), ("chain", (1, 4, 17, 2048))):
        ex, geom, grid, lo, hi = scene(name)
        ctx = ex.scene.ctx
        rays, ext = sweep_rays(name, 2048, seed=43)
        radius = float(0.01 * ext)
        scan = cast(name, rays, radius, None, SCAN)
        over, miss = [], []
        for s in sizes:
            ctx.stats_reset()
            got = cast(name, rays, radius, None, 0, s)
            try:
                over.append(ctx.stats()["stack_overflow"])
            except _native.TirtStackOverflow as err:
                over.append(err.stats["stack_overflow"])
            miss.append(int(((got["t"].view(np.uint32) != scan["t"].view(np.uint32)) | (got["prim"] != scan["prim"])).sum()))
        print(name, "stack sizes", sizes, "queries that dropped an entry", over, "queries that differ from the scan", miss)
        assert all(m <= o for m, o in zip(miss, over)), (sizes, over, miss)
        assert over[0] > 0 and over[-1] == 0 and miss[-1] == 0
        assert all(a >= b for a, b in zip(over, over[1:]))
        ctx.stats_reset()


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
    rays, e = sweep_rays("mesh", 2048, seed=47)
    radius = float(0.01 * e)
    run = lambda x, flags=0: cpu(SweepQuery(x.scene, 64, flags).cast(on_dev(rays), radius, attributes=True))
    a, b = run(ex), run(fresh)
    assert_same(a, b, "updated against fresh")
    assert_same(a, run(ex, SCAN), "updated walk against scan")
    assert not np.array_equal(a["prim"], cast("mesh", rays, radius)["prim"])        # the answers did move


def test_counts(gpu_ctx_ok):
    ex, geom, grid, lo, hi = scene("mesh")
    rays, ext = sweep_rays("mesh", 4096, seed=51)
    n_prim = ex.scene.primitive_count
    rt = on_dev(rays)
    for rad in (0.001, 0.01):
        h, c = SweepQuery(ex.scene).cast_counts(rt, float(rad * ext))
        hs, cs = SweepQuery(ex.scene, 64, SCAN).cast_counts(rt, float(rad * ext))
        torch.cuda.synchronize(DEV)
        c, cs = c.cpu().numpy(), cs.cpu().numpy()
        ok = SE.valid(rays[:, 0:3], rays[:, 3:6], np.zeros(4096, F), np.zeros(4096, F))
        assert torch.equal(h.prim, hs.prim) and torch.equal(h.t.view(torch.int32), hs.t.view(torch.int32))
        assert (cs[ok] == [0, n_prim]).all() and (cs[~ok] == 0).all() and (c[~ok] == 0).all()
        print("radius %g of the extent: primitive tests per query mean %.1f max %d of %d, node tests mean %.1f" % (rad, c[ok, 1].mean(), c[ok, 1].max(), n_prim, c[ok, 0].mean()))
        assert c[ok, 1].max() <= n_prim and c[ok, 1].mean() < 0.5 * n_prim and (c[ok, 0] >= 4).all()      # fewer primitive tests than the scan


# ---- 10. lifecycle ------------------------------------------------------------------------------------------------------------------------------------------
def test_ray_and_point_queries_around_a_cast(gpu_ctx_ok):
    ex, geom, grid, lo, hi = scene("cornell")
    rays, ext = sweep_rays("cornell", 4096, seed=53)
    ok = SE.valid(rays[:, 0:3], rays[:, 3:6], np.zeros(4096, F), np.zeros(4096, F))
    rt = on_dev(rays[ok])
    rq, pq, sq = RayQuery(ex.scene), PointQuery(ex.scene), SweepQuery(ex.scene)
    r0, p0 = rq.closest(rt, attributes=True), pq.closest(rt[:, :3], attributes=True)
    s0 = sq.cast(rt, float(0.01 * ext), attributes=True)
    r1, p1 = rq.closest(rt, attributes=True), pq.closest(rt[:, :3], attributes=True)
    s1 = sq.cast(rt, float(0.01 * ext), attributes=True)
    torch.cuda.synchronize(DEV)
    assert equal_hits(r0, r1) and equal_hits(p0, p1) and equal_hits(s0, s1)
    assert (r0.prim >= 0).any() and (s0.prim >= 0).any()
