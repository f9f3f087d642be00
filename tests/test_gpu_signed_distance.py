"""Signed distance on the device (csrc/tirt_signed_distance.hip, sd_sign in csrc/tirt_closest_point.h, through tirt_query_signed_distance / tirt_signed_distance /
tirt_signed_distance_prepare / _table_download / tirt_kat_signed_distance and ti_raytrace_amd.PointQuery) against the definition of include/tirt.h as
tests/signed_distance_expected.py restates it.  The table and every distance are compared on bits; the signs also against truth that uses no normal
(tests/signed_distance_scenes.py: closed forms and the winding number), under the host test's threshold and cap."""
import numpy as np
import pytest
import torch

import closest_point_expected as E
import signed_distance_expected as SE
import signed_distance_scenes as S
from common import on_device, same_bits as same
from ti_raytrace_amd import PointQuery, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
SCAN = _native.TRAVERSE_EXHAUSTIVE
_FULL = {}


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sd_obj_gpu")


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cpu(h):
    torch.cuda.synchronize(DEV)
    return tuple(None if x is None else x.cpu().numpy() for x in h)


def device_case(name, tmp_dir):
    """tests/signed_distance_scenes.case with the scene on the device (once per module)"""
    c = S.case(name, tmp_dir)
    if "ctx" not in c:
        c["ctx"] = on_device(c["ex"])
    return c


def fresh_scene(name, tmp_dir, tris=None):
    """another scene of the same mesh on a context of its own: no table yet"""
    ex, geom = S.make_scene(name, tmp_dir, tris)
    return ex, geom, on_device(ex)


def special_points(geom, tab):
    """points exactly on the vertices, the edge midpoints and the face centroids, and points on both sides of every vertex and edge along its pseudo-normal;
    then rows with NaN, +inf and -inf coordinates"""
    t = geom.tris.astype(np.float64)
    bases = [t[:, k] for k in range(3)] + [0.5 * (t[:, i] + t[:, j]) for i, j in ((0, 1), (0, 2), (1, 2))]      # rows 1..6 of the table
    on = bases + [t.mean(axis=1)]
    sides = []
    for row, base in zip(range(1, 7), bases):
        N = tab[geom.tri_prim, row, :3].astype(np.float64)
        ln = np.linalg.norm(N, axis=1, keepdims=True)
        ok = np.isfinite(ln[:, 0]) & (ln[:, 0] > 0)
        N = np.where(ok[:, None], N / np.where(ok[:, None], ln, 1.0), 0.0)
        sides += [(base + 0.05 * N)[ok], (base - 0.05 * N)[ok]]
    bad = np.tile(t.reshape(-1, 3).mean(axis=0), (9, 1))
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            bad[3 * j + a, a] = v
    n_on = sum(x.shape[0] for x in on)
    return np.concatenate(on + sides + [bad], axis=0).astype(F), n_on


def full(name, tmp_dir):
    """the device scene, its downloaded table, all queries (the host test's, or 512 uniform ones for the meshes that are not closed, then the special ones)
    and the restatement's answer for them FROM THE DOWNLOADED TABLE"""
    if name not in _FULL:
        c = device_case(name, tmp_dir)
        tab = c["ctx"].signed_distance_table()
        base = c["pts"] if name in S.CLOSED else S.uniform_queries(c["geom"], 512)
        extra, n_on = special_points(c["geom"], c["tab"])
        pts = np.concatenate([base, extra], axis=0)
        _FULL[name] = dict(c, dev_tab=tab, all_pts=pts, n_base=base.shape[0], n_on=n_on, all_want=SE.signed_distance(pts, c["geom"], tab))
    return _FULL[name]


def signed(ex, pts, flags=0, max_distance=None, stack_size=64):
    return cpu(PointQuery(ex.scene, stack_size, flags).signed_distance(on_dev(pts), max_distance, attributes=True))


def assert_signed(got, want, what):
    """got: SignedHits as numpy; want: (sd, d2, prim, q, uv)"""
    sd, prim, q, uv = got
    bad = np.nonzero(prim != want[2])[0]
    assert bad.size == 0, (what, "prim", bad[:8], prim[bad[:8]], want[2][bad[:8]])
    bad = np.nonzero(sd.view(np.uint32) != want[0].view(np.uint32))[0]
    assert bad.size == 0, (what, "sd", bad[:8], sd[bad[:8]], want[0][bad[:8]], prim[bad[:8]], uv[bad[:8]])
    assert same(q, want[3]), (what, "point")
    assert same(uv, want[4]), (what, "uv")


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_table_is_the_restatements(gpu_ctx_ok, tmp_dir, name):
    c = device_case(name, tmp_dir)
    tab = c["ctx"].signed_distance_table()
    assert tab.shape == c["tab"].shape == (c["ex"].scene.primitive_count, 7, 4)
    assert np.array_equal(SE.class_bits(tab), SE.class_bits(c["tab"])), (SE.class_bits(tab), SE.class_bits(c["tab"]))
    bad = np.nonzero(~((tab.view(np.uint32) == c["tab"].view(np.uint32)) | (np.isnan(tab) & np.isnan(c["tab"]))).all(axis=(1, 2)))[0]
    assert bad.size == 0, (name, bad[:4], tab[bad[:2]], c["tab"][bad[:2]])
    rep = PointQuery(c["ex"].scene).mesh_report()
    assert rep == SE.report(c["tab"], c["geom"]) and rep["closed"] == (name in S.CLOSED)
    assert np.array_equal(c["ctx"].signed_distance_table().view(np.uint32), tab.view(np.uint32))      # (asked again: the same table)


def test_minus_zero_is_zero_when_corners_are_matched(gpu_ctx_ok, tmp_dir):
    """every other triangle of the cube writes its zero coordinates as -0: corners are matched by VALUE (three fp32 ==), so the cube stays closed and the
    sums are the cube's; matching bit patterns would find boundary edges everywhere"""
    tris = S.cube_triangles()
    tris[0::2][tris[0::2] == 0.0] = -0.0
    ex, geom, ctx = fresh_scene("cube_negzero", tmp_dir, tris)
    assert np.signbit(geom.tris).any() and not np.signbit(geom.tris[1::2]).any()
    want = SE.table(geom, 12)
    tab = ctx.signed_distance_table()
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32))
    assert PointQuery(ex.scene).mesh_report()["closed"]
    assert np.array_equal(tab[:, 1:], S.case("cube", tmp_dir)["tab"][:, 1:])      # the sums do not see the sign of a zero


# ---- distances: walk == scan == restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_walk_equals_scan_equals_restatement(gpu_ctx_ok, tmp_dir, name):
    c = full(name, tmp_dir)
    pts, want = c["all_pts"], c["all_want"]
    assert_signed(signed(c["ex"], pts, SCAN), want, (name, "scan"))
    assert_signed(signed(c["ex"], pts, 0), want, (name, "walk"))
    sd = want[0]
    finite = np.isfinite(pts).all(axis=1)
    assert (want[2][~finite] == -1).all() and np.isposinf(sd[~finite]).all() and np.isfinite(sd[finite]).all()
    if name in ("cube", "lprism", "quad", "cube_flipped"):
        # exactly on a vertex, an edge or a face of a mesh whose faces lie in coordinate planes: s == 0, and that is positive
        on = slice(c["n_base"], c["n_base"] + c["n_on"])
        assert (sd[on] >= 0).all() and not np.signbit(sd[on]).any() and (sd[on] < 1e-6).all()
    if name in S.CLOSED:
        assert (sd[c["n_base"] + c["n_on"]:][:-9] < 0).any() and (sd[c["n_base"] + c["n_on"]:][:-9] > 0).any()      # both sides of the features


@pytest.mark.parametrize("name", S.CLOSED)
def test_signs_are_the_truth(gpu_ctx_ok, tmp_dir, name):
    c = full(name, tmp_dir)
    pts = c["all_pts"][:-9]
    sd, prim, _, _ = signed(c["ex"], pts)
    d2 = c["all_want"][1][:-9]
    truth = S.inside_truth(name, pts.astype(np.float64))
    far = d2.astype(np.float64) > (S.THRESHOLD * c["extent"]) ** 2
    near_base = int((~far[:c["n_base"]]).sum())
    print("%s: %d of the %d host-test queries nearer than the threshold" % (name, near_base, c["n_base"]))
    assert near_base <= S.CAP * c["n_base"]
    bad = np.nonzero(far & ((sd < 0) != truth))[0]
    assert bad.size == 0, (name, bad[:8], pts[bad[:8]], sd[bad[:8]])
    inside = cpu((PointQuery(c["ex"].scene).inside(on_dev(pts)),))[0]
    assert inside.dtype == np.bool_ and np.array_equal(inside, sd < 0)
    if name in ("lprism", "union"):
        face_sd, _ = SE.sign_from(pts, c["geom"], c["dev_tab"], tuple(w[:-9] for w in c["all_want"][1:]), face_normal_only=True)
        assert int((far & ((face_sd < 0) != truth)).sum()) >= 50      # what an implementation on face normals alone would get wrong


# ---- more triangles than the issue's meshes have: many blocks, a deep tree, the stack's tail in global memory -----------------------------------------
def test_icosphere_of_1280_triangles(gpu_ctx_ok, tmp_dir):
    """60 blocks of corners and a tree of several levels: the table on bits, the signs against the winding number, walk == scan"""
    tris = S.icosphere_triangles(levels=3)
    ex, geom, ctx = fresh_scene("icosphere1280", tmp_dir, tris)
    want_tab = SE.table(geom, 1280)
    tab = ctx.signed_distance_table()
    assert np.array_equal(tab.view(np.uint32), want_tab.view(np.uint32))
    assert ctx.signed_distance_prepare() == dict(SE.report(want_tab, geom))
    pts = np.concatenate([S.uniform_queries(geom, 1024), special_points(geom, want_tab)[0][::7]], axis=0)
    walk, scan = signed(ex, pts), signed(ex, pts, SCAN)
    for a, b in zip(walk, scan):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert_signed(walk, SE.signed_distance(pts, geom, tab), "walk against the restatement")
    finite = np.isfinite(pts).all(axis=1)
    truth = S.winding_number(pts[finite].astype(np.float64), tris) > 0.5
    far = np.abs(walk[0][finite]) > S.THRESHOLD * 2.0                     # (the sphere's extent is 2)
    assert (far & ((walk[0][finite] < 0) != truth)).sum() == 0 and truth.any() and (~truth).any()
    assert far[:1024].mean() > 0.99                           # (the uniform queries; the special ones lie ON the surface by construction)


@pytest.mark.parametrize("tree", [1, 0])
def test_deep_tree_uses_the_stacks_tail(gpu_ctx_ok, tree):
    """600 overlapping triangles with one Morton code (a ~200-level tree in the reference's own LBVH): a corner lies in very many boxes, the build's stack
    goes far beyond its 16 entries in LDS; a 4-entry stack is refused, the largest one gives the restatement's table"""
    from common import long_chain_scene
    ex = long_chain_scene(16, 16)
    ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    ctx = ex.scene.ctx
    geom = E.scene_geometry(ex.scene)
    want_tab = SE.table(geom, ex.scene.primitive_count)
    pts = S.uniform_queries(geom, 512)
    with pytest.raises(_native.TirtError, match=r"error -4:.*ran out of traversal stack \(stack_size 4\)"):
        ctx.signed_distance(pts, stack_size=4)
    try:
        ctx.stats()
    except _native.TirtStackOverflow:
        pass
    tab = ctx.signed_distance_table()
    assert np.array_equal(tab.view(np.uint32), want_tab.view(np.uint32))
    rep = ctx.signed_distance_prepare()
    assert rep["boundary_edges"] == 3 * 630 and rep["primitives"] == 631 and not rep["closed"]
    want = SE.signed_distance(pts, geom, tab)
    assert_signed(signed(ex, pts, SCAN, stack_size=2048), want, "scan")
    assert_signed(signed(ex, pts, 0, stack_size=2048), want, "walk")
    assert ctx.stats()["stack_overflow"] == 0


@pytest.mark.parametrize("tree", [1, 0])
def test_deep_tree_at_the_end_of_the_stacks_lds_part(gpu_ctx_ok, tree):
    """the same scene with the build's stack ending where its LDS part ends (16: no tail, the spill pointer is null) and one entry later (17: a tail of
    one entry per thread): refused as the 4-entry stack is, and the table made afterwards is the restatement's"""
    from common import long_chain_scene
    ex = long_chain_scene(16, 16)
    ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    ctx = ex.scene.ctx
    geom = E.scene_geometry(ex.scene)
    pts = S.uniform_queries(geom, 512)
    for s in (16, 17):
        with pytest.raises(_native.TirtError, match=r"error -4:.*ran out of traversal stack \(stack_size %d\)" % s):
            ctx.signed_distance(pts, stack_size=s)
        try:
            ctx.stats()
        except _native.TirtStackOverflow:
            pass
    tab = ctx.signed_distance_table()
    assert np.array_equal(tab.view(np.uint32), SE.table(geom, ex.scene.primitive_count).view(np.uint32))


# ---- bounds, layouts, sizes ---------------------------------------------------------------------------------------------------------------------
def test_bounds_layouts_and_sizes(gpu_ctx_ok, tmp_dir):
    c = full("union", tmp_dir)
    ex, geom, tab = c["ex"], c["geom"], c["dev_tab"]
    pts = c["all_pts"][:1000]
    want = tuple(w[:1000] for w in c["all_want"])
    n = pts.shape[0]
    with np.errstate(invalid="ignore"):
        t = np.sqrt(want[1]).astype(F)
    dm = np.where(np.arange(n) % 3 == 0, t * F(0.5), np.where(np.arange(n) % 3 == 1, np.nextafter(t, F(np.inf)), F(np.inf))).astype(F)
    dm[::50] = -1.0; dm[7::50] = np.nan
    for flags in (0, SCAN):
        assert_signed(signed(ex, pts, flags, on_dev(dm)), SE.signed_distance(pts, geom, tab, dm), ("per-query bound", flags))
        assert_signed(signed(ex, pts, flags, 0.25), SE.signed_distance(pts, geom, tab, 0.25), ("scalar bound", flags))
    lost = SE.signed_distance(pts, geom, tab, dm)
    assert (lost[2] == -1).any() and np.isposinf(lost[0][lost[2] == -1]).all() and (lost[2] >= 0).any()
    q = PointQuery(ex.scene)
    wide = torch.full((n, 8), 7.0, device=DEV)
    wide[:, :3] = on_dev(pts)
    assert wide[:, :3].stride() == (8, 1)
    assert_signed(cpu(q.signed_distance(wide[:, :3], attributes=True)), want, "strided view")
    e = q.signed_distance(wide[:0, :3], attributes=True)
    assert e.dist.shape == (0,) and e.prim.shape == (0,) and e.point.shape == (0, 3) and e.uv.shape == (0, 2) and q.inside(wide[:0, :3]).shape == (0,)
    for flags in (0, SCAN):
        assert_signed(signed(ex, pts[:65], flags), tuple(w[:65] for w in want), ("n = 65", flags))      # a ragged second wave
    plain = q.signed_distance(on_dev(pts))
    assert plain.point is None and plain.uv is None and same(cpu((plain.dist,))[0], want[0])
    # the host route
    sd, d2, prim, point, uv, counts = c["ctx"].signed_distance(pts, dm)
    assert counts is None and same(d2, lost[1])
    assert_signed((sd, prim, point, uv), lost, "host route")


# ---- the unsigned answers -------------------------------------------------------------------------------------------------------------------------
def test_unsigned_answers_are_untouched(gpu_ctx_ok, tmp_dir):
    c = S.case("union", tmp_dir)
    ex, geom, ctx = fresh_scene("union", tmp_dir)
    pts = on_dev(c["pts"])
    q = PointQuery(ex.scene)
    before = cpu(q.closest(pts, attributes=True))
    rep = q.mesh_report()                                    # (builds the table)
    assert rep["closed"] and rep["primitives"] == 33
    after = cpu(q.closest(pts, attributes=True))
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for flags in (0, SCAN):
        s = cpu(PointQuery(ex.scene, 64, flags).signed_distance(pts, attributes=True))
        u = cpu(PointQuery(ex.scene, 64, flags).closest(pts, attributes=True))
        assert np.array_equal(s[1], u[1]) and np.array_equal(s[2].view(np.uint32), u[2].view(np.uint32)) and np.array_equal(s[3].view(np.uint32), u[3].view(np.uint32))
        assert np.array_equal(np.abs(s[0]), np.sqrt(u[0]))
    want = E.brute_force(c["pts"], geom)
    assert same(before[0], want[0]) and np.array_equal(before[1], want[1])


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------------------
def test_update_vertices_makes_the_table_again(gpu_ctx_ok, tmp_dir):
    shift = np.array([0.75, -0.5, 2.0])
    ex, geom, ctx = fresh_scene("cube", tmp_dir)
    pts = (S.case("cube", tmp_dir)["pts"][:1024].astype(np.float64) + shift).astype(F)
    old = signed(ex, pts)
    ex.scene.update_vertices((S.cube_triangles() + shift).astype(F), first_vertex=0)
    moved, mgeom, mctx = fresh_scene("cube", tmp_dir, S.cube_triangles() + shift)
    a, b = signed(ex, pts), signed(moved, pts)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert_signed(a, SE.signed_distance(pts, mgeom, SE.table(mgeom, 12)), "moved cube")
    assert (a[0] < 0).any() and not np.array_equal(a[0], old[0])
    assert np.array_equal(ctx.signed_distance_table().view(np.uint32), mctx.signed_distance_table().view(np.uint32))


def test_scene_upload_drops_the_table(gpu_ctx_ok, tmp_dir):
    ex, geom, ctx = fresh_scene("cube", tmp_dir)
    cube_tab = ctx.signed_distance_table()
    assert (SE.class_bits(cube_tab) == 0).all()
    sc = ex.scene
    v = np.array(sc.vertex_np, F)
    v[[15, 17]] = v[[17, 15]]                                 # triangle 5 the other way round: the cube_flipped mesh
    ctx.scene_upload(v, sc.primitive_np, sc.material_np, sc.shape_np, sc.light_np, sc.light_count, sc.minboundarynp, sc.maxboundarynp)
    ctx.lbvh_build()
    flipped = S.case("cube_flipped", tmp_dir)
    tab = ctx.signed_distance_table()
    assert np.array_equal(tab.view(np.uint32), flipped["tab"].view(np.uint32))
    assert ctx.signed_distance_prepare()["flipped_edges"] == 6


def test_a_stack_too_small_for_the_build_is_an_error(gpu_ctx_ok, tmp_dir):
    c = S.case("union", tmp_dir)
    ex, geom, ctx = fresh_scene("union", tmp_dir)
    pts = c["pts"][:512]
    ctx.stats_reset()
    sd = signed(ex, pts, stack_size=1)[0]
    assert np.isnan(sd).all()                                # no table: no silent answer
    with pytest.raises(_native.TirtStackOverflow) as err:
        ctx.stats()
    assert err.value.stats["stack_overflow"] > 0
    with pytest.raises(_native.TirtError, match=r"error -4:.*tirt_signed_distance: .*ran out of traversal stack \(stack_size 1\)"):
        ctx.signed_distance(pts, stack_size=1)
    ctx.stats_reset()
    try:
        ctx.stats()
    except _native.TirtStackOverflow:
        pass                                                 # (the walk of the host call above dropped entries as well)
    assert_signed(signed(ex, pts), tuple(w[:512] for w in c["want"]), "stack 64 after the failure")
    assert ctx.stats()["stack_overflow"] == 0
    assert ctx.signed_distance_prepare()["closed"]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing(gpu_ctx_ok, tmp_dir):
    c = device_case("cube", tmp_dir)
    ctx = c["ctx"]
    pts = c["pts"][:100]
    pt = on_dev(pts)
    host = np.ascontiguousarray(pts)
    out = torch.full((100,), -7.0, device=DEV)
    out3 = torch.full((100, 3), -7.0, device=DEV)
    o = out.data_ptr()
    cases = [
        (r"error -2:.*points: not device memory", dict(points=host.ctypes.data, n=100, point_stride=3, out_sd=o)),
        (r"error -2:.*out_sd: not device memory", dict(points=pt.data_ptr(), n=100, point_stride=3, out_sd=host.ctypes.data)),
        (r"error -2:.*null out_sd", dict(points=pt.data_ptr(), n=100, point_stride=3, out_sd=0)),
        (r"error -2:.*dmax: not device memory", dict(points=pt.data_ptr(), n=100, point_stride=3, dmax=host.ctypes.data, out_sd=o)),
        (r"error -2:.*out_point: not device memory", dict(points=pt.data_ptr(), n=100, point_stride=3, out_point=host.ctypes.data, out_sd=o)),
        (r"error -2:.*point_stride < 3", dict(points=pt.data_ptr(), n=100, point_stride=2, out_sd=o)),
        (r"error -2:.*point_out_stride < 3", dict(points=pt.data_ptr(), n=100, point_stride=3, out_point=out3.data_ptr(), point_out_stride=2, out_sd=o)),
        (r"error -2:.*uv_stride < 2", dict(points=pt.data_ptr(), n=100, point_stride=3, out_uv=out3.data_ptr(), uv_stride=1, out_sd=o)),
        (r"error -2:.*dmax_stride < 1", dict(points=pt.data_ptr(), n=100, point_stride=3, dmax=o, dmax_stride=0, out_sd=o)),
        (r"error -2:.*unknown flags", dict(points=pt.data_ptr(), n=100, point_stride=3, flags=4, out_sd=o)),
        (r"error -2:.*stack_size", dict(points=pt.data_ptr(), n=100, point_stride=3, stack_size=0, out_sd=o)),
        (r"error -2:.*counts must be 8-byte aligned", dict(points=pt.data_ptr(), n=100, point_stride=3, flags=_native.COUNT_NODES, counts=o + 4, out_sd=o)),
    ]
    for pattern, kw in cases:
        with pytest.raises(_native.TirtError, match=pattern):
            ctx.query_signed_distance(**kw)
        assert b"tirt_query_signed_distance" in _native.lib().tirt_last_error()
    unbuilt = _native.Context(0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*LBVH not built"):
        unbuilt.query_signed_distance(pt.data_ptr(), 100, 3, o)
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.signed_distance(host)
    with pytest.raises(_native.TirtError, match=r"LBVH not built"):
        unbuilt.signed_distance_prepare()
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
            PointQuery(c["ex"].scene).signed_distance(pt)


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx_ok, tmp_dir):
    ctx = device_case("cube", tmp_dir)["ctx"]
    r = np.random.RandomState(2)
    hand, _ = E.hand_rows()                                  # one point per region of the triangle (0,0,0) (2,0,0) (0,2,0)
    p = np.concatenate([hand[:, 0:3], hand[:, 0:3] * F([1, 1, -1]), r.uniform(-1, 1, (4096, 3)).astype(F)], axis=0)
    tri = np.concatenate([np.tile(hand[:1, 3:12].reshape(1, 3, 3), (14, 1, 1)), r.uniform(-1, 1, (4096, 3, 3)).astype(F)], axis=0)
    N = r.normal(size=(p.shape[0], 7, 3)).astype(F)
    N[:14] = 0.0
    N[np.arange(14), [1, 2, 4, 3, 5, 6, 0] * 2] = F([0.0, 0.0, 1.0])      # only the row of the point's own feature is not zero
    rows, want = SE.kat_rows(p, tri, N)
    got = ctx.kat_signed_distance(rows)
    assert same(got, want), np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][:10]
    assert got[:7, 1].tolist() == [1, 2, 4, 3, 5, 6, 0] and got[7:14, 1].tolist() == [1, 2, 4, 3, 5, 6, 0]
    # N = +z for the feature each point falls on.  A and the interior point lie above the plane (z = 1, 3), the other five IN it: s == 0 is positive.
    # Mirrored in the plane, only those two change sides
    assert (got[:7, 0] > 0).all() and (got[7:14, 0] < 0).tolist() == [True, False, False, False, False, False, True]
    assert np.bincount(got[14:, 1].astype(int), minlength=7).min() > 50
