"""The signed-distance definition (include/tirt.h, "Signed distance") as tests/signed_distance_expected.py restates it, without a device, against truth that
uses no pseudo-normal and no normal at all: analytic inside tests for the cube, the L-prism and the analytic sphere, and the generalised winding number in
float64 for every closed mesh.  Then the feature rule on hand-built (u, v), and the reports of the meshes that are not closed."""
import numpy as np
import pytest

import closest_point_expected as E
import signed_distance_expected as SE
import signed_distance_scenes as S

F = np.float32


@pytest.fixture(scope="module")
def tmp_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sd_obj")


@pytest.mark.parametrize("name", S.CLOSED)
def test_sign_is_inside_outside(tmp_dir, name):
    """4096 uniform queries in 1.5 x the scene box (seed 20261020: the first tried; it keeps the cap on all four meshes) plus, where the mesh has them, points
    at the cube's corners and edges and inside the L-prism at its concave edge.  Every query further than 1e-4 extents from the surface has the true sign,
    and at most 1 % are nearer than that."""
    c = S.case(name, tmp_dir)
    pts, (sd, d2, prim, q, uv), truth, far = c["pts"], c["want"], c["truth"], c["far"]
    assert SE.report(c["tab"], c["geom"])["closed"]
    analytic = S.inside_analytic(name, pts.astype(np.float64))
    if analytic is not None:
        assert np.array_equal(analytic[far], truth[far]), "the winding number and the closed form disagree"
    assert (prim >= 0).all() and np.isfinite(sd).all()
    near = int((~far).sum())
    print("%s: %d queries, %d nearer than %g extents (cap %d), %d inside" % (name, pts.shape[0], near, S.THRESHOLD, int(S.CAP * pts.shape[0]), int(truth.sum())))
    assert near <= S.CAP * pts.shape[0]
    bad = np.nonzero(far & ((sd < 0) != truth))[0]
    assert bad.size == 0, (name, bad[:8], pts[bad[:8]], sd[bad[:8]])
    assert truth[far].any() and (~truth[far]).any()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.abs(sd), SE.tm_sqrt(d2))
    # the shortcut: the winning triangle's own face normal for every feature
    face_sd, _ = SE.sign_from(pts, c["geom"], c["tab"], c["want"][1:], face_normal_only=True)
    wrong = int((far & ((face_sd < 0) != truth)).sum())
    print("%s: the winning triangle's face normal alone has the wrong sign on %d queries" % (name, wrong))
    if name in ("lprism", "union"):
        assert wrong >= 50
        f = SE.feature(uv[:, 0], uv[:, 1])
        assert (f[far & ((face_sd < 0) != truth)] != 0).all()      # on an edge or at a vertex: an interior point's row IS the face normal


def test_union_answers_come_from_all_three_solids(tmp_dir):
    c = S.case("union", tmp_dir)
    sd, d2, prim = c["want"][:3]
    assert (prim[sd < 0] < 12).any() and ((prim[sd < 0] >= 12) & (prim[sd < 0] < 32)).any() and (prim[sd < 0] == 32).any()
    assert c["geom"].sphere_prim.tolist() == [32]
    assert (c["tab"][32] == 0).all()                         # an analytic sphere has no rows


def test_feature_rule():
    cases = [((0.0, 0.0), "A"), ((-0.0, 0.0), "A"), ((1.0, 0.0), "B"), ((0.25, 0.0), "AB"), ((0.0, 1.0), "C"), ((0.0, 0.25), "AC"), ((0.75, 0.25), "BC"),
             ((0.5, 0.5), "BC"), ((0.25, 0.25), "interior"), ((0.3, 0.7), "BC" if F(1.0) - F(0.7) == F(0.3) else "interior"),
             ((np.nan, 0.0), "AB"), ((0.0, np.nan), "AC"), ((np.nan, np.nan), "interior"), ((2.0, 0.0), "AB"), ((1.0, 1.0), "interior")]
    uv = np.array([c[0] for c in cases], F)
    got = SE.feature(uv[:, 0], uv[:, 1])
    assert [SE.ROWS[k] for k in got] == [c[1] for c in cases]
    # the closest points of closest_point_expected.HAND fall on the features they are named after
    rows, _ = E.hand_rows()
    _, _, u, v = E.tri_point(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])
    assert [SE.ROWS[k] for k in SE.feature(u, v)] == [h[0] for h in E.HAND]


def test_cube_table_by_hand(tmp_dir):
    """the cube's pseudo-normals point along the diagonals at the corners and along the bisectors at the edges; a face's diagonal keeps the face normal"""
    c = S.case("cube", tmp_dir)
    tab, tris = c["tab"], c["geom"].tris
    assert (SE.class_bits(tab) == 0).all()
    centre = np.array([0.5, 0.5, 0.5])
    for t in range(12):
        for k in range(3):
            d = tab[t, 1 + k, :3].astype(np.float64)
            want = tris[t, k] - centre
            assert np.allclose(d / np.linalg.norm(d), want / np.linalg.norm(want), atol=1e-6), (t, k, d)
        for row, (i, j) in ((4, (0, 1)), (6, (1, 2)), (5, (2, 0))):
            d = tab[t, row, :3].astype(np.float64)
            m = 0.5 * (tris[t, i] + tris[t, j]) - centre
            m[np.abs(m) < 0.25] = 0.0                         # the edge's midpoint: towards the cube's edge, or the face's centre on a diagonal
            assert np.allclose(d / np.linalg.norm(d), m / np.linalg.norm(m), atol=1e-6), (t, row, d)


def test_reports_of_the_meshes_that_are_not_closed(tmp_dir):
    r = SE.report(S.case("quad", tmp_dir)["tab"], S.case("quad", tmp_dir)["geom"])
    assert r == {"boundary_edges": 4, "nonmanifold_edges": 0, "flipped_edges": 0, "invalid_triangles": 0, "primitives": 2, "closed": False}
    r = SE.report(S.case("cube_flipped", tmp_dir)["tab"], S.case("cube_flipped", tmp_dir)["geom"])
    assert r == {"boundary_edges": 0, "nonmanifold_edges": 0, "flipped_edges": 6, "invalid_triangles": 0, "primitives": 12, "closed": False}
    c = S.case("cube_degenerate", tmp_dir)
    r = SE.report(c["tab"], c["geom"])
    # the sliver is invalid: it is nobody's neighbour (the cube stays closed), its long edge lies on a cube edge that two valid triangles share, its two halves on nothing
    assert r == {"boundary_edges": 2, "nonmanifold_edges": 1, "flipped_edges": 0, "invalid_triangles": 1, "primitives": 13, "closed": False}
    assert SE.class_bits(c["tab"])[12] == (SE.NONMANIFOLD | SE.BOUNDARY << 2 | SE.BOUNDARY << 4 | SE.INVALID_BIT)
    assert np.array_equal(c["tab"][:12, 1:], S.case("cube", tmp_dir)["tab"][:, 1:])      # and it adds nothing to any sum
