"""The winding number on the host: the definition of include/tirt.h ("Winding number") as tests/winding_expected.py restates it, against known answers,
against float64, on a hand-built 4-wide tree (no device), and against the term code of csrc/tirt_winding.h compiled for the host (the library's
tirt_kat_winding_host, and a program of its own under the host sanitizers)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import closest_point_expected as E
import signed_distance_expected as SE
import signed_distance_scenes as S
import winding_expected as W
from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = np.float64
EPS = 2.0 ** -24
HOLE_SEED = 20261021
HOLE_CANDIDATES = 600
HOLE_POINTS = 235            # of the 600 candidates: the pseudo-normal sign says "inside", the float64 winding number is below 0.3


def term_tolerance(n_terms):
    """The bound on |w - truth| for a sum of n_terms exact terms, where every term's hypot(num, den) >= |a||b||c| / 4 (checked by well_conditioned):
    Omega = 2 atan2(num, den).  num and den are each formed by at most 8 roundings of quantities bounded by |a||b||c| (the norms: half an ulp each), so they
    carry absolute errors of at most 8 eps |a||b||c| each, eps = 2^-24, and the angle moves by at most (|d num| + |d den|) / hypot <= 64 eps; tm_atan2 adds
    one ulp of a result of at most pi, 2^-22; doubled: 2 (64 eps + 4 eps) = 136 eps per term.  The quantisation adds half a unit, 2^-31.  Over 4 pi, summed,
    and two more roundings of a result of at most ~1 in wn_result: 2 eps (the conversion of S, and the two products)."""
    return n_terms * (136 * EPS + 2.0 ** -31) / (4 * np.pi) + 3 * EPS


def well_conditioned(q, tris):
    q = np.asarray(q, D)
    a, b, c = (np.asarray(tris, D)[:, k] - q for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(axis=1)
    den = la * lb * lc + (a * b).sum(axis=1) * lc + (a * c).sum(axis=1) * lb + (b * c).sum(axis=1) * la
    return bool((np.hypot(num, den) >= 0.25 * la * lb * lc).all())


def w_of(points, tris, spheres=None):
    points = np.asarray(points, F).reshape(-1, 3)
    return W.answer(points, W.exact_sum(points, tris, spheres))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------------
def test_one_triangle_from_the_origin_is_an_eighth():
    tri = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], D)
    assert well_conditioned([0, 0, 0], tri)
    tol = term_tolerance(1)
    w = w_of([[0, 0, 0]], tri)[0]
    assert abs(float(w) - 0.125) <= tol, (w, tol)
    w = w_of([[0, 0, 0]], tri[:, ::-1])[0]
    assert abs(float(w) + 0.125) <= tol, (w, tol)


def test_cube_inside_outside_and_with_a_face_removed():
    cube = S.cube_triangles()
    tol = term_tolerance(12)
    for q in ([0.5, 0.5, 0.5], [2.0, 1.5, 3.0]):
        assert well_conditioned(q, cube)
    print("tolerance for 12 terms: %.3e" % tol)
    w_in, w_out = w_of([[0.5, 0.5, 0.5], [2.0, 1.5, 3.0]], cube)
    assert abs(float(w_in) - 1.0) <= tol and abs(float(w_out)) <= tol, (w_in, w_out, tol)
    open_cube = cube[2:]                                         # without the face z = 0
    w = w_of([[0.5, 0.5, 0.5]], open_cube)[0]
    assert abs(float(w) - 5.0 / 6.0) <= term_tolerance(10), w


def test_a_point_on_a_face_gets_half_a_turn_from_it():
    """in the interior of the face z = 0 of the cube, on its plane: num is exactly 0 (every z is 0), den < 0 inside the triangle that holds the point and > 0
    for the other: exactly I(2 pi) from the one, 0 from the other, on either orientation (tm_atan2 does not see the sign of a zero)"""
    cube = S.cube_triangles()
    q = np.array([[0.6, 0.3, 0.0]], F)
    two_pi = F(2.0) * F(np.pi)
    for face in (cube[:2], cube[:2][:, ::-1]):
        I = W.quant(W.triangle_omega(q, face))[0]
        assert sorted(I.tolist()) == [0, int(W.quant(two_pi))], I
        assert abs(float(W.result(I.sum())) - 0.5) <= 2 * EPS


def test_zero_area_triangle_and_nan_query():
    sliver = np.array([[[0, 0, 0], [1, 0, 0], [0.5, 0, 0]]], D)
    q = np.array([[0.2, 0.3, 0.4], [0.5, 0.0, 0.0]], F)
    assert (W.triangle_omega(q, sliver) == 0).all() and (W.exact_sum(q, sliver) == 0).all()
    cube = S.cube_triangles()
    assert np.array_equal(W.exact_sum(q, np.concatenate([cube, sliver])), W.exact_sum(q, cube))
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.5, 0.5, 0.5]], F)
    w = w_of(bad, cube)
    assert np.isnan(w[:3]).all() and abs(float(w[3]) - 1.0) <= term_tolerance(12)
    assert W.quant(F(np.nan)) == 0 and W.quant(F(np.inf)) == 0 and W.quant(F(-3.0e9)) == -3221225472000000000 and W.quant(F(8.0e9)) == 0


def test_sphere_term():
    s = np.array([[1.0, 2.0, 3.0, 0.5]], F)
    q = np.array([[1.0, 2.0, 3.2], [1.0, 2.0, 3.5], [1.0, 2.0, 3.6]], F)
    assert np.array_equal(W.sphere_omega(q, s)[:, 0], np.array([W.FOUR_PI, 0, 0], F))      # inside; ON the sphere: len < r is false; outside
    assert float(W.result(W.quant(W.FOUR_PI))) == 1.0


def test_the_integer_sum_is_the_same_under_every_order():
    r = np.random.RandomState(5)
    tris = r.uniform(-1, 1, (7, 3, 3))
    q = r.uniform(-1, 1, (3, 3)).astype(F)
    I = W.quant(W.triangle_omega(q, tris))                       # [3, 7]
    perms = np.array(list(itertools.permutations(range(7))))     # 5040 orders
    running = np.zeros((perms.shape[0], 3), np.int64)
    for k in range(7):
        running += I[:, perms[:, k]].T
    assert (running == I.sum(axis=1)[None, :]).all()
    # ... which a float32 sum of the same terms does not manage
    om = W.triangle_omega(q, tris)
    fsum = np.zeros((perms.shape[0], 3), F)
    for k in range(7):
        fsum += om[:, perms[:, k]].T
    assert len({x.tobytes() for x in fsum}) > 1


# ---- the hand-built tree ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tori():
    """the closed torus of 2 000 triangles and the one with a window removed: triangles, tree, table, 600 queries, their exact sums and float64 answers"""
    closed = W.torus_triangles()
    out = {}
    r = np.random.RandomState(11)
    pts = r.uniform(-1.6, 1.6, (600, 3)).astype(F)
    pts[:, 2] *= F(0.4)
    for name, tris in (("closed", closed), ("open", closed[W.torus_hole()])):
        tree = W.Tree(W.build_tree(tris))
        table, sums = W.moment_table(tree)
        out[name] = dict(tris=tris, tree=tree, table=table, sums=sums, pts=pts, exact=W.exact_sum(pts, tris), w64=W.exact_float64(pts, tris))
    return out


@pytest.mark.parametrize("name", ["closed", "open"])
def test_walk_without_approximation_is_the_exact_sum(tori, name):
    c = tori[name]
    S_inf, counts = W.walk(c["tree"], c["table"], c["pts"], np.inf)
    assert np.array_equal(S_inf, c["exact"])
    assert (counts[:, 1] == c["tris"].shape[0]).all() and (counts[:, 0] == 4 * c["tree"].nodes).all()
    assert np.abs(W.result(c["exact"]).astype(D) - c["w64"]).max() <= term_tolerance(c["tris"].shape[0])


@pytest.mark.parametrize("name", ["closed", "open"])
def test_error_shrinks_with_beta(tori, name):
    c = tori[name]
    worst, mean, leaves = [], [], []
    for beta in (1.5, 2.0, 3.0, 4.0):
        Sb, counts = W.walk(c["tree"], c["table"], c["pts"], beta)
        err = np.abs(W.result(Sb).astype(D) - c["w64"])
        worst.append(err.max()); mean.append(err.mean()); leaves.append(counts[:, 1].mean())
    print(name, "max", worst, "mean", mean, "leaves per query", leaves)
    assert all(a > b for a, b in zip(worst, worst[1:])) and all(a > b for a, b in zip(mean, mean[1:]))
    assert all(a < b for a, b in zip(leaves, leaves[1:])) and leaves[-1] < 0.25 * c["tris"].shape[0]
    assert worst[1] < 0.1 and mean[1] < 0.02                     # beta = 2: nowhere near a lost cluster (a node-sized term is of the order of 1)


def test_moment_rows_of_the_hand_built_tree(tori):
    """what the rows must be whatever the tree: the root's children sum to the whole mesh -- a closed one has no net area vector --, p~ lies in its
    slot's box, r2 reaches the box's farthest corner, rows of slots that name no inner node are zero"""
    c = tori["closed"]
    tree, table, sums = c["tree"], c["table"], c["sums"]
    inv2 = 2.0 ** (2 * tree.e - 37)
    area = sums[0, 3] * inv2
    assert abs(area - 4 * np.pi ** 2 * 1.0 * 0.4) < 0.02 * area                    # the torus' area, 4 pi^2 R r, less the faceting
    assert (np.abs(sums[0, 0:3] * inv2) < 1e-6 * area).all()
    inner = (tree.codes >= 0)
    assert (table[~inner] == 0).all() and inner.sum() == tree.nodes - 1
    p, r2 = table[..., 0:3][inner], table[..., 3][inner]
    mn, mx = tree.box_min[inner], tree.box_max[inner]
    assert ((p >= mn) & (p <= mx)).all()
    far = np.maximum(np.abs(p.astype(D) - mn), np.abs(mx - p.astype(D)))
    assert np.allclose(r2, (far ** 2).sum(axis=1), rtol=1e-5)


# ---- the case the feature exists for ---------------------------------------------------------------------------------------------------------------
def hole_points():
    """(points [235, 3] float32, inside [235] bool) in front of the open torus' window: of HOLE_CANDIDATES points drawn with HOLE_SEED those whose
    pseudo-normal sign (restated: signed_distance_expected.py) disagrees with the float64 winding number's > 0.5 by a margin of 0.2"""
    tris = W.torus_triangles()[W.torus_hole()]
    r = np.random.RandomState(HOLE_SEED)
    ang, rad, z = r.uniform(0.1, np.pi / 2 - 0.1, HOLE_CANDIDATES), r.uniform(1.0, 2.4, HOLE_CANDIDATES), r.uniform(-0.35, 0.35, HOLE_CANDIDATES)
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang), z], axis=1).astype(F)
    geom = E.Geometry(tris, np.arange(tris.shape[0]))
    sd = SE.signed_distance(pts, geom, SE.table(geom, tris.shape[0]))[0]
    w64 = W.exact_float64(pts, tris)
    wrong = ((sd < 0) != (w64 > 0.5)) & (np.abs(w64 - 0.5) > 0.2)
    return pts[wrong], (w64 > 0.5)[wrong], (sd < 0)[wrong]


def test_behind_the_hole_the_pseudo_normal_is_wrong_and_the_winding_number_right(tori):
    pts, truth, pseudo = hole_points()
    print("hole points: %d of %d candidates" % (pts.shape[0], HOLE_CANDIDATES))
    assert pts.shape[0] == HOLE_POINTS >= 20
    assert (pseudo != truth).all() and pseudo.all()              # every one of them: outside, seen as inside through the window
    c = tori["open"]
    for beta in (2.0, np.inf):
        w = W.result(W.walk(c["tree"], c["table"], pts, beta)[0])
        assert np.array_equal(w > 0.5, truth), beta


# ---- the term code compiled for the host -------------------------------------------------------------------------------------------------------------
def kat_rows(n=4000, seed=3):
    """triangle rows (q, A, B, C): random ones, then coincident, on-plane, degenerate, denormal and huge inputs; and sphere rows (q, centre, r)"""
    r = np.random.RandomState(seed)
    rows = r.uniform(-2, 2, (n, 12)).astype(F)
    rows[100:200, 0:3] = rows[100:200, 3:6]                      # q at a corner
    rows[200:300, 0:3] = (rows[200:300, 3:6] + rows[200:300, 6:9]) * F(0.5)      # q on an edge
    rows[300:400, [2, 5, 8, 11]] = 0                             # everything in the plane z = 0
    rows[400:450, 9:12] = rows[400:450, 6:9]                     # two corners coincide: invalid
    rows[450:500] *= F(1.0e-40)                                  # denormal
    rows[500:550] *= F(1.0e-20)
    rows[550:600] *= F(1.0e18)
    rows[600:650] *= F(1.0e30)                                   # products overflow
    rows[650:660, 0] = np.nan
    rows[660:670, 4] = np.inf
    sph = r.uniform(-2, 2, (n // 4, 7)).astype(F)
    sph[:, 6] = np.abs(sph[:, 6])
    sph[:50, 0:3] = sph[:50, 3:6]; sph[50:60, 6] = np.nan; sph[60:70, 6] = np.inf; sph[70:80] *= F(1e30)
    return rows, sph


def kat_expected(rows, is_sphere):
    """(omega, w, I) of the restatement, row by row"""
    q = rows[:, 0:3]
    if is_sphere:
        om = np.array([W.sphere_omega(q[i:i + 1], rows[i:i + 1, 3:7])[0, 0] for i in range(rows.shape[0])], F)
    else:
        om = W.triangle_omega_rows(q, rows[:, 3:12])
    I = W.quant(om)
    return om, W.result(I), I


def assert_kat(got, want, what):
    om, w, I = got
    bad = np.nonzero(I != want[2])[0]
    assert bad.size == 0, (what, "I", bad[:8], I[bad[:8]], want[2][bad[:8]])
    assert np.array_equal(w.view(np.uint32), want[1].view(np.uint32)), (what, "w")
    assert np.array_equal(W.quant(om), I), (what, "I(omega)")
    assert ((om.view(np.uint32) == want[0].view(np.uint32)) | (np.isnan(om) & np.isnan(want[0]))).all(), (what, "omega")


def test_library_host_entry_is_the_restatement():
    rows, sph = kat_rows()
    assert_kat(_native.kat_winding_host(rows), kat_expected(rows, False), "triangles")
    assert_kat(_native.kat_winding_host(sph, True), kat_expected(sph, True), "spheres")
    om = _native.kat_winding_host(rows)[0]
    assert (np.abs(om[np.isfinite(om)]) <= F(2.0) * F(np.pi)).all() and np.isfinite(om[:600]).all()


def test_term_header_stand_alone_under_sanitizers(tmp_path):
    """csrc/tirt_winding.h in a program of its own (tests/winding_term_main.hip: exactly-sized heap arrays, rows from a file) with the host code under
    AddressSanitizer and UndefinedBehaviorSanitizer; the program is run directly and its output compared with numpy"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "winding_term_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "ti_raytrace_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "winding_term_main.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, sph = kat_rows()
    for name, data, is_sphere in (("tri", rows, False), ("sph", sph, True)):
        src, dst = str(tmp_path / (name + ".f32")), str(tmp_path / (name + ".u32"))
        data.tofile(src)
        r = subprocess.run([exe, src, dst, "1" if is_sphere else "0"], capture_output=True, text=True)
        assert r.returncode == 0 and "%d rows" % data.shape[0] in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        out = np.fromfile(dst, np.uint32).reshape(-1, 4)
        assert_kat(_native._kat_winding_out(out), kat_expected(data, is_sphere), name)
