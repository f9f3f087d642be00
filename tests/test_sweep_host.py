"""The sphere-sweep definition (include/tirt.h, "Sphere sweep") without a device: the library's own text compiled for the host (tirt_kat_sweep_host)
against the numpy restatement on every bit, known answers with exactly representable numbers, the tunnelling case a stepped closest-point query
misses, the order rules, the definition's rounding against a float64 evaluation, and SweepQuery's refusals that never reach a device."""
import itertools
import sys

import numpy as np
import pytest

import closest_point_expected as CP
import sweep_expected as SE
from ti_raytrace_amd import _native

F = np.float32
INF = F(np.inf)
M = F(2.0 ** -17)                    # a query length for rows without a scene: about half a cell of a unit scene


def host(rows, is_sphere=False):
    return _native.kat_sweep_host(rows, is_sphere)


def same_rows(got, want):
    return np.array_equal(np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32))


def one(o, d, r, a, b, c, B=np.inf, m=M):
    out = host(SE.tri_rows(o, d, r, m, B, a, b, c))[0]
    return float(out[0]), int(out[1]), out[2:5], out[5:7], float(out[7])


# ---- 1. the host text equals the float32 restatement on every bit ---------------------------------------------------------------------------
def _random_queries(rs, n):
    o = rs.uniform(-0.5, 1.5, (n, 3)).astype(F)
    p1 = rs.uniform(-0.5, 1.5, (n, 3)).astype(F)
    r = rs.choice(np.array([0.0, 0.01, 0.05, 0.3], F), n)
    B = rs.choice(np.array([np.inf, 1.0, 0.5, 0.0], F), n)
    return o, (p1 - o).astype(F), r, B


def test_host_text_equals_the_restatement_on_triangle_rows():
    rs = np.random.RandomState(20261021)
    n = 6000
    o, d, r, B = _random_queries(rs, n)
    a = rs.uniform(0.0, 1.0, (n, 3)).astype(F)
    b = (a + rs.uniform(-0.4, 0.4, (n, 3))).astype(F)
    c = (a + rs.uniform(-0.4, 0.4, (n, 3))).astype(F)
    k = np.arange(n)
    b[k % 17 == 0] = a[k % 17 == 0]                                        # an edge of length 0
    c[k % 19 == 0] = (a + (b - a) * F(2.0))[k % 19 == 0]                   # collinear corners
    c[k % 23 == 0] = b[k % 23 == 0] = a[k % 23 == 0]                       # a point
    d[k % 11 == 0] = 0.0                                                   # a sphere that stands still
    d[k % 13 == 0] = ((b - a) * F(0.75))[k % 13 == 0]                      # parallel to the edge ab
    d[k % 29 == 0] = ((a - c) * F(-1.5))[k % 29 == 0]                      # ... and to ca
    o[k % 31 == 0] = (a + F(0.001))[k % 31 == 0]                           # a start in overlap, next to a corner
    rows = SE.tri_rows(o, d, r, M, B, a, b, c)
    for j, (col, val) in enumerate([(0, np.nan), (1, np.inf), (4, np.nan), (5, -np.inf), (6, np.nan), (6, np.inf), (6, -0.5), (8, np.nan), (8, -1.0), (7, 0.25)]):
        rows[j * 7 + 3::97, col] = val                                     # non-finite o and d, a bad radius, a bad bound; a large m is legal
    got, want = host(rows), SE.kat_expected(rows)
    assert got.dtype == F and want.dtype == F
    codes = np.bincount(got[:, 1].astype(int) + 1, minlength=9)
    print("codes -1 .. 7:", codes)
    assert (codes[:9] > 0).all(), codes                                    # a miss and every one of the eight codes occur
    bad = np.nonzero(~(got.view(np.uint32) == want.view(np.uint32)).all(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    invalid = ~SE.valid(rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 8])
    assert invalid.sum() > 300 and same_rows(got[invalid], np.tile(np.array([np.inf, -1, 0, 0, 0, 0, 0, 0], F), (invalid.sum(), 1)))


def test_host_text_equals_the_restatement_on_sphere_rows():
    rs = np.random.RandomState(20261022)
    n = 4000
    o, d, r, B = _random_queries(rs, n)
    C = rs.uniform(0.0, 1.0, (n, 3)).astype(F)
    R = rs.choice(np.array([0.0, 0.02, 0.2, 0.7, 2.0], F), n)
    k = np.arange(n)
    d[k % 11 == 0] = 0.0
    o[k % 13 == 0] = C[k % 13 == 0]                                        # a start at the centre
    rows = SE.sphere_rows(o, d, r, M, B, C, R)
    for j, (col, val) in enumerate([(2, np.nan), (3, np.inf), (6, np.nan), (6, -1.0), (8, np.nan), (8, -0.0), (12, np.nan)]):
        rows[j * 5 + 2::89, col] = val
    got, want = host(rows, True), SE.kat_expected(rows, True)
    codes = np.bincount(got[:, 1].astype(int) + 1, minlength=11)
    print("codes -1 .. 9:", codes)
    assert codes[0] > 0 and codes[1] > 0 and codes[9] > 0 and codes[10] > 0 and codes[2:9].sum() == 0, codes
    bad = np.nonzero(~(got.view(np.uint32) == want.view(np.uint32)).all(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


# ---- 2. known answers: every number below is exact in fp32 -----------------------------------------------------------------------------------
FLOOR = ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))


def test_drop_onto_the_face():
    t, code, q, uv, d2 = one((1.0, 1.0, 3.0), (0.0, 0.0, -2.0), 0.5, *FLOOR)
    assert (t, code) == (1.25, 1) and list(q) == [1.0, 1.0, 0.0] and list(uv) == [0.25, 0.25] and d2 == 0.25       # T = (h - r) / |d|


def test_drop_onto_an_edge_and_onto_a_corner():
    # 3-4-5: the centre stops 0.5 above the floor's plane, 0.375 outside the edge ab, 0.625 from it
    t, code, q, uv, d2 = one((2.0, -0.375, 3.0), (0.0, 0.0, -1.0), 0.625, *FLOOR)
    assert (t, code) == (2.5, 2) and list(q) == [2.0, 0.0, 0.0] and list(uv) == [0.5, 0.0] and d2 == 0.390625
    # 1-2-2-3: 0.25 above the plane, (0.125, 0.25) outside the corner a, 0.375 from it
    t, code, q, uv, d2 = one((-0.125, -0.25, 3.0), (0.0, 0.0, -1.0), 0.375, *FLOOR)
    assert (t, code) == (2.75, 5) and list(q) == [0.0, 0.0, 0.0] and list(uv) == [0.0, 0.0] and d2 == 0.140625
    # the same drops with the corners renamed reach the other edge and corner codes
    a, b, c = FLOOR
    assert one((2.0, -0.375, 3.0), (0.0, 0.0, -1.0), 0.625, c, a, b)[:2] == (2.5, 3)
    assert one((2.0, -0.375, 3.0), (0.0, 0.0, -1.0), 0.625, b, c, a)[:2] == (2.5, 4)
    assert one((-0.125, -0.25, 3.0), (0.0, 0.0, -1.0), 0.375, c, a, b)[:2] == (2.75, 6)
    assert one((-0.125, -0.25, 3.0), (0.0, 0.0, -1.0), 0.375, b, c, a)[:2] == (2.75, 7)


def test_overlap_touching_and_moving_away():
    assert one((1.0, 1.0, 0.25), (0.0, 0.0, -1.0), 0.5, *FLOOR)[:2] == (0.0, 0)             # a start in overlap
    assert one((1.0, 1.0, 0.25), (0.0, 0.0, 0.0), 0.5, *FLOOR)[:2] == (0.0, 0)              # ... also for a sphere that stands still
    t, code, q, uv, d2 = one((1.0, 1.0, 0.5), (0.0, 0.0, 1.0), 0.5, *FLOOR)                 # touching and moving away: touching is contact
    assert (t, code, d2) == (0.0, 0, 0.25) and list(q) == [1.0, 1.0, 0.0]
    assert one((1.0, 1.0, 0.75), (0.0, 0.0, 1.0), 0.5, *FLOOR)[:2] == (np.inf, -1)          # clear of it and moving away
    assert one((1.0, 1.0, 0.75), (0.0, 0.0, 0.0), 0.5, *FLOOR)[:2] == (np.inf, -1)          # clear of it and standing still
    assert one((1.0, 1.0, 3.0), (0.0, 0.0, -2.0), 0.5, *FLOOR, B=1.0)[:2] == (np.inf, -1)   # the contact at 1.25 lies behind the bound
    assert one((1.0, 1.0, 3.0), (0.0, 0.0, -2.0), 0.5, *FLOOR, B=1.25)[:2] == (1.25, 1)     # ... and on it


def test_a_root_of_exactly_zero_is_ahead_not_overlap():
    """T == 0 is kept for overlap by cp_triangle's own arithmetic.  The centre line (r = 0) from a point IN the floor's plane (z = 0: the plane's
    expression is exactly 0) whose cp_triangle Q is off by a rounding (D2 = 2.8e-14 > 0): the face root is 0 / |v| = 0, the contact is kept, and T is 2^-126"""
    o = np.array((0.9, 1.3, 0.0), F)
    assert CP.tri_point(o, *np.array(FLOOR, F))[0] > 0
    t, code, q, uv, d2 = one(o, (0.25, 0.5, -1.0), 0.0, *FLOOR)
    assert code == 1 and t == float(F(2.0 ** -126)) and 0 < d2 < 1e-12
    assert one(o, (0.25, 0.5, -1.0), 0.0, *FLOOR, B=0.0)[:2] == (np.inf, -1)     # ... which a bound of 0 excludes
    assert one(o, (0.25, 0.5, 1.0), 0.0, *FLOOR)[:2] == (np.inf, -1)             # moving away from it: no contact


def test_a_sphere_larger_than_the_triangle_passing_beside_it():
    small = ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0))
    assert one((-8.0, -3.0, 0.0), (1.0, 0.0, 0.0), 2.0, *small)[:2] == (np.inf, -1)         # 3 > r away at the closest
    t, code, q, uv, d2 = one((-8.0, -1.5, 0.0), (1.0, 0.0, 0.0), 2.0, *small)               # 1.5 < r: the corner a is met first, before x = 0
    assert code == 5 and list(q) == [0.0, 0.0, 0.0]
    assert abs(t - (8.0 - np.sqrt(4.0 - 2.25))) < 1e-6


def test_analytic_sphere_from_outside_and_from_inside():
    C, R = (0.0, 0.0, 0.0), 2.0
    out = host(SE.sphere_rows((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), 0.5, M, np.inf, C, R), True)[0]
    assert list(out) == [2.5, 8.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.25]
    out = host(SE.sphere_rows((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.5, M, np.inf, C, R), True)[0]
    assert list(out) == [1.5, 9.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.25]
    out = host(SE.sphere_rows((0.0, 0.0, 1.75), (0.0, 0.0, 1.0), 0.5, M, np.inf, C, R), True)[0]      # within r of the surface: overlap
    assert list(out[:2]) == [0.0, 0.0] and out[7] == 0.0625
    out = host(SE.sphere_rows((0.0, 0.0, 5.0), (0.0, 0.0, 1.0), 0.5, M, np.inf, C, R), True)[0]       # moving away
    assert list(out) == [np.inf, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_a_zero_area_triangle_answers_as_a_capsule():
    needle = ((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (4.0, 0.0, 0.0))
    t, code, q, uv, d2 = one((1.0, 0.0, 3.0), (0.0, 0.0, -1.0), 0.5, *needle)               # onto its middle: the cylinder about ab
    assert (t, code, d2) == (2.5, 2, 0.25) and list(q) == [1.0, 0.0, 0.0]
    t, code, q, uv, d2 = one((4.375, 0.0, 3.0), (0.0, 0.0, -1.0), 0.625, *needle)           # beyond its end: the sphere about c (3-4-5 again)
    assert (t, code, d2) == (2.5, 7, 0.390625) and list(q) == [4.0, 0.0, 0.0]
    assert one((5.0, 0.0, 3.0), (0.0, 0.0, -1.0), 0.5, *needle)[:2] == (np.inf, -1)         # past the end cap


# ---- 3. tunnelling ------------------------------------------------------------------------------------------------------------------------
def test_one_step_through_a_sheet_that_stepped_sampling_misses():
    a, b, c = np.array(FLOOR, F)
    o, d, r = np.array((1.0, 1.0, 1.0), F), np.array((0.0, 0.0, -2.0), F), F(0.01)          # one step of 2 through a sheet of thickness 0, r = 0.01
    steps = (np.arange(16, dtype=F) + F(0.5)) / F(16.0)
    d2 = CP.tri_point(o[None] + d[None] * steps[:, None], a[None], b[None], c[None])[0]     # what 16 closest-point queries along the step see
    assert (d2 > r * r).all() and d2.min() > 30 * r * r                                     # clearance at every step: the nearest sample is 0.0625 away
    t, code, q, uv, v2 = one(o, d, r, a, b, c, B=1.0)
    assert code == 1 and abs(t - 0.495) < 1e-6 and list(q) == [1.0, 1.0, 0.0]


# ---- 4. candidate order and primitive order ----------------------------------------------------------------------------------------------------
def test_the_answer_does_not_depend_on_which_corner_comes_first():
    """small integers: every coefficient of every candidate's quadratic is exact, so the renamed triangle has the same T on every bit"""
    rs = np.random.RandomState(4)
    n = 3000
    tri = rs.randint(-4, 5, (n, 3, 3)).astype(F)
    o = rs.randint(-8, 9, (n, 3)).astype(F)
    d = rs.randint(-3, 4, (n, 3)).astype(F)
    r = rs.choice(np.array([0.5, 1.0, 2.0], F), n)
    base = host(SE.tri_rows(o, d, r, M, np.inf, tri[:, 0], tri[:, 1], tri[:, 2]))
    assert (np.bincount(base[:, 1].astype(int) + 1, minlength=9) > 0).all()
    edge = {(0, 1): 2, (1, 2): 3, (2, 0): 4}
    for perm in itertools.permutations(range(3)):
        got = host(SE.tri_rows(o, d, r, M, np.inf, tri[:, perm[0]], tri[:, perm[1]], tri[:, perm[2]]))
        assert same_rows(got[:, 0], base[:, 0]), perm                       # T
        # the code permutes: new corner j is old corner perm[j], new edge (j, j + 1) is the old edge between perm[j] and perm[j + 1]
        want = base[:, 1].copy()
        for j in range(3):
            want[got[:, 1] == 5 + j] = 5 + perm[j]
            e = (perm[j], perm[(j + 1) % 3])
            want[got[:, 1] == 2 + j] = edge.get(e, edge.get((e[1], e[0])))
        want[got[:, 1] <= 1] = got[got[:, 1] <= 1, 1]
        # a contact at the same T on two features (a sphere that meets an edge at its end meets the corner too) goes to the first in code order,
        # which renaming changes: those rows are told apart by their contact point, which must still be the same
        differ = want != base[:, 1]
        assert differ.mean() < 0.02, (perm, differ.mean())
        assert np.abs(got[:, 2:5] - base[:, 2:5]).max() <= 1e-5, perm


def test_the_smaller_primitive_id_wins_an_exact_tie():
    tri = np.array(FLOOR, F)
    geom = CP.Geometry(np.stack([tri, tri, tri + F(8.0)]), np.array([5, 2, 1]))
    rays = np.array([[1.0, 1.0, 3.0, 0.0, 0.0, -2.0], [9.0, 9.0, 11.0, 0.0, 0.0, -2.0]], F)
    out = SE.brute_force(rays, 0.5, None, geom, None, None, m=M)
    assert list(out["prim"]) == [2, 1] and list(out["t"]) == [1.25, 1.25] and list(out["code"]) == [1, 1]
    assert np.array_equal(out["normal"], np.array([[0, 0, 1], [0, 0, 1]], F)) and np.array_equal(out["uv"], np.full((2, 2), 0.25, F))
    out = SE.brute_force(rays, 0.5, 1.0, geom, None, None, m=M)             # behind the bound: the distance family's miss
    assert list(out["prim"]) == [-1, -1] and np.isinf(out["t"]).all() and list(out["code"]) == [-1, -1] and not out["normal"].any()


# ---- 5. accuracy against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_accuracy_against_float64(which):
    """The float32 host text against the float64 evaluation of the same definition (tests/sweep_expected.py) on the two sets of profiles/sweep_accuracy.txt.
    Measured there: dense (64 triangles, r = 0.05): 0.93 % of 1500 segments left out as grazing, 833 contacts, max |T32 - T64| |d| = 1.7831e-05, no
    disagreement; sparse (12 triangles, r = 0.02): 0.07 % left out, 115 contacts, max 1.5674e-05, no disagreement.  The bound is twice the measured maximum."""
    m = SE.accuracy_measure(which, _native.kat_sweep_host)
    print(which, m)
    assert m["left_out"] <= 0.05
    assert m["disagree"] == 0
    assert m["contacts"] > 100
    assert m["max_err"] <= 2.0 * SE.ACCURACY_SETS[which]["measured"]


# ---- 6. SweepQuery's refusals that need no device, and the host entry point's -------------------------------------------------------------------
def _query():
    pytest.importorskip("torch")
    from ti_raytrace_amd import SweepQuery, scenes
    ex = scenes.cornell_box(16, 16, 1, device_id=0)
    assert ex.scene._ctx is None
    return SweepQuery(ex.scene), ex.scene


def test_sweep_query_refuses_bad_arguments_without_a_context():
    q, sc = _query()
    import torch
    rays = torch.zeros((10, 6), dtype=torch.float32)
    for call, name in ((q.cast, "cast"), (q.blocked, "blocked"), (q.cast_counts, "cast_counts")):
        with pytest.raises(TypeError, match=r"SweepQuery\.%s: rays must be on the GPU" % name):
            call(rays, 0.5)
        with pytest.raises(TypeError, match=r"%s: rays must be float32" % name):
            call(rays.double(), 0.5)
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(np.zeros((10, 6), np.float32), 0.5)
        with pytest.raises(ValueError, match="N, C >= 6"):
            call(torch.zeros((10, 5)), 0.5)
        with pytest.raises(ValueError, match="N, C >= 6"):
            call(torch.zeros(60), 0.5)
        with pytest.raises(ValueError, match="stride 1"):
            call(torch.zeros((10, 12))[:, ::2], 0.5)
        with pytest.raises(ValueError, match="overlap"):
            call(torch.zeros(64).as_strided((10, 6), (3, 1)), 0.5)
        with pytest.raises(ValueError, match=r"radius must be \[N\] = \[10\]"):
            call(rays, torch.zeros(9))
        with pytest.raises(ValueError, match=r"radius must be \[N\]"):
            call(rays, torch.zeros((10, 1)))
        with pytest.raises(TypeError, match="radius must be float32"):
            call(rays, torch.zeros(10, dtype=torch.float64))
        with pytest.raises(TypeError, match="radius must be a float or a float32 tensor"):
            call(rays, None)
        with pytest.raises(TypeError, match="radius must be a float"):
            call(rays, "0.5")
        with pytest.raises(ValueError, match=r"tmax must be \[N\] = \[10\]"):
            call(rays, 0.5, torch.zeros(11))
        with pytest.raises(TypeError, match="tmax must be None, a float or a float32 tensor"):
            call(rays, 0.5, [1.0])
        with pytest.raises(ValueError, match="positive stride"):
            call(rays, 0.5, torch.zeros(1).expand(10))
    assert sc._ctx is None                                                  # nothing above made a context


def test_sweep_query_constructor_arguments():
    q, sc = _query()
    from ti_raytrace_amd import SweepQuery, SweepHits
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="stack_size"):
            SweepQuery(sc, stack_size=bad)
    with pytest.raises(ValueError, match="flags"):
        SweepQuery(sc, flags=4)
    assert SweepQuery(sc, 128, _native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES).stack_size == 128
    assert SweepHits._fields == ("t", "prim", "code", "point", "uv", "normal")
    assert sc._ctx is None


def test_sweep_query_without_torch(monkeypatch):
    q, sc = _query()
    from ti_raytrace_amd import SweepQuery
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError, match="needs PyTorch"):
        SweepQuery(sc)


def test_the_host_entry_points_refusals():
    lib = _native.lib()
    rows, out = np.zeros(18, F), np.zeros(8, F)
    assert lib.tirt_kat_sweep_host(rows, -1, 0, out) != 0 and b"negative n" in lib.tirt_last_error()
    assert lib.tirt_kat_sweep_host(rows, 1, 2, out) != 0 and b"is_sphere" in lib.tirt_last_error()
    assert lib.tirt_kat_sweep_host(rows, 0, 0, out) == 0
    # the entry points that need a context refuse a null one before they touch a device
    assert lib.tirt_kat_sweep(None, rows, 1, 0, out) != 0 and b"null context" in lib.tirt_last_error()
    assert lib.tirt_kat_sweep(None, rows, 1, 3, out) != 0 and b"is_sphere" in lib.tirt_last_error()
    assert lib.tirt_sweep(None, rows, 1, None, 0.5, None, 64, 0, None, None, None, None, None, None, None, None) != 0 and b"null context" in lib.tirt_last_error()
    assert lib.tirt_query_sweep(None, None, 1, 6, None, 1, 0.5, None, 1, np.inf, 64, 0, None, None, None, None, 3, None, 2, None, 3, None, None, None) != 0
    assert b"null context" in lib.tirt_last_error()
    with pytest.raises(_native.TirtError, match="is_sphere|null"):
        _native.check(lib.tirt_kat_sweep_host(rows, 1, 7, out))
