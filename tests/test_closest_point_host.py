"""The closest-point definition (include/tirt.h, "Closest point") as tests/closest_point_expected.py restates it, without a device: its own rounding
against a float64 evaluation of the same expressions, one hand-placed point per region, exact zeros at the vertices, the tie rule, the bound, and
PointQuery's argument refusals that never reach the library."""
import itertools
import sys

import numpy as np
import pytest

import closest_point_expected as E

F = np.float32
A_, B_, C_, HAND, hand_rows = E.A_, E.B_, E.C_, E.HAND, E.hand_rows


def random_pairs():
    return np.random.RandomState(20261019).uniform(0.0, 1.0, (4096, 4, 3)).astype(F)


# 4 x the largest relative deviation of D2 observed on random_pairs() (the issue's rule for this tolerance): see the test's docstring
TOL_UNIT, TOL_FAR = 4 * 2.0117219191108773e-05, 4 * 0.04980926309426518


def test_restatement_against_float64():
    """The float32 restatement against the same expressions in float64 on 4096 random point / triangle pairs in the unit cube, and on the same pairs
    moved 1000 extents away (p and the triangle both: coordinates ~1000, distances ~1; the float64 run starts from the moved float32 numbers).
    Largest relative deviation of D2 observed: 2.0117e-05 in the unit cube (the pair with the smallest D2, 1.6e-06; the median is 6.2e-08), 4.9809e-02
    at 1000 extents (median 5.4e-05; Q is off by up to 5.8e-05 there, one ulp of 1000, against distances down to 1e-3).  This is the definition's own
    rounding, measured against float64 and not against the device; the tolerances are 4 x these.  No pair changes its region."""
    X = random_pairs()
    for shift, tol in ((0.0, TOL_UNIT), (1000.0, TOL_FAR)):
        Y = (X + F(shift)).astype(F)
        Z = Y.astype(np.float64)
        d32, q32, u32, v32 = E.tri_point(Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3])
        d64, q64, u64, v64 = E.tri_point(Z[:, 0], Z[:, 1], Z[:, 2], Z[:, 3])
        assert d32.dtype == F and q32.dtype == F and u32.dtype == F
        rel = np.abs(d32.astype(np.float64) - d64) / d64
        print("shift %g: largest relative deviation of D2 %.4e, median %.4e" % (shift, rel.max(), np.median(rel)))
        assert rel.max() <= tol, (shift, rel.max())
        assert np.array_equal(E.region(Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3]), E.region(Z[:, 0], Z[:, 1], Z[:, 2], Z[:, 3]))
        assert np.bincount(E.region(Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3]), minlength=7).min() > 100          # every region is well populated


def test_one_hand_placed_point_per_region():
    rows, want = hand_rows()
    d2, q, u, v = E.tri_point(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])
    assert list(E.region(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])) == [0, 1, 2, 3, 4, 5, 6]
    got = np.concatenate([d2[:, None], q, u[:, None], v[:, None]], axis=1)
    assert got.dtype == F
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


def test_a_query_at_a_vertex_is_at_distance_zero():
    r = np.random.RandomState(5)
    tris = r.uniform(-3.0, 3.0, (200, 3, 3)).astype(F)
    expect_uv = {0: (0.0, 0.0), 1: (1.0, 0.0), 2: (0.0, 1.0)}
    for order in itertools.permutations(range(3)):
        t = tris[:, list(order), :]
        for k in range(3):
            d2, q, u, v = E.tri_point(t[:, k], t[:, 0], t[:, 1], t[:, 2])
            assert np.array_equal(d2.view(np.uint32), np.zeros(200, np.uint32)), (order, k)      # +0, exactly
            assert np.array_equal(q, t[:, k]) and (u == expect_uv[k][0]).all() and (v == expect_uv[k][1]).all()


def test_ties_go_to_the_smallest_primitive_id():
    r = np.random.RandomState(6)
    one = r.uniform(-1.0, 1.0, (3, 3))
    other = one + 5.0
    g = E.Geometry(np.stack([one, other, one, one]), [7, 1, 3, 9])
    p = r.uniform(-2.0, 2.0, (64, 3)).astype(F)
    d2, prim, q, uv = E.brute_force(p, g)
    assert (prim == 3).all()
    alone = E.brute_force(p, E.Geometry(one[None], [0]))
    assert np.array_equal(d2.view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(q, alone[2]) and np.array_equal(uv, alone[3])


def test_bound_and_nothing_found():
    g = E.Geometry(np.array([A_, B_, C_])[None], [0], [[0.0, 0.0, 10.0, 1.0]], [1])
    p = np.array([[0.5, 0.5, 3.0]] * 8 + [[np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0]], F)
    dmax = np.array([np.inf, 3.0, np.nextafter(F(3.0), F(0.0)), 0.0, -1.0, np.nan, 1e30, 2.9] + [np.inf] * 3, F)
    d2, prim, q, uv = E.brute_force(p, g, dmax)
    assert list(prim) == [0, 0, -1, -1, -1, -1, 0, -1, -1, -1, -1]
    assert (d2[prim == 0] == 9.0).all() and np.isposinf(d2[prim < 0]).all() and (q[prim < 0] == 0).all() and (uv[prim < 0] == 0).all()
    # the sphere: outside, inside, on it, at its centre
    ps = np.array([[0.0, 0.0, 13.0], [0.0, 0.0, 10.5], [1.0, 0.0, 10.0], [0.0, 0.0, 10.0]], F)
    d2, prim, q, uv = E.brute_force(ps, E.Geometry(np.zeros((0, 3, 3)), [], [[0.0, 0.0, 10.0, 1.0]], [4]))
    assert list(prim) == [4, 4, 4, 4] and list(d2) == [4.0, 0.25, 0.0, 1.0]
    assert np.array_equal(q, np.array([[0, 0, 11], [0, 0, 11], [1, 0, 10], [1, 0, 10]], F)) and (uv == 0).all()


# ---- PointQuery's refusals that need no device -------------------------------------------------------------------------------------------
def _query():
    pytest.importorskip("torch")
    from ti_raytrace_amd import PointQuery, scenes
    ex = scenes.cornell_box(16, 16, 1, device_id=0)
    assert ex.scene._ctx is None
    return PointQuery(ex.scene), ex.scene


def test_point_query_refuses_bad_arguments_without_a_context():
    q, sc = _query()
    import torch
    pts = torch.zeros((10, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU"):
        q.closest(pts)
    with pytest.raises(TypeError, match="GPU"):
        q.closest_counts(pts, 1.0)
    with pytest.raises(TypeError, match="float32"):
        q.closest(pts.double())
    with pytest.raises(TypeError, match="torch.Tensor"):
        q.closest(np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError, match="N, C >= 3"):
        q.closest(pts[:, :2])
    with pytest.raises(ValueError, match="N, C >= 3"):
        q.closest(pts[0])
    with pytest.raises(ValueError, match="stride 1"):
        q.closest(torch.zeros((3, 40))[:, ::4].t())         # [10, 3] with strides (4, 40)
    with pytest.raises(ValueError, match="overlap"):
        q.closest(torch.zeros(30).as_strided((10, 3), (1, 1)))
    assert sc._ctx is None


def test_point_query_constructor_arguments():
    q, sc = _query()
    from ti_raytrace_amd import PointQuery, PointHits, _native
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="stack_size"):
            PointQuery(sc, stack_size=bad)
    with pytest.raises(ValueError, match="flags"):
        PointQuery(sc, flags=4)
    assert PointQuery(sc, 128, _native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES).stack_size == 128
    assert PointHits._fields == ("dist2", "prim", "point", "uv")
    assert sc._ctx is None


def test_point_query_without_torch(monkeypatch):
    q, sc = _query()
    from ti_raytrace_amd import PointQuery
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError, match="needs PyTorch"):
        PointQuery(sc)
