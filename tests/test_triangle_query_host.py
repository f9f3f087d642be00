"""The triangle-distance definition (include/tirt.h, "Triangle distance") without a GPU: tirt_kat_tri_tri_host -- csrc/tirt_triangle_query.h compiled for
the host, the text the kernels run -- against the numpy restatement tests/triangle_query_expected.py on bits; known answers; the restatement against
geometry in float64; the tie rules."""
import itertools

import numpy as np
import pytest

import closest_point_expected as CE
import triangle_query_cases as cases
import triangle_query_expected as E
from common import same_bits as same
from ti_raytrace_amd import _native

F = np.float32
EPS = 2.0 ** -24


def pair_host(T, S):
    """one pair through the host entry -> d2, P, Q, code"""
    o = _native.kat_tri_tri_host(np.concatenate([np.asarray(T, F).reshape(-1), np.asarray(S, F).reshape(-1)])[None], 0)[0]
    return o[0], o[1:4], o[4:7], int(o[7])


# ---- 1. the host twin equals the restatement, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [0, 1, 2])
def test_host_equals_numpy(what):
    rows = cases.ROWS[what]()
    assert rows.shape[0] >= 3000
    got, want = _native.kat_tri_tri_host(rows, what), E.kat_rows(rows, what)
    bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
    assert bad.size == 0, (what, bad[:8], rows[bad[:2]], got[bad[:2]], want[bad[:2]])
    assert same(got, want)
    if what == 0:
        codes = np.bincount(got[:, 7].astype(np.int64) + 1, minlength=22)
        assert (codes[1:] > 0).all(), codes                  # every one of the 21 codes answers somewhere
        assert (got[got[:, 7] >= 15, 0] == 0).all()          # a piercing is distance zero
    if what == 1:
        s, t = got[:, 0], got[:, 1]
        ok = ~np.isnan(got).any(axis=1)
        assert ((s[ok] >= 0) & (s[ok] <= 1) & (t[ok] >= 0) & (t[ok] <= 1)).all()      # what the cull argument needs of the parameters
        d1, d2v = rows[:, 3:6] - rows[:, 0:3], rows[:, 9:12] - rows[:, 6:9]
        A, Ev = E.dot(d1, d1), E.dot(d2v, d2v)
        with np.errstate(invalid="ignore"):
            B = E.dot(d1, d2v); den = A * Ev - B * B
            kinds = [(A <= 0) & (Ev <= 0), (A <= 0) & (Ev > 0), (A > 0) & (Ev <= 0), (A > 0) & (Ev > 0) & (den <= 0), (A > 0) & (Ev > 0) & (den > 0)]
        assert all(k.sum() >= 50 for k in kinds), [int(k.sum()) for k in kinds]      # every branch of the segment pair is taken
    if what == 2:
        assert 200 < (got[:, 0] == 1).sum() < rows.shape[0] - 200


def test_host_entry_refusals_and_empty():
    assert _native.kat_tri_tri_host(np.zeros((0, 18), F), 0).shape == (0, 8)
    lib = _native.lib()
    buf = np.zeros(18, F)
    assert lib.tirt_kat_tri_tri_host(buf, 1, 3, buf) == -2 and lib.tirt_kat_tri_tri_host(buf, -1, 0, buf) == -2


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    S = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], F)
    d2, P, Q, code = pair_host(S + np.array([0, 0, 1], F), S)                   # parallel, offset by 1: every point is 1 away, the first candidate answers
    assert d2 == 1.0 and code == 0 and np.array_equal(P, [0, 0, 1]) and np.array_equal(Q, [0, 0, 0])
    # crossed skew edges: T's edge p0p1 along x at z = 0, the scene's edge ab along y at z = 0.5, the triangles hanging away from each other
    T = np.array([[-1, 0, 0], [1, 0, 0], [0, 0, -3]], F)
    S = np.array([[0, -1, 0.5], [0, 1, 0.5], [0, 0, 3.5]], F)
    d2, P, Q, code = pair_host(T, S)
    assert d2 == 0.25 and code == 6 and np.array_equal(P, [0, 0, 0]) and np.array_equal(Q, [0, 0, 0.5])
    d2, P, Q, code = pair_host(T[[1, 2, 0]], S[[2, 0, 1]])                      # the same edges as e = 2, f = 1
    assert d2 == 0.25 and code == 6 + 3 * 2 + 1
    d2v, _, _, _ = E.tri_point(T, S[None, 0], S[None, 1], S[None, 2])
    assert d2v.min() >= 1.0                                                     # what a vertex-only query reports for this pair: a clearance that is not there
    # an edge through the middle of a big triangle: every vertex is far from the surface, yet it is a penetration
    big = np.array([[-10, -10, 0], [10, -10, 0], [0, 10, 0]], F)
    T = np.array([[0, 0, -1], [0, 0, 1], [0.5, 0, 3]], F)
    d2, P, Q, code = pair_host(T, big)
    assert d2 == 0.0 and 15 <= code <= 17 and code == 15 and np.array_equal(P, Q) and np.abs(P).max() <= 64 * EPS * 10
    assert E.tri_point(T, big[None, 0], big[None, 1], big[None, 2])[0].min() == 1.0
    d2, P, Q, code = pair_host(big, T)                                          # the reverse: a scene edge through the query triangle
    assert d2 == 0.0 and 18 <= code <= 20 and np.array_equal(P, Q) and np.abs(P).max() <= 64 * EPS * 10
    # an edge IN the plane of a triangle that is 80 units away (the Cornell floor under the short block's side, a query coplanar with that side): det is
    # rounding noise and u, v, t fall in range by accident -- the two points of the "hit" are a scene apart, and it is no candidate
    T = np.array([[138.87166, 80.69189, -35.427814], [64.562546, 208.86209, -283.12485], [153.75865, 130.56377, 14.195492]], F)
    floor = np.array([[290, 0, -114], [82, 0, -225], [130, 0, -65]], F)
    seg = np.concatenate([floor[1], floor[2], T.reshape(-1)])[None]
    hit, u, v, t = _native.kat_tri_tri_host(seg, 2)[0]
    assert hit == 0 and 0 <= u and 0 <= v and u + v <= 1 and 0 <= t <= 1      # (in range, and refused)
    d2, P, Q, code = pair_host(T, floor)
    assert code < 15 and 80.0 ** 2 < d2 < 90.0 ** 2 and Q[1] == 0 and P[1] > 80
    # a shared vertex, copied bits, the triangles otherwise apart
    S = np.array([[0.3, 0.1, 0.7], [1.3, 0.2, 0.9], [0.2, 1.4, 0.8]], F)
    for i in range(3):
        for j in range(3):
            T = np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5]], F)
            T[i] = S[j]
            d2, P, Q, code = pair_host(T, S)
            assert d2 == 0.0 and code == i and np.array_equal(P, S[j]) and np.array_equal(Q, S[j])      # (and the first code of those that tie at 0)


# ---- 3. the restatement against geometry, in float64 ---------------------------------------------------------------------------------------------
def bary_grid(tri, N):
    """the (N + 1)(N + 2) / 2 points a + (i / N) ab + (j / N) ac, i + j <= N, in float64"""
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    keep = i + j <= N
    u, v = i[keep] / N, j[keep] / N
    return tri[0] + u[:, None] * (tri[1] - tri[0]) + v[:, None] * (tri[2] - tri[0])


def test_restatement_against_geometry():
    """48 random pairs (a third far apart, a third near, a third with overlapping boxes: many of those cross).  With d the exact distance of the exact
    triangles: every point of a triangle with longest edge L lies in a cell of the N-grid whose edges are <= L / N, so within L / N of a grid point, hence
    d <= sampled_min <= d + (L_T + L_S) / N.  The definition's sqrt(d2) differs from d by tol: P and Q are fp32 points within k eps M per coordinate of
    their exact triangles (the head of csrc/tirt_triangle_query.h; k <= 50 per side is what the walk's margin budgets), so sqrt(d2) >= d - 2 sqrt(3) k eps M,
    and the candidate class that attains d (vertex-face, edge-edge, or a crossing) is evaluated with the same error, so sqrt(d2) <= d + 2 sqrt(3) k eps M.
    tol = 2 sqrt(3) * 50 eps M <= 175 eps M, M = the largest coordinate magnitude of the pair, eps = 2^-24.  |P - Q|^2 in float64 reproduces d2 up to the
    five roundings of dot(P - Q, P - Q): relative (1 + eps)^5 - 1 <= 6 eps (a piercing has P == Q and d2 == 0 exactly)."""
    r = np.random.RandomState(41)
    N = 48
    n_cross = 0
    for k in range(48):
        T = r.uniform(-1, 1, (3, 3)).astype(F)
        S = (r.uniform(-1, 1, (3, 3)) + (np.array([3.0, 0.5, -2.0]) if k % 3 == 0 else (np.array([0.9, 0.0, 0.3]) if k % 3 == 1 else 0.0))).astype(F)
        d2, P, Q, code = E.pair(T, S)
        assert d2.dtype == F and 0 <= code <= 20
        T64, S64, P64, Q64 = T.astype(np.float64), S.astype(np.float64), P.astype(np.float64), Q.astype(np.float64)
        M = max(np.abs(T64).max(), np.abs(S64).max())
        tol = 175 * EPS * M
        assert np.sqrt(CE.tri_point(P64, T64[0], T64[1], T64[2])[0]) <= tol, (k, "P is not on T")
        assert np.sqrt(CE.tri_point(Q64, S64[0], S64[1], S64[2])[0]) <= tol, (k, "Q is not on the scene triangle")
        pq2 = ((P64 - Q64) ** 2).sum()
        assert abs(pq2 - float(d2)) <= 6 * EPS * float(d2), (k, pq2, d2)
        gt, gs = bary_grid(T64, N), bary_grid(S64, N)
        sampled = np.sqrt(((gt[:, None, :] - gs[None, :, :]) ** 2).sum(axis=2).min())
        LT = max(np.linalg.norm(T64[a] - T64[b]) for a, b in E.EDGES)
        LS = max(np.linalg.norm(S64[a] - S64[b]) for a, b in E.EDGES)
        dist = np.sqrt(float(d2))
        assert sampled - (LT + LS) / N - tol <= dist <= sampled + tol, (k, code, dist, sampled, (LT + LS) / N)
        n_cross += int(code >= 15)
    assert n_cross >= 4


# ---- 4. the tie rules ----------------------------------------------------------------------------------------------------------------------------
def test_pair_answer_does_not_depend_on_candidate_order():
    rows = cases.pair_rows(seed=5, n=64)
    d2, P, Q = E.candidates(rows[:, 0:9].reshape(-1, 3, 3), rows[:, 9:18].reshape(-1, 3, 3))
    want = E.select(d2, P, Q)
    with np.errstate(invalid="ignore"):
        ties = ((d2 == want[0][:, None]).sum(axis=1) > 1).sum()
    assert ties > 200                                       # shared corners and edges, copies: many candidates at equal bits
    r = np.random.RandomState(6)
    for order in [np.arange(E.N_CODES)[::-1]] + [r.permutation(E.N_CODES) for _ in range(6)]:
        got = E.select(d2, P, Q, order)
        assert np.array_equal(got[3], want[3]) and all(same(g, w) for g, w in zip(got[:3], want[:3])), order
    # the first code wins at equal bits: the smallest index among the candidates that carry the answer's d2 (none where nothing stands)
    with np.errstate(invalid="ignore"):
        first = np.where((d2 == want[0][:, None]) & (want[0][:, None] < np.inf), np.arange(E.N_CODES)[None, :], 99).min(axis=1)
    assert np.array_equal(np.where(first == 99, -1, first), want[3])
    host = _native.kat_tri_tri_host(rows, 0)
    assert np.array_equal(host[:, 7].astype(np.int32), want[3])


def test_smaller_primitive_id_wins_across_primitives():
    r = np.random.RandomState(7)
    S = r.uniform(-1, 1, (4, 3, 3)).astype(F)
    T = r.uniform(-1, 1, (32, 3, 3)).astype(F) + F(0.5)
    base = E.brute_force(T, CE.Geometry(S, [0, 1, 2, 3]))
    d2_all = E.pair(T[:, None], S[None])[0]                  # [32, 4]: some queries cross two scene triangles and tie at 0 across DIFFERENT triangles too
    assert ((d2_all == base[0][:, None]).sum(axis=1) > 1).any()
    orders = [ids for ids in itertools.permutations(range(10, 18)) if ids[0] % 3 == 0][::997]      # (a sample: 8! orders are more than the point needs)
    assert len(orders) > 10
    for ids in orders:
        got = E.brute_force(T, CE.Geometry(np.concatenate([S, S]), list(ids)))      # every scene triangle twice, under two ids
        tied = np.concatenate([d2_all, d2_all], axis=1) == base[0][:, None]
        assert np.array_equal(got[1], np.where(tied, np.asarray(ids)[None, :], 99).min(axis=1)), ids
        assert same(got[0], base[0])
        col = np.asarray([list(ids).index(p) % 4 for p in got[1]])
        again = E.pair(T, S[col])                            # ... and code and points are the winner's own
        assert np.array_equal(got[2], again[3]) and same(got[3], again[1]) and same(got[4], again[2])


def test_bounds_and_non_finite_queries_in_the_restatement():
    S = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], F)
    g = CE.Geometry(S, [0])
    T = np.stack([S[0] + np.array([0, 0, 1], F), S[0] + np.array([0, 0, 1], F), S[0]])
    T[1, 2, 0] = np.nan                                      # one corner NaN: its finite corners would still answer; the definition says nothing
    d2, prim, code, P, Q = E.brute_force(T, g)
    assert list(prim) == [0, -1, 0] and np.isposinf(d2[1]) and code[1] == -1 and not P[1].any() and not Q[1].any() and d2[2] == 0
    for dmax, want in ((1.0, [0, -1, 0]), (0.999, [-1, -1, 0]), (0.0, [-1, -1, 0]), (-1.0, [-1, -1, -1]), (np.nan, [-1, -1, -1]), (np.inf, [0, -1, 0])):
        assert list(E.brute_force(T, g, dmax)[1]) == want, dmax
    assert list(E.brute_force(T, g, np.array([0.0, 5.0, -0.0], F))[1]) == [-1, -1, 0]


# ---- 5. the torch front end's checks that need no device ----------------------------------------------------------------------------------------
def test_front_end_checks_without_a_device():
    torch = pytest.importorskip("torch")
    from ti_raytrace_amd import TriangleQuery, TriangleClosest

    class NoScene:
        _ctx = None
        _device_id = 0
    with pytest.raises(ValueError, match="TriangleQuery: stack_size"):
        TriangleQuery(NoScene(), stack_size=0)
    with pytest.raises(ValueError, match="TriangleQuery: flags"):
        TriangleQuery(NoScene(), flags=4)
    q = TriangleQuery(NoScene())
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        q.closest(np.zeros((2, 3, 3), F))
    with pytest.raises(TypeError, match="float32"):
        q.closest(torch.zeros((2, 3, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[n, 3, 3\]"):
        q.closest(torch.zeros((2, 9)))
    with pytest.raises(TypeError, match="on the GPU"):
        q.collides(torch.zeros((2, 3, 3)))
    with pytest.raises(TypeError, match="faces must be int32 or int64"):
        q.closest((torch.zeros((4, 3)), torch.zeros((2, 3))))
    assert TriangleClosest._fields == ("d2", "prim", "code", "point_query", "point_scene")
