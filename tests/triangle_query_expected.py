"""The triangle-distance definition of include/tirt.h ("Triangle distance") restated in numpy, operation for operation, from the header's text: the
closest points of two segments, a segment through a triangle, the 21 candidates of a pair in code order with the first-smallest rule, and the brute-force
answer over a scene's triangles with the tie rule of "Closest point".  The arrays' dtype is the arithmetic's: float32 inputs give the definition itself
(numpy rounds every elementwise operation once and fuses nothing), float64 inputs the same expressions in double.  cp_triangle is
closest_point_expected.tri_point, as the header says."""
import numpy as np

from closest_point_expected import dot, limit2, tri_point

EDGES = ((0, 1), (1, 2), (2, 0))             # edge e of a triangle (v0, v1, v2): p0p1, p1p2, p2p0 / ab, bc, ca
N_CODES = 21


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def clamp(x):
    T = x.dtype.type
    return np.where(x < T(0), T(0), np.where(x > T(1), T(1), x))


def seg_seg(p1, q1, p2, q2):
    """[..., 3] each -> s, t, d2 [...], P, Q [..., 3]"""
    T = p1.dtype.type
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        d1, d2v, r = q1 - p1, q2 - p2, p1 - p2
        A, E, F = dot(d1, d1), dot(d2v, d2v), dot(d2v, r)
        C = dot(d1, r)
        B = dot(d1, d2v)
        den = A * E - B * B
        z = np.zeros(np.broadcast(A, E).shape, p1.dtype)
        # the general branch
        s_g = np.where(den > zero, clamp((B * F - C * E) / den), z)
        t_g = (B * s_g + F) / E
        s_lo, s_hi = clamp((-C) / A), clamp((B - C) / A)
        s_gen = np.where(t_g < zero, s_lo, np.where(t_g > one, s_hi, s_g))
        t_gen = np.where(t_g < zero, zero, np.where(t_g > one, one, t_g))
        both = (A <= zero) & (E <= zero)
        a_deg = A <= zero
        e_deg = E <= zero
        s = np.select([both, a_deg, e_deg], [z, z, s_lo], s_gen)
        t = np.select([both, a_deg, e_deg], [z, clamp(F / E), z], t_gen)
        P = p1 + d1 * s[..., None]
        Q = p2 + d2v * t[..., None]
        pq = P - Q
        return s, t, dot(pq, pq), P, Q


def seg_tri(x0, x1, a, b, c):
    """[..., 3] each -> hit (bool), u, v, t [...], X [..., 3]; u = v = t = 0 and X = 0 unless det < 0 or det > 0"""
    T = x0.dtype.type
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        d, E1, E2 = x1 - x0, b - a, c - a
        h = cross(d, E2)
        det = dot(E1, h)
        ok = (det < zero) | (det > zero)
        inv = one / det
        s = x0 - a
        u = dot(s, h) * inv
        q = cross(s, E1)
        v = dot(d, q) * inv
        t = dot(E2, q) * inv
        X = (a + E1 * u[..., None]) + E2 * v[..., None]
        w = (x0 + d * t[..., None]) - X
        mx = lambda x, y: np.where(x > y, x, y)
        m2 = mx(mx(mx(mx(dot(x0, x0), dot(x1, x1)), dot(a, a)), dot(b, b)), dot(c, c))
        hit = ok & (u >= zero) & (v >= zero) & (u + v <= one) & (t >= zero) & (t <= one) & (dot(w, w) <= m2 * T(2.0 ** -38))
        z = np.zeros(det.shape, x0.dtype)
        return hit, np.where(ok, u, z), np.where(ok, v, z), np.where(ok, t, z), np.where(ok[..., None], X, z[..., None])


def candidates(T, S):
    """T [..., 3, 3] the query triangle, S [..., 3, 3] the scene triangle (broadcastable) -> d2 [..., 21] (NaN where a piercing test is no candidate),
    P, Q [..., 21, 3], in code order"""
    shape = np.broadcast(T[..., 0, 0], S[..., 0, 0]).shape
    T = np.broadcast_to(T, shape + (3, 3)); S = np.broadcast_to(S, shape + (3, 3))
    d2s, Ps, Qs = [], [], []
    for j in range(3):                                       # 0..2
        d2, q, _, _ = tri_point(T[..., j, :], S[..., 0, :], S[..., 1, :], S[..., 2, :])
        d2s.append(d2); Ps.append(T[..., j, :]); Qs.append(q)
    for j in range(3):                                       # 3..5
        d2, q, _, _ = tri_point(S[..., j, :], T[..., 0, :], T[..., 1, :], T[..., 2, :])
        d2s.append(d2); Ps.append(q); Qs.append(S[..., j, :])
    for e0, e1 in EDGES:                                     # 6 + 3e + f
        for f0, f1 in EDGES:
            _, _, d2, P, Q = seg_seg(T[..., e0, :], T[..., e1, :], S[..., f0, :], S[..., f1, :])
            d2s.append(d2); Ps.append(P); Qs.append(Q)
    nan = T.dtype.type(np.nan)
    for e0, e1 in EDGES:                                     # 15..17
        hit, _, _, _, X = seg_tri(T[..., e0, :], T[..., e1, :], S[..., 0, :], S[..., 1, :], S[..., 2, :])
        d2s.append(np.where(hit, T.dtype.type(0), nan)); Ps.append(X); Qs.append(X)
    for f0, f1 in EDGES:                                     # 18..20
        hit, _, _, _, X = seg_tri(S[..., f0, :], S[..., f1, :], T[..., 0, :], T[..., 1, :], T[..., 2, :])
        d2s.append(np.where(hit, T.dtype.type(0), nan)); Ps.append(X); Qs.append(X)
    return np.stack(d2s, axis=-1), np.stack(Ps, axis=-2), np.stack(Qs, axis=-2)


def select(d2, P, Q, order=None):
    """the pair's answer from its candidates: it starts as (+inf, code -1, P = Q = 0) and a candidate replaces it iff its d2 is below the answer's.
    order: the sequence in which the codes are offered (default 0..20); the rule "at equal bits the first in CODE order" is then applied explicitly, so the
    result may not depend on it"""
    T = d2.dtype.type
    codes = np.arange(d2.shape[-1]) if order is None else np.asarray(order)
    best = np.full(d2.shape[:-1], np.inf, d2.dtype); code = np.full(d2.shape[:-1], -1, np.int32)
    bp = np.zeros(d2.shape[:-1] + (3,), d2.dtype); bq = bp.copy()
    with np.errstate(invalid="ignore"):
        for k in codes:
            take = (d2[..., k] < best) | ((d2[..., k] == best) & (code >= 0) & (k < code))
            best = np.where(take, d2[..., k], best); code = np.where(take, np.int32(k), code)
            bp = np.where(take[..., None], P[..., k, :], bp); bq = np.where(take[..., None], Q[..., k, :], bq)
    return best, bp, bq, code


def pair(T, S):
    """-> d2 [...], P, Q [..., 3], code [...] int32"""
    return select(*candidates(T, S))


def kat_rows(rows, what):
    """the rows of tirt_kat_tri_tri: what = 0: [n, 18] -> [n, 8]; 1: [n, 12] -> [n, 3]; 2: [n, 15] -> [n, 4]"""
    rows = np.ascontiguousarray(rows, np.float32)
    v = lambda k: rows[:, 3 * k:3 * k + 3]
    if what == 0:
        d2, P, Q, code = pair(rows[:, 0:9].reshape(-1, 3, 3), rows[:, 9:18].reshape(-1, 3, 3))
        return np.concatenate([d2[:, None], P, Q, code.astype(np.float32)[:, None]], axis=1).astype(np.float32)
    if what == 1:
        s, t, d2, _, _ = seg_seg(v(0), v(1), v(2), v(3))
        return np.stack([s, t, d2], axis=1).astype(np.float32)
    hit, u, vv, t, _ = seg_tri(v(0), v(1), v(2), v(3), v(4))
    return np.stack([hit.astype(np.float32), u, vv, t], axis=1).astype(np.float32)


def brute_force(tris, geom, dmax=None, block=64):
    """The answer of the definition for every query triangle [n, 3, 3] float32 against geom.tris (closest_point_expected.Geometry; its spheres take no
    part): (d2 [n], prim [n], code [n], P [n, 3], Q [n, 3]).  Among D2 <= lim2 (and D2 < +inf, never NaN) the smallest D2, at equal bits the smallest
    primitive id; nothing: (+inf, -1, -1, 0, 0)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    n = tris.shape[0]
    lim2 = limit2(np.full(n, np.inf, np.float32) if dmax is None else np.broadcast_to(np.asarray(dmax, np.float32), (n,)))
    lim2 = np.where(np.isfinite(tris).all(axis=(1, 2)), lim2, np.float32(-1.0))      # a T that is not finite finds nothing
    out_d2 = np.full(n, np.inf, np.float32); out_prim = np.full(n, -1, np.int32); out_code = np.full(n, -1, np.int32)
    out_p = np.zeros((n, 3), np.float32); out_q = np.zeros((n, 3), np.float32)
    prim_all = geom.tri_prim.astype(np.int64)
    if geom.tris.shape[0] == 0:
        return out_d2, out_prim, out_code, out_p, out_q
    for s in range(0, n, block):
        d2, P, Q, code = pair(tris[s:s + block, None], geom.tris[None])
        with np.errstate(invalid="ignore"):
            ok = (d2 <= lim2[s:s + block, None]) & (d2 < np.float32(np.inf))
        key = np.where(ok, d2, np.float32(np.inf))
        best = key.min(axis=1)
        tie = ok & (key == best[:, None])
        pid = np.where(tie, prim_all[None, :], np.int64(1) << 40)
        col = pid.argmin(axis=1)
        found = tie.any(axis=1)
        rows = np.arange(d2.shape[0])
        out_d2[s:s + block] = np.where(found, d2[rows, col], np.float32(np.inf))
        out_prim[s:s + block] = np.where(found, prim_all[col], -1)
        out_code[s:s + block] = np.where(found, code[rows, col], -1)
        out_p[s:s + block] = np.where(found[:, None], P[rows, col], np.float32(0))
        out_q[s:s + block] = np.where(found[:, None], Q[rows, col], np.float32(0))
    return out_d2, out_prim, out_code, out_p, out_q
