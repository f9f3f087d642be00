"""Operand rows for the triangle-distance known-answer entries (tirt_kat_tri_tri / tirt_kat_tri_tri_host), shared by the host and the device tests:
the kinds of pairs at which the 21 candidates of include/tirt.h, "Triangle distance", can go wrong."""
import numpy as np

F = np.float32


def _tri(r, n, scale=1.0, centre=0.0):
    return (centre + scale * r.uniform(-1.0, 1.0, (n, 3, 3))).astype(F)


def pair_rows(seed=1, n=256):
    """[N, 18] float32 rows (T, a, b, c): n of each kind"""
    r = np.random.RandomState(seed)
    parts = []
    add = lambda T, S: parts.append(np.concatenate([np.asarray(T, F).reshape(-1, 9), np.asarray(S, F).reshape(-1, 9)], axis=1))
    add(_tri(r, n), _tri(r, n))                                                  # random, overlapping boxes: many cross
    add(_tri(r, n, 0.3, r.uniform(-2, 2, (n, 1, 3))), _tri(r, n, 0.3, r.uniform(-2, 2, (n, 1, 3))))      # random, mostly apart
    add(_tri(r, n, 1000.0), _tri(r, n, 1000.0))                                  # large coordinates
    add(_tri(r, n, 0.05), _tri(r, n, 2.0))                                       # a small triangle against a large one, and the reverse
    add(_tri(r, n, 2.0), _tri(r, n, 0.05))
    T, S = _tri(r, n), _tri(r, n)                                                # one shared vertex, copied bits, at every pair of corners
    for i in range(n):
        T[i, i % 3] = S[i, (i // 3) % 3]
    add(T, S)
    T, S = _tri(r, n), _tri(r, n)                                                # one shared edge, copied bits, in either direction
    for i in range(n):
        e, f = i % 3, (i // 3) % 3
        a, b = (f, (f + 1) % 3) if (i // 9) % 2 == 0 else ((f + 1) % 3, f)
        T[i, e], T[i, (e + 1) % 3] = S[i, a], S[i, b]
    add(T, S)
    S = _tri(r, n)                                                               # the same triangle, and its corners in another order
    add(S, S); add(S[:, [1, 2, 0]], S); add(S[:, [2, 1, 0]], S)
    S = _tri(r, n)                                                               # coplanar: T from barycentric combinations of S (some overlap, some not)
    w = r.uniform(-1.0, 2.0, (n, 3, 3)); w /= w.sum(axis=2, keepdims=True)
    add(np.einsum("nij,njk->nik", w, S.astype(np.float64)), S)
    S = _tri(r, n); S[:, :, 2] = F(0.25)                                         # exactly coplanar in z, and parallel planes (offset exact in fp32)
    T = _tri(r, n); T[:, :, 2] = F(0.25)
    add(T, S)
    T = T.copy(); T[:, :, 2] = F(0.75)
    add(T, S)
    S = _tri(r, n)                                                               # parallel translates: every edge pair e == f is parallel (den == 0 or rounding)
    add(S + np.array([0.5, 0.25, 2.0], F), S)
    T = _tri(r, n); S = _tri(r, n)                                               # degenerate T: a segment (two corners equal), a point (all equal)
    T[: n // 2, 2] = T[: n // 2, 1]
    T[n // 2:, 1] = T[n // 2:, 0]; T[n // 2:, 2] = T[n // 2:, 0]
    add(T, S); add(S, T)                                                         # ... and the degenerate one as the scene triangle
    T = _tri(r, n); T[:, 1] = T[:, 0]; T[:, 2] = T[:, 0]                         # both degenerate: points and segments against each other
    S = _tri(r, n); S[: n // 2, 2] = S[: n // 2, 1]; S[n // 2:, 1] = S[n // 2:, 0]; S[n // 2:, 2] = S[n // 2:, 0]
    add(T, S)
    T = _tri(r, n); S = _tri(r, n)                                               # needles: the third corner on the opposite edge but for a rounding
    t = r.uniform(0, 1, (n, 1)).astype(F)
    T[:, 2] = (T[:, 0] + (T[:, 1] - T[:, 0]) * t).astype(F)
    S[::2, 2] = (S[::2, 0] + (S[::2, 1] - S[::2, 0]) * t[::2]).astype(F)
    add(T, S)
    T = _tri(r, n); S = _tri(r, n)                                               # NaN and +-inf in one coordinate of either triangle
    vals = (np.nan, np.inf, -np.inf)
    for i in range(n):
        (T if i % 2 == 0 else S)[i, (i // 2) % 3, (i // 6) % 3] = vals[(i // 18) % 3]
    add(T, S)
    return np.concatenate(parts, axis=0)


def seg_seg_rows(seed=2, n=256):
    """[N, 12] float32 rows (p1, q1, p2, q2)"""
    r = np.random.RandomState(seed)
    u = lambda: r.uniform(-1.0, 1.0, (n, 3)).astype(F)
    parts = []
    add = lambda *v: parts.append(np.concatenate([np.asarray(x, F) for x in v], axis=1))
    add(u(), u(), u(), u())
    add(u() * F(1000), u() * F(1000), u(), u())
    p = u(); add(p, p, u(), u())                                                 # A <= 0
    p = u(); add(u(), u(), p, p)                                                 # E <= 0
    p, q = u(), u(); add(p, p, q, q)                                             # both
    p, q = u(), u(); add(p, q, p, q); add(p, q, q, p)                            # the same segment
    p, q, s = u(), u(), u(); add(p, q, p + s, q + s)                             # parallel (a rounded translate: den is 0 or rounding noise of either sign)
    p, q = u(), u(); d = (q - p).astype(F)
    add(p, q, (p + d * F(2)).astype(F), (p + d * F(3.5)).astype(F))              # collinear, apart
    add(p, q, (p + d * F(0.25)).astype(F), (p + d * F(0.75)).astype(F))          # collinear, overlapping
    p, q, s = u(), u(), u(); add(p, q, q, s); add(p, q, s, p)                    # a shared end point
    x = np.zeros((n, 3), F); a = r.uniform(0.1, 1.0, (n, 1)).astype(F)           # crossing in a plane, exact: (+-a, 0, 0) x (0, +-a, 0)
    add(x + a * np.array([-1, 0, 0], F), x + a * np.array([1, 0, 0], F), x + a * np.array([0, -1, 0], F), x + a * np.array([0, 1, 0], F))
    bad = [u(), u(), u(), u()]
    for i in range(n):
        bad[i % 4][i, (i // 4) % 3] = (np.nan, np.inf, -np.inf)[(i // 12) % 3]
    add(*bad)
    return np.concatenate(parts, axis=0)


def seg_tri_rows(seed=3, n=256):
    """[N, 15] float32 rows (x0, x1, a, b, c)"""
    r = np.random.RandomState(seed)
    u = lambda: r.uniform(-1.0, 1.0, (n, 3)).astype(F)
    parts = []
    add = lambda *v: parts.append(np.concatenate([np.asarray(x, F) for x in v], axis=1))
    add(u(), u(), u(), u(), u())
    a, b, c = u(), u(), u()
    w = r.dirichlet((1, 1, 1), n)
    inside = (a * w[:, 0:1] + b * w[:, 1:2] + c * w[:, 2:3])
    d = u()
    add((inside - d).astype(F), (inside + d).astype(F), a, b, c)                # through an interior point
    add((inside + d * 0.5).astype(F), (inside + d).astype(F), a, b, c)          # stops short: t < 0
    add(a, u(), a, b, c); add(u(), b, a, b, c)                                   # starts or ends AT a corner, copied bits
    mid = ((a.astype(np.float64) + b) * 0.5)
    add((mid - d).astype(F), (mid + d).astype(F), a, b, c)                      # through an edge's midpoint
    add(a, b, a, b, c); add(b, c, a, b, c)                                       # an edge of the triangle itself: coplanar, det == 0 or noise
    e1, e2 = (b - a).astype(F), (c - a).astype(F)
    add((a + e1 * F(0.3)).astype(F), (a + e2 * F(0.6)).astype(F), a, b, c)      # in the triangle's plane
    add(u(), u(), a, a, c); add(u(), u(), a, a, a)                               # a degenerate triangle
    p = u(); add(p, p, a, b, c)                                                  # a degenerate segment
    bad = [u(), u(), u(), u(), u()]
    for i in range(n):
        bad[i % 5][i, (i // 5) % 3] = (np.nan, np.inf, -np.inf)[(i // 15) % 3]
    add(*bad)
    return np.concatenate(parts, axis=0)


ROWS = {0: pair_rows, 1: seg_seg_rows, 2: seg_tri_rows}
