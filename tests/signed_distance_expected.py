"""The signed-distance definition of include/tirt.h ("Signed distance") restated in numpy on top of closest_point_expected.py: the table of angle-weighted
pseudo-normals (float32, one rounding per operation, tm_atan2 / tm_sqrt through the oracle's orc_kat_math, integer sums, corners matched by brute force:
every corner against every corner), the feature rule, and sd.  Nothing here knows how the device finds the triangles that touch a corner."""
import numpy as np

import closest_point_expected as E
import oracle_api

F = np.float32
ROWS = ("interior", "A", "B", "C", "AB", "AC", "BC")
CLOSED, BOUNDARY, NONMANIFOLD, FLIPPED = 0, 1, 2, 3
INVALID_BIT = 64
SCALE = F(1073741824.0)


def _kat(fn, x, y=None):
    """tm_atan2 (5) / tm_sqrt (7) of csrc/tirt_math.h, as the oracle compiles them"""
    x = np.ascontiguousarray(x, F)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, F)
    out = np.zeros_like(x)
    oracle_api.load().orc_kat_math(fn, x.reshape(-1), y.reshape(-1), out.reshape(-1), x.size)
    return out


def tm_sqrt(x):
    return _kat(7, x)


def tm_atan2(y, x):
    return _kat(5, y, x)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def quant(x):
    """I(x) = (int64) rintf(x * 2^30)"""
    return np.rint(np.asarray(x, F) * SCALE).astype(np.int64)


def feature(u, v):
    """row of the table for a closest point with barycentrics (u, v): the first line of the definition that holds"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    conds = [(v == 0) & (u == 0), (v == 0) & (u == 1), v == 0, (u == 0) & (v == 1), u == 0, u == F(1.0) - v]
    return np.select(conds, [1, 2, 4, 3, 5, 6], 0)


def triangle_terms(tris):
    """tris [T, 3, 3] float32 -> n^ [T, 3], valid [T], the three corner angles [T, 3]"""
    tris = np.ascontiguousarray(tris, F)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(all="ignore"):
        g = cross(b - a, c - a)
        l2 = E.dot(g, g)
        valid = (l2 > 0) & (l2 < F(np.inf))
        nh = g / tm_sqrt(l2)[:, None]
        alpha = np.zeros((tris.shape[0], 3), F)
        for j in range(3):
            e1, e2 = tris[:, (j + 1) % 3] - tris[:, j], tris[:, (j + 2) % 3] - tris[:, j]
            x = cross(e1, e2)
            alpha[:, j] = tm_atan2(tm_sqrt(E.dot(x, x)), E.dot(e1, e2))
    return nh.astype(F), valid, alpha


def table(geom, n_prim):
    """The table of the definition for a closest_point_expected.Geometry: float32 [n_prim, 7, 4]; [:, 0, 3] holds the class bits (view it as int32)"""
    tris, prim = geom.tris, geom.tri_prim
    T = tris.shape[0]
    nh, valid, alpha = triangle_terms(tris)
    with np.errstate(all="ignore"):
        vterm = quant(alpha[:, :, None] * nh[:, None, :])              # [T, 3 corners, 3]
        eterm = quant(nh)                                            # [T, 3]
    tab = np.zeros((n_prim, 7, 4), F)
    bits = np.zeros(n_prim, np.int32)
    edge_row = (4, 6, 5)                                             # AB, BC, CA
    for t in range(T):
        tab[prim[t], 0, :3] = nh[t]
        if not valid[t]:
            bits[prim[t]] |= INVALID_BIT
        for k in range(3):
            v0, v1 = tris[t, k], tris[t, (k + 1) % 3]
            at_v0 = (tris == v0).all(axis=2) & valid[:, None]        # [T, 3]: corner j of t' is at v0 (NaN equals nothing, -0 equals +0)
            vsum = np.zeros(3, np.int64); esum = np.zeros(3, np.int64)
            others = same_way = 0
            for tp, j in zip(*np.nonzero(at_v0)):
                vsum += vterm[tp, j]
                at_next = bool((tris[tp, (j + 1) % 3] == v1).all())
                at_prev = bool((tris[tp, (j + 2) % 3] == v1).all())
                if at_next or at_prev:
                    esum += eterm[tp]
                    if prim[tp] != prim[t]:
                        others += 1
                        same_way += int(at_next)
            tab[prim[t], 1 + k, :3] = [F(int(s)) for s in vsum]
            tab[prim[t], edge_row[k], :3] = [F(int(s)) for s in esum]
            cls = BOUNDARY if others == 0 else (NONMANIFOLD if others >= 2 else (FLIPPED if same_way else CLOSED))
            bits[prim[t]] |= cls << (2 * k)
    tab[:, 0, 3] = bits.view(F)
    return tab


def class_bits(tab):
    return np.ascontiguousarray(tab[:, 0, 3]).view(np.int32)


def report(tab, geom):
    """the five counts of tirt_signed_distance_prepare and `closed`, from a table"""
    bits = class_bits(tab)[geom.tri_prim]
    cls = np.stack([(bits >> (2 * k)) & 3 for k in range(3)], axis=1)
    r = {"boundary_edges": int((cls == BOUNDARY).sum()), "nonmanifold_edges": int((cls == NONMANIFOLD).sum()), "flipped_edges": int((cls == FLIPPED).sum()),
         "invalid_triangles": int(((bits & INVALID_BIT) != 0).sum()), "primitives": int(tab.shape[0])}
    r["closed"] = not any(r[k] for k in ("boundary_edges", "nonmanifold_edges", "flipped_edges", "invalid_triangles"))
    return r


def sign_from(points, geom, tab, answer, face_normal_only=False):
    """sd [N] of the definition from a closest-point answer (d2, prim, q, uv) and a table.  face_normal_only: the shortcut the definition exists to
    avoid -- row 0 whatever the feature -- for the tests that must tell the two apart"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    d2, prim, q, uv = answer
    n = points.shape[0]
    sd = np.full(n, np.inf, F)
    with np.errstate(all="ignore"):
        d = tm_sqrt(d2)
        is_tri = np.isin(prim, geom.tri_prim) & (prim >= 0)
        f = np.where(face_normal_only, 0, feature(uv[:, 0], uv[:, 1]))
        N = tab[np.where(is_tri, prim, 0), f, :3]
        pq = points - q
        s = E.dot(pq, N)
        sd = np.where(is_tri, np.where(s < 0, -d, d), sd)
        for k, sp in enumerate(geom.sphere_prim):
            pc = points - geom.spheres[k, 0:3]
            ln = tm_sqrt(E.dot(pc, pc))
            sd = np.where(prim == sp, np.where(ln < geom.spheres[k, 3], -d, d), sd)
    return sd.astype(F), f


def signed_distance(points, geom, tab, dmax=None):
    """(sd, d2, prim, q, uv) of the definition: closest_point_expected.brute_force, then the sign"""
    ans = E.brute_force(points, geom, dmax)
    return (sign_from(points, geom, tab, ans)[0],) + ans


def kat_rows(p, tri, N):
    """rows of tirt_kat_signed_distance: p [n, 3], tri [n, 3, 3], N [n, 7, 3] -> [n, 33] and the expected [n, 2] (sd, feature)"""
    p, tri, N = np.ascontiguousarray(p, F), np.ascontiguousarray(tri, F), np.ascontiguousarray(N, F)
    rows = np.concatenate([p, tri.reshape(-1, 9), N.reshape(-1, 21)], axis=1)
    d2, q, u, v = E.tri_point(p, tri[:, 0], tri[:, 1], tri[:, 2])
    f = feature(u, v)
    with np.errstate(all="ignore"):
        s = E.dot(p - q, N[np.arange(p.shape[0]), f])
        d = tm_sqrt(d2)
        sd = np.where(s < 0, -d, d)
    return rows, np.stack([sd.astype(F), f.astype(F)], axis=1)
