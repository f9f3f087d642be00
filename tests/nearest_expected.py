"""The definition "K nearest primitives" of include/tirt.h restated in numpy: D2 / Q / u / v of EVERY primitive through closest_point_expected.tri_point /
sphere_point (the terms of "Closest point", unchanged), the set N = {D2 <= lim2 and D2 < +inf}, the order (D2 ascending, at equal bits the smaller
primitive id: np.lexsort((prim, d2))), the padding (+inf, -1, 0, 0) and |N|.  Written from the header alone."""
import numpy as np

import closest_point_expected as E

F = np.float32


def all_primitives(points, geom, block=256):
    """D2 [n, P], Q [n, P, 3], u [n, P], v [n, P] of every surface primitive for every point, and their primitive ids [P]"""
    p = np.ascontiguousarray(points, F).reshape(-1, 1, 3)
    prim = np.concatenate([geom.tri_prim, geom.sphere_prim]).astype(np.int64)
    if p.shape[0] > block:                                   # (rows are independent: blocks only bound the temporaries)
        rows = [all_primitives(p[s:s + block], geom) for s in range(0, p.shape[0], block)]
        return tuple(np.concatenate([r[i] for r in rows], axis=0) for i in range(4)) + (prim,)
    parts = []
    if geom.tris.shape[0]:
        a, b, c = (geom.tris[None, :, k, :] for k in range(3))
        parts.append(E.tri_point(p, a, b, c))
    if geom.spheres.shape[0]:
        parts.append(E.sphere_point(p, geom.spheres[None, :, 0:3], np.broadcast_to(geom.spheres[None, :, 3], (p.shape[0], geom.spheres.shape[0]))))
    d2, q, u, v = (np.concatenate([np.broadcast_to(x[i], (p.shape[0],) + x[i].shape[1:]) for x in parts], axis=1) for i in range(4))
    return d2.astype(F), q.astype(F), u.astype(F), v.astype(F), prim


class Table:
    """the per-primitive terms of a set of points, computed once and shared by every k and bound a test asks for"""

    def __init__(self, points, geom):
        self.n = np.asarray(points).reshape(-1, 3).shape[0]
        self.d2, self.q, self.u, self.v, self.prim = all_primitives(points, geom)

    def nearest(self, k, dmax=None):
        """(d2 [n, k], prim [n, k] int32, point [n, k, 3], uv [n, k, 2], count [n] int32) of the definition"""
        n = self.n
        lim2 = E.limit2(np.full(n, np.inf, F) if dmax is None else np.broadcast_to(np.asarray(dmax, F), (n,)))
        out_d2 = np.full((n, k), np.inf, F); out_prim = np.full((n, k), -1, np.int32)
        out_q = np.zeros((n, k, 3), F); out_uv = np.zeros((n, k, 2), F); count = np.zeros(n, np.int32)
        with np.errstate(invalid="ignore"):
            member = (self.d2 <= lim2[:, None]) & (self.d2 < F(np.inf))
        for i in range(n):
            cols = np.nonzero(member[i])[0]
            count[i] = cols.size
            order = cols[np.lexsort((self.prim[cols], self.d2[i, cols]))][:k]
            m = order.size
            out_d2[i, :m] = self.d2[i, order]; out_prim[i, :m] = self.prim[order]
            out_q[i, :m] = self.q[i, order]
            out_uv[i, :m, 0] = self.u[i, order]; out_uv[i, :m, 1] = self.v[i, order]
        return out_d2, out_prim, out_q, out_uv, count


def nearest(points, geom, k, dmax=None):
    return Table(points, geom).nearest(k, dmax)


def list_of(d2, prim, k, lim2):
    """the list of explicit candidates (d2 float32, prim int32, distinct ids) by a stable sort: (d2 [k], prim [k] padded with (inf, -1), entries held, |N|)"""
    d2 = np.asarray(d2, F).reshape(-1); prim = np.asarray(prim, np.int32).reshape(-1)
    with np.errstate(invalid="ignore"):
        member = (d2 <= F(lim2)) & (d2 < F(np.inf))
    cols = np.nonzero(member)[0]
    order = cols[np.lexsort((prim[cols], d2[cols]))][:k]
    out_d2 = np.full(k, np.inf, F); out_prim = np.full(k, -1, np.int32)
    out_d2[:order.size] = d2[order]; out_prim[:order.size] = prim[order]
    return out_d2, out_prim, int(order.size), int(cols.size)
