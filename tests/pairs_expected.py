"""The definitions "Point pairs" and "Triangle pairs" of include/tirt.h restated in numpy: all D2 through nearest_expected.all_primitives (points) and
triangle_query_expected.pair (triangles), the membership rule {D2 <= lim2 and D2 < +inf}, the order inside a row (D2 ascending, at equal bits the smaller
primitive id: np.lexsort((prim, d2))), row_start as the exclusive prefix sums of the rows' lengths, and the whole-rows-only capacity rule.  Written from the
header alone."""
import numpy as np

import closest_point_expected as CE
import nearest_expected as NE
import triangle_query_expected as TE

F = np.float32


def rows_to_csr(member, d2, prim):
    """member [n, P] bool, d2 [n, P] float32, prim [P] -> (row_start [n + 1] int64, cols [total]: the column of every pair, rows in order, each row ordered)"""
    n = member.shape[0]
    row_start = np.zeros(n + 1, np.int64)
    cols = []
    for i in range(n):
        c = np.nonzero(member[i])[0]
        c = c[np.lexsort((prim[c], d2[i, c]))]
        cols.append(c)
        row_start[i + 1] = row_start[i] + c.size
    return row_start, (np.concatenate(cols) if cols else np.zeros(0, np.int64)).astype(np.int64)


def query_of(row_start):
    """the query index of every pair"""
    return np.repeat(np.arange(row_start.size - 1), np.diff(row_start))


def rows_that_fit(row_start, capacity):
    """(number of rows written, pairs written): a row is written iff row_start[i + 1] <= capacity; the sums only grow, so those rows are a prefix"""
    fits = row_start[1:] <= capacity
    k = int(fits.sum())
    assert fits[:k].all()
    return k, int(row_start[k])


def limit2(n, dmax):
    return CE.limit2(np.full(n, np.inf, F) if dmax is None else np.broadcast_to(np.asarray(dmax, F), (n,)))


class PointTable:
    """the per-primitive terms of a set of points, computed once and shared by every bound a test asks for"""

    def __init__(self, points, geom):
        self.n = np.asarray(points).reshape(-1, 3).shape[0]
        self.d2, self.q, self.u, self.v, self.prim = NE.all_primitives(points, geom)

    def within(self, dmax=None):
        """(row_start [n + 1] int64, prim [total] int32, d2 [total], point [total, 3], uv [total, 2])"""
        lim2 = limit2(self.n, dmax)
        with np.errstate(invalid="ignore"):
            member = (self.d2 <= lim2[:, None]) & (self.d2 < F(np.inf))
        row_start, cols = rows_to_csr(member, self.d2, self.prim)
        q = query_of(row_start)
        return (row_start, self.prim[cols].astype(np.int32), self.d2[q, cols], self.q[q, cols], np.stack([self.u[q, cols], self.v[q, cols]], axis=1).reshape(-1, 2))


class TriangleTable:
    """the pair's answer of every query triangle against every scene triangle, computed once"""

    def __init__(self, tris, geom, block=32):
        tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
        self.n = tris.shape[0]
        self.finite = np.isfinite(tris).all(axis=(1, 2))
        self.prim = geom.tri_prim.astype(np.int64)
        parts = [TE.pair(tris[s:s + block, None], geom.tris[None]) for s in range(0, self.n, block)]
        self.d2, self.P, self.Q, self.code = (np.concatenate([p[i] for p in parts], axis=0) for i in range(4))

    def pairs(self, dmax=0.0):
        """(row_start [n + 1] int64, prim [total] int32, d2 [total], code [total] int32, P [total, 3], Q [total, 3])"""
        lim2 = np.where(self.finite, limit2(self.n, dmax), F(-1.0))      # a T that is not finite has the empty row
        with np.errstate(invalid="ignore"):
            member = (self.d2 <= lim2[:, None]) & (self.d2 < F(np.inf))
        row_start, cols = rows_to_csr(member, self.d2, self.prim)
        q = query_of(row_start)
        return (row_start, self.prim[cols].astype(np.int32), self.d2[q, cols].astype(F), self.code[q, cols].astype(np.int32), self.P[q, cols].astype(F),
                self.Q[q, cols].astype(F))


def ordered_rows(d2, prim, row_len, capacity=None, fill=(np.nan, -1)):
    """tirt_kat_pairs_host by a stable sort: rows of members in the order given -> (row_start, d2 [capacity], prim [capacity]) with `fill` where no row is written"""
    d2 = np.asarray(d2, F).reshape(-1); prim = np.asarray(prim, np.int32).reshape(-1); row_len = np.asarray(row_len, np.int64).reshape(-1)
    row_start = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    capacity = int(row_start[-1]) if capacity is None else int(capacity)
    out_d2 = np.full(capacity, fill[0], F); out_prim = np.full(capacity, fill[1], np.int32)
    rows, _ = rows_that_fit(row_start, capacity)
    for i in range(rows):
        a, b = row_start[i], row_start[i + 1]
        order = np.lexsort((prim[a:b], d2[a:b].view(np.uint32)))      # (members are >= +0 and finite: the bit order is the float order, and -0 is not among them)
        out_d2[a:b] = d2[a:b][order]; out_prim[a:b] = prim[a:b][order]
    return row_start, out_d2, out_prim
