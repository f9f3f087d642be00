"""The winding-number definition of include/tirt.h ("Winding number") restated in numpy: the triangle and sphere terms (float32, one rounding per operation,
tm_atan2 through the oracle's orc_kat_math), the quantisation, the moment rows from a 4-wide tree (a downloaded one, tirt_wide_tree_download, or the
hand-built one of build_tree), the walk over such a tree and its table, and the exact sum in float64.  Nothing here knows how the device finds anything:
the sums are formed over flat lists and the walk is a breadth-first frontier."""
import numpy as np

import closest_point_expected as E
import signed_distance_expected as SE

F = np.float32
D = np.float64
FOUR_PI = F(12.566370614359172)
INV_FOUR_PI = F(0.07957747154594767)
UNIT = F(9.313225746154785e-10)
SCALE = F(1073741824.0)
LIMIT = F(4611686018427387904.0)
THIRD = F(0.3333333432674408)
TR_EMPTY = -0x7fffffff            # (int) 0x80000001
GRID_HALF = 30000.0


# ---- terms ---------------------------------------------------------------------------------------------------------------------------------------
def quant(x):
    """I(x) = (int64) rintf(x * 2^30) if |x * 2^30| < 2^62, else 0 (NaN: 0)"""
    with np.errstate(all="ignore"):
        y = np.asarray(x, F) * SCALE
        ok = np.abs(y) < LIMIT
        return np.where(ok, np.rint(np.where(ok, y, F(0))), F(0)).astype(np.int64)


def result(S):
    """w of a sum of quantised terms"""
    return (np.asarray(S, np.int64).astype(F) * UNIT) * INV_FOUR_PI


def triangle_normal(tris):
    """tris [T, 3, 3] float32 -> g [T, 3], l2 [T], valid [T]"""
    tris = np.ascontiguousarray(tris, F)
    with np.errstate(all="ignore"):
        g = SE.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
        l2 = E.dot(g, g)
    return g, l2, (l2 > 0) & (l2 < F(np.inf))


def _omega(q, tris, valid):
    """the triangle term for q and tris [..., 3, 3] that broadcast against each other"""
    with np.errstate(all="ignore"):
        a, b, c = tris[..., 0, :] - q, tris[..., 1, :] - q, tris[..., 2, :] - q
        la, lb, lc = np.sqrt(E.dot(a, a)), np.sqrt(E.dot(b, b)), np.sqrt(E.dot(c, c))
        num = E.dot(a, SE.cross(b, c))
        den = (((la * lb) * lc + E.dot(a, b) * lc) + E.dot(a, c) * lb) + E.dot(b, c) * la
        om = F(2.0) * SE.tm_atan2(num, den)
    return np.where(valid, om, F(0)).astype(F)


def triangle_omega(q, tris):
    """Omega [N, T] float32 of queries q [N, 3] and triangles [T, 3, 3]; an invalid triangle: 0"""
    q = np.ascontiguousarray(q, F).reshape(-1, 1, 3)
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    return _omega(q, tris[None], triangle_normal(tris)[2][None, :])


def triangle_omega_rows(q, tris):
    """Omega [K] of K (query, triangle) pairs: q [K, 3], tris [K, 3, 3]"""
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    return _omega(q, tris, triangle_normal(tris)[2])


def sphere_omega(q, spheres):
    """Omega [N, S] of analytic spheres [S, 4] (centre, radius)"""
    q = np.ascontiguousarray(q, F).reshape(-1, 1, 3)
    s = np.ascontiguousarray(spheres, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        pc = q - s[None, :, :3]
        ln = np.sqrt(E.dot(pc, pc))
        return np.where(ln < s[None, :, 3], FOUR_PI, F(0)).astype(F)


def finite_rows(points):
    return np.isfinite(np.asarray(points, F)).all(axis=1)


def exact_sum(points, tris, spheres=None, block=512):
    """S [N] int64: the integer sum over every triangle and sphere (a row with a NaN or infinite coordinate: 0; its answer is NaN, answer())"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    S = np.zeros(points.shape[0], np.int64)
    fin = finite_rows(points)
    for lo in range(0, points.shape[0], block):
        p = points[lo:lo + block]
        s = quant(triangle_omega(p, tris)).sum(axis=1) if len(tris) else np.zeros(p.shape[0], np.int64)
        if spheres is not None and len(spheres):
            s = s + quant(sphere_omega(p, spheres)).sum(axis=1)
        S[lo:lo + block] = s
    return np.where(fin, S, 0)


def answer(points, S):
    """w [N] float32 of the sums S: NaN for a row that is not finite"""
    return np.where(finite_rows(points), result(S), F(np.nan)).astype(F)


def exact_float64(points, tris, spheres=None):
    """the winding number in float64, no quantisation: what the fp32 answers are an approximation of"""
    import signed_distance_scenes as S
    p = np.asarray(points, D).reshape(-1, 3)
    w = S.winding_number(p, np.asarray(tris, F).astype(D)) if len(tris) else np.zeros(p.shape[0])
    if spheres is not None:
        for s in np.asarray(spheres, D).reshape(-1, 4):
            w = w + (((p - s[:3]) ** 2).sum(axis=1) < s[3] ** 2)
    return w


# ---- a 4-wide tree: what tirt_wide_tree_download returns, or build_tree below ---------------------------------------------------------------------
class Tree:
    """cnode uint32 [nodes, 16] (only the first wide_nodes are walked), tri float32 [n, 12] records, grid_min / cell float32 [3], root_code"""

    def __init__(self, d):
        self.nodes = int(d["wide_nodes"])
        self.cnode = np.ascontiguousarray(d["cnode"], np.uint32)[:self.nodes]
        self.tri = np.ascontiguousarray(d["tri"], F).reshape(-1, 12)
        self.grid_min = np.asarray(d["grid_min"], F)
        self.cell = np.asarray(d["grid_cell"], F)
        self.root_code = int(d["root_code"])
        self.codes = self.cnode[:, 12:16].view(np.int32).astype(np.int64)          # [nodes, 4]
        planes = self.cnode[:, :12].reshape(self.nodes, 4, 3)
        lo = (planes & np.uint32(0xffff)).astype(np.uint16).view(np.float16).astype(F)
        hi = (planes >> np.uint32(16)).astype(np.uint16).view(np.float16).astype(F)
        self.box_min = (self.grid_min[None, None, :] + lo * self.cell[None, None, :]).astype(F)      # the decode of CP_BOX_GAP
        self.box_max = (self.grid_min[None, None, :] + hi * self.cell[None, None, :]).astype(F)
        ext = F(self.cell.max()) * F(2.0 * GRID_HALF)
        self.e = int((np.asarray(ext, F).view(np.uint32) >> 23) & 0xff) - 126

    # a leaf code, inverted: the record slot and whether it is a triangle's
    @staticmethod
    def leaf_slot(code):
        return (~code) & 0x3fffffff

    @staticmethod
    def leaf_is_tri(code):
        return (((~code) >> 30) & 1) == 0

    def record_tris(self):
        return self.tri[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3)


def triangle_moments(tree):
    """[n, 16] int64: the sixteen integer moments of every record as if it were a triangle (zero where it is invalid)"""
    tris = tree.record_tris()
    g, l2, valid = triangle_normal(tris)
    s2, s3 = D(2.0) ** (37 - 2 * tree.e), D(2.0) ** (37 - 3 * tree.e)
    with np.errstate(all="ignore"):
        h = (F(0.5) * g).astype(F)
        ar = (F(0.5) * np.sqrt(l2)).astype(F)
        gm = tree.grid_min[None, :]
        cen = ((((tris[:, 0] - gm) + (tris[:, 1] - gm)) + (tris[:, 2] - gm)) * THIRD).astype(F)

        def J(x, s):
            y = np.asarray(x, F).astype(D) * s
            ok = np.abs(y) < 4611686018427387904.0
            return np.where(ok, np.rint(np.where(ok, y, 0.0)), 0.0).astype(np.int64)
        cols = [J(h[:, 0], s2), J(h[:, 1], s2), J(h[:, 2], s2), J(ar, s2)]
        cols += [J(ar * cen[:, k], s3) for k in range(3)]
        cols += [J(cen[:, i] * h[:, j], s3) for i in range(3) for j in range(3)]
    m = np.stack(cols, axis=1)
    m[~valid] = 0
    return m


def moment_table(tree):
    """(table [nodes, 4, 16] float32, sums [nodes, 16] int64): the rows of the definition and the integer sums of everything beneath each node"""
    tm = triangle_moments(tree)
    sums = np.zeros((tree.nodes, 16), np.int64)
    for node in range(tree.nodes - 1, -1, -1):               # breadth-first numbering: a child's index is above its parent's
        for c in range(4):
            code = int(tree.codes[node, c])
            if code == TR_EMPTY:
                continue
            if code >= 0:
                assert node < code < tree.nodes, (node, code)
                sums[node] += sums[code]
            elif Tree.leaf_is_tri(code):
                sums[node] += tm[Tree.leaf_slot(code)]
    table = np.zeros((tree.nodes, 4, 16), F)
    inv2, inv3 = D(2.0) ** (2 * tree.e - 37), D(2.0) ** (3 * tree.e - 37)
    gm = tree.grid_min.astype(D)
    for node in range(tree.nodes):
        for c in range(4):
            code = int(tree.codes[node, c])
            if code < 0:
                continue
            m = sums[code]
            mn, mx = tree.box_min[node, c], tree.box_max[node, c]
            has = m[3] > 0
            area = D(m[3]) * inv2
            N = m[0:3].astype(D) * inv2
            M = (m[7:16].astype(D) * inv3).reshape(3, 3)
            if has:
                p = (m[4:7].astype(D) * inv3) / area
                pt = (p + gm).astype(F)
            else:
                p = np.zeros(3, D)
                pt = (F(0.5) * (mn + mx)).astype(F)
            f = np.maximum(np.abs(pt - mn), np.abs(mx - pt)).astype(F)
            r2 = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]
            C = (M - p[:, None] * N[None, :]).astype(F)
            table[node, c] = np.concatenate([pt, [r2], N.astype(F), C.reshape(-1)])
    return table, sums


def far_terms(d, d2, N, C):
    """t0, t1 [K] float32 of K (query, child) pairs: d [K, 3], d2 [K], N [K, 3], C [K, 9]"""
    with np.errstate(all="ignore"):
        s = np.sqrt(d2)
        d3 = d2 * s
        t0 = E.dot(N, d) / d3
        tr = (C[:, 0] + C[:, 4]) + C[:, 8]
        cd = np.stack([E.dot(C[:, 0:3], d), E.dot(C[:, 3:6], d), E.dot(C[:, 6:9], d)], axis=1)
        t1 = tr / d3 - (F(3.0) * E.dot(d, cd)) / (d2 * d3)
    return t0.astype(F), t1.astype(F)


def record_terms(tree, q, code):
    """the quantised term [K] of K (query [K, 3], leaf code [K]) pairs"""
    slot = Tree.leaf_slot(code)
    is_tri = Tree.leaf_is_tri(code)
    rec = tree.tri[slot]
    out = np.zeros(q.shape[0], np.int64)
    k = np.nonzero(is_tri)[0]
    if k.size:
        out[k] = quant(triangle_omega_rows(q[k], rec[k][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]))
    k = np.nonzero(~is_tri & (rec[:, 5].astype(np.int64) == E.SHAPE_SPHERE))[0]
    if k.size:
        with np.errstate(all="ignore"):
            pc = q[k] - rec[k, 0:3]
            ln = np.sqrt(E.dot(pc, pc))
            out[k] = quant(np.where(ln < rec[k, 4], FOUR_PI, F(0)).astype(F))
    return out


def walk(tree, table, points, beta):
    """(S [N] int64, counts [N, 2] int64: child slots examined and leaves evaluated) of the walk of the definition"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    S = np.zeros(n, np.int64)
    counts = np.zeros((n, 2), np.int64)
    with np.errstate(all="ignore"):
        beta2 = F(beta) * F(beta)
    qi = np.nonzero(finite_rows(points))[0]
    code = np.full(qi.shape[0], tree.root_code, np.int64)
    while qi.size:
        leaf = code < 0
        if leaf.any():
            np.add.at(S, qi[leaf], record_terms(tree, points[qi[leaf]], code[leaf]))
            np.add.at(counts[:, 1], qi[leaf], 1)
        qi, code = qi[~leaf], code[~leaf]
        if not qi.size:
            break
        np.add.at(counts[:, 0], qi, 4)
        nq, nc = [], []
        for c in range(4):
            ch = tree.codes[code, c]
            there = ch != TR_EMPTY
            inner = there & (ch >= 0)
            row = table[code, c]
            with np.errstate(all="ignore"):
                d = (row[:, 0:3] - points[qi]).astype(F)
                d2 = E.dot(d, d)
                approx = inner & (d2 > beta2 * row[:, 3])
            k = np.nonzero(approx)[0]
            if k.size:
                t0, t1 = far_terms(d[k], d2[k], row[k, 4:7], row[k, 7:16])
                np.add.at(S, qi[k], quant(t0) + quant(t1))
            go = there & ~approx
            nq.append(qi[go]); nc.append(ch[go])
        qi, code = np.concatenate(nq), np.concatenate(nc)
    return S, counts


# ---- a hand-built tree (no device): median splits into four, breadth-first numbering, planes rounded outward on the grid of the padded root box ---------
def build_tree(tris, spheres=None):
    """a dict as tirt_wide_tree_download's, over triangles [T, 3, 3] (record slot = index) and analytic spheres [S, 4] (slots T ...): a 4-wide tree whose
    every inner node splits its primitives at the median of the longest axis of their centroids, twice; a single primitive: root_code is its leaf code"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    sph = np.zeros((0, 4), F) if spheres is None else np.ascontiguousarray(spheres, F).reshape(-1, 4)
    T, n = tris.shape[0], tris.shape[0] + sph.shape[0]
    rec = np.zeros((n, 12), F)
    rec[:T, 0:3], rec[:T, 4:7], rec[:T, 8:11] = tris[:, 0], tris[:, 1], tris[:, 2]
    rec[T:, 0:3], rec[T:, 4], rec[T:, 5] = sph[:, :3], sph[:, 3], E.SHAPE_SPHERE
    lo = np.concatenate([tris.min(axis=1), sph[:, :3] - sph[:, 3:]], axis=0).astype(D)
    hi = np.concatenate([tris.max(axis=1), sph[:, :3] + sph[:, 3:]], axis=0).astype(D)
    cen = 0.5 * (lo + hi)
    rmin, rmax = lo.min(axis=0), hi.max(axis=0)
    pad = 1.0e-4 * np.linalg.norm(rmax - rmin)
    ext = np.maximum((rmax + pad) - (rmin - pad), 1e-30)
    cell = (ext / (2.0 * GRID_HALF)).astype(F)
    grid_min = ((rmin - pad) + 0.5 * ext).astype(F)

    def planes(ids):
        a = (lo[ids].min(axis=0) - pad - grid_min.astype(D)) / cell.astype(D) - 1.0
        b = (hi[ids].max(axis=0) + pad - grid_min.astype(D)) / cell.astype(D) + 1.0
        ha, hb = a.astype(np.float16), b.astype(np.float16)
        ha = np.where(ha.astype(D) > a, np.nextafter(ha, np.float16(-np.inf)), ha)
        hb = np.where(hb.astype(D) < b, np.nextafter(hb, np.float16(np.inf)), hb)
        return ha.view(np.uint16).astype(np.uint32) | (hb.view(np.uint16).astype(np.uint32) << np.uint32(16))

    def halves(ids):
        if len(ids) < 2:
            return [ids]
        ax = int(np.argmax(cen[ids].max(axis=0) - cen[ids].min(axis=0)))
        order = ids[np.argsort(cen[ids, ax], kind="stable")]
        return [order[:len(order) // 2], order[len(order) // 2:]]

    def leaf_code(i):
        return ~(int(i) | ((1 << 30) if i >= T else 0))
    all_ids = np.arange(n)
    if n == 1:
        return {"wide_nodes": 0, "cnode": np.zeros((0, 16), np.uint32), "tri": rec, "grid_min": grid_min, "grid_cell": cell, "root_code": leaf_code(0)}
    nodes, queue = [], [all_ids]
    at = 0
    while at < len(queue):
        ids = queue[at]; at += 1
        parts = [q for h in halves(ids) for q in halves(h)]
        w = np.zeros(16, np.uint32)
        w[0:12] = np.tile(np.array([0x7b53 | (0xfb53 << 16)], np.uint32), 12)          # empty slots: an inverted box
        codes = np.full(4, TR_EMPTY, np.int64)
        for c, part in enumerate(parts):
            w[3 * c:3 * c + 3] = planes(part)
            if len(part) == 1:
                codes[c] = leaf_code(part[0])
            else:
                codes[c] = len(queue); queue.append(part)
        w[12:16] = codes.astype(np.int32).view(np.uint32)
        nodes.append(w)
    return {"wide_nodes": len(nodes), "cnode": np.stack(nodes), "tri": rec, "grid_min": grid_min, "grid_cell": cell, "root_code": 0}


# ---- meshes --------------------------------------------------------------------------------------------------------------------------------------
def torus_triangles(nu=40, nv=25, R=1.0, r=0.4, centre=(0.0, 0.0, 0.0)):
    """2 nu nv triangles of a torus about the z axis, oriented outward; one float32 position per vertex, shared by its triangles; [T, 3, 3] float64.
    Triangle 2 (i nv + j) + k lies in the quad of ring segment i (the angle about the axis) and tube segment j (0: the outer equator, upward)"""
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    P = np.stack([(R + r * np.cos(v)[None, :]) * np.cos(u)[:, None], (R + r * np.cos(v)[None, :]) * np.sin(u)[:, None],
                  np.broadcast_to(r * np.sin(v)[None, :], (nu, nv))], axis=2) + np.asarray(centre, D)
    P = P.astype(F).astype(D)
    tris = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = P[i, j], P[(i + 1) % nu, j], P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
            tris += [[a, b, c], [a, c, d]]
    return np.array(tris)


def torus_hole(nu=40, nv=25, ring=(0, 10), tube=(-5, 5)):
    """keep-mask [2 nu nv] of torus_triangles with a window removed: ring segments ring[0] .. ring[1] - 1, tube segments tube[0] .. tube[1] - 1 (mod nv):
    by default a quarter of the way round and the outer two fifths of the tube"""
    keep = np.ones((nu, nv, 2), bool)
    for i in range(ring[0], ring[1]):
        for j in range(tube[0], tube[1]):
            keep[i % nu, j % nv] = False
    return keep.reshape(-1)


ACCURACY_SEED = 20261022


def accuracy_queries(tris, n=2000, seed=ACCURACY_SEED):
    """n float32 points uniform in the mesh's box scaled by 1.5 about its centre: the queries of tools/winding_accuracy.py and of the accuracy test"""
    t = np.asarray(tris, D).reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    r = np.random.RandomState(seed)
    return (0.5 * (lo + hi) + 0.75 * (hi - lo) * r.uniform(-1, 1, (n, 3))).astype(F)
