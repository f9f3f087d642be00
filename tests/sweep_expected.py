"""The sphere-sweep definition of include/tirt.h ("Sphere sweep") restated in numpy, operation for operation: the contact time T, the feature code and
Q, u, v of a triangle and of an analytic sphere for a sphere of radius r whose centre moves along o + t d, the query's length m, and the brute-force answer
with its tie rule.  The arrays' dtype is the arithmetic's: float32 inputs give the definition itself (numpy rounds every elementwise operation once and
fuses nothing), float64 inputs the same expressions in double -- the ground truth test_sweep_host.py measures the definition's own rounding against.
Also here: the closest approach of a segment to a triangle in float64 (the distance to a convex set is convex along a line: a golden-section search),
which says whether a query grazes."""
import numpy as np

from closest_point_expected import dot, tri_point, sphere_point

TOL_REL = 2.0 ** -16
T_MIN = 2.0 ** -126                                    # what a candidate whose root is exactly 0 gets: T == 0 is kept for overlap at the start
GRID_CELLS = 60000.0                                   # 2 * TR_GRID_HALF: the padded root box spans this many cells


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def margin(grid_min, cell, o, r):
    """m of the query (o [..., 3], r [...]) on the grid (grid_min [3], cell [3]), in the arrays' dtype"""
    T = o.dtype.type
    gm, cell = np.asarray(grid_min, o.dtype), np.asarray(cell, o.dtype)
    with np.errstate(all="ignore"):
        C = max(max(cell[0], cell[1]), cell[2])
        iE = T(1) / (C * T(GRID_CELLS))
        rho_0 = max(max(abs(gm[0]), abs(gm[1])), abs(gm[2])) * iE
        rho_o = np.maximum(np.maximum(np.abs(o[..., 0] - gm[0]), np.abs(o[..., 1] - gm[1])), np.abs(o[..., 2] - gm[2])) * iE
        rho_q = rho_o + r * iE
        return ((T(0.5) + T(0.5) * (rho_q + rho_0)) * C).astype(o.dtype)


def valid(o, d, r, B):
    with np.errstate(all="ignore"):
        return np.isfinite(o).all(axis=-1) & np.isfinite(d).all(axis=-1) & (r >= 0) & (r < np.inf) & (B >= 0)


def _terms(o, d, r, m):
    T = o.dtype.type
    r2 = r * r
    tol = r * T(TOL_REL) + m
    rh = r + tol
    return r2, rh * rh, dot(d, d)


def _root(a, b, c, ok, sg):
    T = a.dtype.type
    disc = b * b - a * c
    go = ok & (a > T(0)) & (disc >= T(0))
    t = (-b + sg * np.sqrt(np.where(go, disc, T(0)))) / np.where(go, a, T(1))
    return np.where(go, t, T(np.inf))


def _edge(d, nn, r2, m, mm, md, e):
    T = d.dtype.type
    me, de, ee = dot(m, e), dot(d, e), dot(e, e)
    A = ee * nn - de * de
    k = mm - r2
    C = ee * k - me * me
    Bq = ee * md - de * me
    t = _root(A, Bq, C, np.ones(A.shape, bool), T(-1))
    ax = me + t * de
    return np.where((t >= T(0)) & (ax >= T(0)) & (ax <= ee), t, T(np.inf))


def _corner(nn, r2, mm, md):
    T = nn.dtype.type
    t = _root(nn, md, mm - r2, np.ones(mm.shape, bool), T(-1))
    return np.where(t >= T(0), t, T(np.inf))


def tri_sweep(o, d, r, m, B, a, b, c):
    """o, d, a, b, c broadcastable [..., 3], r, m, B broadcastable [...], one float dtype -> T, code (int32), Q [..., 3], u, v, D2 of the verifying call;
    a miss: (+inf, -1, 0, 0, 0, 0).  Rows that are not valid() are the caller's business."""
    T = o.dtype.type
    zero, inf = T(0), T(np.inf)
    shape = np.broadcast(o[..., 0], a[..., 0], r, m, B).shape
    bc3 = lambda x: np.broadcast_to(x, shape + (3,))
    o, d, a, b, c = (bc3(x) for x in (o, d, a, b, c))
    r, m, B = (np.broadcast_to(x, shape) for x in (r, m, B))
    with np.errstate(all="ignore"):
        r2, rhi2, nn = _terms(o, d, r, m)
        c0 = tri_point(o, a, b, c)
        over = c0[0] <= r2
        ab, ac, bc, ca = b - a, c - a, c - b, a - c
        ma, mb, mc = o - a, o - b, o - c
        maa, mbb, mcc = dot(ma, ma), dot(mb, mb), dot(mc, mc)
        mad, mbd, mcd = dot(ma, d), dot(mb, d), dot(mc, d)
        # code 1
        n = cross(ab, ac)
        n2, s, nd = dot(n, n), dot(n, ma), dot(n, d)
        sg = np.where(s < zero, T(-1), T(1))
        hh, vv = s * sg, nd * sg
        go = (n2 > zero) & (vv < zero)
        rl = r * np.sqrt(n2)
        go = go & (hh >= rl)
        t = (hh - rl) / np.where(go, -vv, T(1))
        p = o + d * np.where(go, t, zero)[..., None]
        e0, e1, e2 = dot(cross(ab, p - a), n), dot(cross(bc, p - b), n), dot(cross(ca, p - c), n)
        t1 = np.where(go & (e0 >= zero) & (e1 >= zero) & (e2 >= zero), t, inf)
        cand = [t1, _edge(d, nn, r2, ma, maa, mad, ab), _edge(d, nn, r2, mb, mbb, mbd, bc), _edge(d, nn, r2, mc, mcc, mcd, ca),
                _corner(nn, r2, maa, mad), _corner(nn, r2, mbb, mbd), _corner(nn, r2, mcc, mcd)]
        cand = [np.where(x == zero, T(T_MIN), x) for x in cand]
        cand = np.stack([np.where((x >= zero) & (x <= B), x, inf) for x in cand], axis=-1)      # [..., 7]
        out_t = np.full(shape, inf, o.dtype); out_code = np.full(shape, -1, np.int32)
        out_q = np.zeros(shape + (3,), o.dtype); out_u = np.zeros(shape, o.dtype); out_v = np.zeros(shape, o.dtype); out_d2 = np.zeros(shape, o.dtype)
        done = over.copy()
        for _ in range(7):
            km = cand.argmin(axis=-1)                                  # the first of the smallest: ties go to the lower code
            tm = np.take_along_axis(cand, km[..., None], axis=-1)[..., 0]
            go = ~done & (tm < inf)
            if not go.any():
                break
            idx = np.nonzero(go)
            tg = tm[idx]
            v = tri_point(o[idx] + d[idx] * tg[:, None], a[idx], b[idx], c[idx])
            acc = v[0] <= rhi2[idx]
            hit = tuple(i[acc] for i in idx)
            out_t[hit] = tg[acc]; out_code[hit] = km[idx][acc] + 1
            out_d2[hit] = v[0][acc]; out_q[hit] = v[1][acc]; out_u[hit] = v[2][acc]; out_v[hit] = v[3][acc]
            done[hit] = True
            cand[idx + (km[idx],)] = inf                               # struck out (an accepted row is done anyway)
        out_t[over] = zero; out_code[over] = 0
        out_d2[over] = c0[0][over]; out_q[over] = c0[1][over]; out_u[over] = c0[2][over]; out_v[over] = c0[3][over]
    return out_t, out_code, out_q, out_u, out_v, out_d2


def sphere_sweep(o, d, r, m, B, C, R):
    """the same for an analytic sphere: C [..., 3], R [...]"""
    T = o.dtype.type
    zero, inf = T(0), T(np.inf)
    shape = np.broadcast(o[..., 0], C[..., 0], r, m, B, R).shape
    bc3 = lambda x: np.broadcast_to(x, shape + (3,))
    o, d, C = (bc3(x) for x in (o, d, C))
    r, m, B, R = (np.broadcast_to(x, shape) for x in (r, m, B, R))
    with np.errstate(all="ignore"):
        r2, rhi2, nn = _terms(o, d, r, m)
        c0 = sphere_point(o, C, R)
        over = c0[0] <= r2
        mm_ = o - C
        mm, md = dot(mm_, mm_), dot(mm_, d)
        Ro, Ri = R + r, R - r
        co, ci = mm - Ro * Ro, mm - Ri * Ri
        outside = co > zero
        inside = (Ri > zero) & (ci < zero)
        t = _root(nn, md, np.where(outside, co, ci), outside | inside, np.where(outside, T(-1), T(1)))
        t = np.where(t == zero, T(T_MIN), t)
        go = ~over & (t >= zero) & (t <= B) & (t < inf)
        v = sphere_point(o + d * np.where(go, t, zero)[..., None], C, R)
        acc = go & (v[0] <= rhi2)
        out_t = np.where(over, zero, np.where(acc, t, inf)).astype(o.dtype)
        out_code = np.where(over, 0, np.where(acc, np.where(outside, 8, 9), -1)).astype(np.int32)
        pick = lambda x0, x1: np.where(over, x0, np.where(acc, x1, zero)).astype(o.dtype)
        q = np.where(over[..., None], c0[1], np.where(acc[..., None], v[1], zero)).astype(o.dtype)
    return out_t, out_code, q, np.zeros(shape, o.dtype), np.zeros(shape, o.dtype), pick(c0[0], v[0])


def _rows(n, parts):
    cols = []
    for x, w in parts:
        cols.append(np.broadcast_to(np.asarray(x, np.float32).reshape(-1, w), (n, w)))
    return np.ascontiguousarray(np.concatenate(cols, axis=1), np.float32)


def tri_rows(o, d, r, m, B, a, b, c):
    """the rows tirt_kat_sweep[_host] takes for triangles: (o3, d3, r, m, B, a3, b3, c3) [n, 18] float32; every argument broadcasts over the rows"""
    n = max(np.asarray(x).size // w for x, w in ((o, 3), (d, 3), (r, 1), (m, 1), (B, 1), (a, 3), (b, 3), (c, 3)))
    return _rows(n, ((o, 3), (d, 3), (r, 1), (m, 1), (B, 1), (a, 3), (b, 3), (c, 3)))


def sphere_rows(o, d, r, m, B, C, R):
    """... and for analytic spheres: (o3, d3, r, m, B, C3, R) [n, 13]"""
    n = max(np.asarray(x).size // w for x, w in ((o, 3), (d, 3), (r, 1), (m, 1), (B, 1), (C, 3), (R, 1)))
    return _rows(n, ((o, 3), (d, 3), (r, 1), (m, 1), (B, 1), (C, 3), (R, 1)))


def kat_expected(rows, is_sphere=False, dtype=np.float32):
    """what tirt_kat_sweep[_host] returns for `rows`, by the restatement in `dtype`: [n, 8] (T, code, Q3, u, v, D2); a miss and an invalid row: (+inf, -1, 0 ...)"""
    rows = np.asarray(rows, np.float32).astype(dtype)
    o, d, r, m, B = rows[:, 0:3], rows[:, 3:6], rows[:, 6], rows[:, 7], rows[:, 8]
    if is_sphere:
        t, code, q, u, v, d2 = sphere_sweep(o, d, r, m, B, rows[:, 9:12], rows[:, 12])
    else:
        t, code, q, u, v, d2 = tri_sweep(o, d, r, m, B, rows[:, 9:12], rows[:, 12:15], rows[:, 15:18])
    out = np.concatenate([t[:, None], code[:, None].astype(dtype), q, u[:, None], v[:, None], d2[:, None]], axis=1)
    bad = ~valid(o, d, r, B)
    out[bad] = 0
    out[bad, 0] = np.inf; out[bad, 1] = -1
    return out


def normal(o, d, t, q, hit):
    """the unit vector from Q to c(T), 0 where they coincide and for a miss"""
    T = o.dtype.type
    with np.errstate(all="ignore"):
        w = (o + d * np.where(hit, t, T(0))[..., None]) - q
        l2 = dot(w, w)
        go = hit & (l2 > T(0))
        inv = T(1) / np.sqrt(np.where(go, l2, T(1)))
        return np.where(go[..., None], w * inv[..., None], T(0)).astype(o.dtype)


def brute_force(rays, radius, tmax, geom, grid_min, cell, block=128, dtype=np.float32, m=None):
    """The answer of the definition for every row of rays [N, 6]: a dict of t, prim, code [N], point [N, 3], uv [N, 2], normal [N, 3], d2 [N] (the
    verifying call's).  geom: closest_point_expected.Geometry; grid_min, cell: the scene's grid (Context.wide_tree_download), or m given directly.
    Among T <= B the smallest T, at equal bits the smallest primitive id; nothing: (+inf, -1, -1, 0 ...)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6).astype(dtype)
    n = rays.shape[0]
    T = rays.dtype.type
    o, d = rays[:, 0:3], rays[:, 3:6]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), (n,))).astype(dtype)
    B = np.ascontiguousarray(np.broadcast_to(np.asarray(np.inf if tmax is None else tmax, np.float32), (n,))).astype(dtype)
    ok = valid(o, d, r, B)
    m = margin(grid_min, cell, o, r) if m is None else np.broadcast_to(np.asarray(m, dtype), (n,))
    out = dict(t=np.full(n, np.inf, dtype), prim=np.full(n, -1, np.int32), code=np.full(n, -1, np.int32), point=np.zeros((n, 3), dtype),
               uv=np.zeros((n, 2), dtype), normal=np.zeros((n, 3), dtype), d2=np.zeros(n, dtype))
    prim_all = np.concatenate([geom.tri_prim, geom.sphere_prim]).astype(np.int64)
    tris, sph = geom.tris.astype(dtype), geom.spheres.astype(dtype)
    for s in range(0, n, block):
        sl = slice(s, s + block)
        q = lambda x: x[sl, None]
        parts = []
        if tris.shape[0]:
            parts.append(tri_sweep(o[sl, None, :], d[sl, None, :], q(r), q(m), q(B), tris[None, :, 0], tris[None, :, 1], tris[None, :, 2]))
        if sph.shape[0]:
            parts.append(sphere_sweep(o[sl, None, :], d[sl, None, :], q(r), q(m), q(B), sph[None, :, 0:3], sph[None, :, 3]))
        t, code, pt, u, v, d2 = (np.concatenate([x[k] for x in parts], axis=1) for k in range(6))
        with np.errstate(invalid="ignore"):
            acc = (t <= B[sl, None]) & (t < T(np.inf)) & ok[sl, None]
        key = np.where(acc, t, T(np.inf))
        best = key.min(axis=1)
        tie = acc & (key == best[:, None])
        col = np.where(tie, prim_all[None, :], np.int64(1) << 40).argmin(axis=1)
        found = tie.any(axis=1)
        rows = np.arange(t.shape[0])
        out["t"][sl] = np.where(found, t[rows, col], T(np.inf))
        out["prim"][sl] = np.where(found, prim_all[col], -1)
        out["code"][sl] = np.where(found, code[rows, col], -1)
        out["point"][sl] = np.where(found[:, None], pt[rows, col], T(0))
        out["uv"][sl] = np.where(found[:, None], np.stack([u[rows, col], v[rows, col]], axis=1), T(0))
        out["d2"][sl] = np.where(found, d2[rows, col], T(0))
    out["normal"] = normal(o, d, out["t"], out["point"], out["prim"] >= 0)
    return out


def closest_approach(o, d, B, a, b, c, iters=48):
    """float64: the smallest distance between the segment o + t d, 0 <= t <= B (finite), and the triangle, by a golden-section search on the distance,
    which is convex in t.  Everything broadcastable; -> [...]"""
    o, d, a, b, c = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    f = lambda t: tri_point(o + d * t[..., None], a, b, c)[0]
    shape = np.broadcast(o[..., 0], a[..., 0]).shape
    lo = np.zeros(shape); hi = np.broadcast_to(np.asarray(B, np.float64), shape).copy()
    g = (np.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(iters):
        left = f1 < f2
        hi = np.where(left, x2, hi); lo = np.where(left, lo, x1)
        nx1, nx2 = hi - g * (hi - lo), lo + g * (hi - lo)
        x1n = np.where(left, nx1, x2); x2n = np.where(left, x1, nx2)
        fn = f(np.where(left, nx1, nx2))
        f1, f2 = np.where(left, fn, f2), np.where(left, f1, fn)
        x1, x2 = x1n, x2n
    return np.sqrt(np.minimum(np.minimum(f1, f2), np.minimum(f(lo), f(hi))))


# ---- the two input sets of the accuracy test (test_sweep_host.py; tools/sweep_accuracy.py writes profiles/sweep_accuracy.txt from the same functions) ----
# measured: max |T32 - T64| |d| over the kept queries, as tools/sweep_accuracy.py found it on these inputs (profiles/sweep_accuracy.txt); the test allows twice that
ACCURACY_SETS = {"dense": dict(seed=101, ntri=64, r=0.05, nseg=1500, measured=1.7832e-05),
                 "sparse": dict(seed=202, ntri=12, r=0.02, nseg=1500, measured=1.5674e-05)}
UNIT_GRID = (np.full(3, 0.5, np.float32), np.full(3, np.float32(2.0) / np.float32(GRID_CELLS), np.float32))      # grid_min, cell of the box [-0.5, 1.5]^3
GRAZE = 2.0 ** -8


def accuracy_inputs(which):
    """-> Geometry (triangles in the unit box, edges below 0.4), rays [n, 6] float32 (o, d = p1 - o) with end points in [-0.2, 1.2]^3, r; B = 1"""
    from closest_point_expected import Geometry
    cfg = ACCURACY_SETS[which]
    rs = np.random.RandomState(cfg["seed"])
    centre = rs.uniform(0.115, 0.885, (cfg["ntri"], 1, 3))
    tris = (centre + rs.uniform(-0.115, 0.115, (cfg["ntri"], 3, 3))).astype(np.float32)      # every edge < 0.23 sqrt(3) < 0.4
    p0 = rs.uniform(-0.2, 1.2, (cfg["nseg"], 3)).astype(np.float32)
    p1 = rs.uniform(-0.2, 1.2, (cfg["nseg"], 3)).astype(np.float32)
    return Geometry(tris, np.arange(cfg["ntri"])), np.concatenate([p0, p1 - p0], axis=1), np.float32(cfg["r"])


def accuracy_measure(which, kat_host):
    """kat_host: ti_raytrace_amd._native.kat_sweep_host.  -> dict: left_out (share of grazing queries), n_kept, disagree (kept queries whose float32 and
    float64 answers differ in prim), max_err = max |T32 - T64| |d| over the kept queries with a contact, contacts (kept queries with one)"""
    geom, rays, r = accuracy_inputs(which)
    n, nt = rays.shape[0], geom.tris.shape[0]
    m = margin(UNIT_GRID[0], UNIT_GRID[1], rays[:, 0:3], np.full(n, r, np.float32))
    # float32: the host text on every (query, triangle) row, then the rule across primitives
    o = np.repeat(rays[:, 0:3], nt, axis=0); d = np.repeat(rays[:, 3:6], nt, axis=0)
    rows = tri_rows(o, d, r, np.repeat(m, nt), 1.0, np.tile(geom.tris[:, 0], (n, 1)), np.tile(geom.tris[:, 1], (n, 1)), np.tile(geom.tris[:, 2], (n, 1)))
    t32 = kat_host(rows)[:, 0].reshape(n, nt)
    T32 = t32.min(axis=1)
    P32 = np.where(np.isfinite(T32), t32.argmin(axis=1), -1)      # (argmin: the first of the smallest = the smallest id)
    want = brute_force(rays, r, 1.0, geom, None, None, dtype=np.float64, m=m.astype(np.float64))
    ca = closest_approach(rays[:, None, 0:3], rays[:, None, 3:6], 1.0, geom.tris[None, :, 0], geom.tris[None, :, 1], geom.tris[None, :, 2])
    graze = (np.abs(ca - float(r)) <= float(r) * GRAZE).any(axis=1)
    keep = ~graze
    both = keep & (P32 >= 0) & (want["prim"] >= 0)
    dlen = np.sqrt((rays[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    err = np.abs(T32.astype(np.float64)[both] - want["t"][both]) * dlen[both]
    return dict(left_out=float(graze.mean()), n_kept=int(keep.sum()), disagree=int((P32 != want["prim"])[keep].sum()),
                max_err=float(err.max()) if err.size else 0.0, contacts=int(both.sum()))
