"""The closest-point definition of include/tirt.h ("Closest point") restated in numpy, operation for operation: D2 / Q / u / v of a triangle (Ericson 5.1.5,
regions in the book's order through np.select) and of an analytic sphere, and the brute-force answer with its tie rule.  The arrays' dtype is the
arithmetic's: float32 inputs give the definition itself (numpy rounds every elementwise operation once and fuses nothing), float64 inputs the same
expressions in double, which is what test_closest_point_host.py measures the definition's own rounding against."""
import numpy as np

SHAPE_SPHERE = 1
PRIMITIVE_TRI = 1

# one point per region of the triangle a = (0,0,0), b = (2,0,0), c = (0,2,0), worked out by hand (every number below is exact in fp32):
#   name, p, Q, (u, v), D2
A_, B_, C_ = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
HAND = [
    ("A", (-1.0, -1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0), 3.0),
    ("B", (3.0, -1.0, 0.0), (2.0, 0.0, 0.0), (1.0, 0.0), 2.0),
    ("AB", (0.5, -1.0, 0.0), (0.5, 0.0, 0.0), (0.25, 0.0), 1.0),
    ("C", (-1.0, 3.0, 0.0), (0.0, 2.0, 0.0), (0.0, 1.0), 2.0),
    ("AC", (-1.0, 0.5, 0.0), (0.0, 0.5, 0.0), (0.0, 0.25), 1.0),
    ("BC", (2.0, 2.0, 0.0), (1.0, 1.0, 0.0), (0.5, 0.5), 2.0),
    ("interior", (0.5, 0.5, 3.0), (0.5, 0.5, 0.0), (0.25, 0.25), 9.0),
]


def hand_rows():
    """the seven rows as (p, a, b, c) float32 [7, 12] and their answers [7, 6] (d2, q3, u, v): shared with the device's known-answer test"""
    rows = np.array([list(p) + list(A_) + list(B_) + list(C_) for _, p, _, _, _ in HAND], np.float32)
    want = np.array([[d2] + list(q) + list(uv) for _, _, q, uv, d2 in HAND], np.float32)
    return rows, want


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_point(p, a, b, c):
    """p, a, b, c broadcastable [..., 3] of one float dtype -> D2 [...], Q [..., 3], u [...], v [...]"""
    T = p.dtype.type
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= zero) & (d2 <= zero),                       # A
                 (d3 >= zero) & (d4 <= d3),                         # B
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),        # AB
                 (d6 >= zero) & (d5 <= d6),                         # C
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),        # AC
                 (va <= zero) & (e43 >= zero) & (e56 >= zero)]      # BC
        u_ab = d1 / (d1 - d3)
        v_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        den = one / ((va + vb) + vc)
        u_in, v_in = vb * den, vc * den
        shape = np.broadcast(d1, d1).shape
        full = lambda x: np.broadcast_to(x, shape + (3,))
        zeros, ones = np.zeros(shape, p.dtype), np.ones(shape, p.dtype)
        q_choices = [full(a), full(b), a + ab * u_ab[..., None], full(c), a + ac * v_ac[..., None], b + (c - b) * w_bc[..., None]]
        q_in = (a + ab * u_in[..., None]) + ac * v_in[..., None]
        u = np.select(conds, [zeros, ones, u_ab, zeros, zeros, one - w_bc], u_in)
        v = np.select(conds, [zeros, zeros, zeros, ones, v_ac, w_bc], v_in)
        q = np.stack([np.select(conds, [qc[..., k] for qc in q_choices], q_in[..., k]) for k in range(3)], axis=-1)
        pq = p - q
        return dot(pq, pq), q, u, v


def region(p, a, b, c):
    """0..6 = A, B, AB, C, AC, BC, interior (for the tests that want to know where a point fell)"""
    T = p.dtype.type
    zero = T(0)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= zero) & (d2 <= zero), (d3 >= zero) & (d4 <= d3), (vc <= zero) & (d1 >= zero) & (d3 <= zero), (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero), (va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero)]
        return np.select(conds, list(range(6)), 6)


def sphere_point(p, c, r):
    """p, c [..., 3], r [...] -> D2, Q, u, v"""
    T = p.dtype.type
    with np.errstate(all="ignore"):
        pc = p - c
        ln = np.sqrt(dot(pc, pc))
        d = ln - r
        d = np.where(d < T(0), -d, d)
        d2 = d * d
        q = c + pc * (r / ln)[..., None]
        at_centre = (ln == T(0))[..., None]
        q0 = c + np.stack([r, np.zeros_like(r), np.zeros_like(r)], axis=-1)
        q = np.where(at_centre, np.broadcast_to(q0, q.shape), q)
        z = np.zeros(d2.shape, p.dtype)
        return d2, q, z, z


def limit2(dmax):
    """lim2 of the definition: dmax * dmax in float32, -1 (nothing is found) for a negative or NaN dmax"""
    dmax = np.asarray(dmax, np.float32)
    with np.errstate(all="ignore"):
        return np.where(dmax >= np.float32(0), dmax * dmax, np.float32(-1.0)).astype(np.float32)


class Geometry:
    """the surfaces of a scene, from its host arrays: triangles [nt, 3, 3] with their primitive ids, spheres [ns, 4] (centre, radius) with theirs"""

    def __init__(self, tris, tri_prim, spheres=None, sphere_prim=None):
        self.tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        self.tri_prim = np.asarray(tri_prim, np.int32)
        self.spheres = np.zeros((0, 4), np.float32) if spheres is None else np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        self.sphere_prim = np.zeros(0, np.int32) if sphere_prim is None else np.asarray(sphere_prim, np.int32)


def scene_geometry(scene, vertex=None):
    """Geometry of a ti_raytrace_amd Scene after setup_data_cpu (vertex: other vertex rows than the scene's own)"""
    prim = scene.primitive_np
    vert = np.asarray(scene.vertex_np if vertex is None else vertex, np.float32)
    is_tri = prim[:, 0] == PRIMITIVE_TRI
    tp = np.nonzero(is_tri)[0]
    first = prim[tp, 1]
    tris = np.stack([vert[first, 0:3], vert[first + 1, 0:3], vert[first + 2, 0:3]], axis=1)
    sp, sg = [], []
    for i in np.nonzero(~is_tri)[0]:
        sh = scene.shape_np[prim[i, 1]]
        if int(sh[0]) == SHAPE_SPHERE:
            sp.append(i); sg.append([sh[1], sh[2], sh[3], sh[4]])
    return Geometry(tris, tp, np.asarray(sg, np.float32).reshape(-1, 4), np.asarray(sp, np.int32))


def brute_force(points, geom, dmax=None, block=256):
    """The answer of the definition for every row of points [N, 3] float32: (d2 [N], prim [N], point [N, 3], uv [N, 2]).
    Among D2 <= lim2 (and D2 < +inf, never NaN) the smallest D2, at equal bits the smallest primitive id; nothing: (+inf, -1, 0, 0)."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = points.shape[0]
    lim2 = limit2(np.full(n, np.inf, np.float32) if dmax is None else np.broadcast_to(np.asarray(dmax, np.float32), (n,)))
    out_d2 = np.full(n, np.inf, np.float32); out_prim = np.full(n, -1, np.int32)
    out_q = np.zeros((n, 3), np.float32); out_uv = np.zeros((n, 2), np.float32)
    a, b, c = (geom.tris[None, :, k, :] for k in range(3))
    prim_all = np.concatenate([geom.tri_prim, geom.sphere_prim]).astype(np.int64)
    for s in range(0, n, block):
        p = points[s:s + block, None, :]
        parts = []
        if geom.tris.shape[0]:
            parts.append(tri_point(p, a, b, c))
        if geom.spheres.shape[0]:
            parts.append(sphere_point(p, geom.spheres[None, :, 0:3], np.broadcast_to(geom.spheres[None, :, 3], (p.shape[0], geom.spheres.shape[0]))))
        d2 = np.concatenate([x[0] for x in parts], axis=1)
        q = np.concatenate([x[1] for x in parts], axis=1)
        u = np.concatenate([x[2] for x in parts], axis=1)
        v = np.concatenate([x[3] for x in parts], axis=1)
        with np.errstate(invalid="ignore"):
            ok = (d2 <= lim2[s:s + block, None]) & (d2 < np.float32(np.inf))
        key = np.where(ok, d2, np.float32(np.inf))
        best = key.min(axis=1)
        tie = ok & (key == best[:, None])
        pid = np.where(tie, prim_all[None, :], np.int64(1) << 40)
        col = pid.argmin(axis=1)
        found = tie.any(axis=1)
        rows = np.arange(p.shape[0])
        out_d2[s:s + block] = np.where(found, d2[rows, col], np.float32(np.inf))
        out_prim[s:s + block] = np.where(found, prim_all[col], -1)
        out_q[s:s + block] = np.where(found[:, None], q[rows, col], np.float32(0))
        out_uv[s:s + block] = np.where(found[:, None], np.stack([u[rows, col], v[rows, col]], axis=1), np.float32(0))
    return out_d2, out_prim, out_q, out_uv
