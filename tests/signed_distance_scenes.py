"""The meshes of the signed-distance tests, written as OBJ files and read back through Scene.add_obj (host side only; build_scene is the step onto a device):
1 cube, 2 lprism (an L-shaped prism: one concave edge, two saddle vertices), 3 icosphere (80 triangles), 4 union (cube + L-prism, disjoint, + one analytic
sphere), 5 quad (open), 6 cube_flipped (one triangle's winding reversed), 7 cube_degenerate (one zero-area triangle added).  Every mesh is oriented
outward; the truth the tests hold the signs to never looks at a normal: analytic inside tests and the generalised winding number in float64."""
import os

import numpy as np

import closest_point_expected as E
from ti_raytrace_amd import Example, PT_RGB

F = np.float32
NAMES = ("cube", "lprism", "icosphere", "union", "quad", "cube_flipped", "cube_degenerate")
CLOSED = ("cube", "lprism", "icosphere", "union")
CUBE_LO, CUBE_HI = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0])
L_OFFSET = np.array([3.0, 0.0, 0.0])          # where the L-prism stands in `union`
L_HEIGHT = 1.5
L_POLY = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)      # counter-clockwise; corner 3 is the concave one
UNION_SPHERE = (1.0, 3.5, 0.5, 0.75)          # centre, radius


def cube_triangles(lo=CUBE_LO, hi=CUBE_HI):
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64) * (hi - lo) + lo      # index = x + 2y + 4z
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return np.array([[v[q[0]], v[q[i]], v[q[i + 1]]] for q in quads for i in (1, 2)])


def lprism_triangles(offset=(0.0, 0.0, 0.0), h=L_HEIGHT):
    bot = np.concatenate([L_POLY, np.zeros((6, 1))], axis=1) + offset
    top = bot + np.array([0.0, 0.0, h])
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)]            # corners of the polygon only: no T-junctions
    tris = [[top[i], top[j], top[k]] for i, j, k in cap] + [[bot[i], bot[k], bot[j]] for i, j, k in cap]
    for i in range(6):
        j = (i + 1) % 6
        tris += [[bot[i], bot[j], top[j]], [bot[i], top[j], top[i]]]
    return np.array(tris)


def icosphere_triangles(radius=1.0, centre=(0.0, 0.0, 0.0), levels=1):
    """an icosahedron subdivided `levels` times (80, 320, 1280 ... triangles), every vertex pushed out to the sphere"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    mid = {}

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            m = v[i] + v[j]
            v.append(m / np.linalg.norm(m)); mid[key] = len(v) - 1
        return mid[key]
    out = f
    for _ in range(levels):
        f, out = out, []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    P = (np.array(v) * radius + np.asarray(centre)).astype(F).astype(np.float64)      # one float32 position per vertex, shared by its triangles
    tris = np.array([[P[i], P[j], P[k]] for i, j, k in out])
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    flip = (n * (tris.mean(axis=1) - np.asarray(centre))).sum(axis=1) < 0
    tris[flip] = tris[flip][:, ::-1]
    assert tris.shape == (20 * 4 ** levels, 3, 3)
    return tris


def mesh_triangles(name):
    """[T, 3, 3] float64 of values that float32 holds exactly"""
    if name == "cube":
        return cube_triangles()
    if name == "lprism":
        return lprism_triangles()
    if name == "icosphere":
        return icosphere_triangles()
    if name == "union":
        return np.concatenate([cube_triangles(), lprism_triangles(L_OFFSET)], axis=0)
    if name == "quad":
        return np.array([[[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5]], [[0, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]]], np.float64)
    if name == "cube_flipped":
        t = cube_triangles()
        t[5] = t[5][::-1]
        return t
    if name == "cube_degenerate":                            # a sliver along the cube's edge (0,0,0)-(1,0,0): collinear corners, zero area
        return np.concatenate([cube_triangles(), np.array([[[0, 0, 0], [1, 0, 0], [0.5, 0, 0]]], np.float64)], axis=0)
    raise KeyError(name)


def write_obj(path, tris):
    """a triangle soup as an OBJ with one grey material (positions with nine digits: float32 values survive)"""
    base = os.path.splitext(os.path.basename(path))[0]
    with open(os.path.join(os.path.dirname(path), base + ".mtl"), "w") as f:
        f.write("newmtl grey\nKd 0.8 0.8 0.8\nd 1.0\n")
    with open(path, "w") as f:
        f.write("mtllib %s.mtl\n" % base)
        for p in tris.reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % tuple(p))
        f.write("usemtl grey\n")
        for k in range(tris.shape[0]):
            f.write("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))


def make_scene(name, tmp_dir, tris=None, device_id=0):
    """the example scene of mesh `name` (or of other triangles under that name's rules), read from an OBJ in tmp_dir; host data set up, nothing on a device"""
    tris = mesh_triangles(name) if tris is None else tris
    path = os.path.join(str(tmp_dir), name + ".obj")
    write_obj(path, tris)
    ex = Example.example(24, 24, 4, device_id)
    ex.scene.add_obj(path)
    if name == "union":
        x, y, z, r = UNION_SPHERE
        ex.add_sphere_light(pos=(x, y, z), radius=r, emission=50.0)
    ex.integrator = PT_RGB.PathTrace(24, 24, ex.cam, ex.scene, 64)
    ex.scene.setup_data_cpu()
    geom = E.scene_geometry(ex.scene)
    assert np.array_equal(geom.tris, tris.astype(F)), "the OBJ round trip changed the triangles"
    return ex, geom


# ---- truth that never looks at a normal ------------------------------------------------------------------------------------------------------
def inside_box(p, lo, hi):
    return ((p > lo) & (p < hi)).all(axis=1)


def inside_lprism(p, offset=(0.0, 0.0, 0.0), h=L_HEIGHT):
    q = p - np.asarray(offset)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return (z > 0) & (z < h) & (((x > 0) & (x < 2) & (y > 0) & (y < 1)) | ((x > 0) & (x < 1) & (y > 0) & (y < 2)))


def inside_sphere(p, sphere):
    return ((p - np.asarray(sphere[:3])) ** 2).sum(axis=1) < sphere[3] ** 2


def inside_analytic(name, p):
    """float64 points -> bool, or None where the mesh has no closed form (the icosphere)"""
    p = np.asarray(p, np.float64)
    if name == "cube":
        return inside_box(p, CUBE_LO, CUBE_HI)
    if name == "lprism":
        return inside_lprism(p)
    if name == "union":
        return inside_box(p, CUBE_LO, CUBE_HI) | inside_lprism(p, L_OFFSET) | inside_sphere(p, UNION_SPHERE)
    return None


def winding_number(p, tris):
    """the generalised winding number of float64 points about a triangle mesh: the sum of the signed solid angles (Van Oosterom & Strackee 1983) / 4 pi"""
    p = np.asarray(p, np.float64)
    w = np.zeros(p.shape[0])
    for t in np.asarray(tris, np.float64):
        a, b, c = t[0] - p, t[1] - p, t[2] - p
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        det = (a * np.cross(b, c)).sum(axis=1)
        den = la * lb * lc + (a * b).sum(axis=1) * lc + (b * c).sum(axis=1) * la + (c * a).sum(axis=1) * lb
        w += 2.0 * np.arctan2(det, den)
    return w / (4.0 * np.pi)


def inside_truth(name, p):
    """inside by the winding number of the triangle meshes (> 1/2) or the analytic sphere; checked against the closed forms where there are some"""
    p = np.asarray(p, np.float64)
    ins = winding_number(p, mesh_triangles(name)) > 0.5
    if name == "union":
        ins = ins | inside_sphere(p, UNION_SPHERE)
    return ins


# ---- queries ---------------------------------------------------------------------------------------------------------------------------------
SEED = 20261020


def scene_box(geom):
    t = geom.tris.astype(np.float64).reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    if geom.spheres.shape[0]:
        s = geom.spheres.astype(np.float64)
        lo, hi = np.minimum(lo, (s[:, :3] - s[:, 3:]).min(axis=0)), np.maximum(hi, (s[:, :3] + s[:, 3:]).max(axis=0))
    return lo, hi


def uniform_queries(geom, n=4096, seed=SEED):
    """n float32 points uniform in the scene box scaled by 1.5 about its centre"""
    lo, hi = scene_box(geom)
    r = np.random.RandomState(seed)
    return (0.5 * (lo + hi) + 0.75 * (hi - lo) * r.uniform(-1, 1, (n, 3))).astype(F)


def concave_edge_queries(offset=(0.0, 0.0, 0.0), n=180, seed=SEED + 1):
    """Points INSIDE the L-prism whose nearest surface point lies on its concave edge x = y = 1: a third in the plane y = 1 (x < 1), a third in the
    plane x = 1 (y < 1), a third between the two.  In such a plane p - Q is perpendicular to the normal of the face that lies in it: that face's own
    normal says s == 0, "outside", and the triangle of ONE of the two faces wins the tie at the edge -- for one of the two thirds the winner's normal is wrong."""
    r = np.random.RandomState(seed)
    a, b = r.uniform(0.05, 0.4, n), r.uniform(0.05, 0.4, n)
    z = r.uniform(0.45, L_HEIGHT - 0.45, n)
    group = np.arange(n) * 3 // n
    dx = np.where(group == 2, 0.0, a)
    dy = np.where(group == 0, 0.0, b)
    return (np.stack([1.0 - dx, 1.0 - dy, z], axis=1) + np.asarray(offset)).astype(F)


def cube_corner_queries(n=64, seed=SEED + 2):
    """points outside the cube whose nearest surface point is one of its corners or lies on one of its edges, at distances 0.02 .. 0.3"""
    r = np.random.RandomState(seed)
    corner = r.randint(0, 2, (n, 3)).astype(np.float64)
    out = (2.0 * corner - 1.0) * r.uniform(0.02, 0.3, (n, 3))
    out[n // 2:, 0] = 0.0                                    # the second half: in the plane of a face, beside an edge
    p = corner + out
    p[n // 2:, 0] = r.uniform(0.2, 0.8, n - n // 2)
    return p.astype(F)


def queries(name, geom):
    parts = [uniform_queries(geom)]
    if name == "cube":
        parts.append(cube_corner_queries())
    if name == "lprism":
        parts.append(concave_edge_queries())
    if name == "union":
        parts += [cube_corner_queries(), concave_edge_queries(L_OFFSET)]
    return np.concatenate(parts, axis=0)


# ---- one mesh with everything the tests compare against, made once per process ----------------------------------------------------------------
_CASES = {}
THRESHOLD = 1.0e-4                                            # of the scene's extent: nearer the surface than this no sign is asked for
CAP = 0.01                                                    # at most this share of the queries may be that near


def case(name, tmp_dir):
    """dict: ex (host data set up, not on a device), geom, tab (the restatement's table), and for the closed meshes pts, want = (sd, d2, prim, q, uv) of the
    restatement, truth (inside, without normals), far (D2 above the threshold), extent"""
    import signed_distance_expected as SE
    if name not in _CASES:
        ex, geom = make_scene(name, tmp_dir)
        c = {"ex": ex, "geom": geom, "tab": SE.table(geom, ex.scene.primitive_count)}
        if name in CLOSED:
            lo, hi = scene_box(geom)
            c["extent"] = float((hi - lo).max())
            c["pts"] = queries(name, geom)
            c["want"] = SE.signed_distance(c["pts"], geom, c["tab"])
            c["truth"] = inside_truth(name, c["pts"].astype(np.float64))
            c["far"] = c["want"][1].astype(np.float64) > (THRESHOLD * c["extent"]) ** 2
        _CASES[name] = c
    return _CASES[name]
