"""The triangle-against-pyramid test of the candidate lists' build (csrc/tirt_pvb.h, pvb_beam_triangle_off: the text k_pvb_beam calls) without a GPU:
tirt_kat_beam_triangle_host against an exact restatement of what `off` claims.

THE CLAIM.  Whenever the function answers `off`, no ray of the pixel meets the triangle: the triangle and the pixel's pyramid at 0.5 pixels from the centre -- the
jitter's range -- are disjoint.  The function itself sees the pyramid at 0.55 pixels, in float32, as k_pvb_beam hands it over.  The restatement is float64 where
that decides with room to spare (a separating plane through the eye that holds by 1e-9 of the magnitudes, or a common point that lies 1e-9 inside both) and
rationals (fractions.Fraction over the float32 corners, the float32 eye and the float64 corner directions, all taken as exact) wherever it does not: the triangle
clipped by the pyramid's four half-spaces, closed against closed, so a triangle that only touches the pyramid is NOT disjoint from it.  No row is excluded.

THE YIELD.  Of the random triangles of the headline scene's size that pass the four faces and are disjoint from the pyramid at 0.6 pixels, at least nine in ten
are `off`: the function's tolerance must stay a small part of the twentieth of a pixel between 0.55 and 0.6."""
from fractions import Fraction

import numpy as np
import pytest

from ti_raytrace_amd import _native

f = np.float32
F64 = np.float64
CORNERS = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])      # k_pvb_beam's order of the pyramid's corners
WIDEN = 0.55
GRID_HALF = 30000.0


class Camera:
    """eye on +z looking down -z; film point (u, v) lies on the direction ((u - cx) / fx, (v - cy) / fy, -1).  `headline`: the benchmark's focal length and distance
    (0.8 diagonals of the 2.06 cube); the other one has a power-of-two focal length, so that film points and corners on them are exact in float32"""

    def __init__(self, headline=True):
        self.size = 1024
        self.fx = 2.0 * 1024 / 2.4 if headline else 1024.0
        self.cx = 512.0
        self.eye = np.array([0.0, 0.0, 0.8 * 2.06 * np.sqrt(3.0) if headline else 3.0], f)
        self.cell = np.full(3, 2.12 / (2.0 * GRID_HALF), f)
        self.gmin = (-GRID_HALF * self.cell.astype(F64)).astype(f)

    def direction(self, u, v):
        u, v = np.asarray(u, F64), np.asarray(v, F64)
        return np.stack([(u - self.cx) / self.fx, (v - self.cx) / self.fx, -np.ones(np.broadcast(u, v).shape)], axis=-1)

    def pyramid(self, i, j, half):
        """[..., 4, 3] float64 corner directions (not normalised) of pixel (i, j) at `half` pixels"""
        i, j = np.asarray(i, F64)[..., None], np.asarray(j, F64)[..., None]
        return self.direction(i + half * CORNERS[:, 0], j + half * CORNERS[:, 1])

    def point(self, u, v, t):
        """float32 world point at parameter t on the direction through film point (u, v)"""
        return (self.eye.astype(F64) + np.asarray(t, F64)[..., None] * self.direction(u, v)).astype(f)

    def rows(self, i, j, tris):
        """the host entry's rows for triangles tris [n, 3, 3] against the pixels (i, j) [n]: the 0.55 corner directions normalised and rounded to float32, eps as
        k_pvb_beam forms it (float32, operation by operation)"""
        tris = np.asarray(tris, f).reshape(-1, 3, 3)
        n = tris.shape[0]
        d = self.pyramid(np.broadcast_to(i, n), np.broadcast_to(j, n), WIDEN)
        d32 = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f)
        dg = d32 / self.cell
        og = ((self.eye - self.gmin) / self.cell).astype(f)
        a, b = dg, np.roll(dg, -1, axis=1)
        nn = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(f)
        l1 = (np.abs(nn[..., 0]) + np.abs(nn[..., 1]) + np.abs(nn[..., 2])).astype(f)
        eps = (f(1.0e-5) * l1 * f(((np.abs(og[0]) + np.abs(og[1]) + np.abs(og[2])) + f(3.0) * f(GRID_HALF + 2.0)))).astype(f)
        rows = np.concatenate([np.broadcast_to(self.eye, (n, 3)), np.broadcast_to(self.cell, (n, 3)), d32.reshape(n, 12), eps.reshape(n, 4), tris.reshape(n, 9)], axis=1)
        return np.ascontiguousarray(rows, f)


# ---- the exact restatement ----------------------------------------------------------------------------------------------------------------
def _fr3(x):
    return [Fraction(float(v)) for v in x]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def disjoint_exact(eye32, tri32, D):
    """rationals: the triangle (float32 corners) minus the eye, clipped by the four closed half-spaces of the cone spanned by the directions D [4, 3]"""
    e = _fr3(eye32)
    poly = [[a - b for a, b in zip(_fr3(v), e)] for v in tri32]
    Dq = [_fr3(d) for d in D]
    axis = [sum(d[k] for d in Dq) for k in range(3)]
    for q in range(4):
        n = _cross(Dq[q], Dq[(q + 1) & 3])
        if _dot(n, axis) < 0:
            n = [-x for x in n]
        out = []
        for a in range(len(poly)):
            p, r = poly[a], poly[(a + 1) % len(poly)]
            sp, sr = _dot(n, p), _dot(n, r)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sr < 0) or (sp < 0 and sr > 0):
                t = sp / (sp - sr)
                out.append([p[k] + t * (r[k] - p[k]) for k in range(3)])
        poly = out
        if not poly:
            return True
    return False


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-300)


def disjoint(eye32, tris32, D):
    """[n] bool: triangle r and the cone of D[r] share no point.  float64 certificates first, rationals for the rest; returns (verdict, rows that needed rationals)"""
    V = tris32.astype(F64) - eye32.astype(F64)
    n = V.shape[0]
    axis = D.sum(axis=1)
    face = np.cross(D, np.roll(D, -1, axis=1))
    face = face * np.sign(np.einsum("nqk,nk->nq", face, axis))[..., None]
    # (1) a plane through the eye, one of the four faces or of the three edge planes, with one of the two sets strictly beyond it and the other not across it
    cand = np.concatenate([face, np.cross(V, np.roll(V, -1, axis=1))], axis=1)
    N = _unit(cand)
    P = np.einsum("nck,nqk->ncq", N, _unit(D))
    T = np.einsum("nck,njk->ncj", N, _unit(V))
    ok = (np.linalg.norm(cand, axis=-1) > 0) & (np.linalg.norm(V, axis=-1) > 0).all(axis=1)[:, None]
    big, tiny = 1e-9, 1e-12
    lo = lambda X, m: (X <= m).all(-1)
    hi = lambda X, m: (X >= m).all(-1)
    sep = ok & ((lo(P, tiny) & hi(T, big)) | (lo(P, -big) & hi(T, -tiny)) | (hi(P, -tiny) & lo(T, -big)) | (hi(P, big) & lo(T, tiny)))
    sure_dis = sep.any(axis=1)
    # (2) a common point: a triangle corner well inside the cone, or the centre / a corner direction through the triangle's interior
    Nf = _unit(face)
    inside = (np.einsum("nqk,njk->nqj", Nf, _unit(V)) >= 1e-9).all(axis=1).any(axis=1)
    R = np.concatenate([axis[:, None, :], D], axis=1)
    e1, e2 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]
    pv = np.cross(R, e2[:, None, :])
    det = np.einsum("nrk,nk->nr", pv, e1)
    scale = np.linalg.norm(R, axis=-1) * np.linalg.norm(e1, axis=-1)[:, None] * np.linalg.norm(e2, axis=-1)[:, None]
    good = np.abs(det) > 1e-9 * np.maximum(scale, 1e-300)
    inv = 1.0 / np.where(good, det, 1.0)
    tv = -V[:, 0]
    u = np.einsum("nrk,nk->nr", pv, tv) * inv
    qv = np.cross(tv, e1)
    v = np.einsum("nrk,nk->nr", R, qv) * inv
    t = np.einsum("nk,nk->n", e2, qv)[:, None] * inv
    hit = (good & (u >= 1e-9) & (v >= 1e-9) & (u + v <= 1.0 - 1e-9) & (t > 0)).any(axis=1)
    sure_hit = inside | hit
    assert not (sure_dis & sure_hit).any()
    out = sure_dis.copy()
    rest = np.flatnonzero(~sure_dis & ~sure_hit)
    for r in rest:
        out[r] = disjoint_exact(eye32, tris32[r], D[r])
    return out, rest.size


def check_off_means_disjoint(cam, i, j, tris, label):
    rows = cam.rows(i, j, tris)
    off = _native.kat_beam_triangle_host(rows, 1)
    faces = _native.kat_beam_triangle_host(rows, 0)
    assert not (faces & ~off).any(), "%s: a triangle the four faces drop is listed with the edge planes" % label
    k = np.flatnonzero(off != 0)
    n = rows.shape[0]
    dis, exact = disjoint(cam.eye, rows[k, 22:31].reshape(-1, 3, 3), cam.pyramid(np.broadcast_to(i, n)[k], np.broadcast_to(j, n)[k], 0.5))
    print("%-28s rows %6d, off by a face %6d, off by an edge plane alone %6d, decided in rationals %4d" % (label, n, int(faces.sum()), int((off & ~faces).sum()), exact))
    bad = k[~dis]
    assert bad.size == 0, "%s: row %d is off but meets the pixel's pyramid at 0.5 pixels: %s" % (label, int(bad[0]), rows[bad[0]].tolist())
    return rows, off, faces


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------
def pixels_of(rng, n, cam):
    """pixels all over the film, its corners and its centre among them"""
    fixed = np.array([[0, 0], [cam.size - 1, 0], [0, cam.size - 1], [cam.size - 1, cam.size - 1], [512, 512], [511, 512], [3, 700]])
    p = np.concatenate([fixed, rng.integers(0, cam.size, (57, 2))])
    at = rng.integers(0, p.shape[0], n)
    return p[at, 0], p[at, 1]


def random_triangles(rng, cam, n, spread=0.03, reach=14.0):
    """triangles of the headline scene's size (centre + U[-spread, spread]^3) whose centre projects within `reach` pixels of their pixel's"""
    i, j = pixels_of(rng, n, cam)
    u, v = i + rng.uniform(-reach, reach, n), j + rng.uniform(-reach, reach, n)
    c = cam.eye.astype(F64) + rng.uniform(1.8, 3.9, n)[:, None] * _unit(cam.direction(u, v))
    return i, j, (c[:, None, :] + rng.uniform(-spread, spread, (n, 3, 3))).astype(f)


@pytest.fixture(scope="module")
def headline():
    return Camera(True)


def test_random_triangles_and_the_yield(headline):
    cam, rng = headline, np.random.default_rng(5)
    i, j, tris = random_triangles(rng, cam, 40000)
    rows, off, faces = check_off_means_disjoint(cam, i, j, tris, "random, headline size")
    k = np.flatnonzero(faces == 0)
    dis, exact = disjoint(cam.eye, tris[k], cam.pyramid(i[k], j[k], 0.6))
    # the restatement alone must find what the edge planes are for, in numbers that make nine in ten a statement
    assert dis.sum() >= 2000, "only %d of %d triangles that pass the faces are disjoint from the pyramid at 0.6 pixels" % (int(dis.sum()), k.size)
    got = off[k][dis] != 0
    print("pass the four faces %d, of them disjoint from the pyramid at 0.6 pixels %d (rationals: %d), of those off %d = %.2f %%; listed after the faces %d, after the edges %d"
          % (k.size, int(dis.sum()), exact, int(got.sum()), 100.0 * got.mean(), k.size, int((off == 0).sum())))
    assert got.mean() >= 0.9


def test_hostile_triangles(headline):
    cam, rng = headline, np.random.default_rng(6)
    n = 3000
    # slivers: two corners half a unit apart, the third a ten-thousandth off their line
    i, j, base = random_triangles(rng, cam, n, reach=6.0)
    axis = _unit(rng.normal(size=(n, 3)))
    sl = base.astype(F64)
    sl[:, 1] = sl[:, 0] + 0.5 * axis
    sl[:, 2] = sl[:, 0] + rng.uniform(0.1, 0.9, n)[:, None] * 0.5 * axis + 1e-4 * rng.normal(size=(n, 3))
    check_off_means_disjoint(cam, i, j, sl, "slivers")
    # zero area: the third corner on the line of the other two (as float32 allows, and exactly: the midpoint of corners with few mantissa bits), all three equal
    za = base.copy()
    za[:, 2] = (za[:, 0].astype(F64) + rng.uniform(-1, 2, n)[:, None] * (za[:, 1].astype(F64) - za[:, 0])).astype(f)
    check_off_means_disjoint(cam, i, j, za, "zero area, rounded")
    zb = (np.round(base.astype(F64) * 256.0) / 256.0).astype(f)
    zb[:, 2] = ((zb[:, 0].astype(F64) + zb[:, 1]) / 2.0).astype(f)
    assert np.array_equal(zb[:, 2].astype(F64) * 2.0, zb[:, 0].astype(F64) + zb[:, 1])
    check_off_means_disjoint(cam, i, j, zb, "zero area, exact")
    pt = base.copy(); pt[:, 1] = pt[:, 0]; pt[:, 2] = pt[:, 0]
    rows, off, faces = check_off_means_disjoint(cam, i, j, pt, "three equal corners")
    assert np.array_equal(off, faces), "a point separates nothing by its edges"
    two = base.copy(); two[:, 2] = two[:, 1]
    rows, off, faces = check_off_means_disjoint(cam, i, j, two, "two equal corners")
    assert np.array_equal(off, faces), "a segment has no third corner to orient its plane by"
    # triangles that cover the pixel: corners 3 to 40 pixels away in three sectors around it
    ang = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, (n, 3))
    rad = rng.uniform(3.0, 40.0, (n, 3))
    cov = cam.point(i[:, None] + rad * np.cos(ang), j[:, None] + rad * np.sin(ang), rng.uniform(1.5, 4.0, (n, 3)))
    rows, off, faces = check_off_means_disjoint(cam, i, j, cov, "covering the pixel")
    assert not off.any(), "a triangle that covers its pixel is off"


def test_edges_through_the_eye_and_corners_on_the_pyramid():
    """the exact camera: film points are dyadic, so a corner can sit exactly on the pyramid's edge and an edge exactly on a line through the eye"""
    cam, rng = Camera(False), np.random.default_rng(7)
    n = 2000
    i, j = pixels_of(rng, n, cam)
    # an edge whose line passes through the eye: corners at t = 1 and t = 2 (and 0.5, 4) on one direction, exactly; the third corner anywhere near
    u, v = i + rng.integers(-64, 65, n) / 16.0, j + rng.integers(-64, 65, n) / 16.0
    tri = np.stack([cam.point(u, v, np.full(n, 1.0)), cam.point(u, v, rng.choice([0.5, 2.0, 4.0], n)),
                    cam.point(u + rng.uniform(-20, 20, n), v + rng.uniform(-20, 20, n), rng.uniform(0.5, 4.0, n))], axis=1)
    d = cam.direction(u, v)
    assert np.array_equal(tri[:, 0].astype(F64), cam.eye.astype(F64) + d), "the construction is not exact"
    check_off_means_disjoint(cam, i, j, tri, "edge through the eye, exact")
    tri2 = tri.copy(); tri2[:, 1] = (cam.eye.astype(F64) + rng.uniform(0.3, 5.0, n)[:, None] * d).astype(f)
    check_off_means_disjoint(cam, i, j, tri2, "edge through the eye, rounded")
    # a corner exactly on the pixel's corner at 0.5 pixels, the rest of the triangle pointing away from the pixel: touches, is not disjoint, must be listed
    q = rng.integers(0, 4, n)
    cu, cv = i + 0.5 * CORNERS[q, 0], j + 0.5 * CORNERS[q, 1]
    away = np.stack([CORNERS[q, 0], CORNERS[q, 1]], axis=1)
    r1, r2 = rng.uniform(1.0, 20.0, (2, n)), rng.uniform(0.0, 1.0, (2, n))
    tri = np.stack([cam.point(cu, cv, rng.choice([1.0, 2.0, 4.0], n)),
                    cam.point(cu + away[:, 0] * r1[0], cv + away[:, 1] * r1[0] * r2[0], rng.uniform(1.0, 4.0, n)),
                    cam.point(cu + away[:, 0] * r1[1] * r2[1], cv + away[:, 1] * r1[1], rng.uniform(1.0, 4.0, n))], axis=1)
    rows, off, faces = check_off_means_disjoint(cam, i, j, tri, "corner on the pixel's corner")
    assert not off.any(), "a triangle that touches the pixel's corner is off"


def test_nudged_across_the_faces_and_the_edges(headline):
    """154 shapes x 65 offsets of 1/64 pixel from -0.5 to +0.5 pixels = 10 010 triangles across EACH of the pyramid's 4 faces and 4 edges, 80 080 in all: across a
    face the triangle's nearest corner moves through the face's line; across an edge (the pyramid's corner ray) the triangle's nearest EDGE moves through the pixel's
    corner point, at 45 degrees and at other slopes, the triangle beyond it.  Offset 0 touches; the function may say off only beyond the other side of 0.  That the
    rows reach both verdicts is checked at the end: a fifth of a pixel out, the faces drop every triangle nudged across a face and few of those nudged across an
    edge, which the edge planes drop but for the few whose corners' random depths put them nearly edge-on (their triple product is within its tolerance)."""
    cam, rng = headline, np.random.default_rng(8)
    shapes, steps = 154, np.arange(-32, 33) / 64.0
    i, j = pixels_of(rng, shapes, cam)
    I, J, T, S, kind = [], [], [], [], []
    for s in range(shapes):
        for q in range(4):
            out = CORNERS[q] * np.array([1.0, 0.0]) if q & 1 == 0 else CORNERS[q] * np.array([0.0, 1.0])      # the outward normal of a face on the film
            along = np.array([-out[1], out[0]])
            for kind_, st in (("face", steps), ("edge", steps)):
                for off in st:
                    if kind_ == "face":
                        # nearest corner at (0.5 + off) along `out`, anywhere within the pixel's width along the face; the other two beyond it
                        base = (0.5 + off) * out + rng.uniform(-0.5, 0.5) * along
                        pts = [base, base + rng.uniform(0.5, 15.0) * out + rng.uniform(-10, 10) * along, base + rng.uniform(0.5, 15.0) * out + rng.uniform(-10, 10) * along]
                    else:
                        # an edge at distance `off` beyond the corner point 0.5 * CORNERS[q], normal to a direction between the two faces that meet there
                        w = rng.uniform(0.05, 0.95)
                        nrm = np.array([CORNERS[q][0] * w, CORNERS[q][1] * (1.0 - w)]); nrm /= np.linalg.norm(nrm)
                        tan = np.array([-nrm[1], nrm[0]])
                        foot = 0.5 * CORNERS[q] + off * nrm
                        pts = [foot + rng.uniform(2.0, 12.0) * tan, foot - rng.uniform(2.0, 12.0) * tan, foot + rng.uniform(1.0, 15.0) * nrm + rng.uniform(-3, 3) * tan]
                    pts = np.array(pts)
                    T.append(cam.point(i[s] + pts[:, 0], j[s] + pts[:, 1], rng.uniform(1.8, 3.9, 3)))
                    I.append(i[s]); J.append(j[s]); S.append(off); kind.append(kind_ == "edge")
    I, J, T, S, kind = np.array(I), np.array(J), np.array(T), np.array(S), np.array(kind)
    assert min(int((kind == e).sum()) for e in (False, True)) >= 4 * 10000
    rows, off, faces = check_off_means_disjoint(cam, I, J, T, "nudged by 1/64 pixel")
    assert not off[S <= 0.0].any(), "a triangle that reaches into the pixel's square is off"
    # and the test is not vacuous: beyond a fifth of a pixel the faces drop the triangles nudged across a face and the edge planes those nudged across an edge
    far = S >= 0.2
    print("beyond a fifth of a pixel: off %.4f of those nudged across a face, %.4f of those nudged across an edge (by a face: %.4f)" % (faces[far & ~kind].mean(), off[far & kind].mean(), faces[far & kind].mean()))
    assert faces[far & ~kind].all() and off[far & kind].mean() >= 0.99 and faces[far & kind].mean() < 0.9


def test_refusals():
    lib = _native.lib()
    buf, out = np.zeros(31, f), np.zeros(1, np.int32)
    assert lib.tirt_kat_beam_triangle_host(buf, 1, 2, out) == -2 and lib.tirt_kat_beam_triangle_host(buf, -1, 1, out) == -2
    assert _native.kat_beam_triangle_host(np.zeros((0, 31), f)).shape == (0,)
    nan = Camera(True).rows(5, 5, np.full((1, 3, 3), np.nan, f))
    assert _native.kat_beam_triangle_host(nan, 1)[0] == 0, "a NaN triangle separates nothing"
