"""The camera rays' candidate lists (csrc/tirt_pvb.hip; tirt_primary_beam_lists_download) and the walk of one ray over its pixel's list (pvb_walk_list;
tirt_kat_primary_list_walk) held to their definition in numpy.  No device here, and no oracle: the yardstick is the hit set H of multi_hit_expected.hit_sets --
every verified primitive hit of a ray, which tests/test_multi_hit_host.py holds to the oracle -- over arrays that are already downloadable.

The sentence under test (header of tirt_pvb.hip): EVERY LEAF THAT COULD HOLD A VERIFIED HIT AT DISTANCE <= bound IS ON THE LIST, WITH ALL THE LEAVES IN FRONT OF IT.
Films cannot see most ways of breaking it (a missing leaf shows only when a random jitter lands on it, it is the closest hit and another listed leaf still yields
a hit within the bound), so the sample rays of a pixel are AIMED: at the triangle vertices and edge crossings in and around the pixel's square, at the spheres'
silhouettes, on a lattice that includes the pixel's corners, and a few at random (sample_rows).

  sample_rows      the jitters of every tested pixel, clipped to what a render can draw: [-0.5, nextafter(0.5, 0)]
  jittered_rays    camera_ray_direction restated in float32 (oracle_api.camera_rays plus the jitter): the device's direction bit for bit
  dense_hits       H of every row as a dense [rows, primitives] table of distances (inf: not in H) and its first element
  check_lists      form, the start of the bound, completeness and order, "not everything"
  expected_walk    the verdict and the hit of one row: from H alone (resolved, first element) and from walking the list as given (hit and steps)
  reference_lists  lists made from H itself, for the host test: check_lists must accept them and reject every single defect put into them

Geometry (`Geo`): the leaf code of every primitive and the box its slot in the 4-wide nodes stands for (from tirt_wide_tree_download: from_download; from the
reference's compact rows where there is no device: from_reference).  The two box tests (check 2's "more leaves than a list holds" and check 4) are done in float64
on the box enlarged by k_trace's margin + TR_MARGIN_BEAM_EXTRA + one cell against the pixel's pyramid at half-width 1.5 pixels -- the kernel uses 0.55 and fp32 -- and only
against the pyramid's four faces: permissive on purpose, they catch a list that holds (nearly) every leaf or a bound that came in for no reason."""
import numpy as np

import cutout_expected as ce
import multi_hit_expected as mh
import wide_tree_expected as wt

f = np.float32
INF_VALUE = ce.INF_VALUE
PVB_CMAX = 24
PVB_REACH = f(1.5)
TR_MARGIN_CELLS, TR_MARGIN_PER_RHO, TR_MARGIN_BEAM_EXTRA, TR_FAR_RHO = 0.25, 0.25, 0.05, 8.0
J_LO, J_HI = f(-0.5), np.nextafter(f(0.5), f(0.0))
LATTICE, VERTEX, EDGE, SPHERE, RANDOM = range(5)
KIND_NAMES = ("lattice", "vertex", "edge", "sphere", "random")
ROW_CAP = 160
PROBES = ((0.0, 0.0), (-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0.5))          # k_pvb_probes: the centre, then the corners


# ---- the camera ---------------------------------------------------------------------------------------------------------------------------
def clip_jitter(j):
    return np.clip(np.asarray(j, np.float64).astype(f), J_LO, J_HI).astype(f)


def jittered_rays(cam, H, pixels, jx, jy):
    """camera_ray_direction(cam, i, j, jx, jy) of tirt_device.h in float32, one rounding per operation: oracle_api.camera_rays with the jitter where that has
    + 0.0.  pixels: linear indices p = i * H + j.  Returns [n, 6] (eye, direction)."""
    pixels = np.asarray(pixels, np.int64)
    ii, jj = pixels // H, pixels % H
    jx, jy = np.asarray(jx, f), np.asarray(jy, f)
    x = ((ii.astype(f) + jx).astype(f) - f(cam.cx)).astype(f) / f(cam.fx)
    y = ((jj.astype(f) + jy).astype(f) - f(cam.cy)).astype(f) / f(cam.fy)
    z = np.full_like(x, -1.0)
    M = cam.view_inv_np[0].astype(f)
    w = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] * f(0.0) for r in range(3)]
    n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    inv = f(1.0) / np.sqrt(n2)
    d = np.stack([w[0] * inv, w[1] * inv, w[2] * inv], axis=1).astype(f)
    o = np.broadcast_to(cam.eye_np[0].astype(f), d.shape)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=f)


class Cam64:
    """the camera in float64: q = inverse(upper 3 x 3 of view_inv) (p - eye) is p in camera space, (x, y, -1) ~ q, i + jx = x * fx + cx"""

    def __init__(self, cam):
        self.M = cam.view_inv_np[0].astype(f).astype(np.float64)[:3, :3]
        self.Minv = np.linalg.inv(self.M)
        self.eye = cam.eye_np[0].astype(f).astype(np.float64)
        self.fx, self.fy, self.cx, self.cy = (float(f(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))

    def to_camera(self, p):
        return (np.asarray(p, np.float64) - self.eye) @ self.Minv.T

    def film(self, q):
        """continuous film coordinates (i + jx, j + jy) of camera-space points in front of the eye"""
        return np.stack([-q[..., 0] / q[..., 2] * self.fx + self.cx, -q[..., 1] / q[..., 2] * self.fy + self.cy], axis=-1)

    def direction(self, u, v):
        """unit world direction through film point (u, v)"""
        d = np.stack([(np.asarray(u, np.float64) - self.cx) / self.fx, (np.asarray(v, np.float64) - self.cy) / self.fy, -np.ones(np.shape(u))], axis=-1) @ self.M.T
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    def pyramid(self, i, j, half):
        """(inward face normals [4, 3], unit axis [3]) of pixel (i, j)'s pyramid at `half` pixels from the centre"""
        cu = np.array([-half, half, half, -half]) + i
        cv = np.array([-half, -half, half, half]) + j
        d = self.direction(cu, cv)
        axis = self.direction(np.float64(i), np.float64(j))
        n = np.cross(d, np.roll(d, -1, axis=0))
        n = n * np.sign(n @ axis)[:, None]
        return n / np.linalg.norm(n, axis=1, keepdims=True), axis


# ---- the geometry the lists are about ---------------------------------------------------------------------------------------------------------
class Geo:
    """code [n] uint32: the leaf code of every primitive; lo, hi [n, 3] float64: the box of its slot in world units (None: the root is the leaf); cell [3];
    margin: the enlargement of the two box tests in cells; root_min / root_max (float32) and whether the root is an inner node (the walk's first test)"""

    def __init__(self, code, lo, hi, cell, margin, root_min, root_max, root_inner, far):
        self.code = np.asarray(code, np.uint32)
        self.lo, self.hi, self.cell, self.margin = lo, hi, cell, margin
        self.root_min, self.root_max, self.root_inner, self.far = root_min, root_max, root_inner, far
        self.prim_of = {int(c): p for p, c in enumerate(self.code.tolist())}

    def enlarged(self):
        m = self.margin * self.cell
        return self.lo - m, self.hi + m


def _margin(grid_min, inv_extent, eye):
    rho = float(np.max(np.abs(np.asarray(grid_min, np.float64) - eye) * np.asarray(inv_extent, np.float64)))
    return rho, TR_MARGIN_CELLS + TR_MARGIN_PER_RHO * rho + TR_MARGIN_BEAM_EXTRA + 1.0


def from_download(dl, primitive_np, cam):
    """Geo from Context.wide_tree_download: codes through wide_tree_expected.leaf_code and prim_slot, boxes from the plane words of cnode"""
    primitive_np = np.asarray(primitive_np, np.int64)
    n = primitive_np.shape[0]
    is_shape = primitive_np[:, 0] != wt.PRIMITIVE_TRI
    code = np.array([wt.leaf_code(s, sh) for s, sh in zip(dl["prim_slot"].tolist(), is_shape.tolist())], np.uint32)
    eye = cam.eye_np[0].astype(f).astype(np.float64)
    g0, cell = dl["grid_min"].astype(np.float64), dl["grid_cell"].astype(np.float64)
    rho, margin = _margin(g0, dl["grid_inv_extent"], eye)
    lo = hi = None
    if n >= 2:
        wide = dl["wide_nodes"]
        cn = np.asarray(dl["cnode"], np.uint32)[:wide]
        codes = cn[:, 12:16]
        words = cn[:, :12].reshape(wide, 4, 3)
        leafm = (codes != wt.TR_EMPTY) & ((codes & 0x80000000) != 0)
        at = {int(c): k for k, c in enumerate(codes[leafm].tolist())}
        assert len(at) == n, "cnode holds %d leaf slots for %d primitives" % (len(at), n)
        order = np.array([at[int(c)] for c in code.tolist()])
        w = words[leafm][order]
        lo = g0 + wt.half_value((w & 0xffff).astype(np.uint16)) * cell
        hi = g0 + wt.half_value((w >> 16).astype(np.uint16)) * cell
    return Geo(code, lo, hi, cell, margin, dl["root_min"].astype(f), dl["root_max"].astype(f), n >= 2, rho > TR_FAR_RHO)


def from_reference(compact, primitive_np, cam):
    """Geo without a device: primitive i's code is leaf_code(i), its box the exact box of its leaf row, the grid 65536 cells over the root box"""
    primitive_np = np.asarray(primitive_np, np.int64)
    n = primitive_np.shape[0]
    compact = np.asarray(compact, f)
    rows = compact[ce.leaf_indices(compact)].astype(np.float64)
    code = np.array([wt.leaf_code(i, primitive_np[i, 0] != wt.PRIMITIVE_TRI) for i in range(n)], np.uint32)
    rmin, rmax = compact[0, 2:5], compact[0, 5:8]
    ext = np.maximum((rmax - rmin).astype(np.float64), 1e-30)
    eye = cam.eye_np[0].astype(f).astype(np.float64)
    rho, margin = _margin(0.5 * (rmin.astype(np.float64) + rmax), 1.0 / ext, eye)
    return Geo(code, rows[:, 2:5] if n >= 2 else None, rows[:, 5:8] if n >= 2 else None, ext / 65536.0, margin, rmin, rmax, n >= 2, rho > TR_FAR_RHO)


# ---- the sample rays ----------------------------------------------------------------------------------------------------------------------------
def prims_near(c64, H, pixels, primitive_np, vertex_np, shape_np, widen=2.0):
    """the primitives that are not wholly outside the pyramid of the tested pixels' bounding rectangle widened by `widen` pixels (float64, face by face: a triangle
    whose three corners lie outside one face, a sphere whose centre lies more than its radius outside one): every other primitive can be hit by no tested ray"""
    pixels = np.asarray(pixels, np.int64)
    ii, jj = pixels // H, pixels % H
    u0, u1, v0, v1 = ii.min() - 0.5 - widen, ii.max() + 0.5 + widen, jj.min() - 0.5 - widen, jj.max() + 0.5 + widen
    d = c64.direction(np.array([u0, u1, u1, u0]), np.array([v0, v0, v1, v1]))
    axis = c64.direction(0.5 * (u0 + u1), 0.5 * (v0 + v1))
    nrm = np.cross(d, np.roll(d, -1, axis=0))
    nrm = nrm * np.sign(nrm @ axis)[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    primitive_np = np.asarray(primitive_np, np.int64)
    pos = np.asarray(vertex_np, f)[:, :3].astype(np.float64)
    keep = np.zeros(primitive_np.shape[0], bool)
    tri = primitive_np[:, 0] == wt.PRIMITIVE_TRI
    vi = primitive_np[tri, 1]
    if vi.size:
        sd = np.stack([(pos[vi + k] - c64.eye) @ nrm.T for k in range(3)], axis=1)          # [tri, corner, face]
        keep[tri] = ~(sd < 0.0).all(axis=1).any(axis=1)
    if (~tri).any():
        sh = np.asarray(shape_np, f).reshape(-1, 10)[primitive_np[~tri, 1]].astype(np.float64)
        keep[~tri] = ~(((sh[:, 1:4] - c64.eye) @ nrm.T) < -sh[:, 4:5]).any(axis=1)
    return np.flatnonzero(keep)


def sample_rows(cam, H, pixels, primitive_np, vertex_np, shape_np, seed=20240, prims=None, cap=ROW_CAP):
    """The jitters of the tested pixels (linear indices).  Returns {"at": index into `pixels`, "jx", "jy" (float32, clipped), "kind"}, sorted by `at`, and the
    number of aimed rows dropped by the cap.
      lattice  5 x 5 over {-0.5, -0.25, 0, 0.25, nextafter(0.5, 0)}
      vertex   every triangle vertex whose projection lies within half a pixel of the pixel's square: the jitter aimed at it and the four 1/64 pixel around it
      edge     every triangle edge that crosses the square's boundary: the crossing and the boundary points 1/64 pixel to either side
      sphere   every sphere: the point of its silhouette nearest the pixel centre
      random   16 from a fixed seed
    A pixel with more than `cap` rows keeps a fixed-seed subset of its aimed rows."""
    pixels = np.asarray(pixels, np.int64)
    npx = pixels.shape[0]
    ii, jj = (pixels // H).astype(np.float64), (pixels % H).astype(np.float64)
    c64 = Cam64(cam)
    primitive_np = np.asarray(primitive_np, np.int64)
    sel = np.arange(primitive_np.shape[0]) if prims is None else np.asarray(prims, np.int64)
    tri = sel[primitive_np[sel, 0] == wt.PRIMITIVE_TRI]
    sph = sel[primitive_np[sel, 0] != wt.PRIMITIVE_TRI]
    pos = np.asarray(vertex_np, f)[:, :3]
    at, ju, jv, kind = [], [], [], []

    def add(a, u, v, k):
        at.append(np.asarray(a, np.int64).reshape(-1)); ju.append(np.asarray(u, np.float64).reshape(-1)); jv.append(np.asarray(v, np.float64).reshape(-1))
        kind.append(np.full(at[-1].shape[0], k, np.int64))

    lat = np.array([-0.5, -0.25, 0.0, 0.25, float(J_HI)])
    lu, lv = np.meshgrid(lat, lat, indexing="ij")
    add(np.repeat(np.arange(npx), 25), np.tile(lu.reshape(-1), npx), np.tile(lv.reshape(-1), npx), LATTICE)
    e = 1.0 / 64.0
    if tri.size:
        vi = primitive_np[tri, 1]
        corners = np.stack([pos[vi], pos[vi + 1], pos[vi + 2]], axis=1)                    # [tri, 3, 3] float32
        uniq, inv = np.unique(corners.reshape(-1, 3), axis=0, return_inverse=True)
        inv = inv.reshape(-1, 3)
        q = c64.to_camera(uniq)
        zn = 1e-9 * max(float(np.abs(q).max()), 1e-30)
        front = q[:, 2] < -zn
        # vertices
        uv = c64.film(q[front])
        near = (np.abs(uv[None, :, 0] - ii[:, None]) <= 1.0) & (np.abs(uv[None, :, 1] - jj[:, None]) <= 1.0)
        a, b = np.nonzero(near)
        for du, dv in ((0, 0), (e, 0), (-e, 0), (0, e), (0, -e)):
            add(a, uv[b, 0] - ii[a] + du, uv[b, 1] - jj[a] + dv, VERTEX)
        # edges: unique, clipped to the front of the eye, against the four sides of every square
        ed = np.unique(np.sort(np.concatenate([inv[:, [0, 1]], inv[:, [1, 2]], inv[:, [2, 0]]], axis=0), axis=1), axis=0)
        ed = ed[ed[:, 0] != ed[:, 1]]
        qa, qb = q[ed[:, 0]].copy(), q[ed[:, 1]].copy()
        ok = (qa[:, 2] < -zn) | (qb[:, 2] < -zn)
        qa, qb = qa[ok], qb[ok]
        for x, y in ((qa, qb), (qb, qa)):
            behind = x[:, 2] >= -zn
            s = (-zn - y[behind, 2]) / (x[behind, 2] - y[behind, 2])
            x[behind] = y[behind] + s[:, None] * (x[behind] - y[behind])
        fa, fb = c64.film(qa), c64.film(qb)
        for axis in (0, 1):
            o = 1 - axis
            cen, oth = (ii, jj) if axis == 0 else (jj, ii)
            da = fb[:, axis] - fa[:, axis]
            for side in (-0.5, 0.5):
                with np.errstate(divide="ignore", invalid="ignore"):
                    s = ((cen[:, None] + side) - fa[None, :, axis]) / da[None, :]
                    w = fa[None, :, o] + s * (fb[:, o] - fa[:, o])[None, :] - oth[:, None]
                    hit = (s >= 0.0) & (s <= 1.0) & (np.abs(w) <= 0.5)
                a, b = np.nonzero(hit)
                for dw in (0.0, e, -e):
                    along, across = w[a, b] + dw, np.full(a.shape[0], side)
                    add(a, across if axis == 0 else along, along if axis == 0 else across, EDGE)
    if sph.size:
        sh = np.asarray(shape_np, f).reshape(-1, 10)[primitive_np[sph, 1]].astype(np.float64)
        cdir = sh[:, 1:4] - c64.eye
        L = np.linalg.norm(cdir, axis=1)
        out = L > sh[:, 4]
        if out.any():
            ax = cdir[out] / L[out, None]
            th = np.arcsin(sh[out, 4] / L[out])
            dc = c64.direction(ii, jj)                                                   # [px, 3]
            perp = dc[:, None, :] - (dc @ ax.T)[:, :, None] * ax[None, :, :]
            nrm = np.linalg.norm(perp, axis=2, keepdims=True)
            perp = np.where(nrm > 1e-12, perp / np.maximum(nrm, 1e-300), 0.0)
            d = np.cos(th)[None, :, None] * ax[None] + np.sin(th)[None, :, None] * perp
            qd = d @ c64.Minv.T
            okd = qd[..., 2] < -1e-9
            a, b = np.nonzero(okd)
            uv = c64.film(qd[a, b])
            add(a, uv[:, 0] - ii[a], uv[:, 1] - jj[a], SPHERE)
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.5, 0.5, (npx, 16, 2))
    add(np.repeat(np.arange(npx), 16), r[..., 0], r[..., 1], RANDOM)
    at, kind = np.concatenate(at), np.concatenate(kind)
    jx, jy = clip_jitter(np.concatenate(ju)), clip_jitter(np.concatenate(jv))
    # the cap
    keep = np.ones(at.shape[0], bool)
    aimed = (kind == VERTEX) | (kind == EDGE) | (kind == SPHERE)
    n_aimed = np.bincount(at[aimed], minlength=npx)
    dropped = 0
    crng = np.random.default_rng(seed + 1)
    for k in np.flatnonzero(n_aimed > cap - 41):
        idx = np.flatnonzero(aimed & (at == k))
        drop = crng.permutation(idx)[cap - 41:]
        keep[drop] = False
        dropped += drop.size
    order = np.argsort(at[keep], kind="stable")
    return {"at": at[keep][order], "jx": jx[keep][order], "jy": jy[keep][order], "kind": kind[keep][order]}, dropped


# ---- H as a table -----------------------------------------------------------------------------------------------------------------------------
def dense_hits(sc, compact, rays, prims=None):
    """multi_hit_expected.hit_sets over `rays`: {"sel": the primitives asked, "T", "U", "V" [rows, len(sel)] (T = inf where the primitive is not in the row's H),
    "first": (t, u, v, prim) of H's first element (a miss: INF_VALUE, 0, 0, -1), "leaf": compact index of every asked primitive's leaf}"""
    h = mh.hit_sets(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, compact, rays, prims=prims)
    sel = np.arange(sc.primitive_np.shape[0]) if prims is None else np.asarray(prims, np.int64)
    n, Q = h["t"].shape
    col = np.full(sc.primitive_np.shape[0], -1, np.int64); col[sel] = np.arange(Q)
    T = np.full((n, Q), np.inf, f); U = np.zeros((n, Q), f); V = np.zeros((n, Q), f)
    ok = h["prim"] >= 0
    r = np.broadcast_to(np.arange(n)[:, None], (n, Q))[ok]
    c = col[h["prim"][ok]]
    T[r, c] = h["t"][ok]; U[r, c] = h["u"][ok]; V[r, c] = h["v"][ok]
    if Q:
        first = (h["t"][:, 0].copy(), h["u"][:, 0].copy(), h["v"][:, 0].copy(), h["prim"][:, 0].copy())
    else:
        first = (np.full(n, INF_VALUE, f), np.zeros(n, f), np.zeros(n, f), np.full(n, -1, np.int32))
    return {"sel": sel, "col": col, "T": T, "U": U, "V": V, "first": first, "leaf": ce.leaf_indices(compact)[sel]}


def probe_start(cam, H, pixels, sc, compact, prims=None):
    """start [pixels] float32: "infinite" -- INF_VALUE = 1e6, the distance of a miss, is how the device writes a bound that is none -- if one of the five probe rays
    (the centre, the corners at +-0.5) has no hit in H, else float32(1.5) * the largest of their distances"""
    pixels = np.asarray(pixels, np.int64)
    t = []
    for px, py in PROBES:
        rays = jittered_rays(cam, H, pixels, np.full(pixels.shape[0], px, f), np.full(pixels.shape[0], py, f))
        t.append(dense_hits(sc, compact, rays, prims)["first"][0])
    t = np.stack(t, axis=1)
    miss = (t >= INF_VALUE).any(axis=1)
    return np.where(miss, INF_VALUE, (t.max(axis=1) * PVB_REACH).astype(f)).astype(f)


class Case:
    """everything the checks need about the tested pixels of one (scene, camera, film): `ks` local pixel indices, `pixels` their linear indices, rows, rays, H"""

    def __init__(self, sc, cam, H, order, ks, compact, geo, prims=None, seed=20240):
        self.sc, self.cam, self.H, self.geo, self.compact = sc, cam, H, geo, compact
        self.ks = np.asarray(ks, np.int64)
        self.pixels = np.asarray(order, np.int64)[self.ks]
        self.c64 = Cam64(cam)
        self.prims = prims
        self.rows, self.dropped = sample_rows(cam, H, self.pixels, sc.primitive_np, sc.vertex_np, sc.shape_np, seed, prims)
        self.rays = jittered_rays(cam, H, self.pixels[self.rows["at"]], self.rows["jx"], self.rows["jy"])
        self.hits = dense_hits(sc, compact, self.rays, prims)
        self.start = probe_start(cam, H, self.pixels, sc, compact, prims)
        at = self.rows["at"]
        self.span = np.searchsorted(at, np.arange(self.ks.shape[0] + 1))          # rows of tested pixel a: span[a] .. span[a + 1]

    def name(self, a):
        p = int(self.pixels[a])
        return "pixel k=%d (i=%d, j=%d)" % (int(self.ks[a]), p // self.H, p % self.H)


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------
def _meets(case, a, half, near_limit=None):
    """which primitives' enlarged boxes meet the pyramid of tested pixel a at `half` pixels (face by face, float64) -- and do so nearer than near_limit"""
    geo = case.geo
    n = geo.code.shape[0]
    if geo.lo is None:
        return np.ones(n, bool)
    lo, hi = geo.enlarged()
    p = int(case.pixels[a])
    nrm, axis = case.c64.pyramid(p // case.H, p % case.H, half)
    rel_lo, rel_hi = lo - case.c64.eye, hi - case.c64.eye
    ok = np.ones(n, bool)
    for q in range(4):
        far = np.where(nrm[q] >= 0.0, rel_hi, rel_lo)
        ok &= (far @ nrm[q]) >= 0.0
    if near_limit is not None:
        near = np.where(axis >= 0.0, rel_lo, rel_hi) @ axis
        ok &= near <= near_limit
    return ok


def check_lists(case, lists):
    """lists: {"count" [P], "code" [cmax, P] int32, "nr" [cmax, P] float32, "bound" [P]} in local pixel order (Context.primary_beam_lists_download).  Raises an
    AssertionError that names the pixel and the leaf; returns {"listed", "with_hits", "full", "cut"}: leaves listed and leaves with a non-empty H over the sample
    rows (sums over the tested pixels that have a list), full lists, pixels whose bound came in."""
    geo = case.geo
    tree = set(geo.code.tolist())
    T = case.hits["T"]
    code_of_col = geo.code[case.hits["sel"]]
    stat = {"listed": 0, "with_hits": 0, "full": 0, "cut": 0, "pixels": 0}
    for a, k in enumerate(case.ks.tolist()):
        who = case.name(a)
        n = int(lists["count"][k])
        bound, start = f(lists["bound"][k]), f(case.start[a])
        # 1. form
        assert -1 <= n <= PVB_CMAX, "%s: count %d is outside [-1, %d]" % (who, n, PVB_CMAX)
        assert not bound > start, "%s: bound %r lies above its start %r (1.5 x the farthest probe hit)" % (who, float(bound), float(start))
        if n < 0:
            continue
        codes = lists["code"][:n, k].astype(np.int32).view(np.uint32)
        nr = lists["nr"][:n, k].astype(f)
        for c in codes.tolist():
            assert c in tree, "%s: leaf %#x on its list is no leaf of the tree" % (who, c)
        u, cnt = np.unique(codes, return_counts=True)
        if (cnt > 1).any():
            raise AssertionError("%s: leaf %#x appears %d times on its list" % (who, int(u[cnt > 1][0]), int(cnt[cnt > 1][0])))
        for e in range(n):
            assert np.isfinite(nr[e]) and nr[e] >= 0.0, "%s: leaf %#x has nr %r (finite and >= 0 expected)" % (who, int(codes[e]), float(nr[e]))
            assert e == 0 or nr[e] >= nr[e - 1], "%s: nr falls from %r to %r at leaf %#x (entry %d): the list is not nearest first" % (
                who, float(nr[e - 1]), float(nr[e]), int(codes[e]), e)
            assert nr[e] <= bound, "%s: leaf %#x has nr %r beyond the bound %r" % (who, int(codes[e]), float(nr[e]), float(bound))
        # 2. a bound that came in: only where more leaves than a list holds meet the pyramid nearer than start
        if bound < start:
            m = int(_meets(case, a, 1.5, float(start)).sum())
            assert m > PVB_CMAX, "%s: bound %r came in below its start %r although only %d leaves meet the pixel's pyramid that near (a list holds %d)" % (
                who, float(bound), float(start), m, PVB_CMAX)
            stat["cut"] += 1
        # 3. completeness and order: every hit of every sample ray within the bound is on the list, at nr <= t
        r0, r1 = int(case.span[a]), int(case.span[a + 1])
        t = T[r0:r1]
        nr_of_col = np.full(code_of_col.shape[0], np.inf, f)
        listed_col = {int(c): e for e, c in enumerate(codes.tolist())}
        for q, c in enumerate(code_of_col.tolist()):
            if c in listed_col:
                nr_of_col[q] = nr[listed_col[c]]
        with np.errstate(invalid="ignore"):
            bad = (t <= bound) & ~(nr_of_col[None, :] <= t)
        if bad.any():
            r, q = (int(x) for x in np.argwhere(bad)[0])
            row = r0 + r
            what = "is not on the list" if not np.isfinite(nr_of_col[q]) else "is listed at nr %r, beyond that hit" % float(nr_of_col[q])
            raise AssertionError("%s: its %s ray (jx %r, jy %r) hits primitive %d at t %r <= bound %r, but leaf %#x %s" % (
                who, KIND_NAMES[int(case.rows["kind"][row])], float(case.rows["jx"][row]), float(case.rows["jy"][row]), int(case.hits["sel"][q]), float(t[r, q]),
                float(bound), int(code_of_col[q]), what))
        # 4. not everything: a listed leaf's enlarged box meets the pyramid at 1.5 pixels
        meets = _meets(case, a, 1.5)
        for c in codes.tolist():
            assert meets[geo.prim_of[c]], "%s: leaf %#x is on its list although its box, enlarged, lies outside the pixel's pyramid at 1.5 pixels" % (who, c)
        stat["listed"] += n; stat["pixels"] += 1
        stat["with_hits"] += int(np.isfinite(t).any(axis=0).sum())
        stat["full"] += int(n == PVB_CMAX)
    return stat


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------------
def expected_walk(case, lists):
    """Per sample row: "dead" (the ray fails `slabs` on the root's exact box -- asked where the root is an inner node, as k_trace asks -- or is NaN), "resolved"
    (dead, or the pixel has a list and its bound is none -- INF_VALUE -- or H's first element lies within it), "first" = (t, u, v, prim) of H's first element (a miss: INF_VALUE, 0,
    0, -1): a resolved row's answer bit for bit; and what walking the list AS GIVEN yields, which every row must report whatever `resolved` is: "walk" = (t, u, v,
    prim) and "steps" -- entries are taken in order while nr <= the hit distance so far, a taken leaf's primitive replaces the hit if it is in H and nearer, or as
    near in a leaf of larger compact index."""
    geo, rows = case.geo, case.rows
    n = rows["at"].shape[0]
    o = [case.rays[:, k].copy() for k in range(3)]; d = [case.rays[:, 3 + k].copy() for k in range(3)]
    dead = np.isnan(case.rays[:, 3:6]).any(axis=1)
    if geo.root_inner:
        dead |= ~ce.slabs(o, d, geo.root_min, geo.root_max)
    ft, fu, fv, fp = case.hits["first"]
    k_of_row = case.ks[rows["at"]]
    count = lists["count"][k_of_row]
    bound = lists["bound"][k_of_row].astype(f)
    resolved = dead | ((count >= 0) & ((bound >= INF_VALUE) | ((fp >= 0) & (ft <= bound))))
    T, U, V, leaf, col = case.hits["T"], case.hits["U"], case.hits["V"], case.hits["leaf"], case.hits["col"]
    wt_ = np.full(n, INF_VALUE, f); wu = np.zeros(n, f); wv = np.zeros(n, f); wp = np.full(n, -1, np.int32); wl = np.full(n, -1, np.int64)
    steps = np.zeros(n, np.int64)
    for a, k in enumerate(case.ks.tolist()):
        r = np.arange(int(case.span[a]), int(case.span[a + 1]))
        cnt = int(lists["count"][k])
        alive = ~dead[r] & (cnt >= 0)
        for e in range(max(cnt, 0)):
            c = int(np.int32(lists["code"][e, k]).view(np.uint32))
            nr = f(lists["nr"][e, k])
            alive = alive & (nr <= wt_[r])
            if not alive.any():
                break
            steps[r] += alive
            p = geo.prim_of.get(c, -1)
            q = col[p] if p >= 0 else -1
            if q < 0:
                continue                         # (a leaf no sample ray can hit, or -- a form error check_lists reports -- no leaf at all)
            t = T[r, q]
            take = alive & np.isfinite(t) & ((t < wt_[r]) | ((t == wt_[r]) & (wl[r] >= 0) & (leaf[q] > wl[r])))
            rr = r[take]
            wt_[rr] = t[take]; wu[rr] = U[rr, q]; wv[rr] = V[rr, q]; wp[rr] = p; wl[rr] = leaf[q]
    # a dead row comes back as a miss
    first = (np.where(dead, INF_VALUE, ft).astype(f), np.where(dead, f(0), fu).astype(f), np.where(dead, f(0), fv).astype(f), np.where(dead, -1, fp).astype(np.int32))
    return {"dead": dead, "resolved": resolved, "first": first, "walk": (wt_, wu, wv, wp), "steps": steps}


# ---- lists made from H itself (the host test) ---------------------------------------------------------------------------------------------------
def reference_lists(case, P):
    """Per tested pixel every leaf with a non-empty H over the sample rows, at nr = a little less than the least of its distances, nearest first, bound = start;
    more than a list holds: the nearest PVB_CMAX, and the bound comes in to just below the first one left out (the overflow rule).  Pixels not tested: no list."""
    count = np.full(P, -1, np.int32); code = np.zeros((PVB_CMAX, P), np.int32); nr = np.zeros((PVB_CMAX, P), f); bound = np.zeros(P, f)
    T = case.hits["T"]
    code_of_col = case.geo.code[case.hits["sel"]]
    for a, k in enumerate(case.ks.tolist()):
        t = T[int(case.span[a]):int(case.span[a + 1])]
        tmin = t.min(axis=0) if t.shape[0] else np.full(t.shape[1], np.inf, f)
        near = np.maximum(tmin.astype(np.float64) * (1.0 - 1.0e-3) - 1.0e-6, 0.0).astype(f)
        b = f(case.start[a])
        cols = np.flatnonzero(np.isfinite(tmin) & (tmin <= b))
        cols = cols[np.argsort(near[cols], kind="stable")]
        if cols.size > PVB_CMAX:
            b = min(b, f(near[cols[PVB_CMAX]] * f(0.999999)))
            cols = cols[:PVB_CMAX]
            cols = cols[near[cols] <= b]
        count[k] = cols.size; bound[k] = b
        code[:cols.size, k] = code_of_col[cols].view(np.int32); nr[:cols.size, k] = near[cols]
    return {"count": count, "code": code, "nr": nr, "bound": bound}
