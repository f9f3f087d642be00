"""The motion records and the accumulation with them (include/tirt.h, tirt_motion_enable) restated in numpy f32, operation by operation in the stated
order, one f32 rounding per operation.  The device must give these bits.

  record      the camera ray through the pixel centre and its closest hit (t, u, v, prim): oracle_api.camera_rays and OracleScene.closest_hit(uv=True)
              on the CPU.  For a triangle with first vertex vi, a = 1 - u - v, on vertex rows R [nv, 9] (position 0..2, normal 3..5):
                P(R) = (v1*a + v2*u) + v3*v,   N(R) = x * (1 / sqrt((x.x*x.x + x.y*x.y) + x.z*x.z)),  x = (n1*a + n2*u) + n3*v
              words 0..2 = P(snapshot) - P(current), word 3 = 1, words 4..6 = N(snapshot) - N(current), word 7 = 0; a miss or a shape: eight zeros
  accumulate  temporal_expected.accumulate with two additions to its step 1: X = X + D_motion after X = eye + D * zc, and n_c = n_c + dN before the
              taps' normal test.  Restated here in full, because X is formed inside that function; with a record of zeros the two must agree bit
              for bit (tests/test_motion_host.py holds them to it).

Also what a test needs to move geometry the way the device does: the face normals k_dyn_scatter writes (Scene.cal_normal's, in double from the f32
positions), triangles chosen by a bounding box, and the tiny state machine of the snapshot rule."""
import numpy as np

import oracle_api as oa
from temporal_expected import sq3

f = np.float32
WORDS = 8
INF_VALUE = f(1000000.0)


# ---- moving geometry on the host -----------------------------------------------------------------------------------------------------------
def triangles_inside(rows, lo, hi):
    """indices of the triangles of vertex rows [nv, 9] whose three vertices lie inside the box lo .. hi"""
    tri = np.asarray(rows)[:, 0:3].reshape(-1, 3, 3)
    ok = ((tri >= np.asarray(lo, f)) & (tri <= np.asarray(hi, f))).all(axis=(1, 2))
    return np.nonzero(ok)[0]


def face_normals(pos):
    """[k, 3] float32 per triangle of pos [k, 3, 3] float32: normalize((v1 - v0) x (v2 - v0)) in double, rounded once (Scene.cal_normal, k_dyn_scatter)"""
    p = np.asarray(pos, f).astype(np.float64)
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return (n * inv[:, None]).astype(f)


def moved_rows(rows, tris, new_pos):
    """vertex rows after an update of the triangles `tris` to new_pos [len(tris), 3, 3] without normals: positions as given, face normals"""
    out = np.array(rows, f)
    new_pos = np.asarray(new_pos, f).reshape(-1, 3, 3)
    nrm = face_normals(new_pos)
    for k in range(3):
        out[3 * np.asarray(tris) + k, 0:3] = new_pos[:, k]
        out[3 * np.asarray(tris) + k, 3:6] = nrm
    return out


def translated(rows, tris, shift):
    pos = np.asarray(rows, f)[:, 0:3].reshape(-1, 3, 3)[tris]
    return (pos + np.asarray(shift, f)).astype(f)


def rotated_y(rows, tris, angle):
    """the triangles turned by `angle` about the vertical (y) axis through the middle of their bounding box, in double, rounded once"""
    pos = np.asarray(rows, f)[:, 0:3].reshape(-1, 3, 3)[tris].astype(np.float64)
    c = 0.5 * (pos.reshape(-1, 3).min(axis=0) + pos.reshape(-1, 3).max(axis=0))
    d = pos - c
    cs, sn = np.cos(angle), np.sin(angle)
    out = np.stack([c[0] + cs * d[..., 0] + sn * d[..., 2], pos[..., 1], c[2] - sn * d[..., 0] + cs * d[..., 2]], axis=-1)
    return out.astype(f)


# The Cornell box's two blocks by their bounding boxes (assets/model/cornell_box.obj) and the moves of the tests: the short block pushed sideways by
# about 1.5 pixels at its depth, the tall block turned about its vertical axis (its normals change: dN is not zero)
CASES = {"translate": ((80.0, -1.0, -274.0), (292.0, 166.0, -63.0)), "rotate": ((263.0, -1.0, -458.0), (474.0, 331.0, -245.0))}
SHIFT_PIXELS, ROTATE_ANGLE = 1.5, 0.2


def block_triangles(rows, case):
    """the ten triangles (five faces) of the block of a case of CASES, by bounding box on the vertex rows"""
    tris = triangles_inside(rows, *CASES[case])
    tris = tris[np.asarray(rows)[:, 1].reshape(-1, 3)[tris].max(axis=1) > 0]          # (not the pieces of the floor under the block)
    assert len(tris) == 10, (case, tris)
    return tris


def move(case, rows, cam, W):
    """(triangle indices, their new positions [k, 3, 3]) of a case of CASES on vertex rows, for a camera (fx is in pixels of a film W wide)"""
    tris = block_triangles(rows, case)
    if case == "rotate":
        return tris, rotated_y(rows, tris, ROTATE_ANGLE)
    centre = np.asarray(rows, f)[:, 0:3].reshape(-1, 3, 3)[tris].reshape(-1, 3).astype(np.float64).mean(axis=0)
    depth = float(np.linalg.norm(np.asarray(cam.eye_np, np.float64).reshape(3) - centre))
    return tris, translated(rows, tris, (-SHIFT_PIXELS * depth / float(cam.fx), 0.0, 0.0))


class SnapshotModel:
    """The snapshot rule of include/tirt.h as a state machine over vertex rows: what tirt_vertex_update, tirt_temporal_accumulate, tirt_temporal_reset
    and tirt_scene_upload do to (history valid, moved, snapshot) while motion records are on or off."""

    def __init__(self, rows, motion=True):
        self.rows, self.motion = np.array(rows, f), motion
        self.valid, self.moved, self.snapshot = False, False, None

    def update(self, new_rows):
        if self.motion and self.valid:
            if not self.moved:
                self.snapshot, self.moved = self.rows.copy(), True
        else:
            self.valid = False
        self.rows = np.array(new_rows, f)

    def accumulate(self):
        """('first' | 'static' | 'motion', snapshot rows or None): the branch the accumulate takes and the rows its records compare with"""
        how = "first" if not self.valid else ("motion" if self.motion and self.moved else "static")
        snap = self.snapshot if how == "motion" else None
        self.valid, self.moved = True, False
        return how, snap

    def reset(self):
        self.valid, self.moved = False, False

    upload = reset


# ---- the record ----------------------------------------------------------------------------------------------------------------------------------
def centre_hits(orc, cam, W, H):
    """(hit [W*H] bool, prim [W*H], u, v) of the pixel-centre camera rays through the CPU oracle (its scene holds the CURRENT geometry)"""
    rays = oa.camera_rays(cam, W, H)
    out, prim, _, bary = orc.closest_hit(rays, uv=True)
    return out[:, 0] < INF_VALUE, prim, np.ascontiguousarray(bary[:, 0], f), np.ascontiguousarray(bary[:, 1], f)


def point_normal(rows, vi, a, u, v):
    rows = np.asarray(rows, f)
    v1, v2, v3 = rows[vi, 0:3], rows[vi + 1, 0:3], rows[vi + 2, 0:3]
    n1, n2, n3 = rows[vi, 3:6], rows[vi + 1, 3:6], rows[vi + 2, 3:6]
    a, u, v = a[:, None], u[:, None], v[:, None]
    with np.errstate(all="ignore"):
        P = (v1 * a + v2 * u) + v3 * v
        x = (n1 * a + n2 * u) + n3 * v
        inv = f(1.0) / np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        N = x * inv[:, None]
    return P.astype(f), N.astype(f)


def record(hit, prim, u, v, primitive_np, cur_rows, snap_rows, W, H):
    """[W, H, 8] float32"""
    prim = np.where(hit, prim, 0)
    tri = hit & (primitive_np[prim, 0] == 1)                       # PRIMITIVE_TRI
    vi = np.where(tri, primitive_np[prim, 1], 0)
    a = (f(1.0) - u) - v
    Pc, Nc = point_normal(cur_rows, vi, a, u, v)
    Ps, Ns = point_normal(snap_rows, vi, a, u, v)
    rec = np.zeros((W * H, WORDS), f)
    with np.errstate(all="ignore"):
        rec[:, 0:3] = Ps - Pc
        rec[:, 3] = f(1.0)
        rec[:, 4:7] = Ns - Nc
    rec[~tri] = 0
    return rec.reshape(W, H, WORDS)


# ---- the accumulation with records ---------------------------------------------------------------------------------------------------------------
def accumulate_mv(hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cam, cam_prev, motion, max_history=32.0, sigma_n=0.3, sigma_z=0.1, want_info=False):
    """temporal_expected.accumulate's results and info; info also has tap_i0, tap_j0 [W, H] (the first tap's position where the reprojection lies inside
    the film, else -2) so that a test can tell one reprojection from another"""
    hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, motion = (np.ascontiguousarray(a, f) for a in (hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, motion))
    W, H = hdr_c.shape[:2]
    assert hdr_c.shape == (W, H, 3) and aov_c.shape == (W, H, 8) and mom_c.shape == (W, H, 8) and motion.shape == (W, H, WORDS)
    assert hdr_h.shape == hdr_c.shape and aov_h.shape == aov_c.shape and mom_h.shape == mom_c.shape
    assert all(np.isfinite(v) and v > 0 for v in (max_history, sigma_n, sigma_z))
    NP = W * H
    hc, ac, mc, mv = hdr_c.reshape(NP, 3), aov_c.reshape(NP, 8), mom_c.reshape(NP, 8), motion.reshape(NP, WORDS)
    hh, ah, mh = hdr_h.reshape(NP, 3), aov_h.reshape(NP, 8), mom_h.reshape(NP, 8)
    max_history, sigma_z = f(max_history), f(sigma_z)
    sn2 = f(sigma_n) * f(sigma_n)
    with np.errstate(all="ignore"):
        # 1.
        z, al = ac[:, 6], ac[:, 7]
        m1 = al > 0
        zc = z / al
        rays = oa.camera_rays(cam, W, H)
        eye, D = rays[:, 0:3], rays[:, 3:6]
        X = eye + D * zc[:, None]
        X = X + mv[:, 0:3]                                         # to where the surface was
        nc3 = ac[:, 3:6] + mv[:, 4:7]                              # with the normal it had
        # 2.
        V = cam_prev.view_np[0].astype(f)
        q = [((V[r, 0] * X[:, 0] + V[r, 1] * X[:, 1]) + V[r, 2] * X[:, 2]) + V[r, 3] for r in range(3)]
        m2 = m1 & (q[2] < 0)
        nz = -q[2]
        fi = (q[0] / nz) * f(cam_prev.fx) + f(cam_prev.cx)
        fj = (q[1] / nz) * f(cam_prev.fy) + f(cam_prev.cy)
        inside = (fi > -1) & (fi < W) & (fj > -1) & (fj < H)
        m3 = m2 & inside
        fi, fj = np.where(m3, fi, f(0.0)), np.where(m3, fj, f(0.0))
        fi0, fj0 = np.floor(fi), np.floor(fj)
        i0, j0 = fi0.astype(np.int64), fj0.astype(np.int64)
        wi, wj = fi - fi0, fj - fj0
        e = X - cam_prev.eye_np[0].astype(f)[None, :]
        d_exp = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        ztol = sigma_z * d_exp
        # 3.
        sw = np.zeros(NP, f)
        s_hdr, s_mom = np.zeros((NP, 3), f), np.zeros((NP, 8), f)
        guide_fail = np.zeros(NP, np.int64)
        for a in (0, 1):
            ti = i0 + a
            for b in (0, 1):
                tj = j0 + b
                ok = m3 & (ti >= 0) & (ti < W) & (tj >= 0) & (tj < H)
                t = np.where(ok, ti * H + tj, 0)
                g, mo, hd = ah[t], mh[t], hh[t]
                ok = ok & (g[:, 7] > 0)
                dn = sq3(nc3, g[:, 3:6])
                zh = g[:, 6] / g[:, 7]
                guides = (dn <= sn2) & (np.abs(d_exp - zh) <= ztol)
                guide_fail += ok & ~guides
                ok = ok & guides & (mo[:, 0] > 0) & np.isfinite(hd).all(axis=1) & np.isfinite(mo[:, 1:7]).all(axis=1)
                k = (wi if a else f(1.0) - wi) * (wj if b else f(1.0) - wj)
                sw = np.where(ok, sw + k, sw)
                s_hdr = np.where(ok[:, None], s_hdr + hd * k[:, None], s_hdr)
                s_mom = np.where(ok[:, None], s_mom + mo * k[:, None], s_mom)
        m4 = m3 & (sw >= f(1e-3))
        g_hdr = s_hdr / sw[:, None]
        g_mom = s_mom / sw[:, None]
        nh, mean_h, m2_h, bad_h = g_mom[:, 0], g_mom[:, 1:4], g_mom[:, 4:7], g_mom[:, 7]
        # 4.
        capped = m4 & (nh > max_history)
        fcap = max_history / nh
        m2_h = np.where(capped[:, None], m2_h * fcap[:, None], m2_h)
        bad_h = np.where(capped, bad_h * fcap, bad_h)
        nh = np.where(capped, max_history, nh)
        # 5.
        n_c, mean_c, m2_c, bad_c = mc[:, 0], mc[:, 1:4], mc[:, 4:7], mc[:, 7]
        N = nh + n_c
        take_hist = m4 & (n_c == 0)
        merge = m4 & ~take_hist & ~(N == 0)
        w = n_c / N
        nw = nh * w
        delta = mean_c - mean_h
        mom_m = np.zeros((NP, 8), f)
        mom_m[:, 0] = N
        mom_m[:, 1:4] = mean_h + delta * w[:, None]
        mom_m[:, 4:7] = (m2_h + m2_c) + (delta * delta) * nw[:, None]
        mom_m[:, 7] = bad_h + bad_c
        hdr_m = g_hdr + (hc - g_hdr) * w[:, None]
        mom_hist = np.concatenate([nh[:, None], mean_h, m2_h, bad_h[:, None]], axis=1).astype(f)
        hdr_o = np.where(merge[:, None], hdr_m, np.where(take_hist[:, None], g_hdr, hc))
        own_bad = ~np.isfinite(hc).all(axis=1)
        hdr_o = np.where(own_bad[:, None], hc, hdr_o)
        mom_o = np.where(merge[:, None], mom_m, np.where(take_hist[:, None], mom_hist, mc))
    hdr_o, mom_o = np.ascontiguousarray(hdr_o.reshape(W, H, 3)), np.ascontiguousarray(mom_o.reshape(W, H, 8))
    assert hdr_o.dtype == f and mom_o.dtype == f
    if not want_info:
        return hdr_o, mom_o
    history = merge | take_hist
    info = dict(history=history.reshape(W, H), hit=m1.reshape(W, H), behind=(m1 & ~m2).reshape(W, H), off_film=(m2 & ~m3).reshape(W, H),
                rejected=(m3 & ~history & (guide_fail > 0)).reshape(W, H), rejected_taps=int(guide_fail.sum()), capped=capped.reshape(W, H),
                tap_i0=np.where(m3, i0, -2).reshape(W, H), tap_j0=np.where(m3, j0, -2).reshape(W, H))
    return hdr_o, mom_o, info
