"""The temporal accumulation (include/tirt.h, tirt_temporal_device) restated in numpy f32, operation by operation in the stated order, one f32 rounding
per operation.  The device must give these bits.

  1. al > 0, else NO HISTORY.  zc = z / al;  D = the camera ray through the pixel centre (oracle_api.camera_rays: the oracle's frame-0 rays, which carry
     no jitter -- the arithmetic of camera_ray_direction(cam, i, j, 0, 0));  X = eye + D * zc
  2. q = view_prev[3 x 4] . (X, 1), rows summed left to right;  q.z < 0, else NO HISTORY.  nz = -q.z;  fi = (q.x / nz) * fx + cx;  fj likewise;
     -1 < fi < W and -1 < fj < H, else NO HISTORY;  i0 = floor(fi), wi = fi - i0;  d_exp = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z), e = X - eye_prev
  3. taps (i0 + a, j0 + b), a outer, b inner, k = (a ? wi : 1 - wi) * (b ? wj : 1 - wj); counted if inside the film, al_h > 0, dn <= sigma_n*sigma_n,
     |d_exp - z_h / al_h| <= sigma_z * d_exp, n_h > 0, hdr_h, mean_h and M2_h finite: sw += k, sums += value * k.  sw >= 1e-3, else NO HISTORY; sums / sw
  4. n_h > max_history:  f = max_history / n_h;  n_h = max_history;  M2_h *= f;  bad_h *= f
  5. N = n_h + n_c.  n_c == 0: the history.  N == 0: NO HISTORY.  Else w = n_c / N, delta = mean_c - mean_h, mean_o = mean_h + delta * w,
     M2_o = (M2_h + M2_c) + (delta * delta) * (n_h * w), hdr_o = hdr_h + (hdr_c - hdr_h) * w, n_o = N, bad_o = bad_h + bad_c.
     A pixel whose own hdr_c is not finite keeps hdr_c
  6. NO HISTORY: the current pixel, bit for bit"""
import numpy as np

import oracle_api as oa

f = np.float32
DEFAULTS = dict(max_history=32.0, sigma_n=0.3, sigma_z=0.1)


class Cam:
    """A camera as it stood at one view: copies of what Camera pushes to tirt_camera_set (a Camera object changes under the next move)."""

    def __init__(self, cam):
        self.view_np = np.array(cam.view_np, np.float32).reshape(1, 4, 4)
        self.view_inv_np = np.array(cam.view_inv_np, np.float32).reshape(1, 4, 4)
        self.eye_np = np.array(cam.eye_np, np.float32).reshape(1, 3)
        self.fx, self.fy, self.cx, self.cy = cam.fx, cam.fy, cam.cx, cam.cy


def accumulate(hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cam, cam_prev, max_history=32.0, sigma_n=0.3, sigma_z=0.1, want_info=False):
    """(hdr_o [W, H, 3], mom_o [W, H, 8]) float32; with want_info also a dict of [W, H] masks and counts: history (the pixel took the merge or the
    history), behind (q.z >= 0), off_film (reprojected outside), rejected (reprojected inside the film, a tap with al_h > 0 failed the normal or the
    depth test, and no history came of it), rejected_taps, capped (the cap branch was taken)"""
    hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h = (np.ascontiguousarray(a, f) for a in (hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h))
    W, H = hdr_c.shape[:2]
    assert hdr_c.shape == (W, H, 3) and aov_c.shape == (W, H, 8) and mom_c.shape == (W, H, 8)
    assert hdr_h.shape == hdr_c.shape and aov_h.shape == aov_c.shape and mom_h.shape == mom_c.shape
    assert all(np.isfinite(v) and v > 0 for v in (max_history, sigma_n, sigma_z))
    NP = W * H
    hc, ac, mc = hdr_c.reshape(NP, 3), aov_c.reshape(NP, 8), mom_c.reshape(NP, 8)
    hh, ah, mh = hdr_h.reshape(NP, 3), aov_h.reshape(NP, 8), mom_h.reshape(NP, 8)
    max_history, sigma_z = f(max_history), f(sigma_z)
    sn2 = f(sigma_n) * f(sigma_n)
    with np.errstate(all="ignore"):
        # 1.
        nc3, z, al = ac[:, 3:6], ac[:, 6], ac[:, 7]
        m1 = al > 0
        zc = z / al
        rays = oa.camera_rays(cam, W, H)
        eye, D = rays[:, 0:3], rays[:, 3:6]
        X = eye + D * zc[:, None]
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
                rejected=(m3 & ~history & (guide_fail > 0)).reshape(W, H), rejected_taps=int(guide_fail.sum()), capped=capped.reshape(W, H))
    return hdr_o, mom_o, info


def sq3(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def first(hdr_c, aov_c, mom_c):
    """an accumulate on an empty history: the current film and records copied"""
    return np.array(hdr_c, f), np.array(mom_c, f)


def oracle_view(ex, orc, W, H, seed, frames=2):
    """(hdr, aov, mom) of `frames` frames (1 or 2: frames 0 and 1 give the oracle's exact samples, tests/moments_expected.py) of the example's camera as
    it stands, through the CPU oracle"""
    import aov_expected as ae
    import moments_expected as me
    assert frames in (1, 2)
    orc.set_camera(ex.cam)
    hdr, _ = orc.render(W, H, 0, frames, seed=seed)
    aov, _, _ = ae.expected(ex, orc, W, H, range(frames), seed)
    mom = me.expected([me.oracle_sample(orc, W, H, fr, seed) for fr in range(frames)], W, H)
    return hdr, aov, mom
