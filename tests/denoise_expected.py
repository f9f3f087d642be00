"""The edge-avoiding a-trous denoiser (include/tirt.h, tirt_denoise) restated in numpy f32, tap by tap in the stated order, one f32 rounding
per operation.  exp is the shared tm_exp through the oracle's orc_kat_math fn 2 (tests/test_math.py, tests/test_gpu_math.py: the device's
is the same function bit for bit), so the device must give these bits.

Pixel (i, j) of a [W, H, .] array; from the feature record alb = words 0..2, n = 3..5, z = 6, al = 7.
  prepare   d = fmax(alb + (1 - al), 1e-3),  e = hdr / d,  rz = 1 / fmax(z*z, 1e-12)
  level l   step = 1 << l;  ic = 1 / (s*s), s = sigma_c * 2^-l;  in = 1 / sigma_n^2;  iz = 1 / sigma_z^2
            taps di = -2..2 (outer), dj = -2..2 (inner), q = (i + di*step, j + dj*step) inside the film:
              k = h[|di|] * h[|dj|], h = (0.375, 0.25, 0.0625)
              dc = ((e_p.r-e_q.r)^2 + (e_p.g-e_q.g)^2) + (e_p.b-e_q.b)^2,  dn the same over n,  dz = ((z_p-z_q)*(z_p-z_q)) * rz_p
              x = (dc*ic + dn*in) + dz*iz,  w = k * exp(-x);  counted only if w and all of e_q are finite: sum_c += e_q*w, sum_w += w
            e' = sum_c / sum_w;  a pixel whose own e is not finite keeps it
  finish    out = e * d"""
import numpy as np

import oracle_api as oa

f = np.float32
KERNEL = (f(0.375), f(0.25), f(0.0625))
DEFAULTS = dict(levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1)


def tm_exp(x):
    """the shared exp (tirt_math.h) on a float32 array of any shape"""
    x = np.ascontiguousarray(x, f)
    out = np.zeros_like(x)
    if x.size:
        oa.load().orc_kat_math(2, x.reshape(-1), np.zeros(x.size, f), out.reshape(-1), x.size)
    return out


def sq3(a, b):
    """((a0-b0)^2 + (a1-b1)^2) + (a2-b2)^2 over the last axis"""
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def prepare(hdr, aov):
    alb, n, z, al = aov[:, :, 0:3], aov[:, :, 3:6], aov[:, :, 6], aov[:, :, 7]
    d = np.fmax(alb + (f(1.0) - al)[:, :, None], f(1e-3))
    e = hdr / d
    rz = f(1.0) / np.fmax(z * z, f(1e-12))
    return e, d, n, z, rz


def level(e, n, z, rz, step, ic, in_, iz):
    W, H = z.shape
    sum_c, sum_w = np.zeros((W, H, 3), f), np.zeros((W, H), f)
    for di in range(-2, 3):
        oi = di * step
        i0, i1 = max(0, -oi), min(W, W - oi)               # rows i whose tap row i + oi is inside the film
        for dj in range(-2, 3):
            oj = dj * step
            j0, j1 = max(0, -oj), min(H, H - oj)
            if i0 >= i1 or j0 >= j1:
                continue
            P = (slice(i0, i1), slice(j0, j1))
            Q = (slice(i0 + oi, i1 + oi), slice(j0 + oj, j1 + oj))
            k = KERNEL[abs(di)] * KERNEL[abs(dj)]
            eq = e[Q]
            dc = sq3(e[P], eq)
            dn = sq3(n[P], n[Q])
            zd = z[P] - z[Q]
            dz = (zd * zd) * rz[P]
            x = (dc * ic + dn * in_) + dz * iz
            w = k * tm_exp(-x)
            ok = np.isfinite(w) & np.isfinite(eq).all(axis=2)
            sum_c[P] = np.where(ok[:, :, None], sum_c[P] + eq * w[:, :, None], sum_c[P])
            sum_w[P] = np.where(ok, sum_w[P] + w, sum_w[P])
    out = sum_c / sum_w[:, :, None]
    own = np.isfinite(e).all(axis=2)
    return np.where(own[:, :, None], out, e)


def denoise_expected(hdr, aov, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1):
    """[W, H, 3] float32 from hdr [W, H, 3] and the feature records [W, H, 8]"""
    hdr, aov = np.ascontiguousarray(hdr, f), np.ascontiguousarray(aov, f)
    assert hdr.ndim == 3 and hdr.shape[2] == 3 and aov.shape == hdr.shape[:2] + (8,)
    assert 1 <= levels <= 8 and all(np.isfinite(s) and s > 0 for s in (sigma_c, sigma_n, sigma_z))
    with np.errstate(all="ignore"):
        e, d, n, z, rz = prepare(hdr, aov)
        in_ = f(1.0) / (f(sigma_n) * f(sigma_n))
        iz = f(1.0) / (f(sigma_z) * f(sigma_z))
        for l in range(levels):
            s = f(sigma_c) * f(2.0 ** -l)                   # exact
            ic = f(1.0) / (s * s)
            e = level(e, n, z, rz, 1 << l, ic, in_, iz)
        out = e * d
    assert out.dtype == f
    return out
