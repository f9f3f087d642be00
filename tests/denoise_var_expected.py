"""The variance-guided mode of the a-trous denoiser (include/tirt.h, tirt_denoise_var) restated in numpy f32, tap by tap in the stated order, one
f32 rounding per operation; exp is the shared tm_exp through the oracle (tests/denoise_expected.py).  The device must give these bits.

  prepare    d, e = hdr / d, z as tirt_denoise;  s = -1 unless n >= 2 and t = (v.r/(d.r*d.r) + v.g/(d.g*d.g)) + v.b/(d.b*d.b), v = M2 / (n*(n-1)),
             is KNOWN (0 <= t < inf): then s = t.  A pixel whose s is not known keeps it to the end and has no colour term.
  prefilter  known s:  s = sum(k*s_q) / sum(k) over the in-film 3 x 3 taps (di outer, dj inner) with a known s_q, k = g[|di|]*g[|dj|], g = (0.5, 0.25)
  level l    step = 1 << l;  sc2 = sigma_c*sigma_c;  rz = 1 / fmax(z*z, 1e-12);  cden = sc2*s_p + 1e-12;  taps, k, dc, dn, dz as tirt_denoise
             xc = dc / cden if s_p known else 0;  x = (xc + dn*in) + dz*iz;  w = k * exp(-x);  counted if w and e_q finite:
             sum_c += e_q*w, sum_w += w, and with s_q known  sum_v += (w*w)*s_q, sum_wv += w
             e' as tirt_denoise;  s' = sum_v / (sum_wv*sum_wv) if s_p known and sum_wv > 0 else s_p
  finish     out = e * d"""
import numpy as np

import denoise_expected as de

f = np.float32
DEFAULTS = dict(levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1)
G3 = (f(0.5), f(0.25))


def known(s):
    with np.errstate(invalid="ignore"):
        return (s >= 0) & (s < np.inf)


def prepare(hdr, aov, mom):
    e, d, n, z, _ = de.prepare(hdr, aov)
    cnt = mom[:, :, 0]
    nn = cnt * (cnt - f(1.0))
    v = mom[:, :, 4:7] / nn[:, :, None]
    q = v / (d * d)
    t = (q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]
    with np.errstate(invalid="ignore"):
        ok = (cnt >= 2) & known(t)
    s = np.where(ok, t, f(-1.0)).astype(f)
    return e, d, n, z, s


def prefilter(s):
    W, H = s.shape
    ss, sk = np.zeros((W, H), f), np.zeros((W, H), f)
    kn = known(s)
    for di in range(-1, 2):
        i0, i1 = max(0, -di), min(W, W - di)
        for dj in range(-1, 2):
            j0, j1 = max(0, -dj), min(H, H - dj)
            if i0 >= i1 or j0 >= j1:
                continue
            P = (slice(i0, i1), slice(j0, j1))
            Q = (slice(i0 + di, i1 + di), slice(j0 + dj, j1 + dj))
            k = G3[abs(di)] * G3[abs(dj)]
            ss[P] = np.where(kn[Q], ss[P] + k * s[Q], ss[P])
            sk[P] = np.where(kn[Q], sk[P] + k, sk[P])
    return np.where(kn, ss / sk, s).astype(f)


def level(e, s, n, z, step, sc2, in_, iz):
    W, H = z.shape
    rz = f(1.0) / np.fmax(z * z, f(1e-12))
    colour = known(s)
    cden = sc2 * s + f(1e-12)
    sum_c, sum_w = np.zeros((W, H, 3), f), np.zeros((W, H), f)
    sum_v, sum_wv = np.zeros((W, H), f), np.zeros((W, H), f)
    for di in range(-2, 3):
        oi = di * step
        i0, i1 = max(0, -oi), min(W, W - oi)
        for dj in range(-2, 3):
            oj = dj * step
            j0, j1 = max(0, -oj), min(H, H - oj)
            if i0 >= i1 or j0 >= j1:
                continue
            P = (slice(i0, i1), slice(j0, j1))
            Q = (slice(i0 + oi, i1 + oi), slice(j0 + oj, j1 + oj))
            k = de.KERNEL[abs(di)] * de.KERNEL[abs(dj)]
            eq, sq = e[Q], s[Q]
            dc = de.sq3(e[P], eq)
            dn = de.sq3(n[P], n[Q])
            zd = z[P] - z[Q]
            dz = (zd * zd) * rz[P]
            xc = np.where(colour[P], dc / cden[P], f(0.0))
            x = (xc + dn * in_) + dz * iz
            w = k * de.tm_exp(-x)
            ok = np.isfinite(w) & np.isfinite(eq).all(axis=2)
            sum_c[P] = np.where(ok[:, :, None], sum_c[P] + eq * w[:, :, None], sum_c[P])
            sum_w[P] = np.where(ok, sum_w[P] + w, sum_w[P])
            okv = ok & known(sq)
            sum_v[P] = np.where(okv, sum_v[P] + (w * w) * sq, sum_v[P])
            sum_wv[P] = np.where(okv, sum_wv[P] + w, sum_wv[P])
    out = sum_c / sum_w[:, :, None]
    own = np.isfinite(e).all(axis=2)
    e1 = np.where(own[:, :, None], out, e)
    s1 = np.where(colour & (sum_wv > 0), sum_v / (sum_wv * sum_wv), s)
    return e1.astype(f), s1.astype(f)


def denoise_var_expected(hdr, aov, mom, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1, want_s=False):
    """[W, H, 3] float32 from hdr [W, H, 3], the feature records [W, H, 8] and the moment records [W, H, 8]"""
    hdr, aov, mom = np.ascontiguousarray(hdr, f), np.ascontiguousarray(aov, f), np.ascontiguousarray(mom, f)
    assert hdr.ndim == 3 and hdr.shape[2] == 3 and aov.shape == hdr.shape[:2] + (8,) and mom.shape == aov.shape
    assert 1 <= levels <= 8 and all(np.isfinite(v) and v > 0 for v in (sigma_c, sigma_n, sigma_z))
    with np.errstate(all="ignore"):
        e, d, n, z, s = prepare(hdr, aov, mom)
        s = prefilter(s)
        sc2 = f(sigma_c) * f(sigma_c)
        in_ = f(1.0) / (f(sigma_n) * f(sigma_n))
        iz = f(1.0) / (f(sigma_z) * f(sigma_z))
        for l in range(levels):
            e, s = level(e, s, n, z, 1 << l, sc2, in_, iz)
        out = e * d
    assert out.dtype == f and s.dtype == f
    return (out, s) if want_s else out
