"""numpy restatement of the HDR environment (include/tirt.h, "HDR environment"), operation by operation in float32 with one rounding per operation, so the
device must give these bits.  Built on tests/env_sampling_expected.py and tests/texture_expected.py wherever the operations are shared (clamp, floor, mix, cos,
the table's sums, sample and pdf); only the texel decode, the level and the table's scale are stated here.

  decode(img)                 [w, h, 3] float32: mantissa * 2^(E - 136), exact (np.ldexp), denormals kept
  lookup(img, tx, ty)         texture2D on decoded texels, [n, 3]: the linear colour of the miss branch before env_power
  lookup_8bit(img, tx, ty)    srgb_to_lrgb(texture2D(img)) WITHOUT tex_albedo's non-finite rule: what the miss branch computes for any tx, ty
  e_max(img), cell_q(img), table(img, power)     the sampling table of an RGBE8 image, in the dict of env_sampling_expected.table
  shift_exponents(img, k)     every texel with a mantissa gets k added to its exponent byte (k clipped so that all of them stay in 1 .. 255)
  encode(rgb)                 the encoder Texture.load_array_float states, restated with Python integers ([h, w, 3] float -> [w, h] packed)
  radiance_patch()            context manager: env_sampling_expected.env_radiance is `lookup` inside it (step_on and nee_env then read an RGBE8 image)
"""
import contextlib
import math

import numpy as np

import env_sampling_expected as ee
import texture_expected as te

f = np.float32
TWO24 = f(16777216.0)


def unpack(img):
    """(R, G, B, E) int64 arrays of the packed texels"""
    t = np.asarray(img, np.int32).view(np.uint32).astype(np.int64)
    return (t >> 16) & 255, (t >> 8) & 255, t & 255, (t >> 24) & 255


def pack(r, g, b, e):
    t = (np.asarray(e, np.int64) << 24) | (np.asarray(r, np.int64) << 16) | (np.asarray(g, np.int64) << 8) | np.asarray(b, np.int64)
    return np.ascontiguousarray(t.astype(np.uint32).view(np.int32))


def decode(img):
    r, g, b, e = unpack(img)
    k = (e - 136).astype(np.int32)
    out = np.stack([np.ldexp(c.astype(f), k) for c in (r, g, b)], axis=-1)
    assert out.dtype == f
    return out


def _sample(dec, fx, fy):
    w, h = dec.shape[:2]
    with np.errstate(invalid="ignore"):
        xi = np.clip(fx.astype(np.int64), 0, w - 1)
        yi = np.clip(fy.astype(np.int64), 0, h - 1)
    return dec[xi, yi]


def _texture2d(sample, w, h, u, v):
    """texture_expected.texture2d with the texel fetch as a parameter"""
    u, v = np.asarray(u, f), np.asarray(v, f)
    with np.errstate(all="ignore"):
        x = te._minf(f(w) - f(1.0), te._maxf(f(0.0), (u * f(w)).astype(f)))
        y = te._minf(f(h) - f(1.0), te._maxf(f(0.0), (v * f(h)).astype(f)))
        lx, ly = te.tm_floor(x), te.tm_floor(y)
        wbt, wlr = (y - te.tm_floor(y)).astype(f), (x - te.tm_floor(x)).astype(f)
        lt, rt = sample(lx, ly), sample((lx + f(1.0)).astype(f), ly)
        lb, rb = sample(lx, (ly + f(1.0)).astype(f)), sample((lx + f(1.0)).astype(f), (ly + f(1.0)).astype(f))
        return _mix(_mix(lt, rt, wlr), _mix(lb, rb, wlr), wbt)


def _mix(a, b, t):
    """a * (1 - t) + b * t with every product and the sum rounded to float32"""
    t = t[..., None]
    return ((a * (f(1.0) - t).astype(f)).astype(f) + (b * t).astype(f)).astype(f)


def lookup(img, tx, ty):
    dec = decode(img)
    return _texture2d(lambda fx, fy: _sample(dec, fx, fy), dec.shape[0], dec.shape[1], tx, ty)


def lookup_8bit(img, tx, ty):
    img = np.asarray(img, np.int32)
    with np.errstate(all="ignore"):
        c = _texture2d(lambda fx, fy: te._sample(img, _nan_to_zero(fx), _nan_to_zero(fy)), img.shape[0], img.shape[1], tx, ty)
        return ee.srgb_to_lrgb(c)


def _nan_to_zero(x):
    return np.where(np.isnan(x), f(0.0), x).astype(f)       # (int) of a NaN is 0 on the device; the weights stay NaN, so every channel is NaN whatever the texel


def e_max(img):
    r, g, b, e = unpack(img)
    lit = (r | g | b) != 0
    return int(e[lit].max()) if lit.any() else 0


def texel_lum(img):
    d = decode(img)
    with np.errstate(over="ignore"):
        return (((d[..., 0] + d[..., 1]).astype(f) + d[..., 2]).astype(f) / f(3.0)).astype(f)


def cell_q(img):
    """[h, w] uint32: q(i, j) at [j, i]; env_sampling_expected.cell_q with the RGBE8 level and the scale 2^(152 - E_max) by ldexp"""
    w, h = np.asarray(img).shape
    lum = texel_lum(img)
    x1 = np.minimum(np.arange(w) + 1, w - 1)
    y1 = np.minimum(np.arange(h) + 1, h - 1)
    l00, l10, l01, l11 = lum, lum[x1, :], lum[:, y1], lum[x1, :][:, y1]
    with np.errstate(over="ignore"):
        m = (((l00 + l10).astype(f) + (l01 + l11).astype(f)).astype(f) * f(0.25)).astype(f)          # [w, h]
        el = ((((np.arange(h).astype(f) + f(0.5)).astype(f) / f(h)).astype(f) - f(0.5)).astype(f) * ee.PI_SCENE).astype(f)
        wgt = (m * ee.cos(el)[None, :]).astype(f)
        s = np.rint(np.ldexp(wgt, np.int32(152 - e_max(img))))
    assert s.dtype == f
    q = np.where(s > 0, np.where(s < TWO24, s, TWO24), f(0.0))
    return q.astype(np.uint32).T.copy()


def table(img, power=1.0):
    w, h = np.asarray(img).shape
    if float(power) == 0.0 or max(w, h) > ee.MAX_DIM or w * h > ee.MAX_CELLS:
        return None
    q = cell_q(img)
    rows = np.cumsum(q.astype(np.uint64), axis=1, dtype=np.uint64)
    marg = np.cumsum(rows[:, -1], dtype=np.uint64)
    total = int(marg[-1])
    if total == 0:
        return None
    return {"w": w, "h": h, "q": q, "row_sums": rows, "marginal": marg, "total": total}


def shift_exponents(img, k):
    r, g, b, e = unpack(img)
    lit = (r | g | b) != 0
    if lit.any():
        k = int(np.clip(k, 1 - int(e[lit].min()), 255 - int(e[lit].max())))       # one shift for all texels: k itself is clipped to what the range allows
    return pack(r, g, b, np.where(lit, e + k, e))


def encode(rgb):
    """[h, w, 3] float -> [w, h] packed RGBE8, y = 0 the bottom row: per texel, with exact rational arithmetic on Python floats (math.frexp / math.ldexp / floor)"""
    rgb = np.asarray(rgb, np.float64)
    hgt, wid = rgb.shape[:2]
    out = np.zeros((wid, hgt), np.int64)
    for i in range(hgt):
        for j in range(wid):
            c = [float(x) for x in rgb[i, j]]
            m = max(c)
            if m < 2.0 ** -135:
                continue
            E = min(255, max(1, math.frexp(m)[1] + 128))
            mant = [min(255, int(math.floor(math.ldexp(x, 136 - E)))) for x in c]
            out[j, hgt - 1 - i] = (E << 24) | (mant[0] << 16) | (mant[1] << 8) | mant[2]
    return np.ascontiguousarray(out.astype(np.uint32).view(np.int32))


def miss_term(img, power, rows, hdr=True):
    """radiance out of the miss rows of one shading step WITHOUT bit 1024 on a lit environment with power != 0: radiance + (L * throughput) * power"""
    rows = np.ascontiguousarray(rows)
    rf = rows.view(f)
    _, tx, ty = ee.lookup_coords(rf[:, 8:11])
    with np.errstate(all="ignore"):
        e = lookup(img, tx, ty) if hdr else lookup_8bit(img, tx, ty)
        return (rf[:, 18:21] + ((e * rf[:, 15:18]).astype(f) * f(power)).astype(f)).astype(f)


@contextlib.contextmanager
def radiance_patch():
    old = ee.env_radiance
    ee.env_radiance = lambda img, tx, ty: lookup(img, np.asarray(tx, f), np.asarray(ty, f))
    try:
        yield
    finally:
        ee.env_radiance = old
