"""numpy restatement of the albedo textures (include/tirt.h, "Albedo textures on materials"), operation by operation in float32 with one rounding
per operation, so the device must give these bits.  pow is the shared tm_pow through the oracle's orc_kat_math fn 4 (tests/test_math.py,
tests/test_gpu_math.py: the device's is the same function bit for bit).

  tex_albedo(img [w, h] packed texels, wrap, u, v)
    finite(x) := |x| <= 3.4028234e38;  u, v = finite ? itself : 0;  wrap == 1: u = u - floor(u), v = v - floor(v)
    x = min(w - 1, max(0, u * w)), y likewise;  lx, ly = floor;  wlr = x - floor(x), wbt = y - floor(y)
    sample(fx, fy) = unpack(img[clamp((int)fx, 0, w - 1), clamp((int)fy, 0, h - 1)]) / 255
    c = mix(mix(lt, rt, wlr), mix(lb, rb, wlr), wbt),  mix(a, b, t) = a * (1 - t) + b * t
  hit_uv: (t1 * a + t2 * b) + t3 * c over the vertex rows' columns 6, 7, a = 1 - u - v
  texture_of: the 1-based id rule of a material row
  twin_materials: the untextured material table whose colours are the looked-up ones (the GPU tests compare a textured scene with this twin)
"""
import numpy as np

import oracle_api as oa
from ti_raytrace_amd import SceneData as SCD

f = np.float32
BIG = f(3.4028234e38)


def tm_floor(x):
    """t = (float)(int)x; t > x ? t - 1 : t   (|x| < 2^31)"""
    x = np.asarray(x, f)
    t = np.trunc(x).astype(f)
    return np.where(t > x, t - f(1.0), t).astype(f)


def _maxf(a, b):
    return np.where(a > b, a, b).astype(f)          # a > b ? a : b


def _minf(a, b):
    return np.where(a < b, a, b).astype(f)          # a < b ? a : b


def _sample(img, fx, fy):
    w, h = img.shape
    xi = np.clip(fx.astype(np.int64), 0, w - 1)
    yi = np.clip(fy.astype(np.int64), 0, h - 1)
    texel = img[xi, yi].astype(np.int64)
    ch = [((texel >> 16) & 255), ((texel >> 8) & 255), (texel & 255)]
    return np.stack([c.astype(f) / f(255.0) for c in ch], axis=-1).astype(f)


def _mix(a, b, t):
    t = t[..., None]
    return (a * (f(1.0) - t) + b * t).astype(f)


def texture2d(img, u, v):
    """texture/Texture.py:41-69 on an image [w, h]; u, v float32 arrays of one shape -> [..., 3]"""
    img = np.asarray(img, np.int32)
    w, h = img.shape
    u, v = np.asarray(u, f), np.asarray(v, f)
    x = _minf(f(w) - f(1.0), _maxf(f(0.0), u * f(w)))
    y = _minf(f(h) - f(1.0), _maxf(f(0.0), v * f(h)))
    lx, ly = tm_floor(x), tm_floor(y)
    wbt, wlr = (y - tm_floor(y)).astype(f), (x - tm_floor(x)).astype(f)
    lt, rt = _sample(img, lx, ly), _sample(img, lx + f(1.0), ly)
    lb, rb = _sample(img, lx, ly + f(1.0)), _sample(img, lx + f(1.0), ly + f(1.0))
    return _mix(_mix(lt, rt, wlr), _mix(lb, rb, wlr), wbt)


def tex_albedo(img, wrap, u, v):
    u, v = np.asarray(u, f).copy(), np.asarray(v, f).copy()
    u[~(np.abs(u) <= BIG)] = f(0.0)
    v[~(np.abs(v) <= BIG)] = f(0.0)
    if int(wrap) == 1:
        u = (u - tm_floor(u)).astype(f)
        v = (v - tm_floor(v)).astype(f)
    return texture2d(img, u, v)


def tm_pow(x, y):
    x = np.ascontiguousarray(x, f)
    out = np.zeros_like(x)
    if x.size:
        oa.load().orc_kat_math(4, x.reshape(-1), np.full(x.size, y, f), out.reshape(-1), x.size)
    return out


def srgb_to_lrgb(c):
    """UtilsFunc.py:76-94: c < 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4)"""
    c = np.ascontiguousarray(c, f)
    return np.where(c < f(0.04045), c / f(12.92), tm_pow((c + f(0.055)) / f(1.055), 2.4)).astype(f)


def hit_uv(vertex_np, primitive_np, prim, bu, bv):
    """(t1 * a + t2 * b) + t3 * c per component, a = 1 - u - v; shapes: 0.  -> (u[n], v[n])"""
    prim = np.asarray(prim)
    bu, bv = np.asarray(bu, f), np.asarray(bv, f)
    tri = primitive_np[prim, 0] == SCD.PRIMITIVE_TRI
    vi = np.where(tri, primitive_np[prim, 1], 0)
    a = ((f(1.0) - bu) - bv).astype(f)
    out = []
    for col in (6, 7):
        t1, t2, t3 = vertex_np[vi, col], vertex_np[vi + 1, col], vertex_np[vi + 2, col]
        out.append(np.where(tri, (t1 * a + t2 * bu) + t3 * bv, f(0.0)).astype(f))
    return out[0], out[1]


def texture_of(row, n_textures):
    """the texture number a material row names, or -1: textured iff n_textures >= 1, the row is not an emitter's and 1 <= (int)row[1] <= n_textures"""
    slot = int(row[1]) if np.isfinite(row[1]) else 0
    if n_textures >= 1 and int(row[0]) != SCD.MAT_LIGHT and 1 <= slot <= n_textures:
        return slot - 1
    return -1


def albedo_at(material_np, textures, mat, u, v):
    """the encoded colour of hits on materials mat[n] at uv: the row's words 2..4, or tex_albedo of its texture.  textures: [(img [w, h], wrap)]"""
    mat = np.asarray(mat)
    out = material_np[mat, 2:5].astype(f).copy()
    for m in np.unique(mat):
        t = texture_of(material_np[m], len(textures))
        if t >= 0:
            sel = mat == m
            out[sel] = tex_albedo(textures[t][0], textures[t][1], np.asarray(u, f)[sel], np.asarray(v, f)[sel])
    return out


def twin_materials(material_np, textures, uv_of_material):
    """the twin of a textured table: every textured row gets the looked-up colour at uv_of_material[m] = (u, v) and slot -1"""
    twin = material_np.copy()
    for m in range(material_np.shape[0]):
        t = texture_of(material_np[m], len(textures))
        if t >= 0:
            u, v = uv_of_material[m]
            twin[m, 2:5] = tex_albedo(textures[t][0], textures[t][1], np.array([u], f), np.array([v], f))[0]
        twin[m, 1] = -1.0
    return twin
