"""numpy restatement of the alpha cut-outs (include/tirt.h, "Alpha cut-outs"), operation by operation in float32 with one rounding per operation, so the
device must give these bits.  The oracle knows nothing of textures; tests/test_cutout_host.py shows that with every flag off `closest_hit` below IS the
oracle's closest hit, bit for bit, on every ray it keeps -- which is what entitles it to judge the device with the flags on.

  tex_alpha(img [w, h] packed texels, wrap, u, v): the fourth channel of texture_expected.tex_albedo's lookup (its coordinate code, `coords`, is shared):
    alpha(texel) = (255 - ((texel >> 24) & 255)) / 255;  mix(mix(lt, rt, wlr), mix(lb, rb, wlr), wbt)
  closest_hit: every ray against every primitive -- Moller-Trumbore and the analytic sphere in the reference's operation order (Scene.py:529-638), a
    candidate is 0 < t < INF_VALUE; among the candidates that pass the alpha rule the smallest t wins, and among equal t the larger compact-node index
    of the leaf (the device's equal-distance rule; with strict `t < best` otherwise, the result does not depend on the order of the visits).
  kept: the device also requires that the reference's walk reaches the leaf; `slabs` on the leaf's own exact box implies every ancestor's.  A ray one of
    whose candidates -- in any layer, accepted or not -- fails `slabs` on its own box is EXCLUDED (only for those would the ancestor walk matter).  The
    tests cap the excluded share at 1 %.
"""
import numpy as np

import texture_expected as te
from ti_raytrace_amd import SceneData as SCD

f = np.float32
INF_VALUE = f(1000000.0)
CUTOFF = f(0.5)


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------
def coords(shape, wrap, u, v):
    """steps 1 and 2 of tex_albedo and texture2D's x, y -> (lx, ly, wlr, wbt), all float32"""
    w, h = shape
    u, v = np.asarray(u, f).copy(), np.asarray(v, f).copy()
    u[~(np.abs(u) <= te.BIG)] = f(0.0)
    v[~(np.abs(v) <= te.BIG)] = f(0.0)
    if int(wrap) == 1:
        u = (u - te.tm_floor(u)).astype(f)
        v = (v - te.tm_floor(v)).astype(f)
    x = te._minf(f(w) - f(1.0), te._maxf(f(0.0), u * f(w)))
    y = te._minf(f(h) - f(1.0), te._maxf(f(0.0), v * f(h)))
    lx, ly = te.tm_floor(x), te.tm_floor(y)
    return lx, ly, (x - te.tm_floor(x)).astype(f), (y - te.tm_floor(y)).astype(f)


def _alpha_sample(img, fx, fy):
    w, h = img.shape
    xi = np.clip(fx.astype(np.int64), 0, w - 1)
    yi = np.clip(fy.astype(np.int64), 0, h - 1)
    texel = img[xi, yi].astype(np.int64)
    return ((255 - ((texel >> 24) & 255)).astype(f) / f(255.0)).astype(f)


def _mixf(a, b, t):
    return (a * (f(1.0) - t) + b * t).astype(f)


def tex_alpha(img, wrap, u, v):
    img = np.asarray(img, np.int32)
    lx, ly, wlr, wbt = coords(img.shape, wrap, u, v)
    lt, rt = _alpha_sample(img, lx, ly), _alpha_sample(img, lx + f(1.0), ly)
    lb, rb = _alpha_sample(img, lx, ly + f(1.0)), _alpha_sample(img, lx + f(1.0), ly + f(1.0))
    return _mixf(_mixf(lt, rt, wlr), _mixf(lb, rb, wlr), wbt)


def pack_rgba(rgba):
    """[h, w, 4] uint8, row 0 the top -> [w, h] int32 texels, (255 - A) << 24 | R << 16 | G << 8 | B (Texture.load_array_rgba restated)"""
    a = np.asarray(rgba).astype(np.int64)
    p = ((255 - a[..., 3]) << 24) | (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]
    return np.ascontiguousarray(p[::-1, :].T.astype(np.uint32).view(np.int32))


def cutout_texture_of(row, n_textures, flags):
    """the cut-out texture a triangle's material row names, or -1"""
    t = te.texture_of(row, n_textures)
    return t if (t >= 0 and len(flags) == n_textures and int(flags[t]) == 1) else -1


# ---- the primitive tests ------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(f)


def _cross(a, b):
    return [(a[1] * b[2] - a[2] * b[1]).astype(f), (a[2] * b[0] - a[0] * b[2]).astype(f), (a[0] * b[1] - a[1] * b[0]).astype(f)]


def intersect_tri(o, d, v0, v1, v2):
    """Scene.py:603-638 on E1 = v1 - v0, E2 = v2 - v0; o, d: lists of three [n] arrays; v*: three scalars -> (t, u, v), t = INF_VALUE for no hit"""
    n = o[0].shape[0]
    E1 = [np.full(n, f(v1[k]) - f(v0[k]), f) for k in range(3)]
    E2 = [np.full(n, f(v2[k]) - f(v0[k]), f) for k in range(3)]
    P = _cross(d, E2)
    det = _dot(E1, P)
    pos = det > f(0.0)
    T = [np.where(pos, o[k] - f(v0[k]), f(v0[k]) - o[k]).astype(f) for k in range(3)]
    det = np.where(pos, det, -det).astype(f)
    u = _dot(T, P)
    Q = _cross(T, E1)
    v = _dot(d, Q)
    t = _dot(E2, Q)
    with np.errstate(all="ignore"):
        ok = (det > f(0.0)) & (u >= f(0.0)) & (u <= det) & (v >= f(0.0)) & ((u + v).astype(f) <= det)
        inv = (f(1.0) / det).astype(f)
        t, u, v = (t * inv).astype(f), (u * inv).astype(f), (v * inv).astype(f)
    return np.where(ok, t, INF_VALUE).astype(f), np.where(ok, u, f(0.0)).astype(f), np.where(ok, v, f(0.0)).astype(f)


def intersect_sphere(o, d, c, r):
    """Scene.py:565-596: t = (-b - sqrt(b^2 - 4ac)) / 2 / a where the ray passes within r of the centre, else INF_VALUE"""
    r = f(r)
    oc = [(f(c[k]) - o[k]).astype(f) for k in range(3)]
    oc2 = _dot(oc, oc)
    op = _dot(d, oc)
    with np.errstate(all="ignore"):
        cp = np.sqrt((oc2 - op * op).astype(f)).astype(f)
        a = _dot(d, d)
        b = (f(-2.0) * op).astype(f)
        cc = (oc2 - r * r).astype(f)
        t = (((-b - np.sqrt((b * b - (f(4.0) * a).astype(f) * cc).astype(f)).astype(f)).astype(f) / f(2.0)).astype(f) / a).astype(f)
    return np.where(cp < r, t, INF_VALUE).astype(f)


def slabs(o, d, mn, mx):
    """UtilsFunc.py:494-523 on one box (mn, mx: three scalars each) for rays o, d -> bool [n]"""
    n = o[0].shape[0]
    ret = np.ones(n, bool)
    tmin = np.zeros(n, f); tmax = np.full(n, INF_VALUE, f)
    with np.errstate(all="ignore"):
        for k in range(3):
            par = np.abs(d[k]) < f(0.000001)
            ood = (f(1.0) / d[k]).astype(f)
            t1 = ((f(mn[k]) - o[k]).astype(f) * ood).astype(f)
            t2 = ((f(mx[k]) - o[k]).astype(f) * ood).astype(f)
            lo, hi = np.where(t1 > t2, t2, t1), np.where(t1 > t2, t1, t2)
            ntmin = np.where(lo > tmin, lo, tmin); ntmax = np.where(hi < tmax, hi, tmax)
            ret &= np.where(par, ~((o[k] < f(mn[k])) | (o[k] > f(mx[k]))), ~(ntmin > ntmax))
            tmin = np.where(par, tmin, ntmin).astype(f); tmax = np.where(par, tmax, ntmax).astype(f)
    return ret


def leaf_indices(compact):
    """compact index of every primitive's leaf, from the reference's compact_node rows (word 0 odd: a leaf, word 1 its primitive)"""
    compact = np.asarray(compact)
    rows = np.where((compact[:, 0].astype(np.int64) & 1) == 1)[0]
    out = np.full(rows.size, -1, np.int64)
    out[compact[rows, 1].astype(np.int64)] = rows
    assert (out >= 0).all()
    return out


def closest_hit(vertex_np, primitive_np, material_np, shape_np, textures, flags, rays, leaf=None):
    """-> dict t, u, v (the barycentrics), prim (-1: miss), kept, ties (rays that met two candidates at one distance).  textures: [(img [w, h], wrap)], flags: one 0 / 1 per texture (or empty)"""
    rays = np.ascontiguousarray(rays, f).reshape(-1, 6)
    n = rays.shape[0]
    o = [rays[:, k].copy() for k in range(3)]; d = [rays[:, 3 + k].copy() for k in range(3)]
    best_t = np.full(n, INF_VALUE, f); best_u = np.zeros(n, f); best_v = np.zeros(n, f)
    best_prim = np.full(n, -1, np.int64); best_leaf = np.full(n, -1, np.int64)
    kept = np.ones(n, bool); ties = np.zeros(n, bool)
    if leaf is None:
        leaf = np.arange(primitive_np.shape[0])
    for p in range(primitive_np.shape[0]):
        kind, idx, mat = (int(x) for x in primitive_np[p])
        if kind == SCD.PRIMITIVE_TRI:
            V = vertex_np[idx:idx + 3]
            t, u, v = intersect_tri(o, d, V[0, 0:3], V[1, 0:3], V[2, 0:3])
            mn, mx = V[:, 0:3].min(axis=0), V[:, 0:3].max(axis=0)
        else:
            sh = shape_np[idx]
            t = intersect_sphere(o, d, sh[1:4], sh[4]) if int(sh[0]) == 1 else np.full(n, INF_VALUE, f)
            u = np.zeros(n, f); v = np.zeros(n, f)
            rr = f(sh[4]); mn = sh[1:4].astype(f) - rr; mx = sh[1:4].astype(f) + rr
        cand = (t > f(0.0)) & (t < INF_VALUE)
        kept &= ~(cand & ~slabs(o, d, mn, mx))
        tex = cutout_texture_of(material_np[mat], len(textures), flags) if kind == SCD.PRIMITIVE_TRI else -1
        if tex >= 0:
            a = ((f(1.0) - u) - v).astype(f)
            T = vertex_np[idx:idx + 3, 6:8].astype(f)
            tu = ((T[0, 0] * a + T[1, 0] * u).astype(f) + T[2, 0] * v).astype(f)
            tv = ((T[0, 1] * a + T[1, 1] * u).astype(f) + T[2, 1] * v).astype(f)
            cand &= tex_alpha(textures[tex][0], textures[tex][1], tu, tv) >= CUTOFF
        tie = cand & (t == best_t) & (best_leaf >= 0)
        ties |= tie
        take = cand & ((t < best_t) | (tie & (leaf[p] > best_leaf)))
        best_t = np.where(take, t, best_t).astype(f); best_u = np.where(take, u, best_u).astype(f); best_v = np.where(take, v, best_v).astype(f)
        best_prim = np.where(take, p, best_prim); best_leaf = np.where(take, leaf[p], best_leaf)
    return {"t": best_t, "u": best_u, "v": best_v, "prim": best_prim.astype(np.int32), "kept": kept, "ties": ties}


def hit_record(vertex_np, primitive_np, rays, hit):
    """the words of tirt_trace_closest's 13-word record that the hit (t, u, v, prim) determines without a normal: t, the position (v1 * a + v2 * b) + v3 * c
    (a sphere: o + d * t) and the uv (texture_expected.hit_uv); a miss: INF_VALUE and zeros -> [n, 6]"""
    rays = np.ascontiguousarray(rays, f).reshape(-1, 6)
    t, u, v, prim = hit["t"], hit["u"], hit["v"], hit["prim"]
    n = t.shape[0]
    out = np.zeros((n, 6), f)
    out[:, 0] = t
    isect = prim >= 0
    p = np.where(isect, prim, 0)
    tri = isect & (primitive_np[p, 0] == SCD.PRIMITIVE_TRI)
    vi = np.where(tri, primitive_np[p, 1], 0)
    a = ((f(1.0) - u) - v).astype(f)
    for k in range(3):
        v1, v2, v3 = vertex_np[vi, k], vertex_np[vi + 1, k], vertex_np[vi + 2, k]
        pt = ((v1 * a + v2 * u).astype(f) + v3 * v).astype(f)
        ps = (rays[:, k] + (rays[:, 3 + k] * t).astype(f)).astype(f)
        out[:, 1 + k] = np.where(tri, pt, np.where(isect, ps, f(0.0)))
    tu, tv = te.hit_uv(vertex_np, primitive_np, p, u, v)
    out[:, 4] = np.where(tri, tu, f(0.0)); out[:, 5] = np.where(tri, tv, f(0.0))
    return out
