"""numpy restatement of the roughness, metallic and normal-map textures (include/tirt.h, "Roughness, metallic and normal-map textures on materials"),
operation by operation in float32 with one rounding per operation, so the device must give these bits.  The lookup is texture_expected.tex_albedo,
unchanged; square root and division are IEEE's on both sides.

  material_map(row, word, T): the texture a row names in word 7 (roughness), 8 (metallic), 9 (normal map), or -1: word 1's rule, an emitter none, glass only word 9
  refused_slots(material, T): what check_material_textures refuses, as (row, word)
  rough = c.y, metal = c.z of c = tex_albedo(...)
  normal map:  n = c * 2 - 1;  d1 = t1 - t0, d2 = t2 - t0;  det = d1.x * d2.y - d2.x * d1.y;  det == 0 or not finite, or a shape: N
               T = (e1 * d2.y - e2 * d1.y) / det;  T = T - N * dot(N, T);  T = normalized(T);  T not finite: N
               B = cross(N, T);  Nraw = (T * n.x + B * n.y) + N * n.z;  N' = normalized(Nraw)
  maps_at: the 8 words of tirt_kat_material_maps
"""
import numpy as np

import texture_expected as te
from ti_raytrace_amd import SceneData as SCD

f = np.float32
BIG = te.BIG
WORDS = {"albedo": 1, "rough": 7, "metal": 8, "normal": 9}


def dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(f)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(f)


def normalized(a):
    """taichi's Vector.normalized(): inv = 1 / sqrt(dot(a, a)); a * inv"""
    a = np.asarray(a, f)
    with np.errstate(all="ignore"):
        inv = (f(1.0) / np.sqrt(dot(a, a))).astype(f)
        return (a * inv[..., None]).astype(f)


def _slot(x):
    """(int)x as the device converts: saturating, NaN -> 0"""
    x = float(x)
    if x != x:
        return 0
    return int(max(min(x, 2147483647.0), -2147483648.0))


def honours(row, word):
    t = int(row[0])
    return t != int(SCD.MAT_LIGHT) and not (t == int(SCD.MAT_GLASS) and word in (7, 8))


def material_map(row, word, n_textures):
    s = _slot(row[word])
    return s - 1 if (n_textures >= 1 and honours(row, word) and 1 <= s <= n_textures) else -1


def refused_slots(material_np, n_textures):
    """[(row, word)] that tirt_scene_upload / tirt_material_upload / tirt_texture_upload refuse with n_textures uploaded (none when n_textures == 0)"""
    if n_textures <= 0:
        return []
    return [(i, w) for i, row in enumerate(material_np) for w in (1, 7, 8, 9) if honours(row, w) and _slot(row[w]) > n_textures]


def feature_bits(material_np, n_textures):
    """bits 128 and 256 of the feature word"""
    word = 0
    for row in material_np:
        if material_map(row, 1, n_textures) >= 0:
            word |= 128
        if any(material_map(row, w, n_textures) >= 0 for w in (7, 8, 9)):
            word |= 256
    return word


def hit_normal(vertex_np, primitive_np, prim, bu, bv):
    """hit_attributes' shading normal of triangles: normalized((n0 * a + n1 * u) + n2 * v), a = 1 - u - v; shapes: (0, 0, 0) (they need a ray)"""
    prim = np.asarray(prim)
    bu, bv = np.asarray(bu, f), np.asarray(bv, f)
    tri = primitive_np[prim, 0] == SCD.PRIMITIVE_TRI
    vi = np.where(tri, primitive_np[prim, 1], 0)
    a = ((f(1.0) - bu) - bv).astype(f)
    n0, n1, n2 = vertex_np[vi, 3:6], vertex_np[vi + 1, 3:6], vertex_np[vi + 2, 3:6]
    nn = ((n0 * a[:, None] + n1 * bu[:, None]) + n2 * bv[:, None]).astype(f)
    return np.where(tri[:, None], normalized(nn), f(0.0)).astype(f)


def normal_raw_of(n, N, p, t):
    """the frame part: (Nraw [k, 3], mapped [k]) for decoded texels n [k, 3]"""
    n, N, p, t = np.asarray(n, f), np.asarray(N, f), np.asarray(p, f), np.asarray(t, f)
    with np.errstate(all="ignore"):
        d1, d2 = (t[:, 1] - t[:, 0]).astype(f), (t[:, 2] - t[:, 0]).astype(f)
        det = (d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]).astype(f)
        ok = (det != 0) & (np.abs(det) <= BIG)
        e1, e2 = (p[:, 1] - p[:, 0]).astype(f), (p[:, 2] - p[:, 0]).astype(f)
        T = ((e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) / det[:, None]).astype(f)
        T = (T - N * dot(N, T)[:, None]).astype(f)
        T = normalized(T)
        ok &= (np.abs(T) <= BIG).all(axis=1)
        B = cross(N, T)
        raw = ((T * n[:, 0:1] + B * n[:, 1:2]) + N * n[:, 2:3]).astype(f)
    return np.where(ok[:, None], raw, N).astype(f), ok


def normal_raw(img, wrap, tu, tv, N, p, t):
    """(Nraw [k, 3], mapped [k]): p [k, 3, 3] vertex positions, t [k, 3, 2] vertex uvs, N [k, 3]; where not mapped the row is N itself"""
    c = te.tex_albedo(img, wrap, tu, tv)
    return normal_raw_of((c * f(2.0) - f(1.0)).astype(f), N, p, t)


def mapped_normal(img, wrap, tu, tv, N, p, t):
    raw, ok = normal_raw(img, wrap, tu, tv, N, p, t)
    return np.where(ok[:, None], normalized(raw), np.asarray(N, f)).astype(f)


def tri_rows(vertex_np, primitive_np, prim):
    """(p [n, 3, 3], t [n, 3, 2]) of triangles prim[n]"""
    vi = primitive_np[np.asarray(prim), 1]
    idx = vi[:, None] + np.arange(3)[None, :]
    return vertex_np[idx, 0:3].astype(f), vertex_np[idx, 6:8].astype(f)


def rough_metal_at(material_np, textures, mat, tu, tv):
    """(rough [n], metal [n]) of hits on materials mat[n] at uv: the row's words 6 and 5, or the looked-up .y / .z"""
    mat = np.asarray(mat)
    tu, tv = np.asarray(tu, f), np.asarray(tv, f)
    rough, metal = material_np[mat, 6].astype(f).copy(), material_np[mat, 5].astype(f).copy()
    for m in np.unique(mat):
        sel = mat == m
        for word, out, ch in ((7, rough, 1), (8, metal, 2)):
            k = material_map(material_np[m], word, len(textures))
            if k >= 0:
                out[sel] = te.tex_albedo(textures[k][0], textures[k][1], tu[sel], tv[sel])[:, ch]
    return rough, metal


def normal_at(material_np, textures, vertex_np, primitive_np, prim, tu, tv, N, raw=False):
    """N' (or, raw: (Nraw, mapped)) of hits on primitives prim[n] at uv (tu, tv) with interpolated normal N"""
    prim = np.asarray(prim)
    out = np.asarray(N, f).copy()
    mapped = np.zeros(prim.size, bool)
    tri = primitive_np[prim, 0] == SCD.PRIMITIVE_TRI
    mat = primitive_np[prim, 2]
    for m in np.unique(mat[tri]):
        k = material_map(material_np[m], 9, len(textures))
        if k < 0:
            continue
        sel = np.where(tri & (mat == m))[0]
        p, t = tri_rows(vertex_np, primitive_np, prim[sel])
        r, ok = normal_raw(textures[k][0], textures[k][1], np.asarray(tu, f)[sel], np.asarray(tv, f)[sel], out[sel], p, t)
        out[sel] = r if raw else np.where(ok[:, None], normalized(r), out[sel])
        mapped[sel] = ok
    return (out, mapped) if raw else out


def maps_at(material_np, textures, vertex_np, primitive_np, prim, bu, bv):
    """the (n, 8) words of tirt_kat_material_maps: uv2, rough, metal, N'3, 0"""
    prim = np.asarray(prim)
    tu, tv = te.hit_uv(vertex_np, primitive_np, prim, bu, bv)
    N = hit_normal(vertex_np, primitive_np, prim, bu, bv)
    rough, metal = rough_metal_at(material_np, textures, primitive_np[prim, 2], tu, tv)
    out = np.zeros((prim.size, 8), f)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = tu, tv, rough, metal
    out[:, 4:7] = normal_at(material_np, textures, vertex_np, primitive_np, prim, tu, tv, N)
    return out
