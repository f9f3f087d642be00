"""numpy restatement of the hit set H and its order (include/tirt.h, "First K hits"), operation by operation in float32, over arrays that are already
downloadable: vertices, primitives, shapes, and the reference's compact rows (tirt_lbvh_download; the parents follow from the rows).  The primitive tests,
`slabs`, the leaves' indices and the alpha lookup are tests/cutout_expected.py's.

For each primitive: the candidates 0 < t < B with B = min(1e6, tmax) (tmax <= 0 or NaN: none); where the leaf's own exact box fails `slabs` the rows of its
proper ancestors are asked one by one (the reference's exhaustive walk reaches a leaf iff every proper ancestor's box passes; `slabs` on the leaf's own box
implies theirs); on a scene with cut-outs a tagged triangle's candidate needs tex_alpha >= 0.5.  Sorted by (t, -leaf).  It restates the FULL definition and
leaves no ray out.  tests/test_multi_hit_host.py holds it to the oracle's closest hit on the CPU."""
import numpy as np

import cutout_expected as ce
from ti_raytrace_amd import SceneData as SCD

f = np.float32
INF_VALUE = ce.INF_VALUE


def parents(compact):
    """compact index of every row's parent (-1: the root), from the rows: an internal row's children are the next row and the row word 1 names"""
    compact = np.asarray(compact)
    N = compact.shape[0]
    par = np.full(N, -1, np.int64)
    internal = np.where((compact[:, 0].astype(np.int64) & 1) == 0)[0]
    par[internal + 1] = internal
    par[compact[internal, 1].astype(np.int64)] = internal
    return par


def _sub(arrs, idx):
    return [a[idx] for a in arrs]


def hit_sets(vertex_np, primitive_np, material_np, shape_np, compact, rays, tmax=None, textures=(), flags=(), prims=None):
    """-> dict: t, u, v [n, P] float32 and prim, leaf [n, P] in H's order, padded with 1e6 / 0 / -1; count [n] = |H|.  tmax: None, a scalar or [n].
    prims: only these primitives are asked (P = their number; the caller has shown that no ray can hit another one); `prim` still holds scene indices"""
    rays = np.ascontiguousarray(rays, f).reshape(-1, 6)
    sel = np.arange(primitive_np.shape[0]) if prims is None else np.asarray(prims, np.int64)
    n, P = rays.shape[0], sel.shape[0]
    o = [rays[:, k].copy() for k in range(3)]; d = [rays[:, 3 + k].copy() for k in range(3)]
    tm = np.full(n, np.inf, f) if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, f), (n,)))
    with np.errstate(invalid="ignore"):
        valid = tm > f(0.0)
        B = np.where(tm < INF_VALUE, tm, INF_VALUE).astype(f)
    leaf = ce.leaf_indices(compact)
    par = parents(compact)
    T = np.full((n, P), np.inf, f); U = np.zeros((n, P), f); Vv = np.zeros((n, P), f)
    for q, p in enumerate(sel.tolist()):
        kind, idx, mat = (int(x) for x in primitive_np[p])
        if kind == SCD.PRIMITIVE_TRI:
            V = vertex_np[idx:idx + 3]
            t, u, v = ce.intersect_tri(o, d, V[0, 0:3], V[1, 0:3], V[2, 0:3])
            mn, mx = V[:, 0:3].min(axis=0), V[:, 0:3].max(axis=0)
        else:
            sh = shape_np[idx]
            t = ce.intersect_sphere(o, d, sh[1:4], sh[4]) if int(sh[0]) == 1 else np.full(n, INF_VALUE, f)
            u = np.zeros(n, f); v = np.zeros(n, f)
            rr = f(sh[4]); mn = sh[1:4].astype(f) - rr; mx = sh[1:4].astype(f) + rr
        with np.errstate(invalid="ignore"):
            cand = valid & (t > f(0.0)) & (t < B)
        ask = np.where(cand & ~ce.slabs(o, d, mn, mx))[0]          # within rounding distance of the leaf box's boundary: the ancestors decide
        alive, an = ask, par[leaf[p]]
        while alive.size and an >= 0:
            row = compact[an]
            alive = alive[ce.slabs(_sub(o, alive), _sub(d, alive), row[2:5], row[5:8])]
            an = par[an]
        cand[np.setdiff1d(ask, alive)] = False
        tex = ce.cutout_texture_of(material_np[mat], len(textures), flags) if kind == SCD.PRIMITIVE_TRI else -1
        if tex >= 0:
            a = ((f(1.0) - u) - v).astype(f)
            Tx = vertex_np[idx:idx + 3, 6:8].astype(f)
            tu = ((Tx[0, 0] * a + Tx[1, 0] * u).astype(f) + Tx[2, 0] * v).astype(f)
            tv = ((Tx[0, 1] * a + Tx[1, 1] * u).astype(f) + Tx[2, 1] * v).astype(f)
            cand &= ce.tex_alpha(textures[tex][0], textures[tex][1], tu, tv) >= ce.CUTOFF
        T[:, q] = np.where(cand, t, f(np.inf)); U[:, q] = u; Vv[:, q] = v
    negleaf = np.broadcast_to(-leaf[sel][None, :], (n, P))
    order = np.lexsort((negleaf, T), axis=1)                      # t ascending, then the larger leaf first
    rows = np.arange(n)[:, None]
    Ts = T[rows, order]
    inH = np.isfinite(Ts)
    return {"t": np.where(inH, Ts, INF_VALUE).astype(f), "u": np.where(inH, U[rows, order], f(0.0)).astype(f),
            "v": np.where(inH, Vv[rows, order], f(0.0)).astype(f), "prim": np.where(inH, sel[order], -1).astype(np.int32),
            "leaf": np.where(inH, leaf[sel][order], -1).astype(np.int64), "count": inH.sum(axis=1).astype(np.int32)}


def first_k(h, k):
    """the [n, k] outputs of tirt_query_hits from hit_sets' result: t and prim, padded with 1e6 and -1"""
    n, P = h["t"].shape
    t = np.full((n, k), INF_VALUE, f); prim = np.full((n, k), -1, np.int32)
    m = min(k, P)
    t[:, :m] = h["t"][:, :m]; prim[:, :m] = h["prim"][:, :m]
    return t, prim
