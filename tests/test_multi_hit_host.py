"""First K hits without a device (include/tirt.h, "First K hits"): the three entry points in the header, the binding and the library, the refusals
that need no device, the list code of csrc/tirt_multi_hit.h on the host (tirt_kat_hit_list) against Python's sorted, and the yardstick of the GPU tests
(tests/multi_hit_expected.py) against the oracle's closest hit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import multi_hit_expected as mh
import oracle_api as oa
from ti_raytrace_amd import _native, RayQuery, RayMultiHits, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_query_hits", "tirt_trace_hits", "tirt_kat_hit_list")
f = np.float32


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_library():
    text = header()
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert sorted(_native.SIGNATURES) == sorted(set(re.findall(r"\b(tirt_[a-z_0-9]+)\s*\(", text)))
    assert re.search(r"#define\s+TIRT_HITS_MAX\s+64\b", text) and _native.HITS_MAX == 64
    # the entries beside them keep their signatures
    S = _native.SIGNATURES
    assert len(S["tirt_query_closest"][1]) == 12 and len(S["tirt_query_occluded"][1]) == 11 and len(S["tirt_query_hits"][1]) == 17


def test_refusals_without_a_device():
    L = _native.lib()
    cnt = np.zeros(4, np.int32)
    t = np.zeros(4, f)
    q = lambda ctx, k, out_t, out_count: L.tirt_query_hits(ctx, None, 0, 6, None, 1, float("inf"), k, 64, 0, out_t, None, None, 13, out_count, None, None)
    assert q(None, 1, t.ctypes.data, None) == -2 and b"null context" in L.tirt_last_error()
    assert q(None, 65, t.ctypes.data, None) == -2 and b"TIRT_HITS_MAX" in L.tirt_last_error()
    assert q(None, -1, t.ctypes.data, None) == -2 and b"TIRT_HITS_MAX" in L.tirt_last_error()
    assert q(None, 0, None, None) == -2 and b"without out_count" in L.tirt_last_error()
    assert q(None, 0, None, cnt.ctypes.data) == -2 and b"null context" in L.tirt_last_error()
    h = lambda k, out_count: L.tirt_trace_hits(None, np.zeros(6, f), 1, None, k, 64, 0, None, None, None, out_count, None)
    assert h(65, None) == -2 and b"TIRT_HITS_MAX" in L.tirt_last_error()
    assert h(0, None) == -2 and b"without out_count" in L.tirt_last_error()
    assert h(4, None) == -2 and b"null context" in L.tirt_last_error()
    info = np.zeros(4, np.int32)
    assert L.tirt_kat_hit_list(np.zeros(4, f), 1, 65, 1.0, None, info) == -2
    assert L.tirt_kat_hit_list(np.zeros(4, f), -1, 1, 1.0, t.ctypes.data, info) == -2


def test_ray_query_checks_first():
    assert RayMultiHits._fields == ("t", "prim", "record", "count")
    for name in ("hits", "count"):
        assert callable(getattr(RayQuery, name))
    for name in ("query_hits", "trace_hits"):
        assert callable(getattr(_native.Context, name))
    assert callable(_native.kat_hit_list)
    import torch

    class NoScene:
        _ctx = None
        _device_id = 0
    q = RayQuery(NoScene())
    with pytest.raises(TypeError, match="hits: rays must be a torch.Tensor"):
        q.hits(np.zeros((4, 6), f), 2)
    with pytest.raises(TypeError, match="hits: rays must be float32"):
        q.hits(torch.zeros((4, 6), dtype=torch.float64), 2)
    with pytest.raises(TypeError, match="hits: rays must be on the GPU"):
        q.hits(torch.zeros((4, 6)), 2)
    with pytest.raises(TypeError, match="count: rays must be on the GPU"):
        q.count(torch.zeros((4, 6)))
    with pytest.raises(TypeError, match="count: rays must be a torch.Tensor"):
        q.count([[0.0] * 6])


# ---- the list ---------------------------------------------------------------------------------------------------------------------------
def cands(t, leaf, seed=0):
    """rows (t, u, v, leaf) with distinct u, v (so that an entry is recognisable): float32 words, the leaf as int32"""
    t = np.asarray(t, f); n = t.shape[0]
    c = np.zeros((n, 4), f)
    c[:, 0] = t; c[:, 1] = np.arange(n, dtype=f) + f(0.25); c[:, 2] = np.random.RandomState(seed).uniform(size=n).astype(f)
    c.view(np.int32)[:, 3] = np.asarray(leaf, np.int32)
    return c


def want_list(c, k, bound):
    """Python's sorted: the accepted candidates (0 < t < B, bound > 0) by (t, -leaf), stable, the first k"""
    B = min(f(bound), f(1e6)) if bound > 0 else None
    rows = [tuple(r) for r in c.view(np.uint32).tolist()]
    acc = []
    for r in rows:
        t = np.array([r[0]], np.uint32).view(f)[0]
        if B is not None and t > 0 and t < B:
            acc.append((float(t), -int(np.array([r[3]], np.uint32).view(np.int32)[0]), r))
    ordered = sorted(acc, key=lambda x: (x[0], x[1]))
    return np.array([x[2] for x in ordered[:k]], np.uint32).reshape(-1, 4), len(acc)


def check_list(c, k, bound=float("inf")):
    got, accepted, thr = _native.kat_hit_list(c, k, bound)
    want, n_acc = want_list(c, k, bound)
    assert accepted == n_acc
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want), (k, bound)
    if want.shape[0] == k and k > 0:
        assert np.array_equal(np.array([thr[0]], f).view(np.uint32), want[-1, 0:1]) and thr[1] == int(want[-1:, 3].view(np.int32)[0])
    else:
        assert thr[1] == -1
    return got


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16, 64])
def test_hit_list_against_sorted(k):
    r = np.random.RandomState(k)
    n = 100
    asc = np.arange(1, n + 1, dtype=f) * f(0.5)
    check_list(cands(asc, np.arange(n)), k)                                  # ascending
    check_list(cands(asc[::-1], np.arange(n)), k)                            # descending
    check_list(cands(np.full(n, 2.5, f), r.permutation(n)), k)               # one t, different leaves: the larger leaf first
    tt = r.choice(asc[:7], n)
    check_list(cands(tt, r.randint(0, 5, n)), k)                             # few keys: the same (t, leaf) many times, in arrival order
    check_list(cands(r.uniform(0.1, 50.0, n), r.randint(0, 1000, n)), k)     # more candidates than k
    check_list(cands(r.uniform(0.1, 50.0, 3), [5, 6, 7]), k)                 # fewer than k (k > 3)
    mixed = r.uniform(-1.0, 3.0, n).astype(f)
    mixed[::7] = 0.0; mixed[3::11] = np.nan; mixed[5::13] = 2.0; mixed[1::17] = np.inf
    check_list(cands(mixed, r.randint(0, 50, n)), k, bound=2.0)              # t = 0, negative, NaN, +inf and t exactly AT the bound are out
    check_list(cands(mixed, r.randint(0, 50, n)), k, bound=float("inf"))     # B = 1e6
    for bad in (0.0, -1.0, float("nan")):
        got, accepted, thr = _native.kat_hit_list(cands(asc, np.arange(n)), k, bad)
        assert got.shape == (0, 4) and accepted == 0


def test_hit_list_details():
    # the same (t, leaf) twice: both are kept, in arrival order, while there is room; a full list whose threshold it equals rejects it
    c = cands([1.0, 2.0, 2.0, 3.0], [4, 9, 9, 1])
    got = check_list(c, 4)
    assert list(got[:, 1]) == [0.25, 1.25, 2.25, 3.25]
    got = check_list(c, 2)
    assert list(got[:, 1]) == [0.25, 1.25]
    # equal t: leaf 9 before leaf 4 whatever the arrival order, and it alone for k = 1
    for order in ([0, 1], [1, 0]):
        c = cands([2.0, 2.0], [4, 9])[order]
        assert list(check_list(c, 2)[:, 3].view(np.int32)) == [9, 4]
        assert list(check_list(c, 1)[:, 3].view(np.int32)) == [9]
    # k = 0: the count alone
    got, accepted, thr = _native.kat_hit_list(cands([1.0, 5.0, 3.0], [1, 2, 3]), 0, 4.0)
    assert got.shape == (0, 4) and accepted == 2
    # a bound at 1e6 and beyond is 1e6
    got, accepted, _ = _native.kat_hit_list(cands([999999.0, 1000000.0, 2000000.0], [1, 2, 3]), 3, 3.0e6)
    assert accepted == 1 and got.shape == (1, 4)


# ---- the yardstick is the oracle where it can be asked ----------------------------------------------------------------------------------
def grazing_rays(sc, n, seed):
    """the construction of tests/test_gpu_trace.py::test_quantised_nodes_on_grazing_rays, restated: rays aimed exactly at triangle vertices and edge points
    from 0.3 to 30000 extents away, and axis-parallel rays through vertices, from outside and from the vertex itself"""
    r = np.random.RandomState(seed)
    tri = sc.primitive_np[sc.primitive_np[:, 0] == 1]
    v = sc.vertex_np[:, :3].astype(np.float64)
    ext = float((v.max(axis=0) - v.min(axis=0)).max())
    pick = tri[r.randint(0, tri.shape[0], n), 1]
    corner = v[pick + r.randint(0, 3, n)]
    a, b = v[pick], v[pick + 1]
    w = r.uniform(0, 1, (n, 1))
    edge = a * w + b * (1 - w)
    rays = []
    for target in (corner, edge):
        for dist in (0.3 * ext, 3.0 * ext, 300.0 * ext, 30000.0 * ext):
            d = r.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays.append(np.concatenate([target - d * dist, d], axis=1))
    for ax in range(3):
        d = np.zeros((n, 3)); d[:, ax] = r.choice([-1.0, 1.0], n)
        rays.append(np.concatenate([corner - d * 2.0 * ext, d], axis=1))
        rays.append(np.concatenate([corner, d], axis=1))
    return np.concatenate(rays, axis=0).astype(f)


def scene_rays(ex, W, n_random, seed):
    sc = ex.scene
    lo, hi = sc.vertex_np[:, :3].min(axis=0).astype(np.float64), sc.vertex_np[:, :3].max(axis=0).astype(np.float64)
    r = np.random.RandomState(seed)
    o = lo + (hi - lo) * r.uniform(-0.1, 1.1, size=(n_random, 3))
    d = r.normal(size=(n_random, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([oa.camera_rays(ex.cam, W, W), np.concatenate([o, d], axis=1).astype(f)], axis=0)


@pytest.mark.parametrize("name", ["cornell", "tiny"])
def test_restatement_k1_is_the_oracles_closest_hit(name):
    W = 32
    ex = scenes.cornell_box(W, W, 4, device_id=0) if name == "cornell" else common.tiny_scene(40, device_id=0)
    common.host_only(ex)
    sc = ex.scene
    orc = oa.OracleScene(sc, ex.cam)
    assert orc.lbvh_build() == sc.primitive_count - 1
    compact = orc.lbvh_get()[2]
    rays = np.concatenate([scene_rays(ex, W, 4096 - W * W, 5), grazing_rays(sc, 40, 17)], axis=0)
    want, wprim, _, bary = orc.closest_hit(rays, uv=True)
    h = mh.hit_sets(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, compact, rays)
    t, prim = mh.first_k(h, 1)
    assert np.array_equal(prim[:, 0], wprim), int((prim[:, 0] != wprim).sum())
    assert np.array_equal(bits(t[:, 0]), bits(want[:, 0]))
    assert np.array_equal(bits(h["u"][:, 0]), bits(bary[:, 0])) and np.array_equal(bits(h["v"][:, 0]), bits(bary[:, 1]))
    assert 0.05 < (wprim >= 0).mean() < 0.999 and (h["count"] >= 2).any()      # (rays that hit, rays that miss, rays through several surfaces)
    # the parents the restatement derives are a tree over the rows
    par = mh.parents(compact)
    assert par[0] == -1 and (par[1:] >= 0).all() and (par[1:] < np.arange(1, par.shape[0])).all()
