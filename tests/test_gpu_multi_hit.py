"""First K hits on the device (csrc/tirt_multi_hit.hip through tirt_query_hits / tirt_trace_hits and RayQuery.hits / .count; include/tirt.h "First K hits").
Every comparison is bit for bit on t and exact on prim, count and record: the ordered walk, the EXHAUSTIVE walk and the numpy restatement
(tests/multi_hit_expected.py, held to the oracle by tests/test_multi_hit_host.py) all agree.  A few thousand rays on scenes of tens to hundreds of primitives."""
import numpy as np
import pytest
import torch

import cutout_expected as ce
import cutout_scenes as cs
import multi_hit_expected as mh
import oracle_api as oa
from common import custom_scene, duplicate_code_scene, long_chain_scene, on_device, same_bits, tiny_scene
from ti_raytrace_amd import RayQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EXH = _native.TRAVERSE_EXHAUSTIVE
f = np.float32
INF = f(1e6)
_BUILT = {}


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def cpu(x):
    torch.cuda.synchronize(DEV)
    return None if x is None else x.cpu().numpy()


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Built:
    """a scene on the device with what the restatement needs, downloaded once"""

    def __init__(self, ex, stack=64, uploaded=False):
        if not uploaded:
            ex.build_scene()
        if not ex.cam.view_inv_np.any():
            ex.frame_camera(0.8)
        self.ex, self.sc, self.ctx, self.stack = ex, ex.scene, ex.scene.ctx, stack
        sc = self.sc
        self.vertex = self.ctx.vertex_download(sc.vertex_count)
        self.compact = self.ctx.lbvh_download(sc.primitive_count, False, False, True)[2]
        self.textures, self.flags = (), ()
        self._want = {}

    def want(self, key, rays, tmax=None):
        """the restatement of H for a ray set, computed once per key and left unchanged"""
        if key not in self._want:
            sc = self.sc
            self._want[key] = mh.hit_sets(self.vertex, sc.primitive_np, sc.material_np, sc.shape_np, self.compact, rays, tmax, self.textures, self.flags)
        return self._want[key]

    def hits(self, rays, k, tmax=None, flags=0, attributes=False, count=False, stack=None):
        q = RayQuery(self.sc, stack or self.stack, flags)
        rt = rays if isinstance(rays, torch.Tensor) else on_dev(rays)
        tm = on_dev(tmax) if isinstance(tmax, np.ndarray) else tmax
        h = q.hits(rt, k, tmax=tm, attributes=attributes, count=count)
        return cpu(h.t), cpu(h.prim), cpu(h.record), cpu(h.count)

    def check(self, key, rays, ks, tmax=None, flags_list=(0, EXH)):
        """lists and counts of both walks, with and without the count, against the restatement"""
        w = self.want(key, rays, tmax)
        for k in ks:
            wt, wp = mh.first_k(w, k)
            for flags in flags_list:
                for count in (False, True):
                    t, prim, _, cnt = self.hits(rays, k, tmax, flags, count=count)
                    bad = np.where((bits(t) != bits(wt)).any(axis=1) | (prim != wp).any(axis=1))[0]
                    assert bad.size == 0, "%s k=%d flags=%d count=%s: %d rays differ, first %d: got t %s prim %s, want t %s prim %s" % (
                        key, k, flags, count, bad.size, bad[0], t[bad[0]].tolist(), prim[bad[0]].tolist(), wt[bad[0]].tolist(), wp[bad[0]].tolist())
                    if count:
                        assert np.array_equal(cnt, w["count"]), (key, k, flags, int((cnt != w["count"]).sum()))
        return w


def built(name):
    if name not in _BUILT:
        if name == "cornell":
            b = Built(scenes.cornell_box(32, 32, 4, device_id=0))
        elif name == "tiny":
            b = Built(tiny_scene(40, device_id=0))
        elif name == "chain":
            b = Built(long_chain_scene(32, 32), stack=1024)
        elif name == "duplicates":
            b = Built(duplicate_code_scene(32, 32, device_id=0))
        elif name == "quads":
            b = Built(custom_scene(quad_stack()))
        elif name == "sphere":
            b = Built(custom_scene(sphere_scene_tris()))
        _BUILT[name] = b
    return _BUILT[name]


def ray_set(b, n_random, seed, W=32):
    """camera rays of the W x W film, then rays with origins uniform in (and a little around) the scene's bounds and uniform directions"""
    v = b.vertex[:, :3].astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    r = np.random.RandomState(seed)
    o = lo + (hi - lo) * r.uniform(-0.1, 1.1, size=(n_random, 3))
    d = r.normal(size=(n_random, 3))
    aim = v[r.randint(0, v.shape[0], n_random)] + r.normal(size=(n_random, 3)) * 0.02 * (hi - lo)      # every other one aimed near a vertex: through the surfaces
    d[::2] = (aim - o)[::2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([oa.camera_rays(b.ex.cam, W, W), np.concatenate([o, d], axis=1).astype(f)], axis=0)


# ---- k = 1 is closest() -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "tiny", "chain", "duplicates"])
def test_k1_is_closest(gpu_ctx_ok, name):
    b = built(name)
    rays = ray_set(b, 2000, 3)
    rt = on_dev(rays)
    c = RayQuery(b.sc, b.stack, 0).closest(rt, attributes=True)
    ct, cprim, crec = cpu(c.t), cpu(c.prim), cpu(c.record)
    assert 0.02 < (cprim >= 0).mean() < 0.999
    for flags in (0, EXH):
        for count in (False, True):
            t, prim, rec, _ = b.hits(rt, 1, None, flags, attributes=True, count=count)
            assert np.array_equal(prim[:, 0], cprim) and np.array_equal(bits(t[:, 0]), bits(ct)), (name, flags, count)
            assert same_bits(rec[:, 0], crec), (name, flags, count)
    # a bound just above the closest t keeps it -- it alone: count 1 where nothing ties with it --; AT it (the comparison is strict) and just below, nothing is left
    w = b.check(name, rays, (1, 4))
    assert np.array_equal(bits(w["t"][:, 0]), bits(ct)) and np.array_equal(w["prim"][:, 0], cprim)
    above, below = np.nextafter(ct, f(np.inf)).astype(f), np.nextafter(ct, f(0.0)).astype(f)
    wa = b.check(name + "above", rays, (1, 2), above, flags_list=(0,))
    assert np.array_equal(wa["prim"][:, 0], cprim) and np.array_equal(bits(wa["t"][:, 0]), bits(ct))
    ties = (w["t"][:, 1] == w["t"][:, 0]) & (cprim >= 0)
    assert np.array_equal(wa["count"], np.where(cprim >= 0, 1 + ties, 0))
    for key, tm in (("at", ct.copy()), ("below", below)):
        wb = b.check(name + key, rays, (1, 2), tm, flags_list=(0,))
        assert (wb["count"] == 0).all() and (wb["prim"] == -1).all()


# ---- eviction and padding ---------------------------------------------------------------------------------------------------------------
def quad_stack():
    """twelve parallel quads z = -0.3 j, j = 0 .. 11 (24 triangles), each [-1, 1]^2"""
    tris = []
    for j in range(12):
        z = -0.3 * j
        a, b_, c, d = (-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)
        tris += [[a, b_, c], [a, c, d]]
    return np.asarray(tris, np.float64)


def test_eviction_and_padding(gpu_ctx_ok):
    b = built("quads")
    r = np.random.RandomState(5)
    n = 1500
    xy = r.uniform(-0.9, 0.9, (n, 2))
    along = np.concatenate([xy, np.full((n, 1), 2.0), np.zeros((n, 2)), np.full((n, 1), -1.0)], axis=1)
    along[n // 2:, 2] = -5.0; along[n // 2:, 5] = 1.0                                  # half of them from behind: the lists come out in the other order
    o = np.concatenate([r.uniform(-0.6, 0.6, (n, 2)), np.full((n, 1), 1.5)], axis=1)
    d = np.concatenate([r.uniform(-0.25, 0.25, (n, 2)), np.full((n, 1), -1.0)], axis=1); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([along, np.concatenate([o, d], axis=1)], axis=0).astype(f)
    w = b.check("quads", rays, (1, 2, 5, 12, 16, 64))
    assert (w["count"][:n] == 12).all()                                                # whatever k is (check compares every k's count with it)
    assert 1 <= w["count"][n:].min() and w["count"][n:].max() <= 13 and (w["count"][n:] < 12).any()
    t, prim, rec, cnt = b.hits(rays, 16, attributes=True, count=True)
    assert (t[:n, 12:] == INF).all() and (prim[:n, 12:] == -1).all() and (t[:n, :12] < INF).all() and (np.diff(t[:n, :12], axis=1) > 0).all()
    assert np.array_equal(bits(rec[..., 0]), bits(t))
    # the records: position and uv of every entry from the restatement's (t, u, v, prim); the padding is a miss's record; both walks write the same words
    for j in (0, 5, 11, 14):
        hit = {"t": w["t"][:, j] if j < w["t"].shape[1] else np.full(rays.shape[0], INF, f), "u": w["u"][:, j], "v": w["v"][:, j], "prim": w["prim"][:, j]}
        want = ce.hit_record(b.vertex, b.sc.primitive_np, rays, hit)
        assert np.array_equal(bits(rec[:, j][:, [0, 1, 2, 3, 10, 11]]), bits(want)), j
    _, _, rec_e, _ = b.hits(rays, 16, flags=EXH, attributes=True)
    assert same_bits(rec, rec_e)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------
def test_coincident_triangles(gpu_ctx_ok):
    tri = np.array([[-1.0, -1.0, 0.1], [1.0, -1.0, -0.1], [0.0, 1.2, 0.05]])
    r = np.random.RandomState(2)
    others = [r.uniform(-1.5, 1.5, 3)[None, :] + r.uniform(-0.4, 0.4, (3, 3)) for _ in range(9)]
    b = Built(custom_scene(np.asarray([tri, others[0], tri] + others[1:], np.float64)))
    n = 1200
    o = np.concatenate([r.uniform(-0.7, 0.7, (n, 1)), r.uniform(-0.8, 0.9, (n, 1)), np.full((n, 1), 2.0)], axis=1)
    d = np.zeros((n, 3)); d[:, 2] = -1.0; d[:, :2] = r.uniform(-0.1, 0.1, (n, 2))
    rays = np.concatenate([o, d], axis=1).astype(f)
    w = b.check("coincident", rays, (1, 2, 3))
    leaf = ce.leaf_indices(b.compact)
    first, second = (0, 2) if leaf[0] > leaf[2] else (2, 0)
    t, prim, _, cnt = b.hits(rays, 2, count=True)
    both = np.isin(prim[:, 0], (0, 2))
    assert both.mean() > 0.3
    assert (prim[both, 0] == first).all() and (prim[both, 1] == second).all() and np.array_equal(bits(t[both, 0]), bits(t[both, 1]))
    t1, prim1, _, _ = b.hits(rays, 1)
    assert (prim1[both, 0] == first).all()
    c = RayQuery(b.sc).closest(on_dev(rays))
    assert np.array_equal(cpu(c.prim), prim1[:, 0])


# ---- spheres and far origins ------------------------------------------------------------------------------------------------------------
def sphere_scene_tris():
    r = np.random.RandomState(8)
    return np.asarray([r.uniform(-2.0, 2.0, 3)[None, :] * np.array([1.0, 0.5, 1.0]) + np.array([0.0, 1.5, 0.0]) + r.uniform(-0.5, 0.5, (3, 3)) for _ in range(40)])


def test_spheres_and_far_origins(gpu_ctx_ok):
    """the sphere rule (head of csrc/tirt_multi_hit.hip): a far-origin ray enters through the chain nodes, which hold the sphere beside the root, and must
    not meet the sphere's leaf a second time in the tree: a sphere hit appears once and counts once"""
    b = built("sphere")
    sc = b.sc
    tree = b.ctx.wide_tree_download(sc.primitive_count)
    assert tree["n_far_nodes"] >= 1 and tree["shapes_boxed"] == 1 and tree["far_qcode"] != tree["root_code"]      # the chain is there: the rule is exercised
    sphere = int(np.where(sc.primitive_np[:, 0] != 1)[0][0])
    centre = np.array([0.0, 3.0, 0.0]); radius = 0.75
    v = b.vertex[:, :3].astype(np.float64)
    ext = float((np.maximum(v.max(axis=0), centre + radius) - np.minimum(v.min(axis=0), centre - radius)).max())
    r = np.random.RandomState(4)
    n = 600
    rays = []
    for dist in (0.4, 3.0, 7.0, 9.0, 12.0, 40.0, 1000.0):                            # in extents: inside the scene, near, and beyond TR_FAR_RHO = 8
        d = r.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        target = centre + r.uniform(-1.0, 1.0, (n, 3)) * radius * 1.3              # at the sphere, and past it
        target[n // 2:] = v[r.randint(0, v.shape[0], n - n // 2)] + r.uniform(-0.3, 0.3, (n - n // 2, 3))      # at the triangles around it
        rays.append(np.concatenate([target - d * dist * ext, d], axis=1))
    inside = np.concatenate([np.tile(centre, (n, 1)) + r.uniform(-0.5, 0.5, (n, 3)) * radius, r.normal(size=(n, 3))], axis=1)      # origins inside the sphere
    rays = np.concatenate(rays + [inside], axis=0).astype(f)
    w = b.check("sphere", rays, (1, 3, 8))
    on_sphere = (w["prim"] == sphere).sum(axis=1)
    assert on_sphere.max() == 1 and (on_sphere[:3 * n] == 1).mean() > 0.05 and (on_sphere[3 * n:7 * n] == 1).mean() > 0.05      # near and far rays hit it, once
    t, prim, _, cnt = b.hits(rays, 8, count=True)
    assert ((prim == sphere).sum(axis=1) <= 1).all() and np.array_equal(cnt, w["count"])
    assert np.array_equal(cpu(RayQuery(sc).count(on_dev(rays))), w["count"])


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def test_bounds(gpu_ctx_ok):
    b = built("quads")
    r = np.random.RandomState(6)
    n = 2000
    o = np.concatenate([r.uniform(-0.8, 0.8, (n, 2)), r.uniform(-4.5, 2.0, (n, 1))], axis=1)
    d = r.normal(size=(n, 3)); d[:, 2] *= 4.0; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(f)
    free = b.check("bounds-free", rays, (3,))
    assert (free["count"] >= 3).mean() > 0.3
    b.check("bounds-one", rays, (1, 4, 16), 1.25)
    # per ray: 0, negative, NaN, +inf, and bounds that fall exactly ON a hit's t (strict: that hit is out), just above it, and anywhere
    tm = r.uniform(0.1, 4.0, n).astype(f)
    tm[0::8] = 0.0; tm[1::8] = -1.0; tm[2::8] = np.nan; tm[3::8] = np.inf
    j = r.randint(0, 3, n)
    exact = free["t"][np.arange(n), j]
    sel = np.zeros(n, bool); sel[4::8] = True; sel[5::8] = True
    tm[sel] = exact[sel]
    tm[6::8] = np.nextafter(exact[6::8], f(np.inf))
    w = b.check("bounds-each", rays, (1, 4, 16), tm)
    on = sel & (exact < INF)
    assert on.sum() > 100 and np.array_equal(w["count"][on], j[on])                   # the hit AT the bound is out: exactly the j nearer ones are left
    assert (w["count"][0::8] == 0).all() and (w["count"][1::8] == 0).all() and (w["count"][2::8] == 0).all()
    assert np.array_equal(w["count"][3::8], free["count"][3::8])
    # the same bounds as column 1 of an [N, 3] tensor: a stride of 3
    wide = torch.zeros((n, 3), device=DEV); wide[:, 1] = on_dev(tm)
    q = RayQuery(b.sc)
    h = q.hits(on_dev(rays), 4, tmax=wide[:, 1], count=True)
    wt, wp = mh.first_k(w, 4)
    assert wide[:, 1].stride(0) == 3 and np.array_equal(bits(cpu(h.t)), bits(wt)) and np.array_equal(cpu(h.prim), wp) and np.array_equal(cpu(h.count), w["count"])
    assert np.array_equal(cpu(q.count(on_dev(rays), tmax=wide[:, 1])), w["count"])


# ---- bad rays -------------------------------------------------------------------------------------------------------------------------
def test_bad_rays(gpu_ctx_ok):
    b = built("tiny")
    rays = ray_set(b, 1000, 9)[1024:].copy()
    n = rays.shape[0]
    nan = np.arange(n) % 4 == 0
    at = np.where(nan)[0]
    rays[at, (at // 4) % 6] = np.nan                                                   # a NaN in every component in turn
    zero = np.arange(n) % 4 == 1
    rays[zero, 3:6] = 0.0                                                              # a zero direction: what the restatement says
    w = b.check("bad", rays, (1, 4))
    assert (w["count"][nan] == 0).all() and (w["count"][~nan & ~zero] > 0).any()
    t, prim, rec, cnt = b.hits(rays, 2, attributes=True, count=True)
    assert (cnt[nan] == 0).all() and (prim[nan] == -1).all() and (t[nan] == INF).all()


# ---- cut-outs -------------------------------------------------------------------------------------------------------------------------
def test_cutouts(gpu_ctx_ok):
    ex = cs.layered_scene()
    on_device(ex)
    b = Built(ex, uploaded=True)
    sc = b.sc
    assert b.ctx.shade_features()[0] & _native.SF_CUTOUT
    b.textures, b.flags = cs.textures_of(sc), sc.texture_cutout
    rays = cs.layered_rays(4000)
    w = b.check("cut", rays, (1, 4, 8))
    b.textures, b.flags = (), ()
    solid = b.want("solid", rays)
    assert (w["count"] < solid["count"]).mean() > 0.25 and (w["count"] <= solid["count"]).all()      # hits on transparent texels are absent from list and count
    rt = on_dev(rays)
    c = RayQuery(sc).closest(rt, attributes=True)
    for flags in (0, EXH):
        t, prim, rec, _ = b.hits(rt, 1, flags=flags, attributes=True)
        assert np.array_equal(prim[:, 0], cpu(c.prim)) and same_bits(rec[:, 0], cpu(c.record)), flags
    b.ctx.close()


# ---- the shape of the work ------------------------------------------------------------------------------------------------------------
def test_shape_of_the_work(gpu_ctx_ok):
    ex = scenes.cornell_box(32, 32, 4, device_id=0)      # a context of its own: the option stays with it
    b = Built(ex)
    ctx = b.ctx
    ctx.set_option("query_chunk_rays", 256)
    rays = ray_set(b, 700, 13)[1024 - 350:1024 + 350]
    w = b.want("shape", rays)
    q = RayQuery(b.sc)
    for n in (1, 63, 64, 65, 700):
        for k in (3, 64):                                   # 700 rays: three chunks of 256 and a ragged last wave
            wt, wp = mh.first_k(w, k)
            ctx.stats_reset()
            h = q.hits(on_dev(rays[:n]), k, count=True)
            assert np.array_equal(bits(cpu(h.t)), bits(wt[:n])) and np.array_equal(cpu(h.prim), wp[:n]) and np.array_equal(cpu(h.count), w["count"][:n]), (n, k)
            st = ctx.stats()
            assert st["rays_closest"] == n and st["rays_shadow"] == 0 and st["stack_overflow"] == 0
    # rays as the [:, :6] view of an [N, 8] tensor
    wide = torch.full((700, 8), 7.0, device=DEV); wide[:, :6] = on_dev(rays)
    h = q.hits(wide[:, :6], 3, attributes=True, count=True)
    wt, wp = mh.first_k(w, 3)
    assert np.array_equal(bits(cpu(h.t)), bits(wt)) and np.array_equal(cpu(h.prim), wp) and np.array_equal(bits(cpu(h.record)[..., 0]), bits(wt))
    # a stream of the caller's: the result is consumed on it with no sync in between
    want_sum = torch.from_numpy(wt).to(DEV).sum(dim=1) + torch.from_numpy(w["count"]).to(DEV).float()
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(4):                                  # keep the side stream busy before the rays exist
            big = torch.tanh(big @ big)
        rt = torch.where(big[0, 0] > 2.0, wide * 0.0, wide)      # (tanh <= 1: an exact copy, made after the products)
        h = q.hits(rt[:, :6], 3, count=True)
        consumer = h.t.sum(dim=1) + h.count.float()
    torch.cuda.synchronize(DEV)
    assert torch.equal(consumer.view(torch.int32), want_sum.view(torch.int32))
    # N = 0: empty tensors, no call
    ctx.stats_reset()
    e = q.hits(wide[:0, :6], 5, attributes=True, count=True)
    assert e.t.shape == (0, 5) and e.prim.shape == (0, 5) and e.record.shape == (0, 5, 13) and e.count.shape == (0,) and q.count(wide[:0, :6]).shape == (0,)
    assert ctx.stats()["rays_closest"] == 0
    # per-ray node counts, and the refusals that need a device
    cnt = torch.empty((700, 2), dtype=torch.int32, device=DEV); nh = torch.empty(700, dtype=torch.int32, device=DEV)
    ctx.query_hits(wide.data_ptr(), 700, 8, 0, flags=_native.COUNT_NODES, out_count=nh.data_ptr(), counts=cnt.data_ptr())
    cn = cpu(cnt)
    assert np.array_equal(cpu(nh), w["count"]) and (cn[:, 1] >= w["count"]).all() and (cn[:, 0] >= 1).all()
    out = torch.empty(700 * 4, device=DEV)
    with pytest.raises(_native.TirtError, match=r"error -2:.*hit_stride"):
        ctx.query_hits(wide.data_ptr(), 700, 8, 4, out_hit=out.data_ptr(), hit_stride=12)
    with pytest.raises(_native.TirtError, match=r"error -2:.*tmax_stride"):
        ctx.query_hits(wide.data_ptr(), 700, 8, 4, out_t=out.data_ptr(), tmax=nh.data_ptr(), tmax_stride=0)
    with pytest.raises(_native.TirtError, match=r"error -2:.*not device memory"):
        ctx.query_hits(rays.ctypes.data, 700, 6, 4, out_t=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"error -2:.*ray_stride"):
        ctx.query_hits(wide.data_ptr(), 700, 5, 4, out_t=out.data_ptr())
    with pytest.raises(ValueError, match="k must be"):
        q.hits(wide[:, :6], 0)
    with pytest.raises(ValueError, match="k must be"):
        q.hits(wide[:, :6], 65)
    with pytest.raises(ValueError, match="k must be"):
        q.hits(wide[:, :6], 3.0)
    assert np.array_equal(bits(cpu(q.hits(wide[:, :6], np.int64(3)).t)), bits(wt))      # an int of any kind
    ctx.close()


# ---- the stack ------------------------------------------------------------------------------------------------------------------------
def test_stack(gpu_ctx_ok):
    b = built("chain")
    rays = ray_set(b, 2000, 3)                               # test_k1_is_closest's rays: the restatement is shared
    w = b.want("chain", rays)
    ctx = b.ctx
    ctx.stats_reset()
    b.hits(rays, 4, count=True, stack=2)                      # returns; the dropped entries are counted
    with pytest.raises(_native.TirtStackOverflow) as e:
        ctx.stats()
    assert e.value.stats["stack_overflow"] > 0
    wt, wp = mh.first_k(w, 4)
    for stack in (64, 40):                                   # 40: 16 entries in LDS, the rest in the spill tail
        t, prim, _, cnt = b.hits(rays, 4, count=True, stack=stack)
        assert ctx.stats()["stack_overflow"] == 0, stack
        assert np.array_equal(bits(t), bits(wt)) and np.array_equal(prim, wp) and np.array_equal(cnt, w["count"]), stack


# ---- count() alone, and the host route --------------------------------------------------------------------------------------------------
def test_count_alone_and_host_route(gpu_ctx_ok):
    b = built("quads")
    r = np.random.RandomState(12)
    n = 1500
    o = np.concatenate([r.uniform(-0.9, 0.9, (n, 2)), r.uniform(-4.5, 2.0, (n, 1))], axis=1)
    d = r.normal(size=(n, 3)); d[:, 2] *= 3.0; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(f)
    tm = r.uniform(0.5, 5.0, n).astype(f)
    for key, bound in (("count-free", None), ("count-tm", tm)):
        w = b.want(key, rays, bound)
        for flags in (0, EXH):
            q = RayQuery(b.sc, 64, flags)
            rt = on_dev(rays)
            c = cpu(q.count(rt, None if bound is None else on_dev(bound)))
            h = q.hits(rt, 16, tmax=None if bound is None else on_dev(bound), count=True)
            assert np.array_equal(c, cpu(h.count)) and np.array_equal(c, w["count"]), (key, flags)
            t, prim, rec, cnt, _ = b.ctx.trace_hits(rays, 0, tmax=bound, flags=flags)
            assert np.array_equal(cnt, c) and t.shape == (n, 0)
            t, prim, rec, cnt, _ = b.ctx.trace_hits(rays, 16, tmax=bound, flags=flags, attributes=True)
            assert np.array_equal(bits(t), bits(cpu(h.t))) and np.array_equal(prim, cpu(h.prim)) and np.array_equal(cnt, c)
            assert np.array_equal(bits(rec[..., 0]), bits(t))
    assert (w["count"] > 0).mean() > 0.5 and w["count"].max() <= 13


# ---- closest() and occluded() are untouched -----------------------------------------------------------------------------------------------
def test_closest_and_occluded_around_a_hits_call(gpu_ctx_ok):
    b = built("cornell")
    rays = ray_set(b, 3000, 21)
    rt = on_dev(rays)
    q = RayQuery(b.sc)
    c0 = q.closest(rt, attributes=True)
    o0 = q.occluded(rt, c0.t * 0.75)
    q.hits(rt, 64, attributes=True, count=True)               # the query scratch is shared, and this call grows it
    q.count(rt[:100])
    c1 = q.closest(rt, attributes=True)
    o1 = q.occluded(rt, c0.t * 0.75)
    torch.cuda.synchronize(DEV)
    assert torch.equal(c0.prim, c1.prim) and torch.equal(c0.t.view(torch.int32), c1.t.view(torch.int32))
    assert same_bits(cpu(c0.record), cpu(c1.record), nan_payload=True) and torch.equal(o0, o1)
