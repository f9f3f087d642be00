"""Ray queries on device memory (csrc/tirt_query.hip through tirt_query_closest / tirt_query_occluded and ti_raytrace_amd.RayQuery):
closest hits bit for bit the host route's (Context.trace_closest) and the oracle's, occlusion answers exactly (t < 1e6) & (t < tmax) of
Context.trace_shadow's t for every kind of tmax, strided layouts, refusals, chunking, ordering on the caller's stream, no interference
with PT_RGB, ray counts and stack overflows."""
import numpy as np
import pytest
import torch

import oracle_api as oa
from common import long_chain_scene, same_bits as same
from ti_raytrace_amd import RayQuery, scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EXH = _native.TRAVERSE_EXHAUSTIVE
_SCENES = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def cpu(x):
    torch.cuda.synchronize(DEV)
    return x.cpu().numpy()


def scene(name):
    """built once per module: Cornell box, Teapot (process_normal, env map: NaN smooth normals) and the 100k-triangle headline scene"""
    if name not in _SCENES:
        if name == "cornell":
            ex, W = scenes.cornell_box(64, 64, 4, device_id=0), 64
        elif name == "teapot":
            ex, W = scenes.single_model(64, 64, 4, device_id=0), 64
        else:
            ex, W = scenes.synthetic(256, 256, 4, device_id=0), 256
        ex.build_scene()
        if not ex.cam.view_inv_np.any():
            ex.frame_camera(0.8)
        _SCENES[name] = (ex, W)
    return _SCENES[name]


def ray_set(ex, W, n_random, seed=1):
    """camera rays of the W x W film, then n_random rays with origins uniform in the scene's bounds and uniform directions"""
    lo, hi = ex.scene.minboundarynp[0].astype(np.float64), ex.scene.maxboundarynp[0].astype(np.float64)
    r = np.random.RandomState(seed)
    o = lo + (hi - lo) * r.uniform(size=(n_random, 3))
    d = r.normal(size=(n_random, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rnd = np.concatenate([o, d], axis=1).astype(np.float32)
    return np.concatenate([oa.camera_rays(ex.cam, W, W), rnd], axis=0)


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", ["cornell", "teapot", "synthetic"])
def test_closest_equals_host_route(gpu_ctx_ok, name):
    ex, W = scene(name)
    ctx = ex.scene.ctx
    rays = ray_set(ex, W, 1 << 20)
    rt = on_dev(rays)
    for flags in (0, EXH):
        h = RayQuery(ex.scene, 64, flags).closest(rt, attributes=True)
        want, wprim, _ = ctx.trace_closest(rays, 64, flags)
        assert np.array_equal(cpu(h.prim), wprim), (name, flags)
        assert np.array_equal(bits(cpu(h.t)), bits(want[:, 0])), (name, flags)
        assert np.array_equal(bits(cpu(h.record)), bits(want)), (name, flags)
        assert 0.05 < (wprim >= 0).mean() < 0.999
    if name == "teapot":
        assert np.isnan(want[:, 7:10]).any()                 # the NaN smooth normals went through, bit for bit
    sub = rays[::16]
    for flags in (_native.COUNT_NODES, EXH | _native.COUNT_NODES):
        h, cnt = RayQuery(ex.scene, 64, flags).closest_counts(on_dev(sub))
        _, wprim, wcnt = ctx.trace_closest(sub, 64, flags)
        assert np.array_equal(cpu(h.prim), wprim) and np.array_equal(cpu(cnt), wcnt), (name, flags)


@pytest.mark.parametrize("name", ["cornell", "teapot", "synthetic"])
def test_equals_oracle(gpu_ctx_ok, name):
    ex, W = scene(name)
    o = oa.OracleScene(ex.scene, ex.cam)
    o.lbvh_build()
    if name == "teapot":
        o.process_normal(ex.scene.vertex_index_np)
    rays = ray_set(ex, W, 4096, seed=7)
    rays = rays[np.random.RandomState(0).choice(rays.shape[0], 4096, replace=False)]
    want, wprim, _ = o.closest_hit(rays)
    st, _, _ = o.shadow_hit(rays)
    rt = on_dev(rays)
    for flags in (0, EXH):
        q = RayQuery(ex.scene, 64, flags)
        h = q.closest(rt, attributes=True)
        gprim, grec = cpu(h.prim), cpu(h.record)
        assert np.array_equal(gprim, wprim), (name, flags, int((gprim != wprim).sum()))
        hit = wprim >= 0
        assert np.array_equal(bits(grec[:, 0]), bits(want[:, 0]))
        assert same(grec[hit], want[hit]), (name, flags)
        assert np.array_equal(cpu(q.occluded(rt)), st < 1.0e6), (name, flags)


def tmax_kinds(t):
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        return {"half": (t * f(0.5)).astype(f), "t": t.copy(), "next": np.nextafter(t, f(np.inf)).astype(f), "twice": (t * f(2)).astype(f),
                "inf": np.full_like(t, np.inf), "zero": np.zeros_like(t), "minus1": np.full_like(t, -1.0), "nan": np.full_like(t, np.nan)}


@pytest.mark.parametrize("name", ["cornell", "teapot", "synthetic"])
def test_occluded_is_exact(gpu_ctx_ok, name):
    ex, W = scene(name)
    ctx = ex.scene.ctx
    rays = ray_set(ex, W, 1 << 18, seed=3)
    rt = on_dev(rays)
    t, _, _ = ctx.trace_shadow(rays, 64, 0)
    miss = t >= np.float32(1e6)
    assert miss.any() and (~miss).any()
    kinds = tmax_kinds(t)
    pick = np.random.RandomState(5).randint(0, len(kinds), size=t.shape[0])
    kinds["mixed"] = np.stack(list(kinds.values()), axis=1)[np.arange(t.shape[0]), pick]
    for flags in (0, EXH):
        q = RayQuery(ex.scene, 64, flags)
        for kind, tm in kinds.items():
            want = (t < np.float32(1e6)) & (t < tm)
            got = cpu(q.occluded(rt, on_dev(tm)))
            assert got.dtype == np.bool_
            assert np.array_equal(got, want), (name, flags, kind, int((got != want).sum()))
            if kind == "t":
                assert not got.any()
            if kind == "next":
                assert np.array_equal(got, ~miss)
        for scalar in (float("inf"), 2.0e6, 0.0, -1.0, float("nan"), float(np.median(t[~miss]))):
            want = (t < np.float32(1e6)) & (t < np.float32(scalar))
            assert np.array_equal(cpu(q.occluded(rt, scalar)), want), (name, flags, scalar)
        assert np.array_equal(cpu(q.occluded(rt)), ~miss)
        assert not cpu(q.occluded(rt[torch.from_numpy(miss).to(DEV)], 2.0e6)).any()


def test_layouts_and_refusals(gpu_ctx_ok):
    ex, W = scene("cornell")
    rays = ray_set(ex, W, 50000, seed=11)
    rt = on_dev(rays)
    n = rt.shape[0]
    q = RayQuery(ex.scene)
    wide = torch.full((n, 8), 7.0, device=DEV)
    wide[:, :6] = rt
    view = wide[:, :6]
    assert view.stride() == (8, 1)
    a, b = q.closest(rt, attributes=True), q.closest(view, attributes=True)
    assert torch.equal(a.prim, b.prim) and torch.equal(a.t.view(torch.int32), b.t.view(torch.int32))
    assert torch.equal(a.record.view(torch.int32), b.record.view(torch.int32))
    tm = a.t * 0.75
    tm3 = torch.zeros((n, 3), device=DEV)
    tm3[:, 1] = tm
    assert torch.equal(q.occluded(rt, tm), q.occluded(view, tm3[:, 1]))
    # refusals (TypeError / ValueError before the library is touched)
    with pytest.raises(TypeError):
        q.closest(rt.cpu())
    with pytest.raises(TypeError):
        q.closest(rt.double())
    with pytest.raises(TypeError):
        q.closest(rays)
    with pytest.raises(ValueError):
        q.closest(rt.t().contiguous().t())                 # [N, 6] with stride(1) == N
    with pytest.raises(ValueError):
        q.closest(rt[:, :5])
    with pytest.raises(ValueError):
        q.occluded(rt, tm[:-1])
    with pytest.raises(TypeError):
        q.occluded(rt, tm.double())

    class OtherDevice:                                     # a scene on another device: the rays on cuda:0 are refused
        _ctx = None
        _device_id = 1
    with pytest.raises(ValueError):
        RayQuery(OtherDevice()).closest(rt)
    # empty batches launch nothing
    ctx = ex.scene.ctx
    ctx.stats_reset()
    e = q.closest(rt[:0], attributes=True)
    assert e.t.shape == (0,) and e.prim.shape == (0,) and e.record.shape == (0, 13)
    assert q.occluded(rt[:0]).shape == (0,)
    # the C level: a host pointer is refused with TIRT_ERR_ARG, nothing is launched
    host = np.ascontiguousarray(rays[:100])
    out = torch.empty(100, device=DEV)
    with pytest.raises(_native.TirtError, match=r"error -2:.*not device memory"):
        ctx.query_closest(host.ctypes.data, 100, 6, out_t=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"error -2:.*not device memory"):
        ctx.query_occluded(rt.data_ptr(), 100, 6, host.ctypes.data)
    with pytest.raises(_native.TirtError, match=r"error -2:.*ray_stride"):
        ctx.query_closest(rt.data_ptr(), 100, 5, out_t=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"error -2:.*hit_stride"):
        ctx.query_closest(rt.data_ptr(), 100, 6, out_hit=out.data_ptr(), hit_stride=12)
    with pytest.raises(_native.TirtError, match=r"error -2:.*unknown flags"):
        ctx.query_closest(rt.data_ptr(), 100, 6, flags=4, out_t=out.data_ptr())
    with pytest.raises(_native.TirtError, match=r"error -2:.*stack_size"):
        ctx.query_closest(rt.data_ptr(), 100, 6, stack_size=0, out_t=out.data_ptr())
    st = ctx.stats()
    assert st["rays_closest"] == 0 and st["rays_shadow"] == 0


def test_capturing_stream_is_refused(gpu_ctx_ok):
    ex, W = scene("cornell")
    rt = on_dev(ray_set(ex, W, 1000))
    q = RayQuery(ex.scene)
    s = torch.cuda.Stream(DEV)
    x = torch.zeros(16, device=DEV)
    with torch.cuda.stream(s):
        x.add_(1.0)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_native.TirtError, match="capturing"):
        with torch.cuda.graph(g, stream=s):
            x.add_(1.0)
            q.closest(rt)


def test_chunking(gpu_ctx_ok):
    ex, W = scene("synthetic")
    ctx = ex.scene.ctx
    rays = ray_set(ex, W, (1 << 20) + 7 - W * W, seed=13)
    assert rays.shape[0] == (1 << 20) + 7
    rt = on_dev(rays)
    q = RayQuery(ex.scene)
    a = q.closest(rt, attributes=True)
    tm = a.t * 0.5
    oa_ = q.occluded(rt, tm)
    ctx.set_option("query_chunk_rays", 1000)
    try:
        b = q.closest(rt, attributes=True)
        ob = q.occluded(rt, tm)
        torch.cuda.synchronize(DEV)
    finally:
        ctx.set_option("query_chunk_rays", 1 << 21)
    assert torch.equal(a.prim, b.prim) and torch.equal(a.record.view(torch.int32), b.record.view(torch.int32))
    assert torch.equal(oa_, ob)
    with pytest.raises(_native.TirtError):
        ctx.set_option("query_chunk_rays", 100)


def test_ordered_on_the_callers_stream(gpu_ctx_ok):
    ex, W = scene("synthetic")
    rays = ray_set(ex, W, 1 << 20, seed=17)
    src = on_dev(rays)
    q = RayQuery(ex.scene)
    want = q.closest(src)
    want_occ = q.occluded(src, want.t * 0.5)
    want_sum = want.t * 2.0 + want.prim.float()
    torch.cuda.synchronize(DEV)
    s = torch.cuda.Stream(DEV)
    big = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(s):
        for _ in range(8):                                 # keep the side stream busy before the rays exist
            big = torch.tanh(big @ big)
        rt = torch.where(big[0, 0] > 2.0, src * 0.0, src)   # (tanh <= 1: an exact copy of src, made after the products)
        h = q.closest(rt)
        consumer = h.t * 2.0 + h.prim.float()
        occ = q.occluded(rt, h.t * 0.5)
    torch.cuda.synchronize(DEV)
    assert torch.equal(h.prim, want.prim) and torch.equal(consumer.view(torch.int32), want_sum.view(torch.int32))
    assert torch.equal(occ, want_occ)


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    W = H = 64
    films = []
    for with_queries in (False, True):
        ex = scenes.cornell_box(W, H, 8, device_id=0)
        ex.build_scene()
        rt = on_dev(ray_set(ex, W, 100000, seed=19))
        q = RayQuery(ex.scene)
        for f in (0, 2, 4):
            ex.cam.frame = f; ex.cam.frame_cpu[0] = f
            ex.integrator.render_frames(2)
            if with_queries:
                h = q.closest(rt, attributes=True)
                q.occluded(rt, h.t * 0.5)
            else:
                ex.scene.ctx.sync()
        films.append(ex.integrator.hdr.to_numpy())
    assert np.array_equal(bits(films[0]), bits(films[1]))
    assert (films[0] != 0).any()


def test_ray_counts(gpu_ctx_ok):
    ex, W = scene("cornell")
    ctx = ex.scene.ctx
    rt = on_dev(ray_set(ex, W, 123457, seed=23))
    n = rt.shape[0]
    q = RayQuery(ex.scene)
    ctx.stats_reset()
    q.closest(rt)
    st = ctx.stats()
    assert st["rays_closest"] == n and st["rays_shadow"] == 0
    q.occluded(rt, 1.0)
    q.occluded(rt[:1000])
    st = ctx.stats()
    assert st["rays_closest"] == n and st["rays_shadow"] == n + 1000 and st["stack_overflow"] == 0


def test_host_route_call_shape(gpu_ctx_ok):
    """Context.trace_closest / trace_shadow share the closest-query path (csrc/tirt_query.hip) but keep the host route's shape: one k_trace
    launch per call whatever query_chunk_rays is, on the grid of option trace_grid (not trace_grid_alone), no launches_trace_* counts, every
    ray counted as a closest-hit ray, and the per-ray node counts of RayQuery.closest_counts."""
    ex = scenes.cornell_box(64, 64, 4, device_id=0)       # a context of its own: the options below stay with it
    ex.build_scene()
    if not ex.cam.view_inv_np.any():
        ex.frame_camera(0.8)
    ctx = ex.scene.ctx
    rays = ray_set(ex, 64, 20000, seed=29)
    n = rays.shape[0]
    assert (n + 255) // 256 > 16
    ctx.set_option("trace_grid", 8)
    ctx.set_option("trace_grid_alone", 16)
    ctx.set_option("query_chunk_rays", 1000)
    ctx.stats_reset()
    ctx.set_option("trace_timeline", 1)                   # the second counting launch from now: trace_shadow's if trace_closest made one
    _, prim, _ = ctx.trace_closest(rays, 64, _native.COUNT_NODES)
    t, sprim, _ = ctx.trace_shadow(rays, 64, _native.COUNT_NODES)
    waves = len(ctx.trace_timeline())
    ctx.set_option("trace_timeline", -1)
    st = ctx.stats()
    assert waves == 8 * 4                                  # trace_grid blocks of four waves
    assert st["launches_trace_closest"] == 0 and st["launches_trace_shadow"] == 0
    assert st["rays_closest"] == 2 * n and st["rays_shadow"] == 0
    assert np.array_equal(sprim, prim)
    # per-ray node counts: only with a lane for every ray are they free of the refill order of idle lanes (8 blocks refill all the time),
    # so they are compared on a context with the default grids, as in test_closest_equals_host_route
    ex, _ = scene("cornell")
    ctx = ex.scene.ctx
    _, prim, cnt = ctx.trace_closest(rays, 64, _native.COUNT_NODES)
    t, _, scnt = ctx.trace_shadow(rays, 64, _native.COUNT_NODES)
    h, qcnt = RayQuery(ex.scene, 64, _native.COUNT_NODES).closest_counts(on_dev(rays))
    assert np.array_equal(cpu(qcnt), cnt) and np.array_equal(scnt, cnt)
    assert np.array_equal(cpu(h.prim), prim) and np.array_equal(bits(cpu(h.t)), bits(t))


def test_stack_overflow_is_reported(gpu_ctx_ok):
    """The 600-deep duplicate-Morton chain of test_gpu_trace.py::test_very_long_duplicate_chain in the reference's own LBVH (option
    "traversal_tree" 0, where the reference's 64-entry stack overflows), traced with a 64-entry stack: the ordered walk keeps the far
    children of the chain on its stack and overflows on some camera rays (the exhaustive walk, popping the chain side first, does not).
    The host route and the query drop the same rays, and stats() reports it (a counted condition, not a fault)."""
    W = H = 32
    ex = long_chain_scene(W, H)
    ex.scene.ctx.set_option("traversal_tree", 0)
    ex.build_scene(); ex.frame_camera(0.8)
    rs = np.random.RandomState(9)
    o = rs.uniform(-1.5, 1.5, size=(3000, 3)); d = rs.normal(size=(3000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([oa.camera_rays(ex.cam, W, H), np.concatenate([o, d], axis=1).astype(np.float32)], axis=0)
    ctx = ex.scene.ctx
    ctx.stats_reset()
    ctx.trace_closest(rays, 64, 0)
    with pytest.raises(_native.TirtStackOverflow) as host:
        ctx.stats()
    n_host = host.value.stats["stack_overflow"]
    assert n_host > 0
    RayQuery(ex.scene, 64, 0).closest(on_dev(rays), attributes=True)
    with pytest.raises(_native.TirtStackOverflow) as dev:
        ctx.stats()
    assert dev.value.stats["stack_overflow"] == n_host
    assert ctx.stats()["stack_overflow"] == 0             # reported once
