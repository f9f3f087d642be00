"""The host entries of the queries (tirt_trace_closest / _shadow, tirt_trace_hits, tirt_closest_point / tirt_signed_distance, tirt_nearest, tirt_mesh_distance,
tirt_point_pairs / tirt_mesh_pairs, tirt_sweep) through _native.lib() itself, for what the families' own suites do not reach: every entry stages its arrays
through one object (csrc/tirt_query_stage.h), and an output the caller leaves out is a column that is not copied back -- or, in some entries, not there.

  * every output at once, then each output left out in turn (tirt_sweep: also `blocked` alone): what was asked for has the bits of the full call.  Every
    array starts as the sentinel byte 0xA5 and must come back without it; an array that was not passed cannot be written at all
  * a device-route call, host-route calls that make the staging buffer grow, the device-route call again: the same bits
  * pair lists into arrays that cut the rows: what lies behind the last row that fits stays the sentinel
The cornell scene, n = 257 (five waves, the last one ragged), k = 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import closest_point_expected as E
from ti_raytrace_amd import scenes, _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F, I = np.float32, np.int32
N, K = 257, 3
COUNT = _native.COUNT_NODES
SENT = 0xA5
_EX = []


def cornell():
    """(context, lower corner, largest extent) of the built cornell scene, once per module"""
    if not _EX:
        ex = scenes.cornell_box(16, 16, 1, device_id=0)
        ex.build_scene()
        v = E.scene_geometry(ex.scene).tris.astype(np.float64).reshape(-1, 3)
        _EX.append((ex, v.min(axis=0), float((v.max(axis=0) - v.min(axis=0)).max())))
    ex, lo, ext = _EX[0]
    return ex.scene.ctx, lo, ext


def points(n, seed=5):
    """n float32 points in 1.5 x the scene's box; one row is NaN (such a query finds nothing: its outputs are written all the same)"""
    _, lo, ext = cornell()
    p = (lo + ext * np.random.RandomState(seed).uniform(-0.25, 1.25, (n, 3))).astype(F)
    p[n // 2, 1] = np.nan
    return p


def triangles(n):
    _, _, ext = cornell()
    return (points(n, 6)[:, None, :] + (0.05 * ext * np.random.RandomState(7).uniform(-1, 1, (n, 3, 3))).astype(F)).astype(F)


def rays(n):
    d = np.random.RandomState(8).normal(size=(n, 3))
    return np.concatenate([np.nan_to_num(points(n, 9)), d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(F)


def sentinel(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = SENT
    return a


def no_sentinel(a):
    """no element of `a` still is the fill pattern (an answer has it with probability ~0: -2.9e-16 as a float, -1515870811 as an int, 165 as a flag)"""
    return not (a == sentinel(1, a.dtype)[0]).any() if a.dtype.kind != "f" else not (a.view(np.uint32) == 0xA5A5A5A5).any()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    return a.view(np.uint8).reshape(-1)


def leave_one_out(shapes, call, required=(), extra=(), same_walk=lambda keep: True):
    """shapes: output name -> (shape, dtype).  call(arrays) runs the entry on a dict name -> array or None.  The full call, then one call per output that may
    be left out, then the subsets of `extra` (tuples of the names to keep).  same_walk(keep): false where the outputs left out select another walk -- the answers
    are the same, the visit counts are that walk's and are only held to be written."""
    def run(keep):
        arrays = {k: sentinel(*shapes[k]) if k in keep else None for k in shapes}
        call(arrays)
        return arrays
    full = run(set(shapes))
    for k, a in full.items():
        assert no_sentinel(a), (k, "the full call left part of it unwritten")
    subsets = [set(shapes) - {k} for k in shapes if k not in required] + [set(e) for e in extra]
    assert subsets
    for keep in subsets:
        got = run(keep)
        for k in keep:
            if k == "counts" and not same_walk(keep):
                assert no_sentinel(got[k])
                continue
            assert np.array_equal(bits(got[k]), bits(full[k])), (sorted(set(shapes) - keep), "left out:", k, "differs from the full call")


def check(rc):
    _native.check(rc)


def test_trace_closest_and_shadow(gpu_ctx_ok):
    ctx, _, _ = cornell()
    r = rays(N)
    for fn, width in ((_native.lib().tirt_trace_closest, 13), (_native.lib().tirt_trace_shadow, 1)):
        leave_one_out({"f": ((N, width), F), "prim": ((N,), I), "counts": ((N, 2), I)},
                      lambda a: check(fn(ctx.handle, r.reshape(-1), N, 64, COUNT, a["f"].reshape(-1), a["prim"], ptr(a["counts"]))), required=("f", "prim"))


def test_trace_hits(gpu_ctx_ok):
    ctx, _, _ = cornell()
    r = rays(N)
    leave_one_out({"t": ((N, K), F), "prim": ((N, K), I), "hit": ((N, K, 13), F), "count": ((N,), I), "counts": ((N, 2), I)},
                  lambda a: check(_native.lib().tirt_trace_hits(ctx.handle, r.reshape(-1), N, None, K, 64, COUNT, ptr(a["t"]), ptr(a["prim"]), ptr(a["hit"]),
                                                                ptr(a["count"]), ptr(a["counts"]))), same_walk=lambda keep: "count" in keep)      # (no count: the list's threshold culls too)


def test_closest_point_and_signed_distance(gpu_ctx_ok):
    ctx, _, ext = cornell()
    p = points(N)
    dmax = np.full(N, 2.0 * ext, F)
    shapes = {"d2": ((N,), F), "prim": ((N,), I), "point": ((N, 3), F), "uv": ((N, 2), F), "counts": ((N, 2), I)}
    leave_one_out(shapes, lambda a: check(_native.lib().tirt_closest_point(ctx.handle, p.reshape(-1), N, ptr(dmax), 64, COUNT, ptr(a["d2"]), ptr(a["prim"]),
                                                                           ptr(a["point"]), ptr(a["uv"]), ptr(a["counts"]))))
    shapes["sd"] = ((N,), F)
    leave_one_out(shapes, lambda a: check(_native.lib().tirt_signed_distance(ctx.handle, p.reshape(-1), N, None, 64, COUNT, ptr(a["d2"]), ptr(a["prim"]),
                                                                             ptr(a["point"]), ptr(a["uv"]), ptr(a["counts"]), ptr(a["sd"]))), required=("sd",))


def test_nearest(gpu_ctx_ok):
    ctx, _, _ = cornell()
    p = points(N)
    leave_one_out({"d2": ((N, K), F), "prim": ((N, K), I), "point": ((N, K, 3), F), "uv": ((N, K, 2), F), "count": ((N,), I), "counts": ((N, 2), I)},
                  lambda a: check(_native.lib().tirt_nearest(ctx.handle, p.reshape(-1), N, None, K, 64, COUNT, ptr(a["d2"]), ptr(a["prim"]), ptr(a["point"]),
                                                             ptr(a["uv"]), ptr(a["count"]), ptr(a["counts"]))), same_walk=lambda keep: "count" in keep)      # (no count: the list's threshold culls too)


def test_mesh_distance(gpu_ctx_ok):
    ctx, _, _ = cornell()
    t = triangles(N)
    leave_one_out({"d2": ((N,), F), "prim": ((N,), I), "code": ((N,), I), "points": ((N, 2, 3), F), "counts": ((N, 2), I)},
                  lambda a: check(_native.lib().tirt_mesh_distance(ctx.handle, t.reshape(-1), N, None, 64, COUNT, ptr(a["d2"]), ptr(a["prim"]), ptr(a["code"]),
                                                                   ptr(a["points"]), ptr(a["counts"]))))


def test_sweep(gpu_ctx_ok):
    ctx, _, ext = cornell()
    r = rays(N)
    radius = np.full(N, 0.03 * ext, F)
    leave_one_out({"t": ((N,), F), "prim": ((N,), I), "code": ((N,), I), "point": ((N, 3), F), "uv": ((N, 2), F), "normal": ((N, 3), F), "blocked": ((N,), np.uint8),
                   "counts": ((N, 2), I)},
                  lambda a: check(_native.lib().tirt_sweep(ctx.handle, r.reshape(-1), N, ptr(radius), 0.0, None, 64, COUNT, ptr(a["t"]), ptr(a["prim"]), ptr(a["code"]),
                                                           ptr(a["point"]), ptr(a["uv"]), ptr(a["normal"]), ptr(a["blocked"]), ptr(a["counts"]))),
                  extra=(("blocked",), ("blocked", "counts")), same_walk=lambda keep: bool(keep & {"t", "prim", "code", "point", "uv", "normal"}))      # blocked alone: the walk that stops at the first contact


def pairs_call(ctx, tri, q, dmax, mode, cap, flags, a):
    """a: row_start, d2, prim, and code / points (triangles) or point / uv (points), counts"""
    if tri:
        check(_native.lib().tirt_mesh_pairs(ctx.handle, ptr(q), N, ptr(dmax), mode, cap, 64, flags, ptr(a["row_start"]), ptr(a["d2"]), ptr(a["prim"]), ptr(a["code"]),
                                            ptr(a["points"]), ptr(a["counts"])))
    else:
        check(_native.lib().tirt_point_pairs(ctx.handle, ptr(q), N, ptr(dmax), mode, cap, 64, flags, ptr(a["row_start"]), ptr(a["d2"]), ptr(a["prim"]), ptr(a["point"]),
                                             ptr(a["uv"]), ptr(a["counts"])))


def pairs_setup(tri):
    ctx, _, ext = cornell()
    q = triangles(N) if tri else points(N)
    dmax = np.full(N, 0.3 * ext, F)
    row = np.zeros(N + 1, np.int64)
    pairs_call(ctx, tri, q, dmax, _native.PAIRS_COUNT, 0, 0, {"row_start": row, "d2": None, "prim": None, "code": None, "points": None, "point": None, "uv": None, "counts": None})
    total = int(row[-1])
    assert total > N and (np.diff(row) > 1).any(), "the bound gives rows of several pairs"
    attrs = {"code": ((total,), I), "points": ((total, 2, 3), F)} if tri else {"point": ((total, 3), F), "uv": ((total, 2), F)}
    return ctx, q, dmax, row, total, attrs


@pytest.mark.parametrize("tri", [False, True])
def test_pairs(gpu_ctx_ok, tri):
    """BOTH into arrays that hold every pair.  Without the order (TIRT_PAIRS_UNORDERED: a row is in the walk's order, the same in every call) out_d2 may be
    left out; out_prim only together with the per-pair points, which need it"""
    ctx, q, dmax, _, total, attrs = pairs_setup(tri)
    shapes = {"row_start": ((N + 1,), np.int64), "d2": ((total,), F), "prim": ((total,), I), "counts": ((N, 2), I)}
    shapes.update(attrs)
    flags = COUNT | _native.PAIRS_UNORDERED
    leave_one_out(shapes, lambda a: pairs_call(ctx, tri, q, dmax, _native.PAIRS_BOTH, total, flags, {**dict.fromkeys(("code", "points", "point", "uv")), **a}),
                  required=("row_start", "prim"), extra=(("row_start", "d2", "counts") + (("code",) if tri else ()),))
    # with the order: both keys are needed, the rest may go
    leave_one_out(shapes, lambda a: pairs_call(ctx, tri, q, dmax, _native.PAIRS_BOTH, total, COUNT, {**dict.fromkeys(("code", "points", "point", "uv")), **a}),
                  required=("row_start", "prim", "d2"))


@pytest.mark.parametrize("tri", [False, True])
def test_pairs_into_arrays_that_cut_the_rows(gpu_ctx_ok, tri):
    ctx, q, dmax, row, total, attrs = pairs_setup(tri)
    none = dict.fromkeys(("code", "points", "point", "uv", "counts"))
    full = {"row_start": sentinel((N + 1,), np.int64), "d2": sentinel((total,), F), "prim": sentinel((total,), I)}
    full.update({k: sentinel(*s) for k, s in attrs.items()})
    pairs_call(ctx, tri, q, dmax, _native.PAIRS_BOTH, total, 0, {**none, **full})
    assert np.array_equal(full["row_start"], row)
    cut = int(np.nonzero(np.diff(row) > 1)[0][N // 8])        # a row of several pairs, some way in
    cap = int(row[cut]) + 1                                   # ... of which one pair would fit: the row is not written, nor is any after it
    written = int(row[cut])
    assert 0 < written < cap < total
    got = {"row_start": sentinel((N + 1,), np.int64), "d2": sentinel((cap,), F), "prim": sentinel((cap,), I)}
    got.update({k: sentinel((cap,) + s[0][1:], s[1]) for k, s in attrs.items()})
    pairs_call(ctx, tri, q, dmax, _native.PAIRS_BOTH, cap, 0, {**none, **got})
    assert np.array_equal(got["row_start"], row)              # the lengths are those of all rows
    for k in got:
        if k == "row_start":
            continue
        assert np.array_equal(bits(got[k][:written]), bits(full[k][:written])), k
        assert (bits(got[k][written:]) == SENT).all(), (k, "written behind the last row that fits")


def test_device_route_unchanged_by_host_routes_that_grow_the_stage(gpu_ctx_ok):
    """device route (n = 1024), host route (n = 257), host route (n = 4096: the staging buffer grows), the device route again -- for the closest point, whose
    kernels need no scratch, and for the k nearest, whose lists live in the kernels' scratch"""
    ctx, _, _ = cornell()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    p_dev = torch.from_numpy(points(1024, 11)).to(DEV)

    def device_closest():
        d2, prim = torch.full((1024,), -1.0, device=DEV), torch.full((1024,), -7, dtype=torch.int32, device=DEV)
        point, uv = torch.full((1024, 3), -1.0, device=DEV), torch.full((1024, 2), -1.0, device=DEV)
        ctx.query_closest_point(p_dev.data_ptr(), 1024, 3, out_d2=d2.data_ptr(), out_prim=prim.data_ptr(), out_point=point.data_ptr(), out_uv=uv.data_ptr(), stream=stream)
        torch.cuda.synchronize(DEV)
        return [x.cpu().numpy() for x in (d2, prim, point, uv)]

    def device_nearest():
        d2, prim = torch.full((1024, K), -1.0, device=DEV), torch.full((1024, K), -7, dtype=torch.int32, device=DEV)
        cnt = torch.full((1024,), -7, dtype=torch.int32, device=DEV)
        ctx.query_nearest(p_dev.data_ptr(), 1024, 3, K, out_d2=d2.data_ptr(), out_prim=prim.data_ptr(), out_count=cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize(DEV)
        return [x.cpu().numpy() for x in (d2, prim, cnt)]

    for device, host in ((device_closest, lambda n: ctx.closest_point(points(n, 12))), (device_nearest, lambda n: ctx.nearest(points(n, 12), K))):
        first = device()
        small = host(257)
        large = host(4096)
        again = device()
        for a, b in zip(first, again):
            assert np.array_equal(bits(a), bits(b))
        for a, b in zip(small, large):       # (the same seed: the small call's points are the large call's first 257 up to the NaN rows)
            if a is not None:
                rows = np.setdiff1d(np.arange(257), [257 // 2])
                assert np.array_equal(bits(a[rows]), bits(b[rows]))
