"""Closest-hit and occlusion queries on rays held in PyTorch device tensors (no reference counterpart: the reference's
``Scene.closet_hit`` / ``closet_hit_shadow`` (Scene.py:702-744, 671-699) for rays that already live on the GPU).

    q = RayQuery(scene, stack_size=64, flags=0)           # scene after setup_data_gpu() (Example.build_scene)
    h = q.closest(rays, attributes=False)                 # RayHits(t [N] f32, prim [N] i32, record [N, 13] f32 or None)
    occ = q.occluded(rays, tmax=None)                     # [N] torch.bool: a hit with t < tmax (None = inf, a float, or an [N] f32 tensor)
    m = q.hits(rays, k, tmax=None, attributes=False, count=False)   # RayMultiHits(t [N, k], prim [N, k], record [N, k, 13] or None, count [N] i32 or None)
    c = q.count(rays, tmax=None)                          # [N] int32: all hits with t < tmax

``rays`` is a float32 tensor ``[N, C >= 6]`` on the scene context's device with ``stride(1) == 1`` and any row stride (origin, direction
in the first six columns: an ``[N, 8]`` tensor's ``[:, :6]`` view works).  The outputs come from ``torch.empty`` on that device and the
work is queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host (csrc/tirt_query.hip, include/tirt.h
``tirt_query_closest`` / ``tirt_query_occluded``).  ``record`` is tirt_trace_closest's: t, pos3, gnormal3, normal3, tex3.
"""
import collections
import operator
import os

from . import _native

RayHits = collections.namedtuple("RayHits", ["t", "prim", "record"])
RayMultiHits = collections.namedtuple("RayMultiHits", ["t", "prim", "record", "count"])


def _torch():
    try:
        import torch
    except ImportError as exc:
        raise ImportError("ti_raytrace_amd.RayQuery needs PyTorch (ROCm build); the C-ABI tirt_query_closest / tirt_query_occluded "
                          "(include/tirt.h) works without it") from exc
    return torch


class RayQuery:
    def __init__(self, scene, stack_size=64, flags=0):
        self.torch = _torch()
        if not 1 <= int(stack_size) <= 4096:
            raise ValueError("RayQuery: stack_size must be 1..4096, got %r" % (stack_size,))
        if int(flags) & ~(_native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES):
            raise ValueError("RayQuery: flags are TRAVERSE_EXHAUSTIVE and COUNT_NODES, got %r" % (flags,))
        self.scene = scene
        self.stack_size = int(stack_size)
        self.flags = int(flags)

    def _device(self):
        """the scene context's device, without creating the context"""
        ctx = getattr(self.scene, "_ctx", None)
        if ctx is not None:
            dev = ctx.device_id
        else:
            dev = getattr(self.scene, "_device_id", None)
            if dev is None:
                dev = int(os.environ.get("LOCAL_RANK", "0"))           # what Scene.ctx will pick
        return self.torch.device("cuda", int(dev))

    def _check_rays(self, rays, what):
        torch = self.torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError("RayQuery.%s: rays must be a torch.Tensor, got %s" % (what, type(rays).__name__))
        if rays.dtype != torch.float32:
            raise TypeError("RayQuery.%s: rays must be float32, got %s" % (what, rays.dtype))
        if rays.device.type != "cuda":
            raise TypeError("RayQuery.%s: rays must be on the GPU, got a %s tensor" % (what, rays.device.type))
        if rays.dim() != 2 or rays.shape[1] < 6:
            raise ValueError("RayQuery.%s: rays must be [N, C >= 6] (origin, direction), got shape %s" % (what, tuple(rays.shape)))
        dev = self._device()
        if rays.device != dev:
            raise ValueError("RayQuery.%s: rays are on %s, the scene's context on %s" % (what, rays.device, dev))
        n = rays.shape[0]
        if n > 1 and rays.stride(0) < 6:
            raise ValueError("RayQuery.%s: rows of rays overlap (stride(0) = %d < 6)" % (what, rays.stride(0)))
        if n > 0 and rays.shape[1] > 1 and rays.stride(1) != 1:
            raise ValueError("RayQuery.%s: the last dimension of rays must have stride 1, got %d" % (what, rays.stride(1)))
        return dev, n, (rays.stride(0) if n > 1 else max(rays.shape[1], 6))

    def _check_tmax(self, tmax, dev, n, what):
        """tmax: None (= inf), a float for every ray, or an [N] float32 tensor on the rays' device (any positive stride) -> (address or 0, stride, value for all)"""
        torch = self.torch
        tptr, tstride, tall = 0, 1, float("inf")
        if tmax is None:
            pass
        elif isinstance(tmax, torch.Tensor):
            if tmax.dtype != torch.float32:
                raise TypeError("RayQuery.%s: tmax must be float32, got %s" % (what, tmax.dtype))
            if tmax.device != dev:
                raise ValueError("RayQuery.%s: tmax is on %s, the rays on %s" % (what, tmax.device, dev))
            if tmax.dim() != 1 or tmax.shape[0] != n:
                raise ValueError("RayQuery.%s: tmax must be [N] = [%d], got shape %s" % (what, n, tuple(tmax.shape)))
            if n > 1 and tmax.stride(0) < 1:
                raise ValueError("RayQuery.%s: tmax must have a positive stride, got %d" % (what, tmax.stride(0)))
            if n:
                tptr, tstride = tmax.data_ptr(), (tmax.stride(0) if n > 1 else 1)
        elif isinstance(tmax, (int, float)):
            tall = float(tmax)
        else:
            raise TypeError("RayQuery.%s: tmax must be None, a float or a float32 tensor, got %s" % (what, type(tmax).__name__))
        return tptr, tstride, tall

    def closest(self, rays, attributes=False):
        """Closest hit of every ray, bit for bit Context.trace_closest's: t (1e6 on a miss), prim (-1 on a miss) and, with
        attributes=True, the 13-float record.  Asynchronous on the current stream."""
        torch = self.torch
        dev, n, stride = self._check_rays(rays, "closest")
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        rec = torch.empty((n, 13), dtype=torch.float32, device=dev) if attributes else None
        if n == 0:
            return RayHits(t, prim, rec)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.scene.ctx.query_closest(rays.data_ptr(), n, stride, self.stack_size, self.flags, out_t=t.data_ptr(), out_prim=prim.data_ptr(),
                                     out_hit=rec.data_ptr() if rec is not None else 0, hit_stride=13, stream=stream)
        return RayHits(t, prim, rec)

    def closest_counts(self, rays):
        """closest() with the per-ray N_box / N_leaf counts ([N, 2] int32) of a COUNT_NODES traversal: (RayHits, counts)"""
        torch = self.torch
        dev, n, stride = self._check_rays(rays, "closest_counts")
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_closest(rays.data_ptr(), n, stride, self.stack_size, self.flags | _native.COUNT_NODES, out_t=t.data_ptr(),
                                         out_prim=prim.data_ptr(), counts=counts.data_ptr(), stream=stream)
        return RayHits(t, prim, None), counts

    def occluded(self, rays, tmax=None):
        """[N] bool: the ray's closest hit (Context.trace_shadow's t) lies before tmax -- t < 1e6 and t < tmax.  tmax: None (= inf: any
        hit), a float for every ray, or an [N] float32 tensor on the same device (any stride).  tmax <= 0 or NaN gives False."""
        torch = self.torch
        dev, n, stride = self._check_rays(rays, "occluded")
        tptr, tstride, tall = self._check_tmax(tmax, dev, n, "occluded")
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_occluded(rays.data_ptr(), n, stride, out.data_ptr(), tmax=tptr, tmax_stride=tstride, tmax_all=tall,
                                          stack_size=self.stack_size, flags=self.flags, stream=stream)
        return out.view(torch.bool)

    def hits(self, rays, k, tmax=None, attributes=False, count=False):
        """The first k hits along every ray, in order (include/tirt.h, "First K hits"): RayMultiHits(t [N, k] f32, prim [N, k] i32, record [N, k, 13] f32 or
        None, count [N] i32 or None).  Entry 0 is closest()'s hit, bit for bit; entries beyond a ray's hits are 1e6 and -1.  tmax as for occluded(): only
        hits with t < tmax.  count=True also returns the number of ALL hits below tmax (it may exceed k; the walk then culls by tmax alone).
        Asynchronous on the current stream."""
        torch = self.torch
        dev, n, stride = self._check_rays(rays, "hits")
        try:
            k = None if isinstance(k, bool) else operator.index(k)      # (an int of any kind: numpy's too)
        except TypeError:
            k = None
        if k is None or not 1 <= k <= _native.HITS_MAX:
            raise ValueError("RayQuery.hits: k must be an int in 1..%d (count() returns the count alone)" % _native.HITS_MAX)
        tptr, tstride, tall = self._check_tmax(tmax, dev, n, "hits")
        t = torch.empty((n, k), dtype=torch.float32, device=dev)
        prim = torch.empty((n, k), dtype=torch.int32, device=dev)
        rec = torch.empty((n, k, 13), dtype=torch.float32, device=dev) if attributes else None
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if count else None
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_hits(rays.data_ptr(), n, stride, k, self.stack_size, self.flags, tmax=tptr, tmax_stride=tstride, tmax_all=tall,
                                      out_t=t.data_ptr(), out_prim=prim.data_ptr(), out_hit=rec.data_ptr() if rec is not None else 0, hit_stride=13,
                                      out_count=cnt.data_ptr() if cnt is not None else 0, stream=stream)
        return RayMultiHits(t, prim, rec, cnt)

    def count(self, rays, tmax=None):
        """[N] int32: the number of hits along every ray with t < tmax (crossing parity, thickness, transmittance).  Asynchronous on the current stream."""
        torch = self.torch
        dev, n, stride = self._check_rays(rays, "count")
        tptr, tstride, tall = self._check_tmax(tmax, dev, n, "count")
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_hits(rays.data_ptr(), n, stride, 0, self.stack_size, self.flags, tmax=tptr, tmax_stride=tstride, tmax_all=tall,
                                      out_count=cnt.data_ptr(), stream=stream)
        return cnt
