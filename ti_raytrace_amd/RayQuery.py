"""Closest-hit and occlusion queries on rays held in PyTorch device tensors (no reference counterpart: the reference's
``Scene.closet_hit`` / ``closet_hit_shadow`` (Scene.py:702-744, 671-699) for rays that already live on the GPU).

    q = RayQuery(scene, stack_size=64, flags=0)           # scene after setup_data_gpu() (Example.build_scene)
    h = q.closest(rays, attributes=False)                 # RayHits(t [N] f32, prim [N] i32, record [N, 13] f32 or None)
    occ = q.occluded(rays, tmax=None)                     # [N] torch.bool: a hit with t < tmax (None = inf, a float, or an [N] f32 tensor)

``rays`` is a float32 tensor ``[N, C >= 6]`` on the scene context's device with ``stride(1) == 1`` and any row stride (origin, direction
in the first six columns: an ``[N, 8]`` tensor's ``[:, :6]`` view works).  The outputs come from ``torch.empty`` on that device and the
work is queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host (csrc/tirt_query.hip, include/tirt.h
``tirt_query_closest`` / ``tirt_query_occluded``).  ``record`` is tirt_trace_closest's: t, pos3, gnormal3, normal3, tex3.
"""
import collections
import os

from . import _native

RayHits = collections.namedtuple("RayHits", ["t", "prim", "record"])


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
        tptr, tstride, tall = 0, 1, float("inf")
        if tmax is None:
            pass
        elif isinstance(tmax, torch.Tensor):
            if tmax.dtype != torch.float32:
                raise TypeError("RayQuery.occluded: tmax must be float32, got %s" % tmax.dtype)
            if tmax.device != dev:
                raise ValueError("RayQuery.occluded: tmax is on %s, the rays on %s" % (tmax.device, dev))
            if tmax.dim() != 1 or tmax.shape[0] != n:
                raise ValueError("RayQuery.occluded: tmax must be [N] = [%d], got shape %s" % (n, tuple(tmax.shape)))
            if n > 1 and tmax.stride(0) < 1:
                raise ValueError("RayQuery.occluded: tmax must have a positive stride, got %d" % tmax.stride(0))
            if n:
                tptr, tstride = tmax.data_ptr(), (tmax.stride(0) if n > 1 else 1)
        elif isinstance(tmax, (int, float)):
            tall = float(tmax)
        else:
            raise TypeError("RayQuery.occluded: tmax must be None, a float or a float32 tensor, got %s" % type(tmax).__name__)
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.scene.ctx.query_occluded(rays.data_ptr(), n, stride, out.data_ptr(), tmax=tptr, tmax_stride=tstride, tmax_all=tall,
                                          stack_size=self.stack_size, flags=self.flags, stream=stream)
        return out.view(torch.bool)
