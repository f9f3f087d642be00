"""The first contact of a moving sphere with a scene, for sweeps held in PyTorch device tensors (no reference counterpart; include/tirt.h,
"Sphere sweep": the definition, bit for bit; csrc/tirt_sweep.hip: the walk over the scene's 4-wide nodes).

    q = SweepQuery(scene, stack_size=64, flags=0)         # scene after setup_data_gpu() (Example.build_scene)
    h = q.cast(rays, radius, tmax=None, attributes=False) # SweepHits(t [N] f32, prim [N] i32, code [N] i32, point [N, 3], uv [N, 2], normal [N, 3] or None)
    b = q.blocked(rays, radius, tmax=None)                # [N] torch.bool: some primitive is touched at a t <= tmax
    h, counts = q.cast_counts(rays, radius, tmax=None)    # with the per-query N_box / N_leaf of a COUNT_NODES walk

``rays`` follows ``RayQuery``'s contract: a float32 tensor ``[N, C >= 6]`` on the scene context's device with ``stride(1) == 1`` and any row
stride (origin, direction in the first six columns).  The direction is NOT normalised: with ``d = p1 - p0`` and ``tmax = 1``, ``t`` is the time of
impact within the step.  ``radius`` and ``tmax`` are a float for every query or an ``[N]`` float32 tensor on the same device (any positive
stride); ``tmax=None`` is no bound.  A sphere of radius ``radius`` whose centre moves along ``o + t d`` first touches primitive ``prim`` at ``t``;
``code`` names the feature (0 overlap at the start, 1 face, 2..4 edge ab / bc / ca, 5..7 corner a / b / c, 8 / 9 an analytic sphere from
outside / inside), ``point`` is the contact point with its ``uv`` in the hit record's convention and ``normal`` the unit vector from it to the
centre at contact.  No contact: ``t = inf``, ``prim = -1``, ``code = -1``, attributes 0 -- so does a query with a non-finite ray, a negative or
non-finite radius or a negative or NaN bound.  ``radius = 0`` is the centre line by the sweep's formulas, not ``RayQuery.closest``'s bits.
The outputs come from ``torch.empty`` and the work is queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host.
"""
import collections
import os

from . import _native

SweepHits = collections.namedtuple("SweepHits", ["t", "prim", "code", "point", "uv", "normal"])


def _torch():
    try:
        import torch
    except ImportError as exc:
        raise ImportError("ti_raytrace_amd.SweepQuery needs PyTorch (ROCm build); the C-ABI tirt_query_sweep (include/tirt.h) works without it") from exc
    return torch


class SweepQuery:
    def __init__(self, scene, stack_size=64, flags=0):
        self.torch = _torch()
        if not 1 <= int(stack_size) <= 4096:
            raise ValueError("SweepQuery: stack_size must be 1..4096, got %r" % (stack_size,))
        if int(flags) & ~(_native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES):
            raise ValueError("SweepQuery: flags are TRAVERSE_EXHAUSTIVE and COUNT_NODES, got %r" % (flags,))
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
        """type and layout of the rays (these checks need no device) -> (N, row stride)"""
        torch = self.torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError("SweepQuery.%s: rays must be a torch.Tensor, got %s" % (what, type(rays).__name__))
        if rays.dtype != torch.float32:
            raise TypeError("SweepQuery.%s: rays must be float32, got %s" % (what, rays.dtype))
        if rays.dim() != 2 or rays.shape[1] < 6:
            raise ValueError("SweepQuery.%s: rays must be [N, C >= 6] (origin, direction), got shape %s" % (what, tuple(rays.shape)))
        n = rays.shape[0]
        if n > 1 and rays.stride(0) < 6:
            raise ValueError("SweepQuery.%s: rows of rays overlap (stride(0) = %d < 6)" % (what, rays.stride(0)))
        if n > 0 and rays.stride(1) != 1:
            raise ValueError("SweepQuery.%s: the last dimension of rays must have stride 1, got %d" % (what, rays.stride(1)))
        return n, (rays.stride(0) if n > 1 else max(rays.shape[1], 6))

    def _check_per_query(self, value, name, none_is, n, what):
        """type and layout of radius / tmax: None (where allowed), a float for every query, or an [N] float32 tensor (any positive stride)
        -> (the tensor or None, stride, value for all)"""
        torch = self.torch
        if value is None and none_is is not None:
            return None, 1, none_is
        if isinstance(value, torch.Tensor):
            if value.dtype != torch.float32:
                raise TypeError("SweepQuery.%s: %s must be float32, got %s" % (what, name, value.dtype))
            if value.dim() != 1 or value.shape[0] != n:
                raise ValueError("SweepQuery.%s: %s must be [N] = [%d], got shape %s" % (what, name, n, tuple(value.shape)))
            if n > 1 and value.stride(0) < 1:
                raise ValueError("SweepQuery.%s: %s must have a positive stride, got %d" % (what, name, value.stride(0)))
            return value, (value.stride(0) if n > 1 else 1), none_is if none_is is not None else 0.0
        if isinstance(value, (int, float)) and not isinstance(value, bool):
            return None, 1, float(value)
        raise TypeError("SweepQuery.%s: %s must be %sa float or a float32 tensor, got %s"
                        % (what, name, "None, " if none_is is not None else "", type(value).__name__))

    def _front(self, rays, radius, tmax, what):
        """RayQuery's checks with this method's name: types and layouts first (no device needed), then where the tensors live"""
        n, stride = self._check_rays(rays, what)
        rten, rstride, rall = self._check_per_query(radius, "radius", None, n, what)
        tten, tstride, tall = self._check_per_query(tmax, "tmax", float("inf"), n, what)
        if rays.device.type != "cuda":
            raise TypeError("SweepQuery.%s: rays must be on the GPU, got a %s tensor" % (what, rays.device.type))
        dev = self._device()
        if rays.device != dev:
            raise ValueError("SweepQuery.%s: rays are on %s, the scene's context on %s" % (what, rays.device, dev))
        for ten, name in ((rten, "radius"), (tten, "tmax")):
            if ten is not None and ten.device != dev:
                raise ValueError("SweepQuery.%s: %s is on %s, the rays on %s" % (what, name, ten.device, dev))
        return dev, n, dict(ray_stride=stride, radius=rten.data_ptr() if rten is not None and n else 0, radius_stride=rstride, radius_all=rall,
                            tmax=tten.data_ptr() if tten is not None and n else 0, tmax_stride=tstride, tmax_all=tall, stack_size=self.stack_size)

    def cast(self, rays, radius, tmax=None, attributes=False):
        """The first contact of every sweep, bit for bit Context.sweep's: t (inf where there is none), prim (-1), code (-1) and, with
        attributes=True, the contact point, its (u, v) and the normal.  Asynchronous on the current stream."""
        torch = self.torch
        dev, n, kw = self._front(rays, radius, tmax, "cast")
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        code = torch.empty(n, dtype=torch.int32, device=dev)
        point = torch.empty((n, 3), dtype=torch.float32, device=dev) if attributes else None
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev) if attributes else None
        normal = torch.empty((n, 3), dtype=torch.float32, device=dev) if attributes else None
        if n:
            self.scene.ctx.query_sweep(rays.data_ptr(), n, flags=self.flags, out_t=t.data_ptr(), out_prim=prim.data_ptr(), out_code=code.data_ptr(),
                                       out_point=point.data_ptr() if attributes else 0, out_uv=uv.data_ptr() if attributes else 0,
                                       out_normal=normal.data_ptr() if attributes else 0, stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
        return SweepHits(t, prim, code, point, uv, normal)

    def blocked(self, rays, radius, tmax=None):
        """[N] bool: the sphere touches some primitive at a finite t <= tmax (cast(...).prim >= 0, through a walk that stops at the first accepted contact).
        Asynchronous on the current stream."""
        torch = self.torch
        dev, n, kw = self._front(rays, radius, tmax, "blocked")
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        if n:
            self.scene.ctx.query_sweep(rays.data_ptr(), n, flags=self.flags, out_blocked=out.data_ptr(),
                                       stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
        return out.view(torch.bool)

    def cast_counts(self, rays, radius, tmax=None):
        """cast() with the per-query N_box / N_leaf counts ([N, 2] int32) of a COUNT_NODES walk: (SweepHits, counts)"""
        torch = self.torch
        dev, n, kw = self._front(rays, radius, tmax, "cast_counts")
        t = torch.empty(n, dtype=torch.float32, device=dev)
        prim = torch.empty(n, dtype=torch.int32, device=dev)
        code = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n:
            self.scene.ctx.query_sweep(rays.data_ptr(), n, flags=self.flags | _native.COUNT_NODES, out_t=t.data_ptr(), out_prim=prim.data_ptr(),
                                       out_code=code.data_ptr(), counts=counts.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
        return SweepHits(t, prim, code, None, None, None), counts
