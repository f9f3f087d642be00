"""The edge-avoiding a-trous denoiser on PyTorch device tensors (no reference counterpart; include/tirt.h ``tirt_denoise_device``,
csrc/tirt_denoise.hip).

    out = denoise(hdr, aov, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1, ctx=None)      # a new [W, H, 3] float32 tensor

``hdr`` is a contiguous float32 tensor ``[W, H, 3]`` and ``aov`` one ``[W, H, 8]`` (albedo3, normal3, depth, alpha: what
``PathTrace.aov_to_torch()`` returns, or the sum of the ranks' records of a tiled job), both on one GPU.  ``ctx`` is a ``_native.Context`` of
that device -- ``scene.ctx`` when there is a scene; without one a context per device is made on first use and kept: the filter needs no
scene and no film.  The work is queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host.  The same filter, bit
for bit, as ``PathTrace.denoise()``.

    out = denoise_var(hdr, aov, moments, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1, ctx=None)

is the variance-guided mode (``tirt_denoise_var_device``, the filter of ``PathTrace.denoise_var()``): ``moments`` is a ``[W, H, 8]`` tensor of
sample moments (n, mean3, M2 3, bad: ``PathTrace.moments_to_torch()``, or the ranks' records merged).

    hdr_o, mom_o = temporal_accumulate(hdr, aov, moments, hist_hdr, hist_aov, hist_moments, cam, cam_prev,
                                       max_history=32.0, sigma_n=0.3, sigma_z=0.1, ctx=None)

is the temporal accumulation of ``PathTrace.temporal_accumulate()`` (``tirt_temporal_device``): the history -- an earlier result with the ``aov`` of
that call, or a plain film with its records -- seen from ``cam_prev`` is reprojected into the view of ``cam`` and merged with the current film and
its moments.  ``cam`` / ``cam_prev`` are ``Camera`` objects as they stood at the two views, or the tuples ``(view, view_inv, eye, fx, fy, cx, cy)``
a ``Camera`` pushes.  The guide record of the result is ``aov``: ``denoise_var(hdr_o, aov, mom_o)`` filters it.  ``motion=`` takes a ``[W, H, 8]``
tensor of motion records (``PathTrace.motion_to_torch()``) for geometry that moved between the two views (``tirt_motion_temporal_device``).
"""
from . import _native

_CONTEXTS = {}          # device index -> the context denoise() made for tensors of that device


def _torch():
    try:
        import torch
    except ImportError as exc:
        raise ImportError("ti_raytrace_amd.denoise needs PyTorch (ROCm build); PathTrace.denoise() and the C-ABI tirt_denoise / "
                          "tirt_denoise_device (include/tirt.h) work without it") from exc
    return torch


def _check(fn, tensors):
    """the tensors' types, shapes and device; returns (torch, device, W, H)"""
    torch = _torch()
    for name, t, words in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor, got %s" % (fn, name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s" % (fn, name, t.dtype))
        if t.device.type != "cuda":
            raise TypeError("%s: %s must be on the GPU, got a %s tensor" % (fn, name, t.device.type))
        if t.dim() != 3 or t.shape[2] != words or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("%s: %s must be [W, H, %d], got shape %s" % (fn, name, words, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (fn, name))
    hdr = tensors[0][1]
    for name, t, _ in tensors[1:]:
        if t.device != hdr.device or t.shape[:2] != hdr.shape[:2]:
            raise ValueError("%s: hdr is %s on %s, %s %s on %s" % (fn, tuple(hdr.shape), hdr.device, name, tuple(t.shape), t.device))
    return torch, hdr.device, int(hdr.shape[0]), int(hdr.shape[1])


def _context(fn, ctx, dev):
    if ctx is None:
        ctx = _CONTEXTS.get(dev.index)
        if ctx is None:
            ctx = _CONTEXTS[dev.index] = _native.Context(dev.index)
    elif ctx.device_id != dev.index:
        raise ValueError("%s: the tensors are on %s, the context on device %d" % (fn, dev, ctx.device_id))
    return ctx


def _run(fn, tensors, params, ctx):
    """tensors: hdr and aov for tirt_denoise_device; hdr, aov and moments for tirt_denoise_var_device"""
    torch, dev, W, H = _check(fn, tensors)
    ctx = _context(fn, ctx, dev)
    out = torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    run = ctx.denoise_var_device if len(tensors) == 3 else ctx.denoise_device
    run(*[t.data_ptr() for _, t, _ in tensors], out.data_ptr(), W, H, *params, stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def denoise(hdr, aov, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1, ctx=None):
    return _run("denoise", (("hdr", hdr, 3), ("aov", aov, _native.AOV_WORDS)), (levels, sigma_c, sigma_n, sigma_z), ctx)


def denoise_var(hdr, aov, moments, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1, ctx=None):
    return _run("denoise_var", (("hdr", hdr, 3), ("aov", aov, _native.AOV_WORDS), ("moments", moments, _native.MOM_WORDS)),
                (levels, sigma_c, sigma_n, sigma_z), ctx)


def temporal_accumulate(hdr, aov, moments, hist_hdr, hist_aov, hist_moments, cam, cam_prev, max_history=32.0, sigma_n=0.3, sigma_z=0.1, ctx=None,
                        motion=None):
    fn = "temporal_accumulate"
    tensors = (("hdr", hdr, 3), ("aov", aov, _native.AOV_WORDS), ("moments", moments, _native.MOM_WORDS),
               ("hist_hdr", hist_hdr, 3), ("hist_aov", hist_aov, _native.AOV_WORDS), ("hist_moments", hist_moments, _native.MOM_WORDS))
    torch, dev, W, H = _check(fn, tensors + ((("motion", motion, _native.MOTION_WORDS),) if motion is not None else ()))
    ctx = _context(fn, ctx, dev)
    hdr_o = torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    mom_o = torch.empty((W, H, _native.MOM_WORDS), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if motion is not None:
        ctx.motion_temporal_device(*[t.data_ptr() for _, t, _ in tensors], cam, cam_prev, hdr_o.data_ptr(), mom_o.data_ptr(), W, H, motion.data_ptr(),
                               max_history, sigma_n, sigma_z, stream=stream)
        return hdr_o, mom_o
    ctx.temporal_device(*[t.data_ptr() for _, t, _ in tensors], cam, cam_prev, hdr_o.data_ptr(), mom_o.data_ptr(), W, H,
                        max_history, sigma_n, sigma_z, stream=stream)
    return hdr_o, mom_o
