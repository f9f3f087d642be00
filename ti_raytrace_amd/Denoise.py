"""The edge-avoiding a-trous denoiser on PyTorch device tensors (no reference counterpart; include/tirt.h ``tirt_denoise_device``,
csrc/tirt_denoise.hip).

    out = denoise(hdr, aov, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1, ctx=None)      # a new [W, H, 3] float32 tensor

``hdr`` is a contiguous float32 tensor ``[W, H, 3]`` and ``aov`` one ``[W, H, 8]`` (albedo3, normal3, depth, alpha: what
``PathTrace.aov_to_torch()`` returns, or the sum of the ranks' records of a tiled job), both on one GPU.  ``ctx`` is a ``_native.Context`` of
that device -- ``scene.ctx`` when there is a scene; without one a context per device is made on first use and kept: the filter needs no
scene and no film.  The work is queued on ``torch.cuda.current_stream(device)``: nothing waits for it on the host.  The same filter, bit
for bit, as ``PathTrace.denoise()``.
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


def denoise(hdr, aov, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1, ctx=None):
    torch = _torch()
    for name, t, words in (("hdr", hdr, 3), ("aov", aov, _native.AOV_WORDS)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("denoise: %s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError("denoise: %s must be float32, got %s" % (name, t.dtype))
        if t.device.type != "cuda":
            raise TypeError("denoise: %s must be on the GPU, got a %s tensor" % (name, t.device.type))
        if t.dim() != 3 or t.shape[2] != words or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("denoise: %s must be [W, H, %d], got shape %s" % (name, words, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("denoise: %s must be contiguous" % name)
    if aov.device != hdr.device or aov.shape[:2] != hdr.shape[:2]:
        raise ValueError("denoise: hdr is %s on %s, aov %s on %s" % (tuple(hdr.shape), hdr.device, tuple(aov.shape), aov.device))
    dev = hdr.device
    if ctx is None:
        ctx = _CONTEXTS.get(dev.index)
        if ctx is None:
            ctx = _CONTEXTS[dev.index] = _native.Context(dev.index)
    elif ctx.device_id != dev.index:
        raise ValueError("denoise: the tensors are on %s, the context on device %d" % (dev, ctx.device_id))
    W, H = int(hdr.shape[0]), int(hdr.shape[1])
    out = torch.empty((W, H, 3), dtype=torch.float32, device=dev)
    ctx.denoise_device(hdr.data_ptr(), aov.data_ptr(), out.data_ptr(), W, H, levels, sigma_c, sigma_n, sigma_z,
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    return out
