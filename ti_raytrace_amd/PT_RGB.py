"""Unidirectional path tracer (mirror of the reference's ``integrator/PT_RGB.py``).

``PathTrace.render()`` = one ``@ti.kernel render`` launch of the reference (one sample per
pixel at frame ``cam.frame``, running-mean film, :44-136).  On the device it is not a
per-pixel megakernel but a wavefront pipeline (generate -> trace -> shade -> shadow-trace ->
film) over struct-of-arrays path queues in HBM -- see DESIGN.md.
"""
import numpy as np

from .Scene import DeviceField

MAX_DEPTH = 15           # integrator/PT_RGB.py:21


def default_tile_size(H):
    """Pixels per tile of the multi-GPU film split (tiles go round-robin over the ranks).  8 whole columns when that is a handy size:
    the device library then walks a tile in 8 x 8 pixel blocks (tirt_internal.h, local_to_pixel), which makes the 64 camera rays
    of a wave a compact bundle; otherwise 4096 linear pixels."""
    return 8 * H if (H % 8 == 0 and 4096 <= 8 * H <= 16384) else 4096


class PathTrace:
    def __init__(self, imgSizeX, imgSizeY, cam, scene, stack_size,
                 seed=1, tile_rank=0, tile_count=1, tile_size=None, flags=0, moments=False, aov=False):
        self.imgSizeX = imgSizeX
        self.imgSizeY = imgSizeY
        self.cam = cam
        self.scene = scene
        self.stack_size = stack_size
        # extensions: counter-based RNG seed (the reference's ti.random() is unseeded) and
        # the pixel-tile shard this context renders (multi-GPU)
        self.seed = seed
        self.tile_rank, self.tile_count, self.tile_size = tile_rank, tile_count, tile_size or default_tile_size(imgSizeY)
        self.flags = flags
        self.hdr = DeviceField("hdr", scene, lambda: self._download(True))
        self.rgb_film = DeviceField("rgb_film", scene, lambda: self._download(False))
        # extension: feature buffers of the film's own camera rays, for a denoiser or a compositor
        self.aov = aov
        self._aov_fields()
        # extension: per-pixel sample moments (count, mean, sum of squared deviations) of the pixel-samples the film averages
        self.moments = moments
        self._moment_fields()
        # extension: the film after denoise(), a buffer of its own beside hdr
        self.denoised = DeviceField("denoised", scene, self._denoised_download)

    def _aov_fields(self):
        """the feature buffers as fields (aov=True): first-hit albedo and shading normal [W, H, 3], depth and coverage [W, H], means over the
        film's own camera rays (include/tirt.h, tirt_aov_enable).  Each to_numpy() is one download of the whole record."""
        from . import _native
        words = {"albedo": slice(_native.AOV_ALBEDO, _native.AOV_ALBEDO + 3), "normal": slice(_native.AOV_NORMAL, _native.AOV_NORMAL + 3),
                 "depth": _native.AOV_DEPTH, "alpha": _native.AOV_ALPHA}
        for name, w in words.items():
            setattr(self, name, DeviceField(name, self.scene, lambda w=w: np.ascontiguousarray(self.aov_to_numpy()[:, :, w])))

    def aov_to_numpy(self):
        """[W, H, 8] float32: albedo3, normal3, depth, alpha"""
        return self.scene.ctx.aov_download(self.imgSizeX, self.imgSizeY)

    def aov_to_torch(self):
        """The same as a float32 tensor on the context's device, filled device to device (tirt_aov_export_device)."""
        try:
            import torch
        except ImportError as exc:
            raise ImportError("aov_to_torch needs PyTorch (ROCm build); aov_to_numpy and the C-ABI tirt_aov_download work without it") from exc
        from . import _native
        ctx = self.scene.ctx
        out = torch.empty((self.imgSizeX, self.imgSizeY, _native.AOV_WORDS), dtype=torch.float32, device=torch.device("cuda", ctx.device_id))
        ctx.aov_export_device(out.data_ptr())
        return out

    def _moment_fields(self):
        """the sample moments as fields (moments=True; include/tirt.h, tirt_moments_enable): samples [W, H] (n), mean [W, H, 3], variance [W, H, 3]
        (the sample variance M2 / (n - 1), 0 where n < 2) and bad [W, H] (samples skipped because they were not finite).  Each to_numpy() is one
        download of the whole record."""
        from . import _native

        def variance():
            m = self.moments_to_numpy()
            n = m[:, :, _native.MOM_N:_native.MOM_N + 1]
            ok = n >= 2
            return np.where(ok, m[:, :, _native.MOM_M2:_native.MOM_M2 + 3] / np.where(ok, n - np.float32(1.0), np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        self.samples = DeviceField("samples", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_N]))
        self.mean = DeviceField("mean", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_MEAN:_native.MOM_MEAN + 3]))
        self.variance = DeviceField("variance", self.scene, variance)
        self.bad = DeviceField("bad", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_BAD]))

    def moments_to_numpy(self):
        """[W, H, 8] float32: n, mean3, M2 3, bad"""
        return self.scene.ctx.moments_download(self.imgSizeX, self.imgSizeY)

    def moments_to_torch(self):
        """The same as a float32 tensor on the context's device, filled device to device (tirt_moments_export_device)."""
        try:
            import torch
        except ImportError as exc:
            raise ImportError("moments_to_torch needs PyTorch (ROCm build); moments_to_numpy and the C-ABI tirt_moments_download work without it") from exc
        from . import _native
        ctx = self.scene.ctx
        out = torch.empty((self.imgSizeX, self.imgSizeY, _native.MOM_WORDS), dtype=torch.float32, device=torch.device("cuda", ctx.device_id))
        ctx.moments_export_device(out.data_ptr())
        return out

    def converged(self, threshold):
        """(measured, noisy, bad): this context's pixels with two samples or more, those of them whose standard error still exceeds `threshold` x
        their mean level, and the pixels that skipped a sample that was not finite (include/tirt.h, tirt_moments_converged)."""
        return self.scene.ctx.moments_converged(threshold)

    def denoise(self, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1):
        """Filter hdr with the edge-avoiding a-trous wavelet, guided by the feature buffers (aov=True; include/tirt.h, tirt_denoise), into
        `denoised`.  hdr, rgb_film and the feature buffers are only read.  Asynchronous."""
        self.scene.ctx.denoise(levels, sigma_c, sigma_n, sigma_z)

    def denoise_var(self, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1):
        """The variance-guided mode of denoise() (include/tirt.h, tirt_denoise_var): the colour term is scaled by each pixel's variance of the
        mean, from the sample moments, which are filtered along.  Needs aov=True and moments=True; writes `denoised` as denoise() does.
        A method of its own, as the C-ABI has entry points of its own: denoise() and its parameters stay as they are.  Asynchronous."""
        if not (self.aov and self.moments):
            raise ValueError("denoise_var needs the feature buffers and the sample moments: PT_RGB.PathTrace(..., aov=True, moments=True)")
        self.scene.ctx.denoise_var(levels, sigma_c, sigma_n, sigma_z)

    def _denoised_download(self):
        return self.scene.ctx.denoise_download(self.imgSizeX, self.imgSizeY)

    def denoised_to_torch(self):
        """`denoised` as a float32 tensor [W, H, 3] on the context's device, filled device to device (tirt_denoise_export_device)."""
        try:
            import torch
        except ImportError as exc:
            raise ImportError("denoised_to_torch needs PyTorch (ROCm build); denoised.to_numpy() and the C-ABI tirt_denoise_download work without it") from exc
        ctx = self.scene.ctx
        out = torch.empty((self.imgSizeX, self.imgSizeY, 3), dtype=torch.float32, device=torch.device("cuda", ctx.device_id))
        ctx.denoise_export_device(out.data_ptr())
        return out

    def _download(self, hdr):
        h, r = self.scene.ctx.film_download(self.imgSizeX, self.imgSizeY, want_hdr=hdr, want_rgb=not hdr)
        return h if hdr else r

    def setup_data_cpu(self):
        pass                                  # field placement has no host-side equivalent

    def setup_data_gpu(self):
        self.scene.ctx.film_create(self.imgSizeX, self.imgSizeY, self.tile_rank, self.tile_count, self.tile_size)
        self.cam.attach(self.scene.ctx)
        if self.aov:
            self.scene.ctx.aov_enable(True)
        if self.moments:
            self.scene.ctx.moments_enable(True)

    def render(self):
        """One frame at ``cam.frame`` (the caller advances it with ``cam.update_frame()``)."""
        self.scene.ctx.pt_rgb_render(self.cam.frame, 1, self.seed, MAX_DEPTH, self.stack_size, self.flags)

    def render_frames(self, count):
        """Extension: ``count`` consecutive frames starting at ``cam.frame`` in one call
        (identical film to calling render()/update_frame() ``count`` times)."""
        self.scene.ctx.pt_rgb_render(self.cam.frame, count, self.seed, MAX_DEPTH, self.stack_size, self.flags)
