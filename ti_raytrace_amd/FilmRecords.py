"""What the path tracers share beside the film (no reference counterpart): the feature buffers, the denoised film and, for PT_RGB alone, the
sample moments and the temporal accumulation -- as fields, numpy arrays and torch tensors.  ``PT_RGB.PathTrace`` and ``PT_Spec.PathTrace`` inherit
``FilmRecords``; ``PT_RGB.PathTrace`` also ``SampleMoments`` and ``TemporalAccumulation``.  A class that inherits them has ``scene``, ``imgSizeX``, ``imgSizeY`` and the flags ``aov`` / ``moments``.
"""
import numpy as np

from . import _native
from .Scene import DeviceField


class FilmRecords:
    def _to_torch(self, words, export, what):
        """a new float32 tensor [W, H, words] on the context's device, filled device to device by the context's method `export`; `what` = (this method, what works without torch)"""
        try:
            import torch
        except ImportError as exc:
            raise ImportError("%s needs PyTorch (ROCm build); %s work without it" % what) from exc
        ctx = self.scene.ctx
        out = torch.empty((self.imgSizeX, self.imgSizeY, words), dtype=torch.float32, device=torch.device("cuda", ctx.device_id))
        getattr(ctx, export)(out.data_ptr())
        return out

    def _aov_fields(self):
        """the feature buffers as fields (aov=True): first-hit albedo and shading normal [W, H, 3], depth and coverage [W, H], means over the
        film's own camera rays (include/tirt.h, tirt_aov_enable).  Each to_numpy() is one download of the whole record."""
        words = {"albedo": slice(_native.AOV_ALBEDO, _native.AOV_ALBEDO + 3), "normal": slice(_native.AOV_NORMAL, _native.AOV_NORMAL + 3),
                 "depth": _native.AOV_DEPTH, "alpha": _native.AOV_ALPHA}
        for name, w in words.items():
            setattr(self, name, DeviceField(name, self.scene, lambda w=w: np.ascontiguousarray(self.aov_to_numpy()[:, :, w])))

    def aov_to_numpy(self):
        """[W, H, 8] float32: albedo3, normal3, depth, alpha"""
        return self.scene.ctx.aov_download(self.imgSizeX, self.imgSizeY)

    def aov_to_torch(self):
        """The same as a float32 tensor on the context's device, filled device to device (tirt_aov_export_device)."""
        return self._to_torch(_native.AOV_WORDS, "aov_export_device", ("aov_to_torch", "aov_to_numpy and the C-ABI tirt_aov_download"))

    def denoise(self, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1):
        """Filter hdr with the edge-avoiding a-trous wavelet, guided by the feature buffers (aov=True; include/tirt.h, tirt_denoise), into
        `denoised`.  hdr, rgb_film and the feature buffers are only read.  Asynchronous."""
        self.scene.ctx.denoise(levels, sigma_c, sigma_n, sigma_z)

    def _denoised_download(self):
        return self.scene.ctx.denoise_download(self.imgSizeX, self.imgSizeY)

    def denoised_to_torch(self):
        """`denoised` as a float32 tensor [W, H, 3] on the context's device, filled device to device (tirt_denoise_export_device)."""
        return self._to_torch(3, "denoise_export_device", ("denoised_to_torch", "denoised.to_numpy() and the C-ABI tirt_denoise_download"))

    def _download(self, hdr):
        h, r = self.scene.ctx.film_download(self.imgSizeX, self.imgSizeY, want_hdr=hdr, want_rgb=not hdr)
        return h if hdr else r


class SampleMoments:
    """PT_RGB only: the other integrators' per-frame samples are not RGB radiance per pixel-sample (include/tirt.h).  Beside FilmRecords."""

    def _moment_fields(self):
        """the sample moments as fields (moments=True; include/tirt.h, tirt_moments_enable): samples [W, H] (n), mean [W, H, 3], variance [W, H, 3]
        (the sample variance M2 / (n - 1), 0 where n < 2), bad [W, H] (samples skipped because they were not finite) and sample_count [W, H] (samples + bad).  Each to_numpy() is one
        download of the whole record."""
        def variance():
            m = self.moments_to_numpy()
            n = m[:, :, _native.MOM_N:_native.MOM_N + 1]
            ok = n >= 2
            return np.where(ok, m[:, :, _native.MOM_M2:_native.MOM_M2 + 3] / np.where(ok, n - np.float32(1.0), np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        self.samples = DeviceField("samples", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_N]))
        self.mean = DeviceField("mean", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_MEAN:_native.MOM_MEAN + 3]))
        self.variance = DeviceField("variance", self.scene, variance)
        self.bad = DeviceField("bad", self.scene, lambda: np.ascontiguousarray(self.moments_to_numpy()[:, :, _native.MOM_BAD]))
        # how many frames a pixel was rendered at: samples + bad (after render_adaptive it differs from pixel to pixel)
        def sample_count():
            m = self.moments_to_numpy()
            return np.ascontiguousarray(m[:, :, _native.MOM_N] + m[:, :, _native.MOM_BAD])
        self.sample_count = DeviceField("sample_count", self.scene, sample_count)

    def moments_to_numpy(self):
        """[W, H, 8] float32: n, mean3, M2 3, bad"""
        return self.scene.ctx.moments_download(self.imgSizeX, self.imgSizeY)

    def moments_to_torch(self):
        """The same as a float32 tensor on the context's device, filled device to device (tirt_moments_export_device)."""
        return self._to_torch(_native.MOM_WORDS, "moments_export_device",
                              ("moments_to_torch", "moments_to_numpy and the C-ABI tirt_moments_download"))

    def converged(self, threshold):
        """(measured, noisy, bad): this context's pixels with two samples or more, those of them whose standard error still exceeds `threshold` x
        their mean level, and the pixels that skipped a sample that was not finite (include/tirt.h, tirt_moments_converged)."""
        return self.scene.ctx.moments_converged(threshold)

    def denoise_var(self, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1):
        """The variance-guided mode of denoise() (include/tirt.h, tirt_denoise_var): the colour term is scaled by each pixel's variance of the
        mean, from the sample moments, which are filtered along.  Needs aov=True and moments=True; writes `denoised` as denoise() does.
        A method of its own, as the C-ABI has entry points of its own: denoise() and its parameters stay as they are.  Asynchronous."""
        if not (self.aov and self.moments):
            raise ValueError("denoise_var needs the feature buffers and the sample moments: PT_RGB.PathTrace(..., aov=True, moments=True)")
        self.scene.ctx.denoise_var(levels, sigma_c, sigma_n, sigma_z)


class TemporalAccumulation:
    """PT_RGB only (temporal=True, which needs aov=True and moments=True): the film and the moments of the views rendered so far, carried across camera
    moves (include/tirt.h, tirt_temporal_enable).  The loop of an interactive viewer:

        move the camera;  scene.ctx.film_clear(), cam.frame = 0;  integrator.seed = s + view;  render_frames(k)
        temporal_accumulate();  denoise_temporal();  denoised_to_torch()

    The seed must change per view: a cleared film restarts at frame 0, and the random numbers depend on (seed, pixel, frame) alone."""

    def _temporal_fields(self):
        """accumulated [W, H, 3]: the accumulated film; accumulated_samples [W, H]: the samples behind each of its pixels (n of its moment record)"""
        ctx = lambda: self.scene.ctx
        self.accumulated = DeviceField("accumulated", self.scene, lambda: ctx().temporal_download(self.imgSizeX, self.imgSizeY, want_mom=False)[0])
        self.accumulated_samples = DeviceField("accumulated_samples", self.scene, lambda: np.ascontiguousarray(
            ctx().temporal_download(self.imgSizeX, self.imgSizeY, want_hdr=False)[1][:, :, _native.MOM_N]))

    def _need_temporal(self, what):
        if not self.temporal:
            raise ValueError("%s needs the temporal history: PT_RGB.PathTrace(..., aov=True, moments=True, temporal=True)" % what)

    def temporal_accumulate(self, max_history=32.0, sigma_n=0.3, sigma_z=0.1):
        """Reproject the history into the camera as it stands and merge it with hdr and the sample moments (tirt_temporal_accumulate); the result
        is the new history.  hdr, rgb_film and the records are only read.  Asynchronous."""
        self._need_temporal("temporal_accumulate")
        self.scene.ctx.temporal_accumulate(max_history, sigma_n, sigma_z)

    def temporal_reset(self):
        """Empty the history (a scene upload does so too, and a geometry update unless motion=True; film_clear does not)."""
        self._need_temporal("temporal_reset")
        self.scene.ctx.temporal_reset()

    def denoise_temporal(self, levels=5, sigma_c=3.0, sigma_n=0.3, sigma_z=0.1):
        """denoise_var()'s filter over the accumulated film and moments, guided by the last accumulated view's feature buffers, into `denoised`
        (tirt_temporal_denoise_var).  Asynchronous."""
        self._need_temporal("denoise_temporal")
        self.scene.ctx.temporal_denoise_var(levels, sigma_c, sigma_n, sigma_z)

    def temporal_to_numpy(self):
        """(hdr [W, H, 3], moments [W, H, 8]) float32 of the accumulated film"""
        self._need_temporal("temporal_to_numpy")
        return self.scene.ctx.temporal_download(self.imgSizeX, self.imgSizeY)

    def temporal_to_torch(self):
        """The same as float32 tensors on the context's device, filled device to device (tirt_temporal_export_device)."""
        self._need_temporal("temporal_to_torch")
        try:
            import torch
        except ImportError as exc:
            raise ImportError("temporal_to_torch needs PyTorch (ROCm build); temporal_to_numpy and the C-ABI tirt_temporal_download work without it") from exc
        dev = torch.device("cuda", self.scene.ctx.device_id)
        hdr = torch.empty((self.imgSizeX, self.imgSizeY, 3), dtype=torch.float32, device=dev)
        mom = torch.empty((self.imgSizeX, self.imgSizeY, _native.MOM_WORDS), dtype=torch.float32, device=dev)
        self.scene.ctx.temporal_export_device(hdr.data_ptr(), mom.data_ptr())
        return hdr, mom

    # ---- motion records (motion=True): the accumulation across Scene.update_vertices (include/tirt.h, tirt_motion_enable).  The viewer's loop with an
    # animated mesh:  scene.update_vertices(...) (it rebuilds);  scene.ctx.film_clear(), cam.frame = 0;  integrator.seed = s + step;  render_frames(k);
    # temporal_accumulate();  denoise_temporal() ----
    def _motion_fields(self):
        """motion [W, H, 8]: per pixel where its surface point and shading normal were at the last accumulated view, relative to now (D3, 1, dN3, 0)"""
        self.motion = DeviceField("motion", self.scene, self.motion_to_numpy)

    def _need_motion(self, what):
        if not self.motion_records:
            raise ValueError("%s needs the motion records: PT_RGB.PathTrace(..., aov=True, moments=True, temporal=True, motion=True)" % what)

    def motion_to_numpy(self):
        """[W, H, 8] float32: the motion records of the last temporal_accumulate()"""
        self._need_motion("motion_to_numpy")
        return self.scene.ctx.motion_download(self.imgSizeX, self.imgSizeY)

    def motion_to_torch(self):
        """The same as a float32 tensor on the context's device, filled device to device (tirt_motion_export_device)."""
        self._need_motion("motion_to_torch")
        return self._to_torch(_native.MOTION_WORDS, "motion_export_device", ("motion_to_torch", "motion_to_numpy and the C-ABI tirt_motion_download"))
