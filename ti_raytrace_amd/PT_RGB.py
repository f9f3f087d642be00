"""Unidirectional path tracer (mirror of the reference's ``integrator/PT_RGB.py``).

``PathTrace.render()`` = one ``@ti.kernel render`` launch of the reference (one sample per
pixel at frame ``cam.frame``, running-mean film, :44-136).  On the device it is not a
per-pixel megakernel but a wavefront pipeline (generate -> trace -> shade -> shadow-trace ->
film) over struct-of-arrays path queues in HBM -- see DESIGN.md.
"""
from .FilmRecords import FilmRecords, SampleMoments, TemporalAccumulation
from .Scene import DeviceField
from ._native import SF_LIGHT_POWER

MAX_DEPTH = 15           # integrator/PT_RGB.py:21


def default_tile_size(H):
    """Pixels per tile of the multi-GPU film split (tiles go round-robin over the ranks).  8 whole columns when that is a handy size:
    the device library then walks a tile in 8 x 8 pixel blocks (tirt_internal.h, local_to_pixel), which makes the 64 camera rays
    of a wave a compact bundle; otherwise 4096 linear pixels."""
    return 8 * H if (H % 8 == 0 and 4096 <= 8 * H <= 16384) else 4096


class PathTrace(FilmRecords, SampleMoments, TemporalAccumulation):
    def __init__(self, imgSizeX, imgSizeY, cam, scene, stack_size,
                 seed=1, tile_rank=0, tile_count=1, tile_size=None, flags=0, env_sampling=False, env_share=0.5,
                 light_sampling="uniform", light_uniform_share=0.0, motion=False, temporal=False, moments=False, aov=False):
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
        # extension: the film and the moments accumulated across camera moves
        if temporal and not (aov and moments):
            raise ValueError("temporal=True needs the feature buffers and the sample moments: PT_RGB.PathTrace(..., aov=True, moments=True, temporal=True)")
        self.temporal = temporal
        self._temporal_fields()
        # extension: motion records, so that the accumulation survives Scene.update_vertices
        if motion and not temporal:
            raise ValueError("motion=True needs the temporal history: PT_RGB.PathTrace(..., aov=True, moments=True, temporal=True, motion=True)")
        self.motion_records = motion
        self._motion_fields()
        # extension: light samples aimed at the environment by its brightness, weighted against BSDF sampling (include/tirt.h, "Importance sampling of the
        # environment"); env_share = the part of the light samples the environment gets in a scene that has emitters too
        if not 0.0 < float(env_share) < 1.0:
            raise ValueError("PT_RGB.PathTrace: env_share must lie in (0, 1), got %r" % (env_share,))
        self._env_sampling, self._env_share = bool(env_sampling), float(env_share)
        # extension: emitters chosen by power instead of one entry of the light list in light_count (include/tirt.h, "Choosing emitters by power");
        # light_uniform_share = the part of the emitter samples that still picks uniformly
        self._light_sampling, self._light_uniform_share = self._check_light_sampling(light_sampling, light_uniform_share)
        # extension: the film after denoise(), a buffer of its own beside hdr
        self.denoised = DeviceField("denoised", scene, self._denoised_download)

    def setup_data_cpu(self):
        pass                                  # field placement has no host-side equivalent

    def setup_data_gpu(self):
        self.scene.ctx.film_create(self.imgSizeX, self.imgSizeY, self.tile_rank, self.tile_count, self.tile_size)
        self.cam.attach(self.scene.ctx)
        self.scene.ctx.env_sampling(self._env_sampling, self._env_share)
        self.scene.ctx.light_sampling(self._light_sampling == "power", self._light_uniform_share)
        if self.aov:
            self.scene.ctx.aov_enable(True)
        if self.moments:
            self.scene.ctx.moments_enable(True)
        if self.temporal:
            self.scene.ctx.temporal_enable(True)
        if self.motion_records:
            self.scene.ctx.motion_enable(True)

    @property
    def env_sampling(self):
        """(switch, share) as given; ``env_sampling_active`` says whether the device samples (a lit environment with a table: bit 1024 of the feature word)."""
        return self._env_sampling, self._env_share

    @property
    def env_sampling_active(self):
        return bool(self.scene.ctx.shade_features()[0] & 1024)

    def set_env_sampling(self, on, share=None):
        """Switch the environment's light sample on or off between renders (the film is not cleared)."""
        share = self._env_share if share is None else float(share)
        if not 0.0 < share < 1.0:
            raise ValueError("PT_RGB.PathTrace: env_share must lie in (0, 1), got %r" % (share,))
        self._env_sampling, self._env_share = bool(on), share
        self.scene.ctx.env_sampling(self._env_sampling, self._env_share)

    @staticmethod
    def _check_light_sampling(mode, uniform_share):
        if mode not in ("uniform", "power"):
            raise ValueError("PT_RGB.PathTrace: light_sampling is \"uniform\" or \"power\", got %r" % (mode,))
        if not 0.0 <= float(uniform_share) < 1.0:
            raise ValueError("PT_RGB.PathTrace: light_uniform_share must lie in [0, 1), got %r" % (uniform_share,))
        return mode, float(uniform_share)

    @property
    def light_sampling(self):
        """(mode, uniform share) as given; ``light_sampling_active`` says whether the device chooses by power (bit 4096 of the feature word: mode "power", emitters
        that are all triangles or spheres, a table with a weight in it)."""
        return self._light_sampling, self._light_uniform_share

    @property
    def light_sampling_active(self):
        return bool(self.scene.ctx.shade_features()[0] & SF_LIGHT_POWER)

    def set_light_sampling(self, mode, uniform_share=None):
        """Choose emitters uniformly or by power between renders (the film is not cleared)."""
        self._light_sampling, self._light_uniform_share = self._check_light_sampling(mode, self._light_uniform_share if uniform_share is None else uniform_share)
        self.scene.ctx.light_sampling(self._light_sampling == "power", self._light_uniform_share)

    def render(self):
        """One frame at ``cam.frame`` (the caller advances it with ``cam.update_frame()``)."""
        self.scene.ctx.pt_rgb_render(self.cam.frame, 1, self.seed, MAX_DEPTH, self.stack_size, self.flags)

    def render_frames(self, count):
        """Extension: ``count`` consecutive frames starting at ``cam.frame`` in one call
        (identical film to calling render()/update_frame() ``count`` times)."""
        self.scene.ctx.pt_rgb_render(self.cam.frame, count, self.seed, MAX_DEPTH, self.stack_size, self.flags)

    def pixel_set(self, pixels):
        """Extension: restrict render() / render_frames() to the pixels of `pixels` -- linear indices i * imgSizeY + j of this context's tiles, strictly
        ascending in the context's local order (include/tirt.h, tirt_pixel_set_upload; a single tile of any size that is not whole 8-column groups walks
        them in ascending index) -- or, with None, render every pixel again.  Pixels outside the set are neither read nor written."""
        if pixels is None:
            self.scene.ctx.pixel_set_clear()
        else:
            self.scene.ctx.pixel_set_upload(pixels)

    def render_adaptive(self, threshold, max_samples, min_samples=4, pass_frames=4):
        """Extension (moments=True): passes of `pass_frames` frames starting at ``cam.frame`` -- the caller has rendered exactly the frames before it, or
        none --, each pass only on the pixels whose standard error still exceeds `threshold` x their mean level (converged()'s rule) or that have fewer
        than `min_samples` samples, until no pixel is left or all have `max_samples` (include/tirt.h, tirt_pt_rgb_render_adaptive).  Every pixel holds,
        bit for bit, the film of a dense render of its own sample_count frames.  Returns {"passes", "pixel_samples", "pixels_at_max", "frames"};
        ``cam.frame`` is not advanced.  A pixel is stopped on its own variance estimate, which is biased towards stopping early where few samples
        happen to agree: min_samples is the only guard."""
        if not self.moments:
            raise ValueError("render_adaptive needs the sample moments: PT_RGB.PathTrace(..., moments=True)")
        return self.scene.ctx.pt_rgb_render_adaptive(self.cam.frame, self.seed, threshold, max_samples, min_samples, pass_frames,
                                                     MAX_DEPTH, self.stack_size, self.flags)
