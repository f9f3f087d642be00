"""Primary-hit visualiser (mirror of the reference's ``integrator/Debug.py``).

``Debug.render()`` = one ``@ti.kernel render`` launch of the reference (:44-67): per pixel the camera ray of frame
``cam.frame`` (jittered iff the frame is not 0), its closest hit, and ``hdr[i, j]`` OVERWRITTEN with one view of that hit --
the material colour (``"albedo"``, the live line :65) or a normal mapped to [0, 1] (``"fnormal"`` / ``"normal"`` /
``"gnormal"``, the commented lines :62-64); (0, 0, 0) where the ray misses.  No bounces, no running mean.  On the device it is
three launches: camera directions -> the closest-hit traversal kernel -> the view (csrc/tirt_debug.hip).
"""
from . import _native
from .PT_RGB import default_tile_size
from .Scene import DeviceField

MODES = {"albedo": _native.DEBUG_ALBEDO, "fnormal": _native.DEBUG_FNORMAL, "normal": _native.DEBUG_NORMAL, "gnormal": _native.DEBUG_GNORMAL}


class Debug:
    def __init__(self, imgSizeX, imgSizeY, cam, scene, stack_size,
                 mode="albedo", seed=1, tile_rank=0, tile_count=1, tile_size=None, flags=0):
        if mode not in MODES:
            raise ValueError("Debug: mode %r is not one of %s" % (mode, ", ".join(sorted(MODES))))
        self.imgSizeX = imgSizeX
        self.imgSizeY = imgSizeY
        self.cam = cam
        self.scene = scene
        self.stack_size = stack_size
        # extensions: which view, the counter-based RNG seed of the jitter (the same rays as PT_RGB's at that seed) and
        # the pixel-tile shard this context renders (multi-GPU), as in PT_RGB.PathTrace
        self.mode = mode
        self.seed = seed
        self.tile_rank, self.tile_count, self.tile_size = tile_rank, tile_count, tile_size or default_tile_size(imgSizeY)
        self.flags = flags
        self.hdr = DeviceField("hdr", scene, lambda: self._download(True))
        self.rgb_film = DeviceField("rgb_film", scene, lambda: self._download(False))

    def _download(self, hdr):
        h, r = self.scene.ctx.film_download(self.imgSizeX, self.imgSizeY, want_hdr=hdr, want_rgb=not hdr)
        return h if hdr else r

    def setup_data_cpu(self):
        pass                                  # field placement has no host-side equivalent

    def setup_data_gpu(self):
        self.scene.ctx.film_create(self.imgSizeX, self.imgSizeY, self.tile_rank, self.tile_count, self.tile_size)
        self.cam.attach(self.scene.ctx)

    def render(self):
        """The view at ``cam.frame`` (the caller advances it with ``cam.update_frame()``); asynchronous."""
        self.scene.ctx.debug_render(self.cam.frame, self.seed, MODES[self.mode], self.stack_size, self.flags)
