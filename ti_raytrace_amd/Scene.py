"""Scene container (mirror of the host half of the reference's ``Scene.py``).

Host: OBJ/MTL ingest (``add_obj`` :59-141), analytic shapes (``add_shape`` :188-205), env
(``add_env`` :183-185), struct packing (``setup_data_cpu`` :223-296), uploads + LBVH build
(``setup_data_gpu`` :299-310), ``total_area`` (:747-750), ``process_normal`` (:754-798).
``update_vertices`` (extension): moves triangles of a scene that is already on the device and rebuilds.
Device: everything the reference declares as ``@ti.func`` on this class (``closet_hit``,
``closet_hit_shadow``, ``intersect_*``, ``sample_li`` ...) is HIP code in ``csrc/`` reached
through the C-ABI (``include/tirt.h``); there is no CPU fallback.

Ingest is vectorised numpy instead of the reference's per-vertex Python loops, but the
numbers it produces (primitive order, f32 rounding points, face normals, AABB) follow the
reference; ``tests/test_oracle_golden.py`` pins that against the reference's nodelist.txt.
"""
import os
import sys

import numpy as np

from . import SceneData as SCD
from . import LBvh
from . import Texture as TX
from . import ObjLoader
from . import _native

MAX_STACK_SIZE = 32          # Scene.py:19 (process_normal's point-query stack)
INF_VALUE = 1000000.0


class DeviceField:
    """Stand-in for a Taichi field living on the device: knows its owner and how to read
    itself back (``to_numpy()``), which is all the reference's host code does with fields."""

    def __init__(self, name, owner, reader):
        self.name = name
        self._owner = owner
        self._reader = reader

    @property
    def ctx(self):
        return self._owner.ctx

    def to_numpy(self):
        return self._reader()


class Scene:
    def __init__(self, device_id=None):
        self.maxboundarynp = np.full((1, 3), -INF_VALUE, dtype=np.float32)
        self.minboundarynp = np.full((1, 3), INF_VALUE, dtype=np.float32)

        self.light_cpu = []
        self.material_cpu = []
        self.shape_cpu = []
        self._vertex_chunks = []        # float64 [k, 9] blocks in primitive order
        self._prim_mat = []             # (first_prim, count, material index) per block
        self._shape_prims = []          # (prim index, shape index, material index)

        self.material_count = 0
        self.vertex_count = 0
        self.primitive_count = 0
        self.shape_count = 0
        self.light_count = 0

        self.env = TX.Texture()
        self.env_power = 0.0
        self.textures = []              # albedo textures (add_texture): (Texture, wrap flag), id = index + 1
        self._texture_ids = {}          # (absolute path, wrap flag, cut-out flag) -> id
        self.texture_cutout = []        # per texture: is its alpha channel a cut-out mask (add_texture(cutout=True)); beside `textures`, whose entries stay pairs
        self.bvh = None

        self._device_id = device_id
        self._ctx = None
        self._light_area = np.zeros(1, np.float32)
        self._area_called = False
        self._vertex_np_stale = False       # update_vertices moved the device's rows: vertex_np is read back when it is next asked for

        self.vertex = DeviceField("vertex", self, lambda: self.ctx.vertex_download(self.vertex_count))
        self.primitive = DeviceField("primitive", self, lambda: self.primitive_np.copy())
        self.shape = DeviceField("shape", self, lambda: self.shape_np.copy())
        self.material = DeviceField("material", self, lambda: self.material_np.copy())
        self.light = DeviceField("light", self, lambda: self.light_np.copy())
        self.light_area = DeviceField("light_area", self, lambda: self._light_area.copy())

    # -- device context ---------------------------------------------------------------------
    @property
    def ctx(self):
        if self._ctx is None:
            dev = self._device_id
            if dev is None:
                dev = int(os.environ.get("LOCAL_RANK", "0"))
            self._ctx = _native.Context(dev)
        return self._ctx

    @property
    def vertex_np(self):
        """the packed vertex rows as setup_data_cpu made them (before process_normal), following update_vertices"""
        if self._vertex_np_stale:
            self._vertex_np = self.ctx.vertex_download(self.vertex_count)
            self._vertex_np_stale = False
        return self._vertex_np

    @vertex_np.setter
    def vertex_np(self, value):
        self._vertex_np = value
        self._vertex_np_stale = False

    # -- ingest -------------------------------------------------------------------------------
    def add_obj(self, filename):
        """Scene.py:59-141.  One material per MTL entry in file order; its faces become
        consecutive triangles (9-float vertex rows: pos, normal, uv+0).
        Extension: ``map_Kd`` becomes the material's albedo texture, ``map_d`` an alpha cut-out texture (``_add_opacity_texture``: the ``map_Kd`` file
        itself, or another file of the same size whose alpha or grey value joins the ``map_Kd`` image's RGB; ``map_d`` alone takes ``Kd`` ROUNDED TO 8 BITS
        as its RGB, which quantises the colour; different sizes raise ValueError)."""
        scene = ObjLoader.Wavefront(filename)
        for name in scene.materials:
            src = scene.materials[name]
            material = SCD.Material()
            if (src.emissive[0] > 1.0) and (src.emissive[1] > 1.0) and (src.emissive[2] > 1.0):
                material.type = SCD.MAT_LIGHT
                material.setColor(src.emissive)
            elif src.transparency > 0.99:
                material.type = SCD.MAT_DISNEY
                material.setMetal(0.0)
                material.setRough(0.5)
                material.setColor(src.diffuse)
            else:
                material.type = SCD.MAT_GLASS
                material.setIor(src.optical_density)
                material.setExtinciton(src.shininess)
                material.setColor(src.diffuse)
            material.alebdoTex = -1
            if src.opacity is not None and material.type != SCD.MAT_LIGHT:
                material.alebdoTex = self._add_opacity_texture(src.texture, src.opacity, src.diffuse)      # map_d (with or without map_Kd)
            elif src.texture is not None and material.type != SCD.MAT_LIGHT:
                material.alebdoTex = self.add_texture(src.texture)          # map_Kd
            if material.type != SCD.MAT_LIGHT:                              # map_Pr, map_Pm, norm / map_Bump / bump (one file named twice: one texture)
                for slot, path in zip(("roughTex", "metalTex", "normalTex"), getattr(src, "maps", (None, None, None))):
                    if path is not None and not (material.type == SCD.MAT_GLASS and slot != "normalTex"):
                        setattr(material, slot, self.add_texture(path))
            self.material_cpu.append(material)

            flat = src.vertices
            stride = src.vertex_size
            if stride and flat.size:
                rows = flat.reshape(-1, stride)
                rows = rows[: (rows.shape[0] // 3) * 3]
                block = np.zeros((rows.shape[0], SCD.VER_VEC_SIZE), dtype=np.float64)
                fmt = src.vertex_format
                block[:, 0:3] = rows[:, stride - 3:stride]
                if fmt.startswith("T2F"):
                    block[:, 6:8] = rows[:, 0:2]
                if "N3F" in fmt:
                    off = 2 if fmt.startswith("T2F") else 0
                    block[:, 3:6] = rows[:, off:off + 3]
                self._add_block(block, self.material_count, material.type == SCD.MAT_LIGHT)
            self.material_count += 1

    def add_mesh(self, positions, material, normals=None):
        """Extension (no reference equivalent): append a triangle soup ``positions[k,3,3]``
        with one material -- what ``add_obj`` would produce for a one-material OBJ without
        reading a file.  Used for the synthetic headline scene (BASELINE config 3)."""
        positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        block = np.zeros((positions.shape[0], SCD.VER_VEC_SIZE), dtype=np.float64)
        block[:, 0:3] = positions
        if normals is not None:
            block[:, 3:6] = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        self.material_cpu.append(material)
        self._add_block(block, self.material_count, material.type == SCD.MAT_LIGHT)
        self.material_count += 1

    def _add_block(self, block, mat_index, is_light):
        ntri = block.shape[0] // 3
        if ntri == 0:
            return
        pos = block[:, 0:3]
        self.maxboundarynp[0, :] = np.maximum(self.maxboundarynp[0, :].astype(np.float64), pos.max(axis=0))
        self.minboundarynp[0, :] = np.minimum(self.minboundarynp[0, :].astype(np.float64), pos.min(axis=0))
        self._vertex_chunks.append(block)
        self._prim_mat.append((self.primitive_count, ntri, mat_index, self.vertex_count))
        if is_light:
            self.light_cpu.extend(range(self.primitive_count, self.primitive_count + ntri))
            self.light_count += ntri
        self.vertex_count += 3 * ntri
        self.primitive_count += ntri

    def add_env(self, filename, env_power):
        # The reference ignores `filename` and always loads image/env.png (Scene.py:183-185,
        # quirk B16); here the argument is honoured.
        # Extension: an ``(h, w, 3)`` uint8 array with row 0 the top of the image, as ``add_texture`` takes one.
        if isinstance(filename, (str, bytes, os.PathLike)):
            self.env.load_image(filename)
        else:
            arr = np.asarray(filename)
            if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8 or arr.shape[0] < 1 or arr.shape[1] < 1:
                raise ValueError("Scene.add_env: an image array must be (h, w, 3) uint8, got %s %s" % (arr.dtype, arr.shape))
            self.env.load_array(arr)
        self.env_power = env_power

    def add_env_hdr(self, source, env_power):
        """No reference counterpart (include/tirt.h, "HDR environment"): an environment of linear radiance beyond 8 bits per channel, PT_RGB only.  ``source`` is the
        path of a Radiance ``.hdr`` file (``Texture.load_hdr``) or an ``(h, w, 3)`` float32 / float64 array with row 0 the top of the image
        (``Texture.load_array_float``, which states how it rounds).  ``add_env`` stays what it is: 8-bit images."""
        if isinstance(source, (str, bytes, os.PathLike)):
            self.env.load_hdr(source)
        else:
            self.env.load_array_float(source)
        self.env_power = env_power

    def _add_opacity_texture(self, kd_path, d_path, diffuse):
        """The alpha cut-out texture of an MTL material with a ``map_d`` statement (include/tirt.h, "Alpha cut-outs").
        ``map_d`` names the ``map_Kd`` file: that image with its own alpha channel.  Another file of the same size: its alpha channel -- its grey
        value if it has none -- joins the ``map_Kd`` image's RGB.  ``map_d`` alone: RGB is the material's ``Kd`` ROUNDED TO 8 BITS
        (round(255 * clip(Kd, 0, 1)): the texture takes the place of the row's colour, so the colour is quantised).  Different sizes: ValueError."""
        from PIL import Image
        d_abs = os.path.abspath(os.fsdecode(d_path))
        kd_abs = None if kd_path is None else os.path.abspath(os.fsdecode(kd_path))
        if kd_abs == d_abs:
            return self.add_texture(d_abs, cutout=True)
        key = ("map_d", kd_abs, d_abs, tuple(float(x) for x in diffuse[:3]) if kd_abs is None else None)
        if key in self._texture_ids:
            return self._texture_ids[key]
        if not os.path.isfile(d_abs):
            raise FileNotFoundError("Scene.add_obj: no such map_d image file: %s" % d_abs)
        dimg = Image.open(d_abs)
        has_alpha = "A" in dimg.getbands() or (dimg.mode == "P" and "transparency" in dimg.info)
        alpha = np.asarray(dimg.convert("RGBA"), np.uint8)[:, :, 3] if has_alpha else np.asarray(dimg.convert("L"), np.uint8)
        if kd_abs is None:
            kd8 = np.round(255.0 * np.clip(np.asarray(diffuse[:3], np.float64), 0.0, 1.0)).astype(np.uint8)
            rgb = np.broadcast_to(kd8, alpha.shape + (3,))
        else:
            if not os.path.isfile(kd_abs):
                raise FileNotFoundError("Scene.add_obj: no such map_Kd image file: %s" % kd_abs)
            rgb = np.asarray(Image.open(kd_abs).convert("RGB"), np.uint8)
            if rgb.shape[:2] != alpha.shape:
                raise ValueError("Scene.add_obj: map_d image %s is %d x %d, map_Kd image %s is %d x %d (they must have one size)"
                                 % (d_abs, alpha.shape[1], alpha.shape[0], kd_abs, rgb.shape[1], rgb.shape[0]))
        tid = self.add_texture(np.ascontiguousarray(np.concatenate([rgb, alpha[:, :, None]], axis=2), np.uint8), cutout=True)
        self._texture_ids[key] = tid
        return tid

    def add_texture(self, image, wrap="repeat", cutout=False):
        """Extension (the reference never samples a texture for a surface): a texture for materials -- albedo, or a roughness (.g), metallic (.b) or
        tangent-space normal map for ``Material.roughTex`` / ``metalTex`` / ``normalTex``, all in the same storage.  ``image`` is a path, decoded as
        ``add_env`` decodes its image, or an ``(h, w, 3)`` uint8 array with row 0 the top of the image; ``wrap`` is "repeat" or "clamp".
        Returns the texture's 1-based id: the value to put into ``Material.alebdoTex`` (0 and -1 mean no texture).  The same path with
        the same wrap mode gives the same id.  Textures go to the device with the scene (``setup_data_gpu``); PT_RGB, its feature
        buffers and the Debug albedo view use them, the BDPT and spectral integrators refuse a textured scene (include/tirt.h).
        ``cutout=True``: an alpha cut-out texture for ``Material.alebdoTex`` -- an image file with an alpha channel (one without is opaque) or an
        ``(h, w, 4)`` uint8 array; a hit where the bilinearly looked-up alpha is below 0.5 is no hit, for every ray (include/tirt.h, "Alpha cut-outs").
        The same path gives another id with another ``cutout``."""
        cutout = bool(cutout)
        if wrap not in ("repeat", "clamp"):
            raise ValueError("Scene.add_texture: wrap must be 'repeat' or 'clamp', got %r" % (wrap,))
        flag = 1 if wrap == "repeat" else 0
        tex = TX.Texture()
        if isinstance(image, (str, bytes, os.PathLike)):
            path = os.path.abspath(os.fsdecode(image))
            if (path, flag, cutout) in self._texture_ids:
                return self._texture_ids[(path, flag, cutout)]
            if not os.path.isfile(path):
                raise FileNotFoundError("Scene.add_texture: no such image file: %s" % path)
            if cutout:
                tex.load_image_rgba(path)
            else:
                tex.load_image(path)
            self._texture_ids[(path, flag, cutout)] = len(self.textures) + 1
        elif cutout:
            arr = np.asarray(image)
            if arr.ndim != 3 or arr.shape[2] != 4 or arr.dtype != np.uint8 or arr.shape[0] < 1 or arr.shape[1] < 1:
                raise ValueError("Scene.add_texture: a cut-out image array must be (h, w, 4) uint8, got %s %s" % (arr.dtype, arr.shape))
            tex.load_array_rgba(arr)
        else:
            arr = np.asarray(image)
            if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8 or arr.shape[0] < 1 or arr.shape[1] < 1:
                raise ValueError("Scene.add_texture: an image array must be (h, w, 3) uint8, got %s %s" % (arr.dtype, arr.shape))
            tex.load_array(arr)
        self.textures.append((tex, flag))
        self.texture_cutout.append(1 if cutout else 0)
        return len(self.textures)

    def add_shape(self, shape, mat):
        """Scene.py:188-205.  Does not extend the scene AABB (quirk B8)."""
        if mat.type == SCD.MAT_LIGHT:
            self.light_cpu.append(self.primitive_count)
            self.light_count += 1
        self._shape_prims.append((self.primitive_count, self.shape_count, self.material_count))
        self.primitive_count += 1
        self.shape_cpu.append(shape)
        self.shape_count += 1
        self.material_cpu.append(mat)
        self.material_count += 1

    # -- packing --------------------------------------------------------------------------------
    def cal_normal(self, verts):
        """Scene.py:169-179: triangles whose first vertex has a zero normal get the face
        normal normalize((v1-v0) x (v2-v0)) on all three vertices (double precision)."""
        tri = verts.reshape(-1, 3, SCD.VER_VEC_SIZE)
        n0 = tri[:, 0, 3:6]
        need = np.sqrt(n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1] + n0[:, 2] * n0[:, 2]) == 0.0
        if not need.any():
            return
        a = tri[need, 1, 0:3] - tri[need, 0, 0:3]
        b = tri[need, 2, 0:3] - tri[need, 0, 0:3]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                      a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        n = n * inv[:, None]
        for k in range(3):
            tri[need, k, 3:6] = n

    def setup_data_cpu(self):
        """Scene.py:223-296: host structs -> packed numpy rows; declares the LBVH."""
        self.material_np = np.zeros((self.material_count, SCD.MAT_VEC_SIZE), dtype=np.float32)
        for i, m in enumerate(self.material_cpu):
            m.fillStruct(self.material_np, i)

        if self._vertex_chunks:
            verts = np.concatenate(self._vertex_chunks, axis=0)
        else:
            verts = np.zeros((0, SCD.VER_VEC_SIZE), dtype=np.float64)
        self.cal_normal(verts)
        self.vertex_np = verts.astype(np.float32)
        self.smooth_normal_np = np.zeros((self.vertex_count, 3), dtype=np.float32)

        self.primitive_np = np.zeros((self.primitive_count, SCD.PRI_VEC_SIZE), dtype=np.int32)
        self.vertex_index_np = np.zeros(self.vertex_count, dtype=np.int32)
        for first, ntri, mat, vfirst in self._prim_mat:
            ids = np.arange(ntri, dtype=np.int32)
            self.primitive_np[first:first + ntri, 0] = SCD.PRIMITIVE_TRI
            self.primitive_np[first:first + ntri, 1] = vfirst + 3 * ids
            self.primitive_np[first:first + ntri, 2] = mat
            self.vertex_index_np[vfirst:vfirst + 3 * ntri] = first + np.repeat(ids, 3)
        for prim, sha, mat in self._shape_prims:
            self.primitive_np[prim] = (SCD.PRIMITIVE_SHAPE, sha, mat)

        if self.light_count > 0:
            self.light_np = np.asarray(self.light_cpu, dtype=np.int32)
        else:
            self.light_np = np.zeros(1, dtype=np.int32)          # Scene.py:259-261

        if self.shape_count > 0:
            self.shape_np = np.zeros((self.shape_count, SCD.SHA_VEC_SIZE), dtype=np.float32)
            for i, s in enumerate(self.shape_cpu):
                s.fillStruct(self.shape_np, i)
        else:
            self.shape_np = np.zeros((1, SCD.SHA_VEC_SIZE), dtype=np.float32)

        self.bvh = LBvh.Bvh(self.primitive_count, self.minboundarynp, self.maxboundarynp)
        self.bvh.setup_data_cpu()

        if self.env_power == 0.0:
            self.env.load_black()                                    # Scene.py:295-296

    def setup_data_gpu(self):
        """Scene.py:299-310: uploads, then the device LBVH build."""
        ctx = self.ctx
        # textures outlive a scene upload on the device, and a material row may only name an uploaded one: the old ones go first, the new ones follow the rows
        ctx.texture_upload([])
        ctx.scene_upload(self.vertex_np, self.primitive_np, self.material_np, self.shape_np,
                         self.light_np, self.light_count, self.minboundarynp, self.maxboundarynp)
        self.env.setup_data_gpu(ctx, self.env_power)
        if self.textures:
            ctx.texture_upload([(tex.np_img, flag) for tex, flag in self.textures])
            if any(self.texture_cutout):
                ctx.texture_cutout(self.texture_cutout)
        self.bvh.setup_data_gpu(self.vertex, self.shape, self.primitive)

    # -- kernels ------------------------------------------------------------------------------------
    def total_area(self):
        """Scene.py:747-750 (accumulates, like the reference's ``+=``)."""
        self._light_area[0] += np.float32(self.ctx.total_area())
        self._area_called = True

    def process_normal(self):
        """Scene.py:754-798: angle x area weighted smooth normals via a BVH point query."""
        self.vertex_np                                   # (a stale mirror is read back while the device still holds the un-smoothed normals)
        self.ctx.process_normal(self.vertex_index_np)
        self.normals_processed = True

    # -- moving geometry (extension, no reference equivalent) ------------------------------------------
    def _check_rows(self, rows, name, torch):
        """rows of update_vertices -> (address, vertices, floats per row step, the object that keeps the memory alive)"""
        fn = "Scene.update_vertices"
        is_tensor = torch is not None and isinstance(rows, torch.Tensor)
        if not is_tensor and not isinstance(rows, np.ndarray):
            raise TypeError("%s: %s must be a numpy array or a torch.Tensor, got %s" % (fn, name, type(rows).__name__))
        if rows.dtype != (torch.float32 if is_tensor else np.float32):
            raise TypeError("%s: %s must be float32, got %s" % (fn, name, rows.dtype))
        shape = tuple(rows.shape)
        if not ((len(shape) == 2 and shape[1] == 3) or (len(shape) == 3 and shape[1:] == (3, 3))):
            raise ValueError("%s: %s must be [k, 3] or [k/3, 3, 3], got shape %s" % (fn, name, shape))
        k = shape[0] * (3 if len(shape) == 3 else 1)
        if k % 3:
            raise ValueError("%s: %s must hold whole triangles, got %d vertices" % (fn, name, k))
        if not is_tensor:
            rows = np.ascontiguousarray(rows).reshape(-1, 3)
            return rows.ctypes.data, k, 3, rows
        if rows.device.type != "cuda":
            raise TypeError("%s: %s must be a numpy array or a tensor on the GPU, got a %s tensor" % (fn, name, rows.device.type))
        dev = torch.device("cuda", self._ctx.device_id)
        if rows.device != dev:
            raise ValueError("%s: %s is on %s, the scene's context on %s" % (fn, name, rows.device, dev))
        if k == 0:
            return 0, 0, 3, rows
        if rows.stride(-1) != 1:
            raise ValueError("%s: the last dimension of %s must have stride 1, got %d" % (fn, name, rows.stride(-1)))
        step = rows.stride(-2)
        if rows.dim() == 3 and shape[0] > 1 and rows.stride(0) != 3 * step:
            raise ValueError("%s: the vertices of %s must be evenly spaced (stride(0) == 3 * stride(1)), got strides %s" % (fn, name, tuple(rows.stride())))
        if k > 1 and step < 3:
            raise ValueError("%s: rows of %s overlap (stride = %d < 3)" % (fn, name, step))
        return rows.data_ptr(), k, step, rows

    def update_vertices(self, positions, normals=None, first_vertex=0):
        """Move triangles of a scene that is on the device (after setup_data_gpu) and rebuild the LBVH: vertices ``first_vertex ..
        first_vertex + k - 1`` (whole triangles, in the order of ``vertex_np``) get ``positions`` -- float32 ``[k, 3]`` or ``[k/3, 3, 3]``, a
        numpy array or a torch tensor on the context's device (any row stride with ``stride(-1) == 1``, e.g. ``buf[:, :3]``; the update runs
        after the work queued on ``torch.cuda.current_stream``, nothing has to be synchronised first).  ``normals`` of the same kind and shape
        are stored as they are; without them the triangles get their face normals, as ``cal_normal`` gives a mesh without normals.
        Afterwards the device state -- vertex rows, scene box, Morton codes, trees, shading tables, smooth normals if ``process_normal`` had
        been applied (the rows that are not moved are first given their un-smoothed normals back from ``vertex_np``, so a partial update does
        not smooth them twice) -- is bit for bit that of a fresh scene built from the moved positions, and ``vertex_np``, ``minboundarynp`` /
        ``maxboundarynp`` (the ``bvh``'s too) and ``light_area`` follow.  The call waits for the device (include/tirt.h, tirt_vertex_update).
        The film is not touched: clear it (``ctx.film_clear()``) or keep accumulating, and re-frame the camera if the box matters to it."""
        fn = "Scene.update_vertices"
        torch = sys.modules.get("torch")                  # a tensor cannot be passed without it: never imported here
        if torch is not None and not hasattr(torch, "Tensor"):
            torch = None
        if self.bvh is None or self._ctx is None:
            raise RuntimeError("%s: the scene is not on the device yet (setup_data_cpu / setup_data_gpu first)" % fn)
        pos_ptr, k, pos_step, keep_pos = self._check_rows(positions, "positions", torch)
        nrm_ptr, nrm_step, keep_nrm = 0, 3, None
        on_device = not isinstance(keep_pos, np.ndarray)
        if normals is not None:
            nrm_ptr, nk, nrm_step, keep_nrm = self._check_rows(normals, "normals", torch)
            if isinstance(keep_nrm, np.ndarray) == on_device:
                raise TypeError("%s: positions and normals must both be numpy arrays or both be tensors on the GPU" % fn)
            if nk != k:
                raise ValueError("%s: normals hold %d vertices, positions %d" % (fn, nk, k))
        if int(first_vertex) != first_vertex or first_vertex < 0 or first_vertex % 3:
            raise ValueError("%s: first_vertex must be a non-negative multiple of 3 (whole triangles), got %r" % (fn, first_vertex))
        if first_vertex + k > self.vertex_count:
            raise ValueError("%s: vertices %d .. %d are past the scene's %d" % (fn, first_vertex, first_vertex + k - 1, self.vertex_count))
        if k == 0:
            return
        ctx = self._ctx
        smoothed = getattr(self, "normals_processed", False)
        raw = self.vertex_np if smoothed else None        # the rows before process_normal (never stale while the scene is smoothed: see below)
        stream = torch.cuda.current_stream(keep_pos.device).cuda_stream if on_device else 0
        ctx.vertex_update(int(first_vertex), k, pos_ptr, pos_step, nrm_ptr, nrm_step, device=on_device, stream=stream)
        del keep_pos, keep_nrm                           # (the call has waited for the device)
        self._vertex_np_stale = True                     # from here on the device holds other rows and another box than the mirrors
        try:
            if smoothed:
                # the rows that are not moved hold SMOOTHED normals, and process_normal smooths what it finds: they get the normals a fresh
                # scene starts from again, so that the pass below repeats a fresh scene's and not a second round on top of the first
                for lo_v, hi_v in ((0, int(first_vertex)), (int(first_vertex) + k, self.vertex_count)):
                    if hi_v > lo_v:
                        rows = np.ascontiguousarray(raw[lo_v:hi_v, 0:6])
                        ctx.vertex_update(lo_v, hi_v - lo_v, rows.ctypes.data, 6, rows.ctypes.data + 12, 6)
            ctx.lbvh_build()
        finally:
            lo, hi = ctx.scene_box()
            self.minboundarynp[0, :] = lo                # in place: the Bvh holds the same arrays
            self.maxboundarynp[0, :] = hi
        if smoothed:
            self.process_normal()                        # (reads vertex_np back first: the mirror keeps the un-smoothed rows)
        if self._area_called:
            self._light_area[0] = np.float32(0.0) + np.float32(ctx.total_area())
