"""Example set-ups (mirrors of the reference's ``example/cornell_box.py`` and
``example/single_model.py``) plus the synthetic 100k-triangle headline scene of
BASELINE.json config 3.  Model / image inputs are the reference's own data
files, kept under ``assets/``.
"""
import os

import numpy as np

from . import Example, PT_RGB, BDPT_RGB, PT_Spec, BDPT_SPEC
from . import SceneData as SCD

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


def asset(*parts):
    return os.path.join(ASSETS, *parts)


class cornell_box(Example.example):
    """example/cornell_box.py:12-35."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "cornell_box.obj"))
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **pt_kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.total_area()
        self.frame_camera(0.8)


class single_model(Example.example):
    """example/single_model.py:13-49 with the Teapot line enabled (BASELINE config 2):
    material 0 -> glass (ior 1.3, extinction 5), sphere light, env.png x 5, smooth normals."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, model="Teapot.obj", device_id=None, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", model))
        self.scene.material_cpu[0].type = SCD.MAT_GLASS
        self.scene.material_cpu[0].setIor(1.3)
        self.scene.material_cpu[0].setExtinciton(5.0)
        self.add_sphere_light()
        self.scene.add_env(asset("image", "env.png"), 5.0)
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **pt_kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.process_normal()
        self.scene.total_area()
        self.frame_camera(0.8)


class gallery_sphere(Example.example):
    """The scene of the reference's gallery renders image/glass.png, metal.png and non-metal.png: example/single_model.py
    with sphere.obj and its three material variants (:27-31: glass ior 1.3 / extinction 5; Disney metal 1 rough 0; the
    default Disney).  Those renders predate the committed example -- measured on the images: the sphere is 253 px wide
    (camera at 1.0 x |diagonal|, the committed :46 says 0.8), the light disc has a radius of 37 px at 30 degrees
    elevation (a sphere light near (0, 2, 0) r 0.3; Example.py:27-36 says (0, 20, 0) r 5) and the background is the env
    map seen from yaw pi -- so this class takes those as parameters (defaults = the measured ones).  Used by the
    structure pins of tests/test_oracle_golden.py and tests/test_gpu_gallery.py."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, variant="glass", cam_scale=1.0, yaw=3.14159265,
                 light_pos=(0.0, 2.0, 0.0), light_radius=0.3, emission=50.0, device_id=None, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "sphere.obj"))
        m = self.scene.material_cpu[0]
        if variant == "glass":
            m.type = SCD.MAT_GLASS
            m.setIor(1.3)
            m.setExtinciton(5.0)
        elif variant == "metal":
            m.setMetal(1.0)
            m.setRough(0.0)
        elif variant != "non-metal":
            raise ValueError(variant)
        self.add_sphere_light(pos=light_pos, radius=light_radius, emission=emission)
        self.scene.add_env(asset("image", "env.png"), 5.0)
        self.cam_scale, self.cam_yaw = cam_scale, yaw
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **pt_kwargs)

    def frame_camera(self, scale_factor=None):
        Example.example.frame_camera(self, self.cam_scale if scale_factor is None else scale_factor)
        self.cam.set_view_point(self.cam_yaw, 0.0, 0.0, self.cam.scale)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.process_normal()
        self.scene.total_area()
        self.frame_camera()


class veach_bdpt(Example.example):
    """example/veach_bdpt.py:12-35 (BASELINE config 5): bdpt.obj, BDPT_RGB, smooth normals,
    camera at 0.5 x |diagonal|."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, integrator="bdpt", **kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "bdpt.obj"))
        if integrator == "bdpt":
            self.integrator = BDPT_RGB.BDPT(imgSizeX, imgSizeY, self.cam, self.scene, 64, **kwargs)
        else:
            self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.process_normal()
        self.scene.total_area()
        self.frame_camera(0.5)


class spectral_box(Example.example):
    """example/spectral_box.py:12-43: the Cornell box through PT_Spec, its three diffuse materials turned into tabulated
    reflectance spectra (MAT_SPECTRAL with alebdoTex 0 / 1 / 2 = white / red / green, spectrum/*-spec.csv), D65 emitter."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, **kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "cornell_box.obj"))
        self.integrator = PT_Spec.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **kwargs)
        for k in range(3):
            self.scene.material_cpu[k].type = SCD.MAT_SPECTRAL
            self.scene.material_cpu[k].alebdoTex = k

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.process_normal()
        self.scene.total_area()
        self.frame_camera(0.8)


class sky_dome(Example.example):
    """example/sky_dome.py:11-39: a mirror ball (sphere.obj, Disney metal 1 / rough 0) under the analytic sky, PT_Spec."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, **kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "sphere.obj"))
        self.scene.material_cpu[0].setMetal(1.0)
        self.scene.material_cpu[0].setRough(0.0)
        self.add_sphere_light()
        self.integrator = PT_Spec.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.process_normal()
        self.scene.total_area()
        self.scene.env_power = 0.0
        self.frame_camera(2.0)


def sun_sky_image(w=16, h=8, floor=8, at=(11, 1)):
    """(h, w, 3) uint8, row 0 the top: one texel at 255 -- a "sun" about 480 times the floor in linear light -- on a dim uniform sky."""
    img = np.full((h, w, 3), floor, np.uint8)
    img[at[1], at[0]] = 255
    return img


def hdr_sun_sky(w=16, h=8, floor=0.02, sun=5000.0, at=(11, 1)):
    """(h, w, 3) float32 linear radiance, row 0 the top: one texel at ``sun`` on a uniform sky of ``floor`` -- 250 000 : 1 by default, the ratio of a real sun
    to its sky, which 8 bits per channel times one env_power cannot hold (Scene.add_env_hdr)."""
    img = np.full((h, w, 3), floor, np.float32)
    img[at[1], at[0]] = sun
    return img


def _box(lo, hi):
    """the twelve triangles of an axis-aligned box, outward facing"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]
    return np.array([[c[q[0]], c[q[a]], c[q[a + 1]]] for q in quads for a in (1, 2)], np.float64)


class sun_ground(Example.example):
    """No reference counterpart: a box on a ground quad under a synthetic sky whose light is nearly all in one texel, no emitters -- the case BSDF
    sampling alone handles worst.  ``env_sampling=True`` (the default here) aims the light samples at the sky by its brightness (include/tirt.h,
    "Importance sampling of the environment"); ``env_sampling=False`` renders with the reference's estimator.  Both surfaces are rough metals, or rough
    dielectrics with ``metallic=0.0``.  ``sky``: an ``(h, w, 3)`` uint8 image (default ``sun_sky_image()``), or an HDR sky -- a float32 / float64 array of linear
    radiance such as ``hdr_sun_sky()``, or the path of a ``.hdr`` file -- which goes through ``Scene.add_env_hdr``."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, env_power=20.0, sky=None, env_sampling=True, metallic=1.0, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)

        def disney(colour, rough):
            m = SCD.Material(); m.type = SCD.MAT_DISNEY; m.setMetal(metallic); m.setRough(rough); m.setColor([colour[0], colour[1], colour[2], 1.0]); m.alebdoTex = -1
            return m
        g = 2.0
        self.scene.add_mesh(np.array([[(-g, 0, -g), (-g, 0, g), (g, 0, g)], [(-g, 0, -g), (g, 0, g), (g, 0, -g)]], np.float64), disney((0.7, 0.7, 0.7), 0.8))
        self.scene.add_mesh(_box((-0.5, 0.0, -0.5), (0.5, 1.5, 0.5)), disney((0.8, 0.4, 0.2), 0.5))
        is_path = isinstance(sky, (str, bytes, os.PathLike))
        if (is_path and os.fsdecode(sky).lower().endswith(".hdr")) or (sky is not None and not is_path and np.asarray(sky).dtype in (np.float32, np.float64)):
            self.scene.add_env_hdr(sky, env_power)
        else:
            self.scene.add_env(sun_sky_image() if sky is None else sky, env_power)
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, env_sampling=env_sampling, **pt_kwargs)

    def frame_camera(self, scale_factor=0.6):
        Example.example.frame_camera(self, scale_factor)
        self.cam.set_view_point(1.96, 0.7, 0.0, self.cam.scale)      # across the shadow, from above

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.total_area()
        self.frame_camera()


class lamp_and_embers(Example.example):
    """No reference counterpart: a ground quad under one bright two-triangle lamp and ``n_embers`` small dim emissive triangles scattered above the ground -- the
    case a uniform choice among the light list's entries handles worst: the lamp holds over 95 % of the emitted power (emission x area) and gets two entries in
    ``n_embers + 2``.  ``light_sampling="power"`` (the default here) chooses emitters by power (include/tirt.h, "Choosing emitters by power");
    ``"uniform"`` renders with the reference's estimator.  The ground is a rough metal, or a rough dielectric with ``metallic=0.0``."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, n_embers=254, metallic=1.0, light_sampling="power", lamp_emission=640.0, lamp_size=0.25,
                 ember_emission=0.5, ember_size=0.04, ember_seed=7, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        ground = SCD.Material(); ground.type = SCD.MAT_DISNEY; ground.setMetal(metallic); ground.setRough(0.8); ground.setColor([0.7, 0.7, 0.7, 1.0]); ground.alebdoTex = -1
        g = 2.0
        self.scene.add_mesh(np.array([[(-g, 0, -g), (-g, 0, g), (g, 0, g)], [(-g, 0, -g), (g, 0, g), (g, 0, -g)]], np.float64), ground)

        def emitter(e):
            m = SCD.Material(); m.type = SCD.MAT_LIGHT; m.setColor([e, e, e]); m.alebdoTex = -1
            return m
        # the lamp: lamp_size x lamp_size at height 2, facing down -- small and bright, so that BSDF sampling seldom finds it (area 1 / 16, power 40: the embers
        # below hold n * 0.5 * 0.0008 = 0.1 at the default 254)
        a = 0.5 * float(lamp_size)
        self.scene.add_mesh(np.array([[(-a, 2.0, -a), (a, 2.0, a), (-a, 2.0, a)], [(-a, 2.0, -a), (a, 2.0, -a), (a, 2.0, a)]], np.float64), emitter(lamp_emission))
        # the embers: right triangles of leg ember_size in horizontal planes, facing up and down alike (an emitter radiates from both faces)
        if n_embers > 0:
            u = splitmix64_unit(ember_seed, 3 * n_embers).reshape(n_embers, 3)
            c = np.stack([u[:, 0] * 3.0 - 1.5, 0.1 + u[:, 1] * 0.8, u[:, 2] * 3.0 - 1.5], axis=1)
            s = float(ember_size)
            tri = np.stack([c, c + np.array([s, 0.0, 0.0]), c + np.array([0.0, 0.0, s])], axis=1)
            self.scene.add_mesh(tri, emitter(ember_emission))
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, light_sampling=light_sampling, **pt_kwargs)

    def frame_camera(self, scale_factor=0.6):
        # at the ground's centre, from below the lamp's height: the film shows the lit ground and the embers, never the lamp itself (a pixel on the lamp's edge
        # would carry more variance than all the light samples of the film together)
        self.cam.scale = 5.0 * scale_factor
        self.cam.set_target(0.0, 0.0, 0.0)
        self.cam.set_view_point(1.96, 0.6, 0.0, self.cam.scale)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.total_area()
        self.frame_camera()


# ---- synthetic scene -------------------------------------------------------------------------
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix64_unit(seed, count):
    """u[k] in [0,1) from SplitMix64 with state seed + (k+1)*golden (53-bit mantissa)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(1, count + 1, dtype=np.uint64) * _GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def synthetic_triangles(ntri=100000, seed=1234, spread=0.03):
    """positions[ntri,3,3]: centroid c ~ U[-1,1]^3, vertex = c + U[-spread,spread]^3.
    Twelve stream values per triangle: c.xyz, then the three vertex offsets."""
    u = splitmix64_unit(seed, 12 * ntri).reshape(ntri, 4, 3)
    c = u[:, 0, :] * 2.0 - 1.0
    off = (u[:, 1:4, :] * 2.0 - 1.0) * spread
    return c[:, None, :] + off


class synthetic(Example.example):
    """BASELINE config 3: ``ntri`` random triangles, one Disney material (0.8 grey, metal 0,
    rough 0.5 = what a material-less OBJ gets, Scene.py:75-79), sphere light (0,3,0) r 0.75
    Le 50, black env, face normals, no process_normal, cornell_box camera rule."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, ntri=100000, scene_seed=1234,
                 spread=0.03, device_id=None, **pt_kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        mat = SCD.Material()
        mat.type = SCD.MAT_DISNEY
        mat.setMetal(0.0)
        mat.setRough(0.5)
        mat.setColor([0.8, 0.8, 0.8, 1.0])
        mat.alebdoTex = -1
        self.scene.add_mesh(synthetic_triangles(ntri, scene_seed, spread), mat)
        self.add_sphere_light(pos=(0.0, 3.0, 0.0), radius=0.75, emission=50.0)
        self.integrator = PT_RGB.PathTrace(imgSizeX, imgSizeY, self.cam, self.scene, 64, **pt_kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.total_area()
        self.frame_camera(0.8)


class prism_rainbow(Example.example):
    """example/prism_rainbow.py:13-66: a glass prism (model/prism1.obj: glass, wall, ground) lit by a sphere light and by a LASER beam
    (SceneData.SHPAE_LASER, radius 0.1, from (1, 0, 9) along -z) that the prism disperses into a spectrum, through BDPT_SPEC -- the light
    sub-path is the only way light from an emitter without a surface reaches the film."""

    def __init__(self, imgSizeX, imgSizeY, sample_count, device_id=None, laser_emission=500.0, sphere_emission=500.0, with_sphere_light=True, **kwargs):
        Example.example.__init__(self, imgSizeX, imgSizeY, sample_count, device_id)
        self.scene.add_obj(asset("model", "prism1.obj"))
        # (with_sphere_light=False: the laser alone, which is what the reference's gallery image of this example shows -- everything but the
        # spectrum on the wall is black there)
        if with_sphere_light:
            self.add_sphere_light(pos=(0.0, 20.0, 0.0), radius=5.0, emission=sphere_emission)
        shape = SCD.Shape()
        shape.type = SCD.SHPAE_LASER
        shape.pos = [1.0, 0.0, 9.0]
        shape.setRadius(0.1)
        shape.setNormal([0.0, 0.0, -1.0])
        mat = SCD.Material()
        mat.type = SCD.MAT_LIGHT
        mat.setColor([laser_emission, laser_emission, laser_emission])
        self.scene.add_shape(shape, mat)
        self.integrator = BDPT_SPEC.BDPT(imgSizeX, imgSizeY, self.cam, self.scene, 1024, **kwargs)

    def build_scene(self):
        Example.example.build_scene(self)
        self.scene.total_area()
        self.cam.scale = 10.0
        self.cam.set_target(0.0, 0.0, 0.0)
        self.cam.update()
