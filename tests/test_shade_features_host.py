"""The scene feature word (include/tirt.h, tirt_shade_features) without a GPU: for every scene of scenes.py the word the library derives from
the packed tables (material, primitive, shape and light rows, the environment image) equals the word derived here from the scene's Python
objects, and it follows a material, a light and an environment change.  The word selects the instantiation of k_shade / k_shade_spec."""
import os
import re

import numpy as np
import pytest

import common
from ti_raytrace_amd import _native, scenes
from ti_raytrace_amd import SceneData as SCD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = {
    "cornell": lambda: scenes.cornell_box(16, 16, 4, device_id=0),
    "teapot": lambda: scenes.single_model(16, 16, 4, device_id=0),
    "gallery_glass": lambda: scenes.gallery_sphere(16, 16, 4, variant="glass", device_id=0),
    "gallery_metal": lambda: scenes.gallery_sphere(16, 16, 4, variant="metal", device_id=0),
    "gallery_non_metal": lambda: scenes.gallery_sphere(16, 16, 4, variant="non-metal", device_id=0),
    "veach": lambda: scenes.veach_bdpt(16, 16, 4, device_id=0, integrator="pt"),
    "spectral_box": lambda: scenes.spectral_box(16, 16, 4, device_id=0),
    "sky_dome": lambda: scenes.sky_dome(16, 16, 4, device_id=0),
    "synthetic": lambda: scenes.synthetic(16, 16, 4, ntri=200, device_id=0),
    "prism": lambda: scenes.prism_rainbow(16, 16, 4, device_id=0),
    "prism_laser_only": lambda: scenes.prism_rainbow(16, 16, 4, device_id=0, with_sphere_light=False),
    "spot_laser": lambda: common.spot_laser_scene(16, 16, device_id=0),
}
# what each scene is known to hold (a second, hand-written opinion beside expected())
KNOWN = {
    "cornell": _native.SF_LIGHT_TRI,
    "teapot": _native.SF_GLASS | _native.SF_ENV | _native.SF_LIGHT_SPHERE,
    "synthetic": _native.SF_LIGHT_SPHERE,
    "sky_dome": _native.SF_LIGHT_SPHERE,
    "spectral_box": _native.SF_LIGHT_TRI,
    "prism_laser_only": _native.SF_GLASS | _native.SF_LIGHT_SPOT_LASER,
    "spot_laser": _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPOT_LASER,
}


def expected(scene):
    """the word from the Python-side description: material_cpu, light_cpu / shape_cpu, env"""
    f = 0
    if any(m.type == SCD.MAT_GLASS for m in scene.material_cpu):
        f |= _native.SF_GLASS
    if scene.env_power != 0.0 or (scene.env.np_img is not None and (np.asarray(scene.env.np_img) & 0xFFFFFF).any()):
        f |= _native.SF_ENV
    if scene.light_count == 0:
        f |= _native.SF_NO_LIGHT
    shape_of = {prim: sha for prim, sha, _ in scene._shape_prims}
    for prim in scene.light_cpu[:scene.light_count]:
        if prim not in shape_of:
            f |= _native.SF_LIGHT_TRI
            continue
        t = scene.shape_cpu[shape_of[prim]].type
        f |= {SCD.SHPAE_SPHERE: _native.SF_LIGHT_SPHERE, SCD.SHPAE_SPOT: _native.SF_LIGHT_SPOT_LASER,
              SCD.SHPAE_LASER: _native.SF_LIGHT_SPOT_LASER}.get(t, _native.SF_LIGHT_OTHER)
    return f


def from_tables(scene):
    return _native.shade_features_host(scene.material_np, scene.primitive_np, scene.shape_np, scene.light_np, scene.light_count,
                                       env=scene.env.np_img, env_power=scene.env_power)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_feature_word_of_every_scene(name):
    ex = SCENES[name]()
    ex.scene.setup_data_cpu()
    got, want = from_tables(ex.scene), expected(ex.scene)
    assert got == want, (name, bin(got), bin(want))
    if name in KNOWN:
        assert got == KNOWN[name], (name, bin(got), bin(KNOWN[name]))


def test_feature_word_follows_material_light_and_environment_changes():
    ex = SCENES["synthetic"]()
    sc = ex.scene
    sc.setup_data_cpu()
    assert from_tables(sc) == _native.SF_LIGHT_SPHERE
    # a material becomes glass, and stops being it
    sc.material_cpu[0].type = SCD.MAT_GLASS; sc.material_cpu[0].setIor(1.3)
    sc.setup_data_cpu()
    assert from_tables(sc) == expected(sc) == _native.SF_GLASS | _native.SF_LIGHT_SPHERE
    sc.material_cpu[0].type = SCD.MAT_DISNEY
    sc.setup_data_cpu()
    assert from_tables(sc) == expected(sc) == _native.SF_LIGHT_SPHERE
    # the sphere light becomes a spot; a laser joins it
    sc.shape_cpu[0].type = SCD.SHPAE_SPOT
    sc.setup_data_cpu()
    assert from_tables(sc) == expected(sc) == _native.SF_LIGHT_SPOT_LASER
    sc.shape_cpu[0].type = SCD.SHPAE_SPHERE
    sh = SCD.Shape(); sh.type = SCD.SHPAE_LASER; sh.pos = [0.0, 2.0, 0.0]; sh.setRadius(0.1); sh.setNormal([0.0, -1.0, 0.0])
    mat = SCD.Material(); mat.type = SCD.MAT_LIGHT; mat.setColor([5.0, 5.0, 5.0])
    sc.add_shape(sh, mat)
    sc.setup_data_cpu()
    assert from_tables(sc) == expected(sc) == _native.SF_LIGHT_SPHERE | _native.SF_LIGHT_SPOT_LASER
    # the environment: power alone, a texel alone, neither
    sc.env_power = 2.0
    assert from_tables(sc) == expected(sc) and from_tables(sc) & _native.SF_ENV
    sc.env_power = 0.0
    assert not from_tables(sc) & _native.SF_ENV
    img = np.zeros((4, 4, 3), np.int32); img[1, 2, 1] = 9
    sc.env.load_array(img)
    assert from_tables(sc) == expected(sc) and from_tables(sc) & _native.SF_ENV
    # no emitter at all: the light list keeps one unused entry (Scene.py:259-261)
    bare = scenes.Example.example(8, 8, 1, 0)
    m = SCD.Material(); m.type = SCD.MAT_DISNEY; m.setColor([0.5, 0.5, 0.5, 1.0])
    bare.scene.add_mesh(scenes.synthetic_triangles(20, 3, 0.1), m)
    bare.scene.setup_data_cpu()
    assert from_tables(bare.scene) == expected(bare.scene) == _native.SF_NO_LIGHT


def test_an_emitter_of_unknown_kind_gets_the_generic_kernel():
    ex = SCENES["synthetic"]()
    ex.scene.shape_cpu[0].type = SCD.SHPAE_QUAD
    ex.scene.setup_data_cpu()
    assert from_tables(ex.scene) == expected(ex.scene) == _native.SF_LIGHT_OTHER


def test_header_binding_and_kernels_agree_on_the_bits():
    dev = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_device.h")).read()
    for name in ("SF_GLASS", "SF_ENV", "SF_LIGHT_TRI", "SF_LIGHT_SPOT_LASER", "SF_NO_LIGHT", "SF_LIGHT_SPHERE", "SF_LIGHT_OTHER"):
        m = re.search(r"\b%s = (\d+)u" % name, dev)
        assert m and int(m.group(1)) == getattr(_native, name), name
    assert "shade_specialize" in _native.OPTIONS
    api = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_api.hip")).read()
    dyn = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_dynamic.hip")).read()
    assert api.count("refresh_shade_features(c);") >= 3 and "refresh_shade_features(c);" in dyn      # scene, material, environment; vertex updates
    render = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_render.hip")).read()
    n_spec = len(re.findall(r"\bk_shade_spec<SF_\w+>", render))
    assert 2 <= n_spec <= 6, n_spec
    # k_shade's instantiations are named once, inside shade_inst<>(): one table holds them, and every word the binding lists is an entry that a render can launch
    assert len(re.findall(r"\bShadeInst\s+\w+\s*\[", render)) == 1 and "KatStepInst" not in render
    words = _native.SHADE_INSTANTIATIONS + (_native.SHADE_INSTANTIATION_MAPS,) + _native.SHADE_INSTANTIATIONS_ENV + _native.SHADE_INSTANTIATIONS_HDR + _native.SHADE_INSTANTIATIONS_POWER
    assert len(set(words)) == 19
    for feat in words:
        assert _native.shade_instantiation(feat, 1, 0) == feat, feat
