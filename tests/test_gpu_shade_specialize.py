"""k_shade / k_shade_spec compiled per scene feature set (option "shade_specialize", include/tirt.h): the film a scene gets from the narrowest
instantiation that covers its feature word equals the film of the generic kernel bit for bit, NaN positions included, with the same ray counts --
for one scene per instantiation and for scenes only the generic kernel serves; and the word the context holds follows the uploads."""
import numpy as np
import pytest

import common
from ti_raytrace_amd import _native, scenes, Example, PT_RGB
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu

W, H, FRAMES = 45, 27, 9          # ragged, non-square; nine frames


def env_only_scene():
    """Disney triangles under env.png and no emitter: NEE has nothing to sample (light_count == 0)"""
    ex = Example.example(W, H, FRAMES, 0)
    m = SCD.Material(); m.type = SCD.MAT_DISNEY; m.setMetal(0.2); m.setRough(0.4); m.setColor([0.7, 0.6, 0.5, 1.0]); m.alebdoTex = -1
    ex.scene.add_mesh(scenes.synthetic_triangles(3000, 5, 0.08), m)
    ex.scene.add_env(scenes.asset("image", "env.png"), 2.0)
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, ex.scene, 64)
    return ex


SCENES = {
    # name: (constructor, needs the plain-Example epilogue, feature word, word of the instantiation it must get -- None: the generic kernel)
    "synthetic": (lambda: scenes.synthetic(W, H, FRAMES, ntri=20000, device_id=0), False, _native.SF_LIGHT_SPHERE, _native.SF_LIGHT_SPHERE),
    "cornell": (lambda: scenes.cornell_box(W, H, FRAMES, device_id=0), False, _native.SF_LIGHT_TRI, _native.SF_LIGHT_TRI),
    "veach_pt": (lambda: scenes.veach_bdpt(W, H, FRAMES, device_id=0, integrator="pt"), False, None, None),
    "teapot_env": (lambda: scenes.single_model(W, H, FRAMES, device_id=0), False, _native.SF_GLASS | _native.SF_ENV | _native.SF_LIGHT_SPHERE, None),
    "spectral_cornell": (lambda: scenes.spectral_box(W, H, FRAMES, device_id=0), False, _native.SF_LIGHT_TRI, _native.SF_LIGHT_TRI),
    "spectral_sky_dome": (lambda: scenes.sky_dome(W, H, FRAMES, device_id=0), False, _native.SF_LIGHT_SPHERE, _native.SF_LIGHT_SPHERE),
    "env_only": (env_only_scene, True, _native.SF_ENV | _native.SF_NO_LIGHT, None),
    "spot_laser": (lambda: common.spot_laser_scene(W, H, device_id=0), True, _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPOT_LASER, None),
}
INSTANTIATIONS = (_native.SF_LIGHT_SPHERE, _native.SF_LIGHT_TRI)       # the narrow ones of tirt_render.hip, narrowest first (both kernels)


def build(name):
    make, plain, word, _ = SCENES[name]
    ex = make()
    ex.build_scene()
    if plain:
        ex.scene.total_area(); ex.frame_camera(0.8)
    return ex, word


def render(ex, specialize):
    ctx = ex.scene.ctx
    ctx.film_clear()
    ctx.set_option("shade_specialize", specialize)
    ctx.stats_reset()
    ex.integrator.render_frames(FRAMES)
    hdr = ex.integrator.hdr.to_numpy()
    st = ctx.stats()
    return hdr, (st["rays_closest"], st["rays_shadow"], st["paths"], st["shaded"], st["stack_overflow"])


def same_film(a, b):
    """bit for bit where both are numbers, NaN exactly where the other has NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_specialised_film_equals_the_generic_film(gpu_ctx_ok, name):
    ex, word = build(name)
    sc, ctx = ex.scene, ex.scene.ctx
    got_word, on = ctx.shade_features()
    host_word = _native.shade_features_host(sc.material_np, sc.primitive_np, sc.shape_np, sc.light_np, sc.light_count, env=sc.env.np_img, env_power=sc.env_power)
    assert on == 1 and got_word == host_word, (bin(got_word), bin(host_word))
    if word is not None:
        assert got_word == word, (bin(got_word), bin(word))
    covering = [m for m in INSTANTIATIONS if got_word & ~m == 0]
    want_inst = SCENES[name][3]
    if name != "veach_pt":
        assert (covering[0] if covering else None) == want_inst, (bin(got_word), covering)
    spec, st_spec = render(ex, 1)
    gen, st_gen = render(ex, 0)
    again, _ = render(ex, 1)
    print("%s: feature word %s, %d NaN values, %d rays" % (name, bin(got_word), int(np.isnan(gen).sum()), st_gen[0] + st_gen[1]))
    assert st_spec == st_gen and st_gen[4] == 0, (st_spec, st_gen)
    assert np.isfinite(gen).any() and float(np.nan_to_num(gen).sum()) > 0.0
    assert same_film(spec, gen), "%s: %d values differ" % (name, int((spec.view(np.uint32) != gen.view(np.uint32)).sum()))
    assert same_film(again, spec)
    assert ctx.shade_features()[1] == 1


def test_the_feature_word_does_not_go_stale(gpu_ctx_ok):
    """a material edit, an environment upload and a vertex update on a live context each refresh the word, and the films keep agreeing"""
    ex, _ = build("synthetic")
    sc, ctx = ex.scene, ex.scene.ctx
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE
    base, _ = render(ex, 1)
    mats = sc.material_np.copy()
    mats[0, 0] = SCD.MAT_GLASS; mats[0, 5] = 1.3; mats[0, 6] = 5.0
    ctx.material_upload(mats)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE | _native.SF_GLASS
    glass1, _ = render(ex, 1)
    glass0, _ = render(ex, 0)
    assert same_film(glass1, glass0) and not same_film(glass1, base)
    ctx.material_upload(sc.material_np)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE
    back, _ = render(ex, 1)
    assert same_film(back, base)
    img = np.zeros((8, 4), np.int32)
    ctx.env_upload(img, 0.0)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE
    img[3, 1] = 0x00400000
    ctx.env_upload(img, 0.0)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE | _native.SF_ENV
    ctx.env_upload(np.zeros((8, 4), np.int32), 1.5)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE | _native.SF_ENV
    lit1, _ = render(ex, 1)
    lit0, _ = render(ex, 0)
    assert same_film(lit1, lit0)
    ctx.env_upload(np.zeros((8, 4), np.int32), 0.0)
    rows = np.ascontiguousarray(sc.vertex_np[:3, 0:3] * np.float32(1.01), np.float32)
    ctx.vertex_update(0, 3, rows.ctypes.data, 3)
    ctx.lbvh_build()
    assert ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE
    moved1, _ = render(ex, 1)
    moved0, _ = render(ex, 0)
    assert same_film(moved1, moved0)


def test_degenerate_shading_normals_under_a_black_environment(gpu_ctx_ok):
    """Vertex normals that cancel give NaN shading normals.  A Disney hit with such a normal ends its path (pdf -1), so without glass no ray
    with a NaN direction is ever traced -- the narrow instantiations' answer to a miss in a direction that is not finite (no environment lookup)
    is a safeguard; whatever the degenerate normals produce, both kernels must produce it in the same places."""
    ex = scenes.synthetic(W, H, FRAMES, ntri=4000, spread=0.3, device_id=0)
    ex.scene.setup_data_cpu()
    v = ex.scene.vertex_np
    v[0::3, 3:6] = (1.0, 0.0, 0.0); v[1::3, 3:6] = (-1.0, 0.0, 0.0); v[2::3, 3:6] = (0.0, 0.0, 0.0)      # normals that interpolate to zero along an edge
    v[: 3 * 2000, 3:6] = 0.0                                                                           # and half the triangles with no normal at all
    ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
    ex.scene.total_area(); ex.frame_camera(0.8)
    assert ex.scene.ctx.shade_features()[0] == _native.SF_LIGHT_SPHERE
    spec, st1 = render(ex, 1)
    gen, st0 = render(ex, 0)
    print("NaN values: %d of %d" % (int(np.isnan(gen).sum()), gen.size))
    assert st1 == st0 and same_film(spec, gen)
