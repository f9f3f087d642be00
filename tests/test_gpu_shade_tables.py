"""The tables k_shade reads instead of recomputing what depends on a primitive or a light alone: the geometric normal and the area in the
128-byte shading record of a primitive (k_shade_records), and the per-light record of Scene.sample_li (k_light_records: area, choice pdf,
emission, the two edges of the sampled point).  Every entry must equal, bit for bit, what the un-hoisted device function returns for that
primitive or light (tirt_kat_shade_tables runs those: hit_attributes, get_prim_area, get_prim_random_point_normal, light_shape_visible),
and a material edit must reach the next render."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
import oracle_api
from ti_raytrace_amd import scenes
from ti_raytrace_amd import SceneData as SCD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(name):
    if name == "cornell":                       # mesh light (two triangles), face normals
        ex = scenes.cornell_box(32, 32, 4, device_id=0)
    elif name == "teapot":                      # smooth normals (Scene.process_normal), sphere light, glass
        ex = scenes.single_model(32, 32, 4, device_id=0)
    elif name == "synthetic":                   # the headline's kind of scene: triangle soup and a sphere light
        ex = scenes.synthetic(32, 32, 4, ntri=5000, device_id=0)
    elif name == "spot_laser":                  # quad light + the two shape emitters without a surface
        ex = common.spot_laser_scene(32, 32, device_id=0)
    elif name == "sphere_spot_laser":           # sphere light + spot + laser; the quad turned grey stays in the light list
        ex = common.spot_laser_scene(32, 32, device_id=0, with_quad_light=False)
        ex.add_sphere_light(pos=(278.0, 400.0, -280.0), radius=60.0, emission=30.0)
    else:
        raise AssertionError(name)
    ex.build_scene()
    if name in ("spot_laser", "sphere_spot_laser"):          # (a plain Example: the scene classes do this in their build_scene)
        ex.scene.total_area(); ex.frame_camera(0.8)
    return ex


SCENES = ("cornell", "teapot", "synthetic", "spot_laser", "sphere_spot_laser")


def test_shading_record_is_one_128_byte_line():
    """host: the record strides are what the kernels index with (8 quads of 16 bytes), in the header's words and in the device code"""
    dev = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_device.h")).read()
    api = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_api.hip")).read()
    assert re.search(r"const float4 \*r = rec \+ \(size_t\)prim \* 8;", dev)
    assert re.search(r"constexpr int LIGHT_REC_QUADS = 8;", dev)
    assert re.search(r"c->shade_rec\.ensure\(sizeof\(float4\) \* 8 \* \(size_t\)c->n\)", api)
    assert C.sizeof(C.c_float) * 4 * 8 == 128


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_shading_records_equal_the_unhoisted_functions(gpu_ctx_ok, name):
    ex = build(name)
    sc, ctx = ex.scene, ex.scene.ctx
    n = sc.primitive_count
    rec = ctx.shade_table_download(0, n)
    assert rec.shape == (n, 8, 4) and rec.nbytes == 128 * n
    kat = ctx.kat_shade_tables(0, n)
    vertex = sc.vertex.to_numpy().reshape(-1, 9)            # (after process_normal where the scene runs it)
    tri = sc.primitive_np[:, 0] == SCD.PRIMITIVE_TRI
    assert tri.any()
    ti = np.nonzero(tri)[0]
    v0 = sc.primitive_np[ti, 1]
    # the copies the record always held
    for k in range(3):
        assert np.array_equal(bits(rec[ti, k, :3]), bits(vertex[v0 + k, 0:3]))
        assert np.array_equal(bits(rec[ti, 3 + k, :3]), bits(vertex[v0 + k, 3:6]))
    assert np.array_equal(bits(rec[:, 0, 3]).view(np.int32), sc.primitive_np[:, 2])
    # the hoisted entries: gnor and area of a triangle in quad 6, the area of a shape in (1, 2)
    assert np.array_equal(bits(rec[ti, 6, :3]), bits(kat[ti, :3])), "gnor differs from hit_attributes'"
    assert np.array_equal(bits(rec[ti, 6, 3]), bits(kat[ti, 3])), "area differs from get_prim_area's"
    si = np.nonzero(~tri)[0]
    assert np.array_equal(bits(rec[si, 1, 2]), bits(kat[si, 3])), "shape area differs from get_prim_area's"
    assert not rec[:, 7].any()
    # and they are what they claim to be.  Only on well-shaped triangles (|cross| > 0.1 x longest edge squared), where neither the fp32 cross
    # product nor Heron's formula cancels: there both are good to a few 1e-6 relative, 1e-3 leaves two orders of room
    p = vertex[:, 0:3].astype(np.float64)
    e = np.stack([p[v0 + 1] - p[v0], p[v0 + 2] - p[v0], p[v0 + 2] - p[v0 + 1]], axis=1)
    g = np.cross(e[:, 0], e[:, 1])
    ln = np.linalg.norm(g, axis=1)
    ok = ln > 0.1 * (e ** 2).sum(axis=2).max(axis=1)
    assert ok.any()
    assert np.allclose(rec[ti[ok], 6, :3], g[ok] / ln[ok, None], rtol=0.0, atol=1e-3)
    assert np.allclose(rec[ti[ok], 6, 3], 0.5 * ln[ok], rtol=1e-3, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_light_records_equal_the_unhoisted_functions(gpu_ctx_ok, name):
    ex = build(name)
    sc, ctx = ex.scene, ex.scene.ctx
    nl = sc.light_count
    assert nl >= 1
    rec = ctx.shade_table_download(1, nl)
    kat = ctx.kat_shade_tables(1, nl)
    assert np.array_equal(bits(rec[:, 0, 3]), bits(kat[:, 0])), "area"
    assert np.array_equal(bits(rec[:, 1, 3]), bits(kat[:, 1])), "choice pdf"
    assert np.array_equal(bits(rec[:, 3:6, 3]), bits(kat[:, 2:5])), "emission"
    lp = sc.light_np[:nl]
    tri = sc.primitive_np[lp, 0] == SCD.PRIMITIVE_TRI
    kind = bits(rec[:, 2, 3]).view(np.int32)
    assert np.array_equal(kind[tri], np.full(int(tri.sum()), -1))
    shp = sc.shape_np[sc.primitive_np[lp[~tri], 1]]
    assert np.array_equal(kind[~tri], shp[:, 0].astype(np.int32))
    # emission is the light's material colour; a laser is chosen with 1 / light_count
    assert np.array_equal(bits(rec[:, 3:6, 3]), bits(sc.material_np[sc.primitive_np[lp, 2], 2:5]))
    laser = np.zeros(nl, bool); laser[~tri] = shp[:, 0].astype(np.int32) == SCD.SHPAE_LASER
    assert np.array_equal(bits(rec[laser, 1, 3]), bits(np.full(int(laser.sum()), np.float32(1.0) / np.float32(nl), np.float32)))
    if name in ("spot_laser", "sphere_spot_laser"):
        assert laser.sum() == 1 and (kind == SCD.SHPAE_SPOT).sum() == 1
    if name == "sphere_spot_laser":
        assert (kind == SCD.SHPAE_SPHERE).sum() == 1

    # whole NEE set-ups: light choice, sampled point, the three normalisations of its normal, visibility factor, pdf -- un-hoisted against the records
    rng = np.random.RandomState(5)
    m = 4096
    lo, hi = sc.minboundarynp[0].astype(np.float64), sc.maxboundarynp[0].astype(np.float64)
    inp = np.concatenate([rng.uniform(0.0, 1.0, size=(m, 3)), lo + rng.uniform(0.0, 1.0, size=(m, 3)) * (hi - lo)], axis=1).astype(np.float32)
    inp[:nl, 0] = (np.arange(nl) + 0.5) / nl                 # every light at least once
    inp[0, 0] = np.float32(1.0)                              # the clamp of the light index
    both = ctx.kat_shade_tables(2, m, inp)
    assert np.array_equal(bits(both[:, 0]), bits(both[:, 1])), \
        "sample_li from the light records differs from the un-hoisted functions in %d of %d set-ups" % (
            int((bits(both[:, 0]) != bits(both[:, 1])).any(axis=1).sum()), m)
    assert np.isfinite(both[:, 0, 0:3]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "sphere_spot_laser"))
def test_material_edit_reaches_the_next_render(gpu_ctx_ok, oracle_lib, name):
    """no stale table: after tirt_material_upload the light records carry the new emission, and the film is the oracle's for the new materials"""
    W = H = 32
    ex = build(name)
    sc, ctx = ex.scene, ex.scene.ctx
    ex.integrator.render_frames(2)
    before = ex.integrator.hdr.to_numpy()
    rec0 = ctx.shade_table_download(1, sc.light_count)

    for i in range(sc.material_count):
        if int(sc.material_np[i, 0]) == SCD.MAT_LIGHT:
            sc.material_np[i, 2:5] *= np.float32([0.5, 2.0, 0.25])
        elif int(sc.material_np[i, 0]) == SCD.MAT_DISNEY:
            sc.material_np[i, 2:5] = np.float32([0.3, 0.6, 0.9]) * (0.5 + 0.5 * sc.material_np[i, 2:5])
    ctx.material_upload(sc.material_np)
    rec1 = ctx.shade_table_download(1, sc.light_count)
    lp = sc.light_np[:sc.light_count]
    assert np.array_equal(bits(rec1[:, 3:6, 3]), bits(sc.material_np[sc.primitive_np[lp, 2], 2:5]))
    assert not np.array_equal(bits(rec1[:, 3:6, 3]), bits(rec0[:, 3:6, 3]))
    kat = ctx.kat_shade_tables(1, sc.light_count)
    assert np.array_equal(bits(rec1[:, 3:6, 3]), bits(kat[:, 2:5]))

    ctx.film_clear()
    ex.integrator.render_frames(2)
    got = ex.integrator.hdr.to_numpy()
    assert not np.array_equal(got, before)
    orc = oracle_api.OracleScene(sc, ex.cam)
    orc.lbvh_build()
    want, _ = orc.render(W, H, 0, 2, seed=ex.integrator.seed)
    assert common.same_bits(got, want), "film after a material edit differs from the oracle's in %d pixels" % int((got != want).any(axis=2).sum())
