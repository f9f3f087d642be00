"""One PT_Spec shading step per instantiation of k_shade_spec against the CPU oracle (tirt_kat_shade_spec_step / orc_kat_shade_spec_step on the rows of
tests/shade_spec_step_cases.py): every output word of every row -- integers equal, floats bit-identical, NaN exactly where the oracle has NaN.  The device side is
k_shade_spec<FEAT, true>: the render kernel's own text with a row in place of a queued path.  What no per-function vector (tirt_kat_spec) and no film reaches:
light_sample_rec<FEAT> with one emitter kind in the narrow instantiations, the five-factor NEE product in four channels, the tint taken from the surface that was
hit, disney_evaluate_pdf(N, V = next_dir, L = -direction) for the continuation, the continuation test on channels 0..2 through maxf with NaN, the glass branch's
wavelength pick, the emitter hit at fCosTheta == 0, and the sky below the horizon, along the sun and for non-finite directions.

Five mutations of that code, one at a time, were run through this file and through test_gpu_spectral.py on an MI355X; the table with the row counts is in
docs/HISTORY.md, "known-answer tests of one PT_Spec shading step"."""
import numpy as np
import pytest

import oracle_api
import shade_spec_step_cases as cases
from ti_raytrace_amd import _native
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu

_live = {}


def device_scene(name):
    """(ex with its scene and spectral tables on device 0, orc, rows, the oracle's answers); one context per scene and process.  The device builds the
    RGB -> spectrum table (held bit for bit to the oracle's by test_gpu_spectral.py), the oracle gets the same arrays."""
    if name not in _live:
        if "table" not in _live:
            _live["table"] = _native.Context(0)          # (any context builds the same table; PT_Spec caches it per process)
        ex, orc, rows = cases.build(name, build_table=_live["table"].spec_table_build)
        ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
        word, _ = ex.scene.ctx.shade_features()
        assert word == cases.SCENES[name][1], (bin(word), bin(cases.SCENES[name][1]))
        _live[name] = (ex, orc, rows, orc.kat_shade_spec_step(rows))
    return _live[name]


PAIRS = [(name, feat) for name in sorted(cases.SCENES) for feat in cases.SCENES[name][2]]


@pytest.mark.parametrize("name,feat", PAIRS, ids=["%s-%d" % p for p in PAIRS])
def test_device_step_equals_oracle_step(gpu_ctx_ok, oracle_lib, name, feat):
    ex, orc, rows, want = device_scene(name)
    got = ex.scene.ctx.kat_shade_spec_step(feat, rows)
    assert got.shape == (rows.shape[0], _native.KAT_SPEC_STEP_OUT)
    report = cases.first_differences(got, want, rows, ex)
    assert not report, "%s on instantiation %d:\n%s" % (name, feat, "\n".join(report))
    assert int((want.view(np.int32)[:, 4] == 1).sum()) > 10000 and int(np.isnan(want[:, 0:4]).any(axis=1).sum()) > 100      # (the rows shade, and carry NaN)


@pytest.mark.parametrize("name", ["grid_mesh", "grid_sphere"])
def test_narrow_instantiation_equals_the_generic_one(gpu_ctx_ok, oracle_lib, name):
    """device against device, NaN payloads included: if this fails and the oracle comparison of one side holds, the other side moved"""
    ex, orc, rows, want = device_scene(name)
    narrow, generic = cases.SCENES[name][2]
    a = ex.scene.ctx.kat_shade_spec_step(narrow, rows)
    b = ex.scene.ctx.kat_shade_spec_step(generic, rows)
    bad = np.where((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%d rows differ between instantiation %d and %d, first: %s" % (
        bad.size, narrow, generic, "\n".join(cases.describe(rows, want, int(k), ex) for k in bad[:8]))


@pytest.mark.parametrize("name", ["grid_mesh", "grid_sphere"])
def test_step_follows_a_material_upload(gpu_ctx_ok, oracle_lib, name):
    """a permuted material table (Disney rows among themselves, emitter rows among themselves: the feature word stays): the same rows give the oracle's
    answers for the new table -- the material rows k_shade_spec reads and the light records were refreshed"""
    ex, orc, rows, want_before = device_scene(name)
    sc, ctx = ex.scene, ex.scene.ctx
    base = sc.material_np.copy()
    perm = base.copy()
    for kind in (SCD.MAT_DISNEY, SCD.MAT_LIGHT):
        idx = np.where(base[:, 0] == kind)[0]
        assert idx.size >= 2
        perm[idx] = base[np.roll(idx, 7 if idx.size > 7 else 1)]
    assert not np.array_equal(perm, base)
    narrow = cases.SCENES[name][2][0]
    W = cases.OUT_WORDS
    try:
        sc.material_np = perm
        orc2 = oracle_api.OracleScene(sc, ex.cam)
        assert orc2.lbvh_build() == sc.primitive_count - 1
        orc2.set_spectral(ex.integrator.tables())
        want = orc2.kat_shade_spec_step(rows)
        assert int((want[:, :W].view(np.uint32) != want_before[:, :W].view(np.uint32)).any(axis=1).sum()) > 10000      # (the new table matters)
        ctx.material_upload(perm)
        assert ctx.shade_features()[0] == cases.SCENES[name][1]
        for feat in cases.SCENES[name][2]:
            report = cases.first_differences(ctx.kat_shade_spec_step(feat, rows), want, rows, ex)
            assert not report, "%s after material_upload, instantiation %d:\n%s" % (name, feat, "\n".join(report))
    finally:
        sc.material_np = base
        ctx.material_upload(base)
    assert not cases.first_differences(ctx.kat_shade_spec_step(narrow, rows), want_before, rows, ex)


def test_refusals(gpu_ctx_ok, oracle_lib):
    """each an error code before anything is launched"""
    ex, orc, rows, want = device_scene("generic")
    ctx = ex.scene.ctx
    some = rows[:64]
    for feat in (_native.SF_LIGHT_SPHERE, _native.SF_LIGHT_TRI):                       # a narrow instantiation on a scene it does not cover
        with pytest.raises(_native.TirtError, match="cover"):
            ctx.kat_shade_spec_step(feat, some)
    for feat in (0, _native.SF_GLASS | _native.SF_ENV | _native.SF_LIGHT_SPHERE, 126, 128, 255):      # not an instantiation at all
        with pytest.raises(_native.TirtError, match="instantiation"):
            ctx.kat_shade_spec_step(feat, some)
    hit = np.where(some.view(np.float32)[:, 11] < cases.INF_VALUE)[0]
    assert hit.size
    for prim in (-1, ex.scene.primitive_count, 1 << 30, -(1 << 31)):
        bad = some.copy()
        bad[hit[-1], 14] = np.int64(prim).astype(np.int32).view(np.uint32)
        with pytest.raises(_native.TirtError, match="prim outside"):
            ctx.kat_shade_spec_step(_native.SF_ALL, bad)
    for pixel in (0x7fffffff, 0x80000000, 0xffffffff):
        bad = some.copy(); bad[0, 1] = pixel
        with pytest.raises(_native.TirtError, match="pixel outside"):
            ctx.kat_shade_spec_step(_native.SF_ALL, bad)
    with pytest.raises(_native.TirtError, match="stride"):
        _native.kat_shade_spec_step(ctx.handle, _native.SF_ALL, some, in_stride=22)
    with pytest.raises(_native.TirtError, match="stride"):
        _native.kat_shade_spec_step(ctx.handle, _native.SF_ALL, some, out_stride=28)
    # a context with a scene and no spectral tables, and one without a scene
    probe = cases.rgb.grid_sphere()
    cases.rgb.common.host_only(probe)
    probe.integrator.setup_data_cpu(); probe.integrator.setup_data_gpu(); probe.scene.setup_data_gpu()
    with pytest.raises(_native.TirtError, match="spectral tables"):
        probe.scene.ctx.kat_shade_spec_step(_native.SF_ALL, some[some.view(np.float32)[:, 11] >= cases.INF_VALUE])
    empty = _native.Context(0)
    try:
        with pytest.raises(_native.TirtError, match="no scene"):
            empty.kat_shade_spec_step(_native.SF_ALL, some)
    finally:
        empty.close()
    miss = some.copy()                                                               # a miss may carry any prim word
    miss.view(np.float32)[:, 11] = np.inf; miss[:, 14] = 0xffffffff
    assert not cases.first_differences(ctx.kat_shade_spec_step(_native.SF_ALL, miss), orc.kat_shade_spec_step(miss), miss, ex)
    assert not cases.first_differences(ctx.kat_shade_spec_step(_native.SF_ALL, some), want[:64], some, ex)      # and the context still works
