"""The oracle's spectral shading step (oracle.c, pt_spec_step / orc_kat_shade_spec_step) and the rows the step tests feed it (tests/shade_spec_step_cases.py),
without a GPU: the step chained with the oracle's traversal and AddSplat IS the oracle's PT_Spec renderer, every branch a scene can reach is taken by at least 100
of its rows, the hero wavelengths reach both ends of their range, and the device entry point refuses bad arguments before it needs a device.

The issue that asked for these tests wanted rows with `Lambda + 300` within one table step of 830 nm.  No row can have that: Lambda = 360 + 100 * rand with
rand < 1 (HeroSample.py:5-8: four wavelengths 100 nm apart from [360, 460)), so the longest wavelength a path carries is below 760 nm.  What is asserted instead is
the end of the range that exists: rows with Lambda + 300 within 1 nm (the step of the observer's and the illuminant's tables) of 760 -- beyond the tabulated
reflectances (380 .. 755 nm) and beyond the sky model (720 nm) --, and rows with Lambda within 1 nm of 360, below the tabulated reflectances."""
import numpy as np
import pytest

import oracle_api
import shade_spec_step_cases as cases
from test_shade_step_host import camera_rays
from ti_raytrace_amd import _native
from ti_raytrace_amd import SceneData as SCD

SSB = oracle_api.SSB


def chained_film(orc, cam, W, H, frame, seed):
    """pt_spec_pixel's loop and AddSplat in Python: closest hit -> step -> shadow test -> next ray for every pixel of one frame, then orc_kat_spec 9 on a cleared film"""
    n = W * H
    o, d = camera_rays(orc, cam, W, H, frame, seed)
    thr = np.ones((n, 4), np.float32); rad = np.zeros((n, 4), np.float32)
    live = np.arange(n)
    final = np.zeros((n, 4), np.float32)
    for depth in range(cases.MAX_DEPTH):
        if live.size == 0:
            break
        m = live.size
        out, prim, _, bary = orc.closest_hit(np.concatenate([o, d], axis=1), uv=True)
        rows = np.zeros((m, cases.IN_WORDS), np.uint32)
        f = rows.view(np.float32)
        rows[:, 0] = seed; rows[:, 1] = live; rows[:, 2] = frame; rows[:, 3] = depth; rows[:, 4] = depth == cases.MAX_DEPTH - 1
        f[:, 5:8] = o; f[:, 8:11] = d; f[:, 11] = out[:, 0]; f[:, 12] = bary[:, 0]; f[:, 13] = bary[:, 1]
        rows[:, 14] = prim.view(np.uint32)
        f[:, 15:19] = thr; f[:, 19:23] = rad
        st = orc.kat_shade_spec_step(rows)
        si = st.view(np.int32)
        rad = st[:, 0:4].copy()
        sh = np.where(si[:, 16] == 1)[0]
        if sh.size:
            _, sprim, _ = orc.shadow_hit(np.ascontiguousarray(st[sh, 17:23]))
            add = sh[sprim == si[sh, 27]]
            with np.errstate(invalid="ignore", over="ignore"):
                rad[add] = rad[add] + st[add, 23:27]
        go = si[:, 5] == 1
        final[live[~go]] = rad[~go]
        live = live[go]
        o, d, thr, rad = st[go, 6:9].copy(), st[go, 9:12].copy(), st[go, 12:16].copy(), rad[go]
    assert live.size == 0
    f32 = np.float32
    lam = cases.hero_lambda(orc, np.stack([np.full(n, seed), np.arange(n), np.full(n, frame)], axis=1).astype(np.uint32))
    coff = f32(1.0) / (f32(frame) + f32(1.0))
    splat = np.concatenate([final, lam[:, None], np.full((n, 1), coff, f32), np.zeros((n, 3), f32)], axis=1)
    return orc.kat_spec(9, splat, 3).reshape(W, H, 3)


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_the_step_is_the_renderer(oracle_lib, name):
    """orc_kat_shade_spec_step + orc_closest_hit_uv_batch + orc_shadow_hit_batch + AddSplat chained in Python give the pixels of orc_pt_spec_render bit for bit"""
    ex, orc = cases.host_scene(name)
    W, H = cases.FILM_W, cases.FILM_H
    for frame, seed in ((0, 1), (3, 1), (1, 77)):
        want, _ = orc.spec_render(W, H, frame, 1, seed=seed, max_depth=cases.MAX_DEPTH)
        got = chained_film(orc, ex.cam, W, H, frame, seed)
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        assert np.array_equal(nan_w, nan_g), (name, frame, int(nan_w.sum()), int(nan_g.sum()))
        same = want.view(np.uint32)[~nan_w] == got.view(np.uint32)[~nan_w]
        assert same.all(), "%s frame %d: %d values differ" % (name, frame, int((~same).sum()))
        assert np.isfinite(want).any() and float(np.abs(np.nan_to_num(want, posinf=0.0, neginf=0.0)).sum()) > 0.0


MISS = ("miss_finite", "miss_nonfinite", "miss_below")
WITH_LIGHTS = ("emit_front", "emit_back", "nee", "nee_nopdf", "nee_reject")
# the branch bits each scene permits, written out (not derived from what the rows give)
EXPECTED_BRANCHES = {
    "grid_sphere": WITH_LIGHTS + ("end_pdf", "end_thr", "light_sphere") + MISS,
    "grid_mesh": WITH_LIGHTS + ("end_pdf", "end_thr", "light_tri") + MISS,
    "generic": WITH_LIGHTS + ("end_pdf", "end_thr", "glass_reflect", "glass_refract", "light_tri", "light_sphere", "light_spot", "light_laser") + MISS,
    "sky_only": ("end_pdf", "end_thr") + MISS,
}


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_no_branch_is_vacuous(oracle_lib, name):
    """every branch the scene can reach is taken by at least 100 rows, and no row takes a branch the scene cannot reach"""
    ex, orc, rows = cases.build(name)
    word = _native.shade_features_host(ex.scene.material_np, ex.scene.primitive_np, ex.scene.shape_np, ex.scene.light_np, ex.scene.light_count,
                                       env=ex.scene.env.np_img, env_power=ex.scene.env_power)
    assert word == cases.SCENES[name][1], (bin(word), bin(cases.SCENES[name][1]))
    assert 20000 <= rows.shape[0] <= 120000, rows.shape
    want = orc.kat_shade_spec_step(rows)
    branch = want.view(np.uint32)[:, cases.BRANCH_WORD]
    counts = {b: int(((branch & bit) != 0).sum()) for b, bit in SSB.items()}
    print(name, rows.shape[0], counts)
    for b in EXPECTED_BRANCHES[name]:
        assert counts[b] >= 100, (name, b, counts[b])
    for b in SSB:
        if b not in EXPECTED_BRANCHES[name]:
            assert counts[b] == 0, (name, b, counts[b])
    f = rows.view(np.float32)
    hit = f[:, 11] < cases.INF_VALUE
    # the material grid: at least 30 Disney materials are hit in the grid scenes
    if name.startswith("grid"):
        mats = np.unique(ex.scene.primitive_np[rows.view(np.int32)[hit, 14], 2])
        assert (ex.scene.material_np[mats, 0] == SCD.MAT_DISNEY).sum() >= 30
    # the hero wavelengths reach both ends of their range (module docstring: why 760 and not 830)
    lam = cases.hero_lambda(orc, rows)
    assert lam.min() >= 360.0 and lam.max() < 460.0
    assert int((lam < 361.0).sum()) >= 100 and int((lam + np.float32(300.0) > 759.0).sum()) >= 100, (int((lam < 361.0).sum()), int((lam + 300.0 > 759.0).sum()))
    # the states the continuation test is about: channels 0..2 dead and channel 3 alive, the reverse, a NaN in exactly one of the three
    thr = f[:, 15:19]
    shaded = want.view(np.int32)[:, 4] == 1
    dead3 = (thr[:, 0:3] == 0.0).all(axis=1) & (thr[:, 3] > 0.0)
    for sel in (dead3, (thr[:, 0:3] > 0.0).all(axis=1) & (thr[:, 3] == 0.0)) + tuple(np.isnan(thr[:, k]) & (np.isnan(thr[:, 0:3]).sum(axis=1) == 1) for k in range(3)):
        assert int((sel & shaded).sum()) >= 100
    # ... and a throughput dead in 0..2 ends the path whatever channel 3 holds
    assert ((branch[dead3 & shaded] & SSB["end_thr"]) != 0).all()
    # emitters: the zero direction makes fCosTheta exactly +-0, which is not a front hit
    if "emit_back" in EXPECTED_BRANCHES[name]:
        light = np.zeros(rows.shape[0], bool)
        light[hit] = ex.scene.material_np[ex.scene.primitive_np[rows.view(np.int32)[hit, 14], 2], 0] == SCD.MAT_LIGHT
        zero = light & (f[:, 8:11] == 0.0).all(axis=1)
        assert int(zero.sum()) >= 100 and (branch[zero] == SSB["emit_back"]).all()
        assert np.array_equal(want.view(np.uint32)[zero, 0:4], rows[zero, 19:23])            # the radiance passes through, bit for bit


def test_rows_are_deterministic(oracle_lib):
    a = cases.build("sky_only")[2]
    cases._cache.clear()
    b = cases.build("sky_only")[2]
    assert a.shape == b.shape and np.array_equal(a, b)


def test_oracle_refuses_a_row_without_a_primitive(oracle_lib):
    ex, orc, rows = cases.build("sky_only")
    bad = rows[:4].copy()
    bad.view(np.float32)[:, 11] = 1.0
    bad[2, 14] = np.uint32(ex.scene.primitive_count)
    with pytest.raises(ValueError):
        orc.kat_shade_spec_step(bad)
    bad[2, 14] = np.uint32(0xffffffff)
    with pytest.raises(ValueError):
        orc.kat_shade_spec_step(bad)


def test_entry_point_refuses_bad_strides_and_feature_words_without_a_device():
    """tirt_kat_shade_spec_step checks what needs no context first: these refusals come back before a context is touched (a null one here)"""
    rows = np.zeros((4, _native.KAT_SPEC_STEP_IN), np.uint32)
    rows.view(np.float32)[:, 11] = 2.0e6
    for kwargs, word in (({"in_stride": 22}, "stride"), ({"out_stride": 28}, "stride")):
        with pytest.raises(_native.TirtError, match=word):
            _native.kat_shade_spec_step(None, _native.SF_ALL, rows, **kwargs)
    for feat in (0, _native.SF_GLASS | _native.SF_ENV | _native.SF_LIGHT_SPHERE, _native.SF_LIGHT_SPHERE | _native.SF_LIGHT_TRI, 128, 255, 0xffffffff):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_spec_step(None, feat, rows)
    for feat in (_native.SF_LIGHT_SPHERE, _native.SF_LIGHT_TRI, _native.SF_ALL):                 # the three real ones get as far as the context
        with pytest.raises(_native.TirtError, match="null context"):
            _native.kat_shade_spec_step(None, feat, rows)
