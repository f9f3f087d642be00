"""The oracle's shading step (oracle.c, pt_rgb_step / orc_kat_shade_step) and the rows the step tests feed it (tests/shade_step_cases.py), without a GPU:
the step chained with the oracle's traversal IS the oracle's renderer, every branch a scene can reach is taken by at least 100 of its rows, and the
device entry point refuses bad arguments before it needs a device."""
import ctypes as C

import numpy as np
import pytest

import oracle_api
import shade_step_cases as cases
from ti_raytrace_amd import _native

SB = oracle_api.SB


def camera_rays(orc, cam, W, H, frame, seed):
    """Camera.py:122-142 in float32, with the frame's jitter (oracle.c pt_rgb_pixel, k_generate)"""
    f = np.float32
    pix = np.arange(W * H)
    ii, jj = pix // H, pix % H
    jx = np.zeros(W * H, f); jy = np.zeros(W * H, f)
    if frame != 0:
        jx = np.array([orc.L.orc_kat_rand(seed, int(p), frame, 0) for p in pix], f) - f(0.5)
        jy = np.array([orc.L.orc_kat_rand(seed, int(p), frame, 1) for p in pix], f) - f(0.5)
    x = ((ii.astype(f) + jx) - f(cam.cx)) / f(cam.fx)
    y = ((jj.astype(f) + jy) - f(cam.cy)) / f(cam.fy)
    z = np.full_like(x, -1.0)
    M = cam.view_inv_np[0].astype(f)
    w = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] * f(0.0) for r in range(3)]
    inv = f(1.0) / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    d = np.stack([w[0] * inv, w[1] * inv, w[2] * inv], axis=1).astype(f)
    return np.broadcast_to(cam.eye_np[0].astype(f), d.shape).copy(), d


def chained_radiance(orc, cam, W, H, frame, seed):
    """pt_rgb_pixel's loop in Python: closest hit -> step -> shadow test -> next ray, for every pixel of one frame"""
    n = W * H
    o, d = camera_rays(orc, cam, W, H, frame, seed)
    thr = np.ones((n, 3), np.float32); rad = np.zeros((n, 3), np.float32); pdf = np.ones(n, np.float32); spec = np.ones(n, np.uint32)
    live = np.arange(n)
    final = np.zeros((n, 3), np.float32)
    for depth in range(cases.MAX_DEPTH):
        if live.size == 0:
            break
        m = live.size
        out, prim, _, bary = orc.closest_hit(np.concatenate([o, d], axis=1), uv=True)
        head = np.zeros((m, 5), np.uint32)
        head[:, 0] = seed; head[:, 1] = live; head[:, 2] = frame; head[:, 3] = depth; head[:, 4] = depth == cases.MAX_DEPTH - 1
        rows = cases.pack(head, o, d, out[:, 0], bary[:, 0], bary[:, 1], prim, np.concatenate([thr, rad, pdf[:, None]], axis=1), spec)
        st = orc.kat_shade_step(rows)
        si = st.view(np.int32)
        rad = st[:, 0:3].copy()
        sh = np.where(si[:, 16] == 1)[0]
        if sh.size:
            _, sprim, _ = orc.shadow_hit(np.ascontiguousarray(st[sh, 17:23]))
            add = sh[sprim == si[sh, 26]]
            rad[add] = rad[add] + st[add, 23:26]
        go = si[:, 4] == 1
        final[live[~go]] = rad[~go]
        live = live[go]
        o, d, thr, pdf, spec, rad = st[go, 5:8].copy(), st[go, 8:11].copy(), st[go, 11:14].copy(), st[go, 14].copy(), si[go, 15].astype(np.uint32), rad[go]
    assert live.size == 0
    return final


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_the_step_is_the_renderer(oracle_lib, name):
    """orc_kat_shade_step + orc_closest_hit_batch + orc_shadow_hit_batch chained in Python give the pixels of orc_pt_rgb_render bit for bit"""
    ex, orc = cases.host_scene(name)
    W, H = cases.FILM_W, cases.FILM_H
    f32 = np.float32
    for frame, seed in ((0, 1), (3, 1), (1, 77)):
        want, _ = orc.render(W, H, frame, 1, seed=seed)
        rad = chained_radiance(orc, ex.cam, W, H, frame, seed).reshape(W, H, 3)
        coff = f32(1.0) / (f32(frame) + f32(1.0))
        with np.errstate(invalid="ignore", over="ignore"):
            got = rad * coff + np.zeros_like(rad) * (f32(1.0) - coff)            # PT_RGB.py:134-136 on a cleared film
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        assert np.array_equal(nan_w, nan_g), (name, frame, int(nan_w.sum()), int(nan_g.sum()))
        same = want.view(np.uint32)[~nan_w] == got.view(np.uint32)[~nan_w]
        assert same.all(), "%s frame %d: %d values differ" % (name, frame, int((~same).sum()))
        assert np.isfinite(want).any() and float(np.nan_to_num(want, posinf=0.0).sum()) > 0.0


COMMON_DISNEY = ("lobe_diffuse", "lobe_specular", "end_pdf", "miss_finite", "miss_nonfinite")
WITH_LIGHTS = ("emit_mis", "emit_spec", "nee", "nee_nopdf", "nee_reject")
# the branch bits each scene's feature word permits, written out (not derived from what the rows give)
EXPECTED_BRANCHES = {
    "grid_sphere": COMMON_DISNEY + WITH_LIGHTS + ("light_sphere",),
    "grid_mesh": COMMON_DISNEY + WITH_LIGHTS + ("light_tri",),
    "generic": COMMON_DISNEY + WITH_LIGHTS + ("glass_reflect", "glass_refract", "extinct", "light_tri", "light_sphere", "light_spot", "light_laser"),
    "env_only": COMMON_DISNEY,
}


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_no_branch_is_vacuous(oracle_lib, name):
    """every branch the scene can reach is taken by at least 100 rows, and no row takes a branch the scene cannot reach"""
    ex, orc, rows = cases.build(name)
    word = _native.shade_features_host(ex.scene.material_np, ex.scene.primitive_np, ex.scene.shape_np, ex.scene.light_np, ex.scene.light_count,
                                       env=ex.scene.env.np_img, env_power=ex.scene.env_power)
    assert word == cases.SCENES[name][1], (bin(word), bin(cases.SCENES[name][1]))
    assert 60000 <= rows.shape[0] <= 200000, rows.shape
    branch = orc.kat_shade_step(rows).view(np.uint32)[:, 28]
    counts = {b: int(((branch & bit) != 0).sum()) for b, bit in SB.items()}
    print(name, rows.shape[0], counts)
    for b in EXPECTED_BRANCHES[name]:
        assert counts[b] >= 100, (name, b, counts[b])
    for b in SB:
        if b not in EXPECTED_BRANCHES[name]:
            assert counts[b] == 0, (name, b, counts[b])
    # the material grid: at least 30 Disney materials are hit in the grid scenes
    if name.startswith("grid"):
        f = rows.view(np.float32)
        hit = f[:, 11] < cases.INF_VALUE
        mats = np.unique(ex.scene.primitive_np[rows.view(np.int32)[hit, 14], 2])
        assert (ex.scene.material_np[mats, 0] == 0.0).sum() >= 30


def test_rows_are_deterministic(oracle_lib):
    a = cases.build("env_only")[2]
    cases._cache.clear()
    b = cases.build("env_only")[2]
    assert a.shape == b.shape and np.array_equal(a, b)


def test_oracle_refuses_a_row_without_a_primitive(oracle_lib):
    ex, orc, rows = cases.build("env_only")
    bad = rows[:4].copy()
    bad.view(np.float32)[:, 11] = 1.0
    bad[2, 14] = np.uint32(ex.scene.primitive_count)
    with pytest.raises(ValueError):
        orc.kat_shade_step(bad)


def test_entry_point_refuses_bad_strides_and_feature_words_without_a_device():
    """tirt_kat_shade_step checks what needs no context first: these refusals come back before a context is touched (a null one here)"""
    rows = np.zeros((4, _native.KAT_STEP_IN), np.uint32)
    rows.view(np.float32)[:, 11] = 2.0e6
    for kwargs, word in (({"in_stride": 22}, "stride"), ({"out_stride": 27}, "stride")):
        with pytest.raises(_native.TirtError, match=word):
            _native.kat_shade_step(None, _native.SF_ALL, rows, **kwargs)
    for feat in (0, _native.SF_GLASS | _native.SF_ENV | _native.SF_LIGHT_SPHERE, _native.SF_LIGHT_SPHERE | _native.SF_LIGHT_TRI, 128, 0xffffffff):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)
    for feat in _native.SHADE_INSTANTIATIONS:                 # the three real ones get as far as the context
        with pytest.raises(_native.TirtError, match="null context"):
            _native.kat_shade_step(None, feat, rows)
