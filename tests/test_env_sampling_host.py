"""The environment's sampling table, its inverse and its pdf as the restatement states them (tests/env_sampling_expected.py; include/tirt.h, "Importance
sampling of the environment"): properties that need no device, and the refusals that need none."""
import os

import numpy as np
import pytest

import env_sampling_expected as ee
from ti_raytrace_amd import _native, PT_RGB, Example, Texture
from ti_raytrace_amd import SceneData as SCD

f = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def packed(rgb):
    t = Texture.Texture(); t.load_array(rgb)
    return t.np_img


def random_sky(w, h, seed, lo=1):
    return np.random.RandomState(seed).randint(lo, 256, (h, w, 3)).astype(np.uint8)


SKIES = {"1x1": random_sky(1, 1, 1), "2x1": random_sky(2, 1, 2), "7x5": random_sky(7, 5, 3, lo=0), "sun": ee.sun_sky()}


@pytest.mark.parametrize("name", sorted(SKIES))
def test_cell_weights_sum_to_total_exactly(name):
    tab = ee.table(packed(SKIES[name]))
    assert tab is not None
    assert int(tab["q"].astype(object).sum()) == tab["total"] == int(tab["marginal"][-1])
    assert np.array_equal(tab["row_sums"][:, -1], np.diff(np.concatenate([[0], tab["marginal"]]).astype(np.uint64)))
    assert tab["q"].max() <= 1 << 24
    assert tab["q"].shape == (tab["h"], tab["w"])


def test_sun_cells_carry_the_sun():
    """the four cells whose lookup mixes the bright texel hold most of the table: the 255 texel is 30 x the floor in 8 bits, ~480 x in linear light"""
    tab = ee.table(packed(ee.sun_sky()))
    q = tab["q"].astype(np.float64)
    top4 = np.sort(q.reshape(-1))[-4:].sum()
    assert top4 / q.sum() > 0.5


@pytest.mark.parametrize("name", ["7x5", "sun", "2x1"])
def test_inverse_lands_in_the_sampled_cell(name):
    """directions of samples whose within-cell offsets lie in [0.05, 0.95] are looked up in the cell they were drawn from, and carry its pdf"""
    tab = ee.table(packed(SKIES[name]))
    r = np.random.RandomState(5)
    ra, rb = r.randint(0, 1 << 24, 3000).astype(f) / f(1 << 24), r.randint(0, 1 << 24, 3000).astype(f) / f(1 << 24)
    i, j, tx, ty, d = ee.sample(tab, ra, rb)
    assert (tab["q"][j, i] > 0).all()                                        # a cell of weight 0 is never drawn
    offx, offy = tx * f(tab["w"]) - i, ty * f(tab["h"]) - j
    inner = (offx >= 0.05) & (offx <= 0.95) & (offy >= 0.05) & (offy <= 0.95)
    assert inner.sum() > 1500
    li, lj, ltx, lty, p = ee.pdf(tab, d)
    assert np.array_equal(li[inner], i[inner]) and np.array_equal(lj[inner], j[inner])
    assert np.abs(ltx - tx)[inner].max() < 1e-5 and np.abs(lty - ty)[inner].max() < 1e-5
    assert (p[inner] > 0).all()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_edge_randoms():
    tab = ee.table(packed(SKIES["7x5"]))
    top = f(1.0) - f(2.0 ** -24)
    i, j, tx, ty, d = ee.sample(tab, [0.0, top, 0.0, top], [0.0, 0.0, top, top])
    nz_rows = np.where(tab["row_sums"][:, -1] > 0)[0]
    assert j[0] == nz_rows[0] and j[1] == nz_rows[-1]
    assert (tx >= 0).all() and (tx <= 1).all() and (ty >= 0).all() and (ty <= 1).all()
    assert np.isfinite(d).all()


def test_mean_of_inverse_pdf_is_the_sphere():
    """mean(1 / pdf) over 256 x 256 stratified samples of a strictly positive table estimates the measure of the sampled domain, 4 pi, within 4 of its
    own standard errors.  Recorded: 7 x 5 random sky (texels 1..255), mean 12.567183 against 4 pi = 12.566371, standard error 0.020964."""
    tab = ee.table(packed(random_sky(7, 5, 11)))
    assert (tab["q"] > 0).all()
    n = 256
    r = np.random.RandomState(9)
    ka = (np.arange(n)[:, None] * (1 << 16) + r.randint(0, 1 << 16, (n, n))).reshape(-1)
    kb = (np.arange(n)[None, :] * (1 << 16) + r.randint(0, 1 << 16, (n, n))).reshape(-1)
    _, _, _, _, d = ee.sample(tab, ka.astype(f) / f(1 << 24), kb.astype(f) / f(1 << 24))
    p = ee.pdf(tab, d)[4].astype(np.float64)
    assert (p > 0).all()
    inv = 1.0 / p
    mean, se = inv.mean(), inv.std(ddof=1) / np.sqrt(inv.size)
    print("mean(1/pdf) = %.6f, 4 pi = %.6f, standard error %.6f" % (mean, 4 * np.pi, se))
    assert abs(mean - 4 * np.pi) <= 4 * se, (mean, se)


def test_no_table_for_black_or_unlit():
    assert ee.table(packed(np.zeros((4, 8, 3), np.uint8))) is None
    assert ee.table(packed(SKIES["sun"]), power=0.0) is None
    one = ee.table(packed(SKIES["1x1"]))
    assert one["q"].shape == (1, 1) and one["total"] == int(one["q"][0, 0]) > 0
    i, j, tx, ty, d = ee.sample(one, [0.25], [0.75])
    assert (i[0], j[0]) == (0, 0) and tx[0] == f(0.75) and ty[0] == f(0.25)
    two = ee.table(packed(SKIES["2x1"]))
    assert two["q"].shape == (1, 2)


def test_pdf_is_zero_at_the_poles():
    tab = ee.table(packed(SKIES["7x5"]))
    p = ee.pdf(tab, np.array([[0, 1, 0], [0, -1, 0], [1e-7, 1, 0]], f))[4]
    assert (p == 0).all()


def test_host_feature_word_with_the_switch():
    material = np.zeros((1, 10), np.float32)
    primitive = np.array([[1, 0, 0]], np.int32); shape = np.zeros((1, 10), np.float32); light = np.zeros(1, np.int32)
    args = (material, primitive, shape, light, 0)
    sun, black = packed(SKIES["sun"]), packed(np.zeros((2, 2, 3), np.uint8))
    base = _native.shade_features_host(*args, env=sun, env_power=2.0)
    assert base & _native.SF_ENV and not base & _native.SF_ENV_SAMPLE
    assert _native.shade_features_host_env(*args, env=sun, env_power=2.0, env_sampling=False) == base
    assert _native.shade_features_host_env(*args, env=sun, env_power=2.0, env_sampling=True) == base | _native.SF_ENV_SAMPLE
    assert not _native.shade_features_host_env(*args, env=sun, env_power=0.0, env_sampling=True) & _native.SF_ENV_SAMPLE
    assert not _native.shade_features_host_env(*args, env=black, env_power=2.0, env_sampling=True) & _native.SF_ENV_SAMPLE
    assert not _native.shade_features_host_env(*args, env=None, env_power=2.0, env_sampling=True) & _native.SF_ENV_SAMPLE


@pytest.mark.parametrize("share", [0.0, 1.0, -0.5, 1.5, float("nan")])
def test_share_outside_the_open_interval_is_refused(share):
    with pytest.raises(_native.TirtError, match="share"):
        _native.env_sampling(None, 1, share)
    ex = Example.example(16, 12, 4, 0)
    with pytest.raises(ValueError, match="env_share"):
        PT_RGB.PathTrace(16, 12, ex.cam, ex.scene, 64, env_sampling=True, env_share=share)


def test_switch_needs_a_context_after_its_arguments():
    with pytest.raises(_native.TirtError, match="null context"):
        _native.env_sampling(None, 1, 0.5)
    L = _native.lib()
    assert L.tirt_env_sampling(None, 2, 0.5) == -2 and b"0 or 1" in L.tirt_last_error()


def test_add_env_takes_an_array():
    ex = Example.example(16, 12, 4, 0)
    ex.scene.add_env(SKIES["sun"], 20.0)
    assert ex.scene.env.np_img.shape == (16, 8) and ex.scene.env_power == 20.0
    assert np.array_equal(ex.scene.env.np_img, packed(SKIES["sun"]))
    with pytest.raises(ValueError, match="uint8"):
        ex.scene.add_env(SKIES["sun"].astype(np.float32), 1.0)


@pytest.mark.parametrize("metal,consistent", [(1.0, True), (0.0, False)])
def test_where_the_reference_sampler_draws_from_its_stated_pdf(metal, consistent):
    """Why the environment sample carries the ratio of the drawn to the stated density (include/tirt.h, step 5).  For directions L drawn by Disney.sample, mean(cos / pdf(L)) over the draws with pdf > 0 estimates the integral
    of cos over the hemisphere, pi, exactly when the draws have the density the pdf states.  Measured with the oracle's functions, 20 000 draws, roughness 0.8,
    incidence 0.6 rad: metallic 1 gives 3.14 +- 0.03; metallic 0 gives 2.33 +- 0.01 -- there the switch-off estimator (BSDF sampling weighted by 1 / pdf) is
    a quarter darker than the plain integral of f * cos * L: it converges to the integral of (drawn / stated) * f * cos * L, and a light sample has to estimate that
    integrand to agree with it.  The diffuse lobe is drawn by cos / pi and stated as 1 / pi: drawn = stated + 0.5 * (1 - metallic) / pi * (cos - 1)."""
    import oracle_api as oa
    import shade_step_cases as cases
    L = oa.load()
    ex = Example.example(8, 8, 4, 0)
    ex.scene.add_mesh(np.array([[[0, 0, 0], [1, 0, 0], [0, 0, 1]]], float), cases.disney(metal, 0.8, (0.7, 0.7, 0.7)))
    ex.add_sphere_light(); ex.scene.setup_data_cpu()
    row = np.ascontiguousarray(ex.scene.material_np[0], f)
    N, d = np.array([0, 1, 0], f), np.array([np.sin(0.6), -np.cos(0.6), 0], f)
    r = np.random.RandomState(1).rand(20000, 3).astype(f)
    vals = np.zeros(r.shape[0])
    out, ev = np.zeros(3, f), np.zeros(2, f)
    for k in range(r.shape[0]):
        L.orc_kat_disney_sample(row, d, N, r[k].copy(), out)
        L.orc_kat_disney(row, N, (-d).astype(f), out.copy(), ev)
        vals[k] = out[1] / ev[1] if ev[1] > 0 else 0.0
    mean, se = vals.mean(), vals.std(ddof=1) / np.sqrt(vals.size)
    print("metallic %.0f: mean(cos / pdf) = %.4f +- %.4f, pi = %.4f" % (metal, mean, se, np.pi))
    assert (abs(mean - np.pi) <= 4 * se) == consistent, (mean, se)
