"""The definition of the emitter choice by power (include/tirt.h, "Choosing emitters by power") on its numpy restatement: bounds, scale invariance, the exact
inverse, the probabilities, and -- with a small direct-lighting estimator on scenes.lamp_and_embers -- that the choice changes the variance, not the mean."""
import numpy as np
import pytest

import common
import light_sampling_expected as le
import oracle_api
from ti_raytrace_amd import scenes

f = np.float32


def areas(n, seed):
    return (np.random.RandomState(seed).rand(n) * 2.0 + 0.01).astype(f)


def grey(e):
    e = np.asarray(e, f).reshape(-1)
    return np.stack([e, e, e], axis=1)


def test_bounds():
    rng = np.random.RandomState(1)
    em = grey(np.exp(rng.uniform(-20, 20, 5000)))
    tab = le.table(em, areas(5000, 2))
    assert tab["q"].max() <= 1 << 24 and tab["q"].min() >= 1
    assert tab["q"].max() >= 1 << 23                                      # the largest weight uses the top bit of the scale
    assert tab["total"] == int(tab["q"].astype(object).sum()) and tab["total"] < 1 << 64
    # the bound of the sums: 2^31 entries of 2^24 stay below 2^64
    assert (1 << 31) * (1 << 24) < 1 << 64
    # a light at 2^-30 of the maximum still gets q = 1; one that takes no part gets 0
    tab = le.table(grey([1.0, 2.0 ** -30, 0.0, -3.0, np.nan, np.inf, 2.0 ** -140]), np.ones(7, f))
    assert tab["q"].tolist() == [1 << 23, 1, 0, 0, 0, 0, 1] and tab["e_max"] == 1
    # a degenerate triangle's NaN area, an infinite area, a zero area
    tab = le.table(grey([1.0, 1.0, 1.0, 1.0]), np.array([np.nan, np.inf, 0.0, 0.5], f))
    assert tab["q"].tolist() == [0, 0, 0, 1 << 23]
    # nothing takes part: no table
    tab = le.table(grey([0.0, -1.0]), np.ones(2, f))
    assert tab["total"] == 0 and (tab["P"] == 0).all()


@pytest.mark.parametrize("k", [-40, -3, 1, 17, 60])
def test_scaling_every_emission_by_a_power_of_two_gives_the_same_table(k):
    rng = np.random.RandomState(3)
    em = rng.uniform(0.0, 8.0, (300, 3)).astype(f)
    em[::7] = 0
    ar = areas(300, 4)
    a, b = le.table(em, ar, 0.25), le.table(np.ldexp(em, k).astype(f), ar, 0.25)
    assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["prefix"], b["prefix"]) and b["e_max"] == a["e_max"] + k
    assert np.array_equal(a["P"].view(np.uint32), b["P"].view(np.uint32))


@pytest.mark.parametrize("name,q", [("one", [5]), ("two", [1, 3]), ("zeros", [0, 4, 0, 0, 9, 0]), ("equal", [7] * 5), ("big", [1 << 24, 1, 1]), ("odd", [3, 1, 4, 1, 5, 9, 2, 6])])
def test_pick_is_the_exact_inverse(name, q):
    """every k in [0, 2^24) lands in the entry whose integer interval holds floor(k * total / 2^24)"""
    q = np.array(q, np.uint64)
    prefix = np.cumsum(q, dtype=np.uint64)
    total = int(prefix[-1])
    tab = {"n": q.shape[0], "q": q.astype(np.uint32), "prefix": prefix, "total": total, "u": f(0.0)}
    k = np.arange(1 << 24, dtype=np.uint64)
    r = (k.astype(f) / f(1 << 24)).astype(f)
    idx, P, uni = le.pick(tab, r)
    t = (k * np.uint64(total)) >> np.uint64(24)
    lo = np.concatenate([[0], prefix[:-1]]).astype(np.uint64)
    assert not uni.any()
    assert (t >= lo[idx]).all() and (t < prefix[idx]).all() and (q[idx] > 0).all()
    # every entry with a weight is reached, in proportion: its count of k is q / total of 2^24 to within one
    counts = np.bincount(idx, minlength=q.shape[0])
    assert (np.abs(counts - q.astype(np.float64) / total * (1 << 24)) <= 1.0).all()


def test_probabilities_sum_to_one():
    rng = np.random.RandomState(5)
    for n, u in ((1, 0.0), (2, 0.0), (65, 0.25), (1000, 0.0), (1000, 0.5), (5000, float(f(1.0) - f(2.0 ** -24)))):
        tab = le.table(grey(np.exp(rng.uniform(-8, 8, n))), areas(n, n), u)
        s = float(tab["P"].astype(np.float64).sum())
        assert abs(s - 1.0) <= (n + 2) * 2.0 ** -24, (n, u, s)             # each P is a handful of f32 roundings of a value <= 1
        assert (tab["P"] > 0).all()
    # the uniform share reaches what the weights do not
    tab = le.table(grey([1.0, 0.0, 1.0]), np.ones(3, f), 0.25)
    assert tab["P"][1] == f(f(0.25) / f(3.0)) and tab["q"][1] == 0
    idx, P, uni = le.pick(tab, np.array([0.0, 0.1, 0.2, 0.24, 0.25, 0.9], f))
    assert idx.tolist() == [0, 1, 2, 2, 0, 2] and uni.tolist() == [True] * 4 + [False] * 2


def lamp_scene(metallic=1.0):
    ex = scenes.lamp_and_embers(16, 12, 4, 0, metallic=metallic)
    ex.scene.setup_data_cpu()
    ex.frame_camera()
    return ex


def test_lamp_and_embers_is_what_the_feature_is_for():
    ex = lamp_scene()
    sc = ex.scene
    assert sc.light_count == 256
    tab = le.table(*le.scene_lists(sc))
    lamp = float(tab["q"][:2].astype(np.float64).sum()) / tab["total"]
    assert lamp > 0.95, lamp
    assert (tab["q"][2:] >= 1).all() and tab["P"][:2].sum() > 0.95 and 2.0 / sc.light_count < 0.01


def test_choice_changes_the_variance_not_the_mean():
    """direct light on three ground points under uniform and under power choice: equal means within 4 standard errors, a smaller variance under power"""
    sc = lamp_scene().scene
    em, ar = le.scene_lists(sc)
    power = le.table(em, ar)
    uniform = dict(power); uniform["P"] = np.full(power["n"], 1.0 / power["n"], f)
    count = 200000
    for k, point in enumerate(((0.0, 0.0, 0.0), (1.2, 0.0, -0.7), (-1.6, 0.0, 1.5))):
        a = le.direct_light_samples(sc, uniform, point, (0.0, 1.0, 0.0), count, 10 + k)
        b = le.direct_light_samples(sc, power, point, (0.0, 1.0, 0.0), count, 20 + k)
        se = np.sqrt(a.var() / count + b.var() / count)
        assert abs(a.mean() - b.mean()) <= 4.0 * se, (point, a.mean(), b.mean(), se)
        assert b.var() < a.var(), (point, a.var(), b.var())
        assert a.mean() > 0


def test_lamp_and_embers_has_no_nan_pixel_on_the_oracle():
    """the agreement test of tests/test_gpu_light_sampling.py reads sample moments: the reference estimator must keep every pixel of the 16 x 12 film finite"""
    for metallic in (1.0, 0.0):
        ex = lamp_scene(metallic)
        orc = oracle_api.OracleScene(ex.scene, ex.cam)
        assert orc.lbvh_build() == ex.scene.primitive_count - 1
        film, _ = orc.render(16, 12, 0, 32, seed=11)
        orc.close()
        assert np.isfinite(film).all() and film.sum() > 0
