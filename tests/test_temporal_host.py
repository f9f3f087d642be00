"""What the temporal accumulation can be held to without a device: the numpy restatement of its definition (tests/temporal_expected.py) on hand-made
histories over the oracle's Cornell films at 24 x 20 -- no history, every tap rejected, a current pixel without samples, the cap --, its merge against
the float64 moments of the concatenated samples, and what the accumulation buys on an orbit of views (tools/temporal_quality.py)."""
import os
import re
import sys

import numpy as np
import pytest

import denoise_var_expected as dv
import moments_expected as me
import temporal_expected as te
from common import same_bits
from test_film_shapes import make, oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
W, H, SEED = 24, 20, 5
QUALITY = os.path.join(ROOT, "profiles", "temporal_quality.txt")


@pytest.fixture(scope="module")
def films():
    """two record sets of one camera (seeds 5 and 6, 2 frames each), that camera, and the oracle's exact samples behind them"""
    ex = make("cornell", W, H, 0.8)
    orc = oracle(ex, "cornell")
    cam = te.Cam(ex.cam)
    a = te.oracle_view(ex, orc, W, H, SEED)
    b = te.oracle_view(ex, orc, W, H, SEED + 1)
    xs = [me.oracle_sample(orc, W, H, fr, s) for s in (SEED, SEED + 1) for fr in range(2)]
    assert (a[2][:, :, 0] == 2).all() and (b[2][:, :, 0] == 2).all() and 0.5 < (a[1][:, :, 7] > 0).mean() < 1.0      # hits and misses
    return a, b, cam, xs


def test_no_history_gives_the_current_records_exactly(films):
    a, b, cam, _ = films
    zero = [np.zeros_like(x) for x in a]
    hdr, mom, info = te.accumulate(*b, *zero, cam, cam, want_info=True)                  # an empty history: al_h = 0, n_h = 0 everywhere
    assert same_bits(hdr, b[0], True) and same_bits(mom, b[2], True) and not info["history"].any()
    # every tap rejected: on the normal (the history's normals turned round), on the depth (the history twice as far), on both
    flipped, far = a[1].copy(), a[1].copy()
    flipped[:, :, 3:6] *= -1
    far[:, :, 6] *= 2
    for aov_h, what in ((flipped, "normal"), (far, "depth")):
        hdr, mom, info = te.accumulate(*b, a[0], aov_h, a[2], cam, cam, want_info=True)
        assert same_bits(hdr, b[0], True) and same_bits(mom, b[2], True), what
        assert not info["history"].any() and info["rejected"].sum() == (b[1][:, :, 7] > 0).sum() and info["rejected_taps"] >= info["rejected"].sum(), what
    # a history that is not finite, or has no samples, is no history either
    for word, value in ((1, np.nan), (5, np.inf), (0, 0.0)):
        mom_h = a[2].copy(); mom_h[:, :, word] = value
        hdr, mom = te.accumulate(*b, a[0], a[1], mom_h, cam, cam)
        assert same_bits(hdr, b[0], True) and same_bits(mom, b[2], True), (word, value)
    hdr_h = a[0].copy(); hdr_h[:, :, 2] = np.nan
    hdr, mom = te.accumulate(*b, hdr_h, a[1], a[2], cam, cam)
    assert same_bits(hdr, b[0], True) and same_bits(mom, b[2], True)
    # behind the previous camera: it stood in the middle of the box and looked the other way, with the back wall behind it
    ex = make("cornell", W, H, 0.8)
    ex.cam.set_view_point(np.pi, 0.0, 0.0, 0.05 * ex.cam.scale)
    hdr, mom, info = te.accumulate(*b, *a, cam, te.Cam(ex.cam), want_info=True)
    assert info["behind"].sum() >= 1 and not info["history"][info["behind"]].any() and same_bits(hdr[info["behind"]], b[0][info["behind"]], True)


def test_a_current_pixel_without_samples_takes_the_history_exactly(films):
    """Every word of the hand-made history is a power of two and the same on every pixel: value * k is exact, the sums are value * sw, and the quotient is the
    value again, whatever the bilinear weights are -- so the history must come out bit for bit wherever the surface was hit."""
    a, b, cam, _ = films
    rec = np.float32([4, 0.5, 0.25, 2, 2, 1, 0.5, 1])
    hdr_h = np.full((W, H, 3), 0.25, np.float32)
    mom_h = np.broadcast_to(rec, (W, H, 8)).copy()
    mom_c = np.zeros((W, H, 8), np.float32)                        # n_c = 0: nothing was rendered at these pixels
    hit = b[1][:, :, 7] > 0
    for hdr_c in (b[0], np.zeros_like(b[0])):
        hdr, mom, info = te.accumulate(hdr_c, b[1], mom_c, hdr_h, b[1], mom_h, cam, cam, sigma_n=4.0, sigma_z=10.0, want_info=True)
        assert np.array_equal(info["history"], hit) and hit.sum() > W * H // 2
        assert same_bits(mom[hit], mom_h[hit], True) and same_bits(hdr[hit], hdr_h[hit], True)
        assert same_bits(mom[~hit], mom_c[~hit], True) and same_bits(hdr[~hit], hdr_c[~hit], True)
    # the cap: n 4 -> 2, M2 and bad halved, the mean and hdr as they were
    hdr, mom, info = te.accumulate(b[0], b[1], mom_c, hdr_h, b[1], mom_h, cam, cam, max_history=2.0, sigma_n=4.0, sigma_z=10.0, want_info=True)
    assert np.array_equal(info["capped"], hit)
    assert same_bits(mom[hit], np.broadcast_to(np.float32([2, 0.5, 0.25, 2, 1, 0.5, 0.25, 0.5]), (int(hit.sum()), 8)), True) and same_bits(hdr[hit], hdr_h[hit], True)
    # a film pixel that is not finite stays, and its moment words still take the history
    hdr_c = b[0].copy()
    i, j = np.argwhere(hit)[3]
    hdr_c[i, j, 1] = np.nan
    hdr, mom = te.accumulate(hdr_c, b[1], mom_c, hdr_h, b[1], mom_h, cam, cam, sigma_n=4.0, sigma_z=10.0)
    assert same_bits(hdr[i, j], hdr_c[i, j]) and same_bits(mom[i, j], rec, True) and np.isnan(hdr).sum() == 1


def measured_merge_deviation():
    line = re.search(r"^merge deviation: mean ([0-9.e+-]+)\s+M2 ([0-9.e+-]+)", open(QUALITY).read(), re.M)
    return float(line.group(1)), float(line.group(2))


def test_the_merge_agrees_with_float64_moments_of_the_concatenated_samples(films):
    """Two record sets of one camera merged by the restatement against the float64 moments of the four samples.  The bilinear weights of an identical
    camera are 1 - O(1e-6) on the pixel itself and O(1e-6) on a neighbour, so the deviation is rounding plus that much of a neighbour.  With guides that
    reject nothing (sigma_n 4, sigma_z 10) every pixel whose camera rays hit in the current view merges, and n_o = 4 exactly.  The bound is four times
    the worst deviation tools/temporal_quality.py measured and wrote to profiles/temporal_quality.txt (mean 9.537e-07, M2 2.543e-06, each relative to
    the largest value of its kind on the film): a check of the restatement's arithmetic, not of the device."""
    a, b, cam, xs = films
    hdr, mom, info = te.accumulate(*b, *a, cam, cam, max_history=1e6, sigma_n=4.0, sigma_z=10.0, want_info=True)
    n, mean, m2, bad = me.welford64(xs, W, H)
    hit = b[1][:, :, 7] > 0
    assert (n == 4).all() and (bad == 0).all() and np.array_equal(info["history"], hit) and (mom[:, :, 0][hit] == 4).all()
    assert same_bits(mom[~hit], b[2][~hit], True) and same_bits(hdr[~hit], b[0][~hit], True)
    d_mean = float(np.abs(mom[:, :, 1:4] - mean)[hit].max() / np.abs(mean[hit]).max())
    d_m2 = float(np.abs(mom[:, :, 4:7] - m2)[hit].max() / np.abs(m2[hit]).max())
    b_mean, b_m2 = measured_merge_deviation()
    print("merge deviation: mean %.3e (bound %.3e)  M2 %.3e (bound %.3e)" % (d_mean, 4 * b_mean, d_m2, 4 * b_m2))
    assert d_mean <= 4 * b_mean and d_m2 <= 4 * b_m2
    # hdr is merged with the same weight: the mean of the two 2-frame films where both are finite
    both = 0.5 * (a[0].astype(np.float64) + b[0])
    assert float(np.abs(hdr - both)[hit].max() / np.abs(both[hit]).max()) <= 4 * b_mean
    # at the default guides the pixels that merge are a subset, and they give the same n
    _, mom_d, info_d = te.accumulate(*b, *a, cam, cam, want_info=True)
    assert not (info_d["history"] & ~hit).any() and info_d["history"].sum() > hit.sum() // 2 and (mom_d[:, :, 0][info_d["history"]] == 4).all()


def test_accumulation_improves_the_denoised_film_of_a_moving_camera():
    """An orbit of 8 views of the Cornell box at 64 x 48, 2 frames each (tools/temporal_quality.py; profiles/temporal_quality.txt has the numbers and the
    sweep behind the defaults): at the last view, against the oracle's 256-frame film, the accumulated film through tirt_denoise_var is better than
    tirt_denoise_var of the 2-frame film alone.  Measured: raw 0.2169, tirt_denoise_var 0.1919, accumulated 0.1166, accumulated + tirt_denoise_var 0.1066."""
    import temporal_quality as q
    views, ref = q.orbit()
    hdr, aov, mom, _ = views[-1]
    acc_h, acc_m, share = q.run(views)
    alone = q.rel_l2(dv.denoise_var_expected(hdr, aov, mom), ref)
    both = q.rel_l2(dv.denoise_var_expected(acc_h, aov, acc_m), ref)
    print("raw %.4f, tirt_denoise_var %.4f, accumulated %.4f, accumulated + tirt_denoise_var %.4f, share with a history %.3f"
          % (q.rel_l2(hdr, ref), alone, q.rel_l2(acc_h, ref), both, share))
    assert both < alone, (both, alone)
