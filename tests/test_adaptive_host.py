"""What adaptive sampling can be held to without a device: the numpy restatement of the selection (tests/adaptive_expected.py) against float64 on made-up
records, the local order against a scalar restatement of local_to_pixel, the invariant the feature rests on -- the oracle's film at a pixel depends on
nothing but that pixel's frames --, and the stop counts the GPU test's scene gives on the CPU (that test must not be vacuous)."""
import collections

import numpy as np
import pytest

import adaptive_expected as ax
import moments_expected as me
from test_film_shapes import make, oracle

SEED = 5


def rec_row(n, mean, m2, bad=0.0):
    return [n, mean[0], mean[1], mean[2], m2[0], m2[1], m2[2], bad]


def listed64(rec, t, lo, hi):
    """the rule in float64, a Python comparison per pixel"""
    out = []
    for n, m0, m1, m2_, q0, q1, q2, bad in np.asarray(rec, np.float64).reshape(-1, 8):
        total = n + bad
        if not total < hi:
            out.append(False); continue
        if total < lo or n < 2:
            out.append(True); continue
        nn = n * (n - 1)
        v = (q0 + q1 + q2) / nn
        Y = (m0 + m1 + m2_) / 3
        out.append(bool(v > t * t * Y * Y))          # False when v or Y is NaN
    return np.array(out)


CASES = [       # (what, record, listed at threshold 0.3, min 4, max 32)
    ("nothing rendered", rec_row(0, (0, 0, 0), (0, 0, 0)), True),
    ("one sample", rec_row(1, (1, 1, 1), (0, 0, 0)), True),
    ("two samples, below min_samples", rec_row(2, (1, 1, 1), (0, 0, 0)), True),
    ("four samples that agree", rec_row(4, (1, 1, 1), (0, 0, 0)), False),
    ("four samples, standard error well above 0.3 x the level", rec_row(4, (1, 1, 1), (4, 4, 4)), True),         # v = 1, t2 Y^2 = 0.09
    ("four samples, standard error well below", rec_row(4, (1, 1, 1), (0.1, 0.1, 0.1)), False),                  # v = 0.025
    ("bad samples count towards min_samples", rec_row(2, (1, 1, 1), (0, 0, 0), bad=2), False),
    ("... but one finite sample is never measured", rec_row(1, (1, 1, 1), (0, 0, 0), bad=3), True),
    ("... up to max_samples", rec_row(1, (1, 1, 1), (0, 0, 0), bad=31), False),
    ("black without variance: converged", rec_row(8, (0, 0, 0), (0, 0, 0)), False),
    ("zero mean with variance: noisy at any threshold", rec_row(8, (1, -1, 0), (2, 2, 2)), True),
    ("NaN M2: not noisy", rec_row(8, (1, 1, 1), (np.nan, 1, 1)), False),
    ("NaN mean: not noisy", rec_row(8, (np.nan, 1, 1), (9, 9, 9)), False),
    ("NaN M2 below min_samples: still listed", rec_row(3, (1, 1, 1), (np.nan, 1, 1)), True),
    ("total at max_samples", rec_row(32, (1, 1, 1), (900, 900, 900)), False),
    ("total above max_samples", rec_row(40, (1, 1, 1), (900, 900, 900)), False),
    ("total at max_samples through bad", rec_row(30, (1, 1, 1), (900, 900, 900), bad=2), False),
    ("one short of max_samples, noisy", rec_row(31, (1, 1, 1), (900, 900, 900)), True),
]


def test_select_against_float64_on_made_up_records():
    rec = np.array([c[1] for c in CASES], np.float32).reshape(len(CASES), 1, 8)
    want = np.array([c[2] for c in CASES])
    got = ax.listed(rec, 0.3, 4, 32)[:, 0]
    for (what, _, w), g in zip(CASES, got):
        assert g == w, what
    assert np.array_equal(listed64(rec, 0.3, 4, 32), want)
    assert np.array_equal(ax.select(rec, 0.3, 4, 32), np.flatnonzero(want).astype(np.int32))
    # random records away from the decision boundary: f32 and float64 agree (v / (t2 Y^2) within 1 +- 1e-4 is left out: that is where roundings decide)
    r = np.random.RandomState(3)
    N = 4000
    rnd = np.zeros((N, 1, 8), np.float32)
    rnd[:, 0, 0] = r.randint(0, 40, N); rnd[:, 0, 7] = r.randint(0, 3, N)
    rnd[:, 0, 1:4] = r.uniform(0, 2, (N, 3)); rnd[:, 0, 4:7] = r.uniform(0, 1, (N, 3)) ** 4 * 300
    with np.errstate(all="ignore"):
        d = rnd.astype(np.float64)
        ratio = (d[:, 0, 4:7].sum(axis=1) / (d[:, 0, 0] * (d[:, 0, 0] - 1))) / (0.2 * 0.2 * (d[:, 0, 1:4].sum(axis=1) / 3) ** 2)
    clear = ~(np.abs(ratio - 1) < 1e-4)
    a, b = ax.listed(rnd, 0.2, 4, 32)[:, 0], listed64(rnd, 0.2, 4, 32)
    assert clear.sum() > N - 10 and np.array_equal(a[clear], b[clear]) and 0.2 < a.mean() < 0.8
    # the rule is tirt_moments_converged's where both apply: among the measured pixels past min_samples and short of max_samples, listed == noisy
    sub = (rnd[:, 0, 0] + rnd[:, 0, 7] >= 4) & (rnd[:, 0, 0] >= 2) & (rnd[:, 0, 0] + rnd[:, 0, 7] < 32)
    assert me.converged(rnd[sub], 0.2)[1] == int(a[sub].sum())


def local_to_pixel(k, rank, count, ts, H, blocked):
    """csrc/tirt_internal.h, one pixel at a time"""
    lt, within = divmod(k, ts)
    if blocked:
        rows = H >> 3
        b, l = within >> 6, within & 63
        bc, bj = divmod(b, rows)
        within = ((bc << 3) + (l >> 3)) * H + (bj << 3) + (l & 7)
    return (lt * count + rank) * ts + within


@pytest.mark.parametrize("W,H,ranks,ts", [(24, 20, 1, 4096), (24, 20, 3, 100), (32, 24, 2, 8 * 24), (32, 24, 1, 16 * 24), (1, 1, 1, 4096), (13, 7, 2, 10)])
def test_local_order(W, H, ranks, ts):
    blocked = H % 8 == 0 and ts % (8 * H) == 0 and (W * H) % ts == 0
    assert blocked == ((W, H) == (32, 24))
    seen = []
    for rank in range(ranks):
        got = ax.local_order(W, H, rank, ranks, ts)
        assert got.dtype == np.int32
        assert got.tolist() == [local_to_pixel(k, rank, ranks, ts, H, blocked) for k in range(len(got))]
        assert ((got // ts) % ranks == rank).all()
        if blocked:
            assert (np.diff(got) < 0).any()              # local order is not pixel order
            i, j = got[:64] // H, got[:64] % H
            assert i.max() - i.min() == 7 and j.max() - j.min() == 7          # the first wave is an 8 x 8 block
        seen += got.tolist()
    assert sorted(seen) == list(range(W * H))
    # select keeps that order
    rec = np.zeros((W, H, 8), np.float32)
    rec[::2, :, 0] = 32                                # every other column is done
    order = ax.local_order(W, H, ranks - 1, ranks, ts)
    got = ax.select(rec, 0.3, 4, 32, order=order)
    assert got.tolist() == [p for p in order.tolist() if (p // H) % 2 == 1]


def test_oracle_film_at_a_pixel_depends_on_that_pixels_frames_alone():
    """Cornell 13 x 7.  The oracle takes the camera's intrinsics (fx, fy, cx, cy) from the camera object, not from the film it is asked for, and numbers
    pixels p = i*H + j: a film of another WIDTH under the same camera has the same pixel index and the same camera ray at every (i, j) both hold, so the two
    films must agree there bit for bit -- whatever the other pixels are.  So must a film of which only a stretch of pixels is rendered at all."""
    W, H, N = 13, 7, 8
    ex = make("cornell", W, H, 0.8)
    orc = oracle(ex, "cornell")
    whole, _ = orc.render(W, H, 0, N, seed=SEED)
    assert (whole != 0).any(axis=2).mean() > 0.5 and len(np.unique(whole.reshape(-1, 3), axis=0)) > W * H // 2
    for other in (9, 20):
        film, _ = orc.render(other, H, 0, N, seed=SEED)
        w = min(W, other)
        assert np.array_equal(film[:w].view(np.uint32), whole[:w].view(np.uint32)), other
    some, _ = orc.render(W, H, 0, N, seed=SEED, p_begin=30, p_end=41)
    flat, part = whole.reshape(-1, 3), some.reshape(-1, 3)
    assert np.array_equal(part[30:41].view(np.uint32), flat[30:41].view(np.uint32)) and (part[:30] == 0).all() and (part[41:] == 0).all()
    # and the frames a pixel has are all that matters: frames 0 .. 3 then 4 .. 7 into the same film is the 8-frame film
    half, _ = orc.render(W, H, 0, 4, seed=SEED)
    both, _ = orc.render(W, H, 4, 4, seed=SEED, hdr=half.copy())
    assert np.array_equal(both.view(np.uint32), whole.view(np.uint32))
    assert not np.array_equal(half, whole)


def stop_counts(W, H, threshold, frames=32, pass_frames=4, min_samples=4):
    """the oracle's one-frame films scaled back in float64 are approximate samples (exact where frame + 1 is a power of two, moments_expected.recover): Welford
    over them, the dense records at every pass boundary, the pass loop"""
    ex = make("cornell", W, H, 0.8)
    orc = oracle(ex, "cornell")
    xs = [(orc.render(W, H, fr, 1, seed=SEED)[0].astype(np.float64) * (fr + 1)).astype(np.float32) for fr in range(frames)]
    recs, rec = {0: np.zeros((W, H, 8), np.float32)}, None
    for m in range(pass_frames, frames + 1, pass_frames):
        rec = me.expected(xs[m - pass_frames:m], W, H, rec=rec)
        recs[m] = rec
    n_p, info = ax.simulate(recs, threshold, min_samples, frames, pass_frames)
    return dict(sorted(collections.Counter(n_p.reshape(-1).tolist()).items())), n_p, info


def test_the_gpu_tests_scene_spreads_its_stop_counts():
    """Cornell 24 x 20, seed 5, threshold 0.3, passes of 4, at least 4 and at most 32 samples: what tests/test_gpu_adaptive.py runs.  The device's counts may
    differ by a few pixels (these samples are approximate, and its camera is placed by another helper); the three shares are what that test asserts."""
    hist, n_p, info = stop_counts(24, 20, 0.3)
    print("24 x 20, 0.3:", hist, info)
    assert hist == {4: 103, 8: 19, 12: 21, 16: 16, 20: 13, 24: 18, 28: 12, 32: 278}
    P = n_p.size
    assert len(hist) >= 5 and hist[4] >= 0.1 * P and hist[32] >= 0.1 * P and P - hist[4] - hist[32] >= 0.1 * P
    assert info == {"passes": 8, "pixel_samples": int(n_p.sum()), "pixels_at_max": 278, "frames": 32}
    print("21 %% of the pixels stop after 4 samples, %.0f %% need all 32" % (100.0 * hist[32] / P))
    assert round(100.0 * hist[4] / P) == 21 and round(100.0 * hist[32] / P) == 58
    hist2, n_p2, _ = stop_counts(24, 20, 0.2)
    print("24 x 20, 0.2:", hist2)
    assert hist2[4] == 69 and hist2[32] == 367 and P - 69 - 367 == 44          # 9 % in between: too few for the test
    hist1, _, _ = stop_counts(24, 20, 0.1)
    print("24 x 20, 0.1:", hist1)
    assert len(hist1) == 2                                                     # vacuous
    hist3, _, _ = stop_counts(13, 7, 0.3)
    print("13 x 7, 0.3:", hist3)
    assert hist3 == {4: 19, 8: 5, 12: 2, 16: 4, 20: 3, 24: 2, 28: 1, 32: 55}
    # a tighter threshold never stops a pixel earlier
    assert (n_p2 >= n_p).all()
