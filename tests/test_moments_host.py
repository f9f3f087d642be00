"""What the sample moments and the variance-guided filter can be held to without a device: the numpy restatement of Welford's update against
float64, its handling of samples that are not finite, the identity that recovers the oracle's exact per-frame samples, the filter's restatement on
pixels without a variance, bindings and refusals that need no GPU, and the quality of the variance-guided filter on the oracle's films."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import denoise_expected as de
import denoise_var_expected as dv
import moments_expected as me
from test_film_shapes import make, oracle
from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)
SEED = 5


def test_welford_f32_against_float64():
    """N samples of magnitude <= X.  Every update rounds three times per channel, each by at most eps / 2 of a value bounded by 2 X (mean, delta)
    or 4 X^2 (a term of M2) or 4 N X^2 (M2 itself), and carries the mean's error (<= 2 N eps X) into a product with a factor <= 2 X: after N updates
    |mean error| <= 2 N eps X and |M2 error| <= 8 N^2 eps X^2."""
    W, H, N = 7, 5, 50
    r = np.random.RandomState(1)
    xs = [(r.uniform(0.0, 1.0, (W, H, 3)) ** 3 * 20.0).astype(np.float32) for _ in range(N)]
    X = max(float(x.max()) for x in xs)
    rec = me.expected(xs, W, H)
    n, mean, m2, bad = me.welford64(xs, W, H)
    assert rec.dtype == np.float32 and (rec[:, :, 0] == N).all() and (rec[:, :, 7] == 0).all() and (n == N).all() and (bad == 0).all()
    e_mean, e_m2 = np.abs(rec[:, :, 1:4] - mean).max(), np.abs(rec[:, :, 4:7] - m2).max()
    print("mean error %.3e (bound %.3e), M2 error %.3e (bound %.3e)" % (e_mean, 2 * N * EPS * X, e_m2, 8 * N * N * EPS * X * X))
    assert e_mean <= 2 * N * EPS * X and e_m2 <= 8 * N * N * EPS * X * X
    # against the two-pass definition as well
    stack = np.stack(xs).astype(np.float64)
    assert np.abs(mean - stack.mean(axis=0)).max() < 1e-12 * X * N and np.abs(m2 - ((stack - stack.mean(axis=0)) ** 2).sum(axis=0)).max() < 1e-10 * X * X * N


def test_samples_that_are_not_finite_are_counted_and_skipped():
    W, H = 3, 2
    r = np.random.RandomState(2)
    xs = [r.uniform(0.0, 4.0, (W, H, 3)).astype(np.float32) for _ in range(6)]
    clean = me.expected([x[1:] for x in xs], W - 1, H)                    # row 0 gets the bad samples
    xs[1][0, 0, 2] = np.nan; xs[3][0, 0, 0] = np.inf; xs[4][0, 1] = -np.inf; xs[0][0, 1, 1] = np.nan
    rec = me.expected(xs, W, H)
    assert not np.isnan(rec).any() and np.isfinite(rec).all()
    assert rec[0, 0, 0] == 4 and rec[0, 0, 7] == 2 and rec[0, 1, 0] == 4 and rec[0, 1, 7] == 2
    assert np.array_equal(rec[1:], clean)                                # the other pixels do not notice
    good = [x[0, 0] for k, x in enumerate(xs) if k not in (1, 3)]
    alone = me.expected([g.reshape(1, 1, 3) for g in good], 1, 1)
    assert np.array_equal(rec[0, 0, :7], alone[0, 0, :7])                 # a skipped sample leaves n, mean and M2 exactly as they were
    one = me.expected(xs[:1], W, H)
    assert (one[1:, :, 0] == 1).all() and np.array_equal(one[1:, :, 1:4], xs[0][1:]) and (one[1:, :, 4:7] == 0).all()      # the first sample: mean = x, M2 = 0
    first_bad = me.fold(np.zeros((1, 8), np.float32), np.array([[np.nan, 1.0, 2.0]], np.float32))
    assert np.array_equal(first_bad, np.array([[0, 0, 0, 0, 0, 0, 0, 1]], np.float32))


@pytest.mark.parametrize("kind,W,H", [("cornell", 24, 20), ("cornell", 13, 7), ("teapot", 24, 20)])
def test_power_of_two_frames_give_the_oracles_exact_samples(kind, W, H):
    ex = make(kind, W, H, 0.8)
    orc = oracle(ex, kind)
    bad = 0
    for fr in me.EXACT_FRAMES:
        hdr, _ = orc.render(W, H, fr, 1, seed=SEED)
        x = me.oracle_sample(orc, W, H, fr, SEED)               # asserts the identity and the absence of subnormals
        coff = np.float32(1.0) / np.float32(fr + 1)
        with np.errstate(invalid="ignore"):
            back = x * coff
        fin = np.isfinite(hdr)
        assert np.array_equal(back[fin], hdr[fin]) and np.array_equal(np.isnan(back), np.isnan(hdr))
        if fr == 0:
            assert np.array_equal(x[fin], hdr[fin])
        bad += int((~np.isfinite(x)).any(axis=2).sum())
        # the sample is what the running mean of the frames before and this one took in: folding the film by hand gives the oracle's film
        if fr == 1:
            two, _ = orc.render(W, H, 0, 2, seed=SEED)
            x0 = me.oracle_sample(orc, W, H, 0, SEED)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(x * coff + x0 * (np.float32(1.0) - coff), two, equal_nan=True)
    for seed in (1, 2, 3):
        assert np.isfinite(me.oracle_sample(orc, W, H, 0, seed)).all()
    print(kind, W, H, "pixel-samples that are not finite:", bad)
    if kind == "teapot":
        assert bad >= 1          # what tests/test_gpu_moments.py needs of this film: the `bad` word is exercised
    with pytest.raises(AssertionError):
        me.recover(np.zeros((1, 1, 3), np.float32), 2)          # frame 2: 1/3 is no power of two


def test_converged_restatement():
    rec = np.zeros((2, 3, 8), np.float32)
    rec[0, 0] = [4, 1, 1, 1, 0.12, 0.12, 0.12, 0]         # v = 0.03, Y = 1: standard error 0.1732
    rec[0, 1] = [1, 5, 5, 5, 0, 0, 0, 0]                 # one sample: not measured
    rec[0, 2] = [2, 0, 0, 0, 0, 0, 0, 3]                 # measured, black, no variance: converged; bad
    rec[1, 0] = [2, 0, 0, 0, 1, 0, 0, 0]                 # black mean with variance: noisy at every threshold
    assert me.converged(rec, 0.1) == (3, 2, 1) and me.converged(rec, 0.2) == (3, 1, 1)
    mine = np.zeros((2, 3), bool); mine[0] = True
    assert me.converged(rec, 0.1, mine) == (2, 1, 1)


def test_filter_restatement_without_variances_and_on_one_pixel():
    W, H = 9, 6
    r = np.random.RandomState(3)
    hdr = r.uniform(0, 2, (W, H, 3)).astype(np.float32)
    aov = np.zeros((W, H, 8), np.float32)
    aov[:, :, 0:3] = r.uniform(0.2, 1, (W, H, 3)); aov[:, :, 3:6] = [0, 0, 1]; aov[:, :, 6] = r.uniform(1, 1.2, (W, H)); aov[:, :, 7] = 1
    mom = np.zeros((W, H, 8), np.float32)
    mom[:, :, 0] = 1                                      # one sample everywhere: no pixel has a variance
    a, s = dv.denoise_var_expected(hdr, aov, mom, sigma_c=0.01, want_s=True)
    b = dv.denoise_var_expected(hdr, aov, mom, sigma_c=100.0)
    assert (s == -1).all() and np.array_equal(a, b) and np.isfinite(a).all() and not np.array_equal(a, hdr)      # the guides alone: sigma_c plays no part
    mom[:, :, 0] = 4; mom[:, :, 4:7] = (hdr * 0.5) ** 2 * 4
    mom[4, 3, 0] = 0                                      # one pixel without: it keeps -1, its neighbours do not catch it
    c, s = dv.denoise_var_expected(hdr, aov, mom, want_s=True)
    assert s[4, 3] == -1 and (np.delete(s.reshape(-1), 4 * H + 3) >= 0).all() and np.isfinite(s).all() and np.isfinite(c).all()
    assert not np.array_equal(c, dv.denoise_var_expected(hdr, aov, mom, sigma_c=0.5))
    # zero variance everywhere: the colour term is dc / 1e-12, only equal colours mix -- a film of one colour stays
    mom[:, :, 0] = 4; mom[:, :, 4:7] = 0
    flat = np.ones((W, H, 3), np.float32) * aov[:, :, 0:3]
    out = dv.denoise_var_expected(flat, aov, mom)
    assert np.abs(out - flat).max() <= 4 * EPS
    one = dv.denoise_var_expected(hdr[:1, :1], aov[:1, :1], mom[:1, :1], levels=8)
    assert np.abs(one - hdr[:1, :1]).max() <= 2 * EPS * float(hdr[0, 0].max())      # one pixel: e / d * d


def test_bindings_defaults_and_refusals_without_a_device():
    text = open(os.path.join(ROOT, "include", "tirt.h")).read()
    for name in ("tirt_moments_enable", "tirt_moments_download", "tirt_moments_export_device", "tirt_moments_converged", "tirt_denoise_var",
                 "tirt_denoise_var_device"):
        assert name in _native.SIGNATURES and re.search(r"\b%s\s*\(" % name, text), name
    assert int(re.search(r"#define TIRT_MOM_WORDS (\d+)", text).group(1)) == _native.MOM_WORDS == me.WORDS == 8
    for word in ("N", "MEAN", "M2", "BAD"):
        assert int(re.search(r"#define TIRT_MOM_%s (\d+)" % word, text).group(1)) == getattr(_native, "MOM_" + word)
    sigma = float(re.search(r"#define TIRT_DENOISE_VAR_SIGMA_C ([0-9.]+)f", text).group(1))
    assert _native.DENOISE_VAR_DEFAULTS == dv.DEFAULTS and sigma == dv.DEFAULTS["sigma_c"]
    assert ctypes.sizeof(_native.DenoiseParams) == 16          # tirt_denoise_t is untouched; tirt_denoise_var_t has the same four fields
    lib = _native.lib()
    out = (ctypes.c_uint64 * 3)()
    prm = _native.DenoiseParams(5, 1.0, 0.3, 0.1)
    for rc in (lib.tirt_moments_enable(None, 1), lib.tirt_moments_download(None, None), lib.tirt_moments_export_device(None, None),
               lib.tirt_moments_converged(None, 0.1, out), lib.tirt_denoise_var(None, ctypes.byref(prm)),
               lib.tirt_denoise_var_device(None, None, None, None, None, 4, 4, ctypes.byref(prm), None)):
        assert rc == -2 and b"null context" in lib.tirt_last_error()
    # PathTrace.denoise_var() says what it needs before it reaches the library
    ex = make("cornell", 8, 8, 0.8)
    for kw in (dict(), dict(aov=True), dict(moments=True)):
        from ti_raytrace_amd import PT_RGB
        it = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, **kw)
        assert it.moments == bool(kw.get("moments")) and all(hasattr(it, a) for a in ("samples", "mean", "variance", "bad"))
        with pytest.raises(ValueError, match="aov=True, moments=True"):
            it.denoise_var()
    with pytest.raises(AssertionError):
        dv.denoise_var_expected(np.zeros((2, 2, 3)), np.zeros((2, 2, 8)), np.zeros((2, 2, 8)), levels=9)


def test_the_variance_guided_filter_improves_the_oracles_films():
    """Cornell 64 x 48 at 4 and at 16 frames against the oracle's 256: at its defaults the variance-guided filter has a lower rel-L2 than the
    unfiltered film (tools/denoise_var_quality.py writes the sweep behind the default sigma_c to profiles/denoise_var_quality.txt).
    Measured: 4 frames 0.1911 -> 0.1545 (tirt_denoise 0.1640), 16 frames 0.1115 -> 0.1023 (tirt_denoise 0.1125)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_var_quality as q
    data, ref = q.inputs((4, 16))
    for frames, (hdr, aov, mom) in sorted(data.items()):
        assert (mom[:, :, 0] == frames).all() and (mom[:, :, 7] == 0).all()
        raw = q.rel_l2(hdr, ref)
        var = q.rel_l2(dv.denoise_var_expected(hdr, aov, mom), ref)
        old = q.rel_l2(de.denoise_expected(hdr, aov), ref)
        print("%2d frames: unfiltered %.4f, tirt_denoise %.4f, tirt_denoise_var %.4f" % (frames, raw, old, var))
        assert var < raw, (frames, var, raw)
