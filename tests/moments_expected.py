"""The sample moments of the path tracer (include/tirt.h, tirt_moments_enable) restated in numpy f32, one rounding per operation in the stated
order, and the exact per-frame pixel-samples of the CPU oracle that they are folded over.

Record, per pixel: n, mean3, M2 3, bad.  Per sample x = (r, g, b):
  a channel that is NaN or +-inf:  bad = bad + 1, nothing else
  otherwise  n = n + 1;  per channel  delta = x - mean;  mean = mean + delta / n;  M2 = M2 + delta * (x - mean)      (the new mean)

The samples.  OracleScene.render folds a frame f into its film with coff = 1 / (f + 1): hdr = x * coff + hdr * (1 - coff).  Into a zeroed film
one frame leaves fl(x * coff), and that product is exact when f + 1 is a power of two (and x * coff is not subnormal): x = hdr * (f + 1) bit
for bit; frame 0 leaves x itself.  So frames 0, 1, 3, 7, 15, 31 at one seed, and frame 0 at any seed, give exact samples; `oracle_sample`
asserts the identity on every value it returns."""
import numpy as np

from ti_raytrace_amd import _native

f = np.float32
WORDS = _native.MOM_WORDS
EXACT_FRAMES = (0, 1, 3, 7, 15, 31)
TINY = np.finfo(np.float32).tiny


def fold(rec, x):
    """rec [N, 8] after one more sample x [N, 3] per pixel (a new array)"""
    rec = np.ascontiguousarray(rec, f).copy()
    x = np.ascontiguousarray(x, f)
    assert rec.ndim == 2 and rec.shape[1] == WORDS and x.shape == (rec.shape[0], 3)
    ok = np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        n = (rec[:, 0] + f(1.0)).astype(f)
        out = rec.copy()
        out[:, 0] = n
        for ch in range(3):
            mean, m2, xc = rec[:, 1 + ch], rec[:, 4 + ch], x[:, ch]
            delta = (xc - mean).astype(f)
            new = (mean + (delta / n).astype(f)).astype(f)
            out[:, 1 + ch] = new
            out[:, 4 + ch] = (m2 + (delta * (xc - new).astype(f)).astype(f)).astype(f)
    rec[ok] = out[ok]
    rec[~ok, 7] = rec[~ok, 7] + f(1.0)
    return rec


def expected(samples, W, H, mine=None, rec=None):
    """[W, H, 8] after the samples of the iterable `samples` ([W, H, 3] each, in order); mine: [W, H] mask of the pixels this rank owns (the others
    stay zero); rec: the records so far"""
    rec = np.zeros((W * H, WORDS), f) if rec is None else np.ascontiguousarray(rec, f).reshape(W * H, WORDS).copy()
    for x in samples:
        rec = fold(rec, np.ascontiguousarray(x, f).reshape(W * H, 3))
    rec = rec.reshape(W, H, WORDS)
    if mine is not None:
        rec[~mine] = 0
    assert not np.isnan(rec).any()
    return rec


def recover(hdr, frame):
    """the exact samples from the oracle's one-frame film of `frame` (f + 1 a power of two), the identity asserted"""
    k = int(frame) + 1
    assert k & (k - 1) == 0, "frame + 1 must be a power of two"
    hdr = np.ascontiguousarray(hdr, f)
    with np.errstate(all="ignore"):
        x = (hdr * f(k)).astype(f)
        coff = f(1.0) / f(k)
        back = (x * coff).astype(f)
    fin = np.isfinite(hdr)
    assert not ((np.abs(hdr[fin]) < TINY) & (hdr[fin] != 0)).any(), "a subnormal film value: the product was not exact"
    assert not np.isinf(x[fin]).any(), "the sample overflowed on the way back"
    assert (back[fin] == hdr[fin]).all() and (np.isnan(back) == np.isnan(hdr)).all() and (np.isinf(back) == np.isinf(hdr)).all()
    return x


def oracle_sample(orc, W, H, frame, seed, **kw):
    """[W, H, 3]: the pixel-samples of one frame as the oracle computes them, exactly"""
    hdr, _ = orc.render(W, H, int(frame), 1, seed=seed, **kw)
    return recover(hdr, frame)


def welford64(samples, W, H):
    """the same moments in float64 (finite samples only counted): n, mean, M2, bad as [W, H], [W, H, 3], [W, H, 3], [W, H]"""
    n = np.zeros((W, H)); mean = np.zeros((W, H, 3)); m2 = np.zeros((W, H, 3)); bad = np.zeros((W, H))
    for x in samples:
        x = np.asarray(x, np.float64).reshape(W, H, 3)
        ok = np.isfinite(x).all(axis=2)
        n1 = n + ok
        with np.errstate(all="ignore"):
            delta = np.where(ok[:, :, None], x - mean, 0.0)
            mean1 = mean + np.where(ok[:, :, None], delta / np.maximum(n1, 1)[:, :, None], 0.0)
            m2 = m2 + np.where(ok[:, :, None], delta * (x - mean1), 0.0)
        mean, n = mean1, n1
        bad = bad + ~ok
    return n, mean, m2, bad


def converged(rec, threshold, mine=None):
    """tirt_moments_converged on a downloaded record [W, H, 8], in f32 in the stated order: (measured, noisy, bad)"""
    rec = np.ascontiguousarray(rec, f)
    own = np.ones(rec.shape[:2], bool) if mine is None else mine
    n = rec[:, :, 0]
    measured = own & (n >= 2)
    t2 = f(threshold) * f(threshold)
    with np.errstate(all="ignore"):
        nn = (n * (n - f(1.0)).astype(f)).astype(f)
        v = ((rec[:, :, 4] / nn).astype(f) + (rec[:, :, 5] / nn).astype(f)).astype(f) + (rec[:, :, 6] / nn).astype(f)
        Y = (((rec[:, :, 1] + rec[:, :, 2]).astype(f) + rec[:, :, 3]).astype(f) / f(3.0)).astype(f)
        noisy = measured & (v.astype(f) > (t2 * (Y * Y).astype(f)).astype(f))
    return int(measured.sum()), int(noisy.sum()), int((own & (rec[:, :, 7] > 0)).sum())
