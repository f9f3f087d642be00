"""What a BDPT film may be, per pixel-channel, given the oracle's list of contributions (oracle.c, orc_bd_record; oracle_api.BD_RECORD) -- plain numpy,
float64.  The device and the oracle compute every single contribution from the same tirt_math.h with contraction off, so a contribution is the same
bits on both; what differs is the ORDER in which the contributions of one (frame, pixel-channel) are added in fp32: the oracle adds them one after
the other in pixel order, the device with float atomics in whatever order the waves retire, some of them pre-summed pairwise (k_bd_resolve).  So the
device's film is not the oracle's to the bit, but it is one of the fp32 sums of the same numbers, and those all lie in an interval this module computes.

Used by tests/test_bdpt_bound_host.py (the bound itself held to the oracle, to other summation orders and to mutated lists) and
tests/test_gpu_bdpt_bound.py (the device held to the bound)."""
import numpy as np

U = 2.0 ** -24                  # unit round-off of fp32, round to nearest
TINY = 2.0 ** -149              # the spacing of fp32's subnormals: an fp32 product that underflows is off by at most half of it
EVAL = 2.0 ** -50               # float64 evaluation of R, A and the recurrence below: relative 2^-53 per operation, a few operations per frame


def gamma(k):
    """Higham's gamma_k for fp32, elementwise; gamma(0) = 0"""
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def owned_records(records, rank, ranks, tile):
    """the records a rank of a tiled film (film_create(W, H, rank, ranks, tile)) produces: those whose SOURCE pixel p lies in one of its tiles -- the
    contribution itself may land on any pixel q of the rank's full-size film"""
    return records[(records["p"] // tile) % ranks == rank]


def _index(records, W, H, frames, frame_begin):
    f = records["frame"].astype(np.int64) - frame_begin
    q = records["q"].astype(np.int64)
    assert ((f >= 0) & (f < frames) & (q >= 0) & (q < W * H)).all(), "a record outside the film or the frames asked for"
    return ((f * (W * H) + q) * 3)[:, None] + np.arange(3)[None, :]


def planes(records, W, H, frames, frame_begin=0):
    """per frame and pixel-channel, [frames, W, H, 3]: R, the float64 sum of the contributions; A, the float64 sum of their absolute values; n, how many are
    not zero (the device skips the all-zero ones, and adding a zero changes no fp32 sum); bad, whether one of them is not finite (R and A leave those out)"""
    idx = _index(records, W, H, frames, frame_begin).reshape(-1)
    v = records["r"].astype(np.float64).reshape(-1)
    fin = np.isfinite(v)
    size = frames * W * H * 3
    vv = np.where(fin, v, 0.0)
    R = np.bincount(idx, weights=vv, minlength=size)
    A = np.bincount(idx, weights=np.abs(vv), minlength=size)
    n = np.bincount(idx, weights=(vv != 0.0).astype(np.float64), minlength=size).astype(np.int64)
    bad = np.bincount(idx, weights=(~fin).astype(np.float64), minlength=size) > 0
    shape = (frames, W, H, 3)
    return R.reshape(shape), A.reshape(shape), n.reshape(shape), bad.reshape(shape)


def blend_constants(frame):
    """c = 1.0f / (frame + 1.0f) and d = 1.0f - c as k_bdpt_film and the oracle form them, in fp32"""
    c = np.float32(1.0) / (np.float32(np.int32(frame)) + np.float32(1.0))
    return c, np.float32(1.0) - c


def blend(hdr, rad, frame):
    """one step of the running mean in fp32, as written in k_bdpt_film and oracle.c: hdr = rad * c + hdr * d"""
    c, d = blend_constants(frame)
    with np.errstate(invalid="ignore", over="ignore"):
        return (rad * c + hdr * d).astype(np.float32)


def replay(records, W, H, frames, frame_begin=0, order=None):
    """The film fp32 arithmetic makes of the records when each frame's radiance plane is summed one record after the other, in the order given (default: the
    records' own, which is the oracle's -- then this IS the oracle's film, bit for bit: test_bdpt_bound_host.py) and blended frame after frame.  Returns
    (film [W, H, 3], planes [frames, W, H, 3]), float32."""
    idx = _index(records, W, H, frames, frame_begin)
    val = records["r"].astype(np.float32)
    if order is not None:
        idx, val = idx[order], val[order]
    rad = np.zeros(frames * W * H * 3, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(rad, idx.reshape(-1), val.reshape(-1))            # unbuffered: one fp32 addition per entry, in the entries' order
    rad = rad.reshape(frames, W, H, 3)
    hdr = np.zeros((W, H, 3), np.float32)
    for f in range(frames):
        hdr = blend(hdr, rad[f], frame_begin + f)
    return hdr, rad


def film_bound(records, W, H, frames, frame_begin=0):
    """(Hx, E, exact_mask_frame0, excluded), each [W, H, 3]: every film that fp32 arithmetic can make of the records by adding each frame's contributions to a
    pixel-channel in ANY order or tree and then blending the frames as k_bdpt_film does lies within E of Hx, outside `excluded`.

    Notation, per frame f and pixel-channel: n non-zero contributions, R their exact sum, A the sum of their absolute values, u = 2^-24.

    The radiance plane.  Every fp32 addition returns (a + b)(1 + eps), |eps| <= u, exactly so (an fp32 sum never underflows inexactly).  A summation of n numbers
    in any order, sequential, pairwise or mixed, makes n - 1 additions and each number passes through at most n - 1 of them, so the computed sum is
    sum x_i (1 + theta_i) with |theta_i| <= gamma(n - 1), gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 4.2): it
    lies within g = gamma(n - 1) A of R.  n = 0 gives exactly 0, n = 1 the number itself, and n = 2 ONE addition, which is commutative: for n <= 2 every
    order gives the same bits, the oracle's.  That is `exact_mask_frame0` for the first frame, where the blend changes nothing (c = 1, d = 0, 0 from a cleared film).

    The film.  hdr_f = fl(fl(rad c) + fl(hdr_{f-1} d)) with the fp32 constants c = 1.0f / (f + 1.0f), d = 1.0f - c, which the device and the oracle form alike and
    which are therefore exact data here (blend_constants).  Write rad = R_f + dr with |dr| <= g_f, hdr_{f-1} = Hx_{f-1} + dh with |dh| <= E_{f-1}, and follow the
    exact values as Hx_f = c R_f + d Hx_{f-1}.  With one (1 + eps) per product and one for the sum,
        hdr_f = (rad c (1 + e1) + hdr_{f-1} d (1 + e2)) (1 + e3)
        hdr_f - Hx_f = c dr + d dh + rad c ((1 + e1)(1 + e3) - 1) + hdr_{f-1} d ((1 + e2)(1 + e3) - 1)
    and |(1 + e)(1 + e') - 1| <= 2 u + u^2 <= 3 u, |rad| <= |R_f| + g_f, |hdr_{f-1}| <= |Hx_{f-1}| + E_{f-1}, c, d >= 0, so
        E_f = c g_f + d E_{f-1} + 3 u (c (|R_f| + g_f) + d (|Hx_{f-1}| + E_{f-1})),      E_{-1} = Hx_{-1} = 0.
    Two terms no larger than 2^-26 of that keep the statement rigorous rather than wider: the two products may underflow (fp32 then errs by at most half a
    subnormal spacing each: + 2^-149), and R, A, Hx and E are themselves evaluated in float64 (+ 2^-50 (|Hx_f| + E_f)).

    excluded: a pixel-channel one of whose records is not finite, or whose film in the oracle's own order is not finite (an overflow).  No interval means
    anything there; the device's film must be non-finite exactly where the oracle's is (assert_film_within)."""
    R, A, n, bad = planes(records, W, H, frames, frame_begin)
    Hx = np.zeros((W, H, 3)); E = np.zeros((W, H, 3))
    for f in range(frames):
        c, d = (np.float64(x) for x in blend_constants(frame_begin + f))
        g = gamma(np.maximum(n[f] - 1, 0)) * A[f]
        E = c * g + d * E + 3.0 * U * (c * (np.abs(R[f]) + g) + d * (np.abs(Hx) + E)) + TINY
        Hx = c * R[f] + d * Hx
        E = E + EVAL * (np.abs(Hx) + E)
    film, _ = replay(records, W, H, frames, frame_begin)
    excluded = bad.any(axis=0) | ~np.isfinite(film)
    exact0 = (n[0] <= 2) & ~excluded if frames >= 1 and frame_begin == 0 else np.zeros((W, H, 3), bool)
    return Hx, E, exact0, excluded


def violations(got, want, Hx, E, exact, excluded):
    """elementwise: where `got` is not an admissible film.  want: the oracle's film (replay); exact: where got must be want's bits (None: nowhere)"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    with np.errstate(invalid="ignore"):
        out = ~(np.abs(got.astype(np.float64) - Hx) <= E)                       # (a NaN is outside every interval)
    if exact is not None:
        out = np.where(exact, got.view(np.uint32) != want.view(np.uint32), out)
    return np.where(excluded, np.isfinite(got) != np.isfinite(want), out)


def assert_film_within(got, records, W, H, frames, frame_begin=0, what=""):
    """`got` [W, H, 3] is a film of `frames` frames that fp32 arithmetic can have made of the records: non-finite exactly where the oracle's is on the excluded
    pixel-channels; after ONE frame from 0 the oracle's bits wherever at most two contributions met (the zeros included); within E of Hx everywhere else
    and after every later frame.  Returns what a caller may want to print: the largest error / bound ratio, the numbers of pixel-channels exact, bounded and
    excluded, and the median of E / |Hx| over the lit ones."""
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape == (W, H, 3), (what, got.shape)
    Hx, E, exact0, excluded = film_bound(records, W, H, frames, frame_begin)
    want, _ = replay(records, W, H, frames, frame_begin)
    exact = exact0 if (frames == 1 and frame_begin == 0) else None
    bad = violations(got, want, Hx, E, exact, excluded)
    if bad.any():
        rows = []
        for i, j, ch in np.argwhere(bad)[:8]:
            q = i * H + j
            m = (records["q"] == q) & (records["r"][:, ch] != 0)
            rows.append("pixel (%d, %d) ch %d: got %r, oracle %r, Hx %.9g, E %.3g, %s; contributions (frame, p, e, l, value): %s" % (
                i, j, ch, got[i, j, ch], want[i, j, ch], Hx[i, j, ch], E[i, j, ch],
                "excluded" if excluded[i, j, ch] else ("exact" if exact is not None and exact[i, j, ch] else "bounded"),
                [(int(r["frame"]), int(r["p"]), int(r["e"]), int(r["l"]), float(r["r"][ch])) for r in records[m][:12]]))
        raise AssertionError("%s: %d of %d pixel-channels outside what the contributions allow after %d frame(s)\n%s" % (what, int(bad.sum()), bad.size, frames, "\n".join(rows)))
    inside = ~excluded if exact is None else ~excluded & ~exact
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(inside, np.abs(got.astype(np.float64) - Hx) / E, 0.0)
        lit = ~excluded & (Hx != 0)
        rel = float(np.median(E[lit] / np.abs(Hx[lit]))) if lit.any() else 0.0
    return {"ratio": float(ratio.max()), "exact": int(0 if exact is None else exact.sum()), "bounded": int(inside.sum()), "excluded": int(excluded.sum()), "rel_bound": rel}
