"""The pixel set and the adaptive driver of the path tracer (include/tirt.h, tirt_pixel_set_from_moments / tirt_pt_rgb_render_adaptive) restated in numpy:
which pixels the moment records still list, in f32 with one rounding per operation in the stated order (the arithmetic of moments_expected.converged), the
order of the list, and the pass loop over the DENSE records -- a pixel rendered at frames 0 .. m-1 and then left alone holds the dense record of m frames.

  total = n + bad;  nn = n * (n - 1);  v = (M2.r / nn + M2.g / nn) + M2.b / nn;  Y = ((mean.r + mean.g) + mean.b) / 3;  t2 = threshold * threshold
  listed  <=>  total < max_samples  and  ( total < min_samples  or  n < 2  or  v > t2 * (Y * Y) )            (a comparison with a NaN is false)"""
import numpy as np

f = np.float32


def local_order(W, H, tile_rank=0, tile_count=1, tile_size=4096):
    """the linear pixel indices p = i*H + j of a rank's tiles in the order the device walks them (csrc/tirt_internal.h, local_to_pixel): tile by tile, inside
    a tile ascending p -- or, when the tiles are whole groups of 8 columns of a film whose height is a multiple of 8, in 8 x 8 pixel blocks down each group"""
    NP = W * H
    blocked = H % 8 == 0 and tile_size % (8 * H) == 0 and NP % tile_size == 0
    out = []
    for t in range(tile_rank, (NP + tile_size - 1) // tile_size, tile_count):
        within = np.arange(min(tile_size, NP - t * tile_size))
        if blocked:
            rows = H // 8
            b, l = within >> 6, within & 63
            bc, bj = b // rows, b % rows
            within = ((bc << 3) + (l >> 3)) * H + (bj << 3) + (l & 7)
        out.append(t * tile_size + within)
    return np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)


def listed(rec, threshold, min_samples, max_samples):
    """[W, H] bool: the rule above on a record [W, H, 8], f32 in the stated order"""
    rec = np.ascontiguousarray(rec, f)
    n, bad = rec[..., 0], rec[..., 7]
    t2 = f(threshold) * f(threshold)
    with np.errstate(all="ignore"):
        total = (n + bad).astype(f)
        nn = (n * (n - f(1.0)).astype(f)).astype(f)
        v = (((rec[..., 4] / nn).astype(f) + (rec[..., 5] / nn).astype(f)).astype(f) + (rec[..., 6] / nn).astype(f)).astype(f)
        Y = (((rec[..., 1] + rec[..., 2]).astype(f) + rec[..., 3]).astype(f) / f(3.0)).astype(f)
        noisy = v > (t2 * (Y * Y).astype(f)).astype(f)
        return (total < f(max_samples)) & ((total < f(min_samples)) | (n < f(2.0)) | noisy)


def select(rec, threshold, min_samples, max_samples, mine=None, order=None):
    """the list tirt_pixel_set_from_moments makes of a downloaded record [W, H, 8]: int32 pixel indices in local order.  mine: [W, H] mask of the rank's own
    pixels (default all); order: the rank's pixels in local order (local_order; default ascending p over `mine`)"""
    W, H = rec.shape[:2]
    on = listed(rec, threshold, min_samples, max_samples).reshape(-1)
    if order is None:
        own = np.ones(W * H, bool) if mine is None else np.asarray(mine, bool).reshape(-1)
        order = np.flatnonzero(own)
    order = np.asarray(order, np.int64)
    return order[on[order]].astype(np.int32)


def simulate(recs_by_n, threshold, min_samples, max_samples, pass_frames, mine=None):
    """(n_p [W, H] int64, info): the frames every pixel has when tirt_pt_rgb_render_adaptive(frame_begin 0) returns, from recs_by_n[m] = the DENSE records
    [W, H, 8] after m frames for every pass boundary m the loop reaches; info = what the call reports.  A pixel's own record after it stopped at m frames is
    recs_by_n[m] at that pixel: the rule is evaluated on exactly those."""
    first = recs_by_n[0] if 0 in recs_by_n else np.zeros_like(next(iter(recs_by_n.values())))
    W, H = first.shape[:2]
    own = np.ones((W, H), bool) if mine is None else np.asarray(mine, bool)
    n_p = np.zeros((W, H), np.int64)
    rec = np.zeros((W, H, 8), f)
    info = {"passes": 0, "pixel_samples": 0, "pixels_at_max": 0, "frames": 0}
    done = 0
    while True:
        on = listed(rec, threshold, min_samples, max_samples) & own
        count = int(on.sum())
        if count == 0:
            break
        assert (n_p[on] == done).all(), "a listed pixel has every frame so far: the sets only shrink"
        F = min(pass_frames, max_samples - done)
        done += F
        n_p[on] = done
        rec[on] = np.ascontiguousarray(recs_by_n[done], f)[on]
        info["passes"] += 1; info["pixel_samples"] += count * F; info["frames"] = done
        if done == max_samples:
            info["pixels_at_max"] = count
            break
    return n_p, info
