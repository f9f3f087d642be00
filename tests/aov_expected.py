"""The feature buffers of the path tracer (include/tirt.h, tirt_aov_enable) as the CPU oracle's hit records give them, in numpy f32.

Per frame the camera rays of debug_views.camera_rays (the jitter of that frame and seed) and their closest hits; per pixel eight words
-- albedo3, normal3, depth, alpha, zeros on a miss -- folded into the record with the film's recurrence (integrator/PT_RGB.py:134-136), one
f32 rounding per operation, frames in ascending order.  No transcendental function is on this path: the device must match bit for bit."""
import numpy as np

import debug_views as dv
from ti_raytrace_amd import _native

f = np.float32
WORDS = _native.AOV_WORDS


def samples(scene, rays, hit, prim):
    """[n, 8]: the values of one frame from hit records (t, pos3, gnormal3, normal3, tex3) and primitive ids, in ray order"""
    n = hit.shape[0]
    ok = hit[:, 0] < dv.INF_VALUE
    x = np.zeros((n, WORDS), f)
    x[:, _native.AOV_ALBEDO:_native.AOV_ALBEDO + 3] = dv.compose(scene, rays, hit, prim, "albedo", n, 1).reshape(n, 3)
    x[ok, _native.AOV_NORMAL:_native.AOV_NORMAL + 3] = hit[ok, 7:10]
    x[ok, _native.AOV_DEPTH] = hit[ok, 0]
    x[ok, _native.AOV_ALPHA] = f(1.0)
    return x


def fold(acc, x, frame):
    """a = x * coff + a * (1 - coff), coff = 1 / (frame + 1): k_film's running mean"""
    coff = f(1.0) / (f(int(frame)) + f(1.0))
    keep = f(1.0) - coff
    with np.errstate(invalid="ignore"):
        new = (x * coff).astype(f)
        old = (acc * keep).astype(f)
        return (new + old).astype(f)


def expected(ex, orc, W, H, frames, seed, mine=None, acc=None):
    """[W, H, 8] after the frames of the iterable `frames` (ascending) of an example whose camera is set (orc: its OracleScene, LBVH built, smooth
    normals applied where the example has them).  mine: [W, H] mask of the pixels this rank owns (the others stay zero); acc: records so far."""
    acc = np.zeros((W * H, WORDS), f) if acc is None else np.ascontiguousarray(acc, f).reshape(W * H, WORDS).copy()
    hits = misses = 0
    for frame in frames:
        rays = dv.camera_rays(ex.cam, W, H, frame, seed)
        hit, prim = dv.closest_hits(orc, rays)
        ok = hit[:, 0] < dv.INF_VALUE
        hits += int(ok.sum()); misses += int((~ok).sum())
        acc = fold(acc, samples(ex.scene, rays, hit, prim), frame)
    acc = acc.reshape(W, H, WORDS)
    if mine is not None:
        acc[~mine] = 0
    return acc, hits, misses
