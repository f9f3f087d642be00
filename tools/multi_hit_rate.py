"""Rate of RayQuery.hits / .count (csrc/tirt_multi_hit.hip) on one GPU against what a caller had before them.

    python tools/multi_hit_rate.py [--reps 5] [--out profiles/multi_hit_rate.txt]

Scene: the headline synthetic 100k-triangle scene (camera of a 1024 x 1024 film).  Ray sets: the 1 Mi camera rays of that film and 1 Mi rays with
origins uniform in the scene's bounds and uniform directions.  Each line is timed with torch events on the current stream around one call, median of
`--reps` after one warm-up call.  Four comparisons:
  1. hits(k = 1) against closest() of the same library on the same rays
  2. hits(k = 4) and hits(k = 16) against k successive closest() calls, each from the previous hit pushed along the ray by an epsilon (the loop a caller
     writes today, its tensor arithmetic included; it is not exact: it skips or repeats surfaces closer together than the epsilon)
  3. count() against hits(k = 16, count = True)
  4. the ordered walk against the EXHAUSTIVE one (hits(k = 4) and count())
and the mean N_box / N_leaf per ray of every walk (a COUNT_NODES call of its own, not timed)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ti_raytrace_amd import RayQuery, scenes, _native     # noqa: E402
import oracle_api as oa                                    # noqa: E402  (numpy camera rays)

DEV = torch.device("cuda", 0)
EPS = 1.0e-4      # of the scene's extent: the push of the peeling loop


def timed(fn, reps):
    fn()
    torch.cuda.synchronize(DEV)
    ms = []
    s = torch.cuda.current_stream(DEV)
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def random_rays(ex, n, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    o = lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=g)
    d = torch.randn((n, 3), device=DEV, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).contiguous()


def peel(q, rays, k, eps):
    """k successive closest() calls: the origin moves to the hit plus eps along the ray (rays that have missed stay where they are)"""
    cur = rays.clone()
    ts = []
    for _ in range(k):
        h = q.closest(cur)
        hit = h.t < 1.0e6
        cur[:, 0:3] += cur[:, 3:6] * torch.where(hit, h.t + eps, torch.zeros_like(h.t))[:, None]
        ts.append(h.t)
    return ts


def node_counts(ctx, rays, k, count, flags):
    n = rays.shape[0]
    cnt = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    t = torch.empty((n, max(k, 1)), dtype=torch.float32, device=DEV)
    c = torch.empty(n, dtype=torch.int32, device=DEV)
    ctx.query_hits(rays.data_ptr(), n, rays.stride(0), k, flags=flags | _native.COUNT_NODES, out_t=t.data_ptr() if k else 0,
                   out_count=c.data_ptr() if count else 0, counts=cnt.data_ptr())
    torch.cuda.synchronize(DEV)
    m = cnt.float().mean(dim=0)
    return float(m[0]), float(m[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_hit_rate.txt"))
    a = ap.parse_args()
    W = 1024
    ex = scenes.synthetic(W, W, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    q, qx = RayQuery(ex.scene), RayQuery(ex.scene, 64, _native.TRAVERSE_EXHAUSTIVE)
    ext = float((ex.scene.maxboundarynp[0] - ex.scene.minboundarynp[0]).max())
    lines = ["# python tools/multi_hit_rate.py   (one MI355X)",
             "# 100k-triangle headline scene (bench.py's), camera of a 1024^2 film.  ms = torch events on the current stream around one call, median of %d after" % a.reps,
             "# 1 warm-up call.  peel_k = k successive closest() calls, each from the previous hit pushed %.0e extents along the ray (tensor arithmetic included)." % EPS,
             "# N_box / N_leaf = mean box tests / primitive tests per ray (a COUNT_NODES call of its own).  mean |H| = the mean number of hits along a ray.",
             "%-11s %-26s %9s %9s %8s %8s" % ("rays", "query", "ms", "Mrays/s", "N_box", "N_leaf")]
    res = {}
    for name, rays in (("camera_1Mi", torch.from_numpy(oa.camera_rays(ex.cam, W, W)).to(DEV)), ("random_1Mi", random_rays(ex, 1 << 20, 1))):
        n = rays.shape[0]
        _, cc = q.closest_counts(rays)
        cm = cc.float().mean(dim=0)
        kinds = [("closest", lambda: q.closest(rays), (float(cm[0]), float(cm[1]))),
                 ("hits_k1", lambda: q.hits(rays, 1), node_counts(ctx, rays, 1, False, 0)),
                 ("peel_4", lambda: peel(q, rays, 4, EPS * ext), None),
                 ("hits_k4", lambda: q.hits(rays, 4), node_counts(ctx, rays, 4, False, 0)),
                 ("peel_16", lambda: peel(q, rays, 16, EPS * ext), None),
                 ("hits_k16", lambda: q.hits(rays, 16), node_counts(ctx, rays, 16, False, 0)),
                 ("hits_k16_count", lambda: q.hits(rays, 16, count=True), node_counts(ctx, rays, 16, True, 0)),
                 ("count", lambda: q.count(rays), node_counts(ctx, rays, 0, True, 0)),
                 ("hits_k4_exhaustive", lambda: qx.hits(rays, 4), node_counts(ctx, rays, 4, False, _native.TRAVERSE_EXHAUSTIVE)),
                 ("count_exhaustive", lambda: qx.count(rays), node_counts(ctx, rays, 0, True, _native.TRAVERSE_EXHAUSTIVE))]
        for kind, fn, nodes in kinds:
            ms = timed(fn, a.reps)
            res[(name, kind)] = ms
            lines.append("%-11s %-26s %9.3f %9.1f %8s %8s" % (name, kind, ms, n / ms / 1e3, "%.1f" % nodes[0] if nodes else "", "%.1f" % nodes[1] if nodes else ""))
            print(lines[-1], flush=True)
        h = q.hits(rays, 16, count=True)
        same = bool(torch.equal(q.hits(rays, 1).t[:, 0].view(torch.int32), q.closest(rays).t.view(torch.int32)))
        lines.append("# %s: mean |H| = %.2f, rays with more than 16 hits: %.4f, hits(k = 1).t == closest().t bit for bit: %s" % (
            name, float(h.count.float().mean()), float((h.count > 16).float().mean()), same))
        print(lines[-1], flush=True)
    lines.append("#")
    for name in ("camera_1Mi", "random_1Mi"):
        r = lambda kind: res[(name, kind)]
        lines.append("# %s: hits(k=1) / closest() = %.2fx the time; hits(k=4) / peel_4 = %.2fx; hits(k=16) / peel_16 = %.2fx; count() / hits(k=16, count) = %.2fx; "
                     "exhaustive / ordered: hits(k=4) %.1fx, count() %.1fx" % (name, r("hits_k1") / r("closest"), r("hits_k4") / r("peel_4"), r("hits_k16") / r("peel_16"),
                                                                                r("count") / r("hits_k16_count"), r("hits_k4_exhaustive") / r("hits_k4"),
                                                                                r("count_exhaustive") / r("count")))
        if r("hits_k4") > r("peel_4"):
            lines.append("# %s: hits(k = 4) is SLOWER than four closest() calls (%.3f against %.3f ms)." % (name, r("hits_k4"), r("peel_4")))
        print(lines[-1], flush=True)
    assert ctx.stats()["stack_overflow"] == 0
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
