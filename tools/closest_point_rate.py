"""Rate of the closest-point queries on device memory (ti_raytrace_amd.PointQuery: csrc/tirt_closest_point.hip) on one GPU.

    python tools/closest_point_rate.py [--reps 5] [--out profiles/closest_point_rate.txt]

Scene: the headline synthetic 100k-triangle scene.  Query sets of 1 Mi points: (a) uniform in the root box, in the order they were drawn;
(b) surface samples pushed out by 1 % of the extent along the face normal; (c) set (b) with max_distance = 2 % of the extent; (d) set (a)
sorted in Morton order (30-bit codes over the root box) and in a fresh random permutation, which is what sorting the caller's queries for
coherence would buy.  Per set: Mqueries/s (torch events on the current stream around one call, median of `--reps` after two warm-up calls)
and the mean N_box / N_leaf per query of a COUNT_NODES walk.  For scale, in the same run: RayQuery.closest on 1 Mi random rays, and the
scan (TRAVERSE_EXHAUSTIVE) on 16 Ki queries of set (a).  Writes a table to --out and prints it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from ti_raytrace_amd import PointQuery, RayQuery, scenes, _native     # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, reps):
    for _ in range(2):
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


def morton_order(p, lo, hi):
    """argsort of 30-bit Morton codes of p over the box [lo, hi]"""
    g = ((p - lo) / (hi - lo)).clamp(0.0, 1.0).mul(1023.0).long()

    def spread(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        x = (x | (x << 2)) & 0x09249249
        return x
    return torch.argsort(spread(g[:, 0]) | (spread(g[:, 1]) << 1) | (spread(g[:, 2]) << 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_point_rate.txt"))
    a = ap.parse_args()
    n = a.n
    ex = scenes.synthetic(64, 64, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    g = torch.Generator(device=DEV); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    ext = float((hi - lo).max())
    uni = (lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=g)).contiguous()
    tris = torch.from_numpy(np.ascontiguousarray(ex.scene.vertex_np[:, 0:3], np.float32).reshape(-1, 3, 3)).to(DEV)
    k = torch.randint(0, tris.shape[0], (n,), device=DEV, generator=g)
    b = torch.rand((n, 2), device=DEV, generator=g)
    flip = b.sum(dim=1) > 1.0
    b = torch.where(flip[:, None], 1.0 - b, b)
    t = tris[k]
    nrm = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    surf = (t[:, 0] + (t[:, 1] - t[:, 0]) * b[:, 0:1] + (t[:, 2] - t[:, 0]) * b[:, 1:2] + nrm * (0.01 * ext)).contiguous()
    sets = [("a_uniform", uni, None), ("b_surface_1pct", surf, None), ("c_surface_1pct_max_2pct", surf, 0.02 * ext),
            ("d_uniform_morton", uni[morton_order(uni, lo, hi)].contiguous(), None),
            ("d_uniform_permuted", uni[torch.randperm(n, device=DEV, generator=g)].contiguous(), None)]
    q = PointQuery(ex.scene)
    lines = ["# python tools/closest_point_rate.py --reps %d   (one MI355X)" % a.reps,
             "# 100k-triangle headline scene (scenes.synthetic), %d queries per set.  ms = torch events on the current stream around one call of" % n,
             "# PointQuery.closest (dist2 + prim), median of %d after 2 warm-up calls; N_box (four per node visit) / N_leaf (primitive tests) = means per" % a.reps,
             "# query of a COUNT_NODES walk; found = fraction of queries with an answer.",
             "%-26s %9s %12s %10s %10s %8s" % ("set", "ms", "Mqueries/s", "N_box", "N_leaf", "found")]
    for name, pts, dmax in sets:
        ms = timed(lambda: q.closest(pts, dmax), a.reps)
        h, cnt = q.closest_counts(pts, dmax)
        cnt = cnt.double()
        lines.append("%-26s %9.3f %12.1f %10.1f %10.1f %8.4f" % (name, ms, pts.shape[0] / ms / 1e3, float(cnt[:, 0].mean()), float(cnt[:, 1].mean()),
                                                                  float((h.prim >= 0).double().mean())))
        print(lines[-1], flush=True)
    sub = uni[:1 << 14].contiguous()
    scan = PointQuery(ex.scene, 64, _native.TRAVERSE_EXHAUSTIVE)
    ms = timed(lambda: scan.closest(sub), a.reps)
    same = bool(torch.equal(scan.closest(sub).prim, q.closest(sub).prim))
    lines.append("%-26s %9.3f %12.3f %10.1f %10.1f %8s   (16 Ki queries of set a; equals the walk: %s)" % ("scan_16Ki", ms, sub.shape[0] / ms / 1e3, 0.0, float(ex.scene.primitive_count), "", same))
    d = torch.randn((n, 3), device=DEV, generator=g)
    rays = torch.cat([uni, d / d.norm(dim=1, keepdim=True)], dim=1).contiguous()
    rq = RayQuery(ex.scene)
    ms = timed(lambda: rq.closest(rays), a.reps)
    _, rc = rq.closest_counts(rays)
    rc = rc.double()
    lines.append("%-26s %9.3f %12.1f %10.1f %10.1f %8s   (RayQuery.closest on %d random rays from the points of set a: Mrays/s)"
                 % ("rays_closest", ms, n / ms / 1e3, float(rc[:, 0].mean()), float(rc[:, 1].mean()), "", n))
    assert ctx.stats()["stack_overflow"] == 0
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
