"""Rate of the k-nearest and count-within queries on device memory (ti_raytrace_amd.PointQuery.nearest / .count_within: csrc/tirt_nearest.hip) on one GPU.

    python tools/nearest_rate.py [--reps 5] [--out profiles/nearest_rate.txt]

Scene: the headline synthetic 100k-triangle scene.  1 Mi query points uniform in the root box, in the order they were drawn.  Rows: closest() for scale;
nearest(k) for k = 1, 4, 16, 64 without a bound and with max_distance = 2 % of the extent; count_within at 1 % and 2 % of the extent.  Per row: ms (torch
events on the current stream around one call, dist2 + prim, median of `--reps` after two warm-up calls), Mqueries/s, the time per RETURNED neighbour
(ms over the entries that are not padding), the ratio to closest() of the same run, and the mean N_box / N_leaf per query of a COUNT_NODES walk.
Writes a table to --out and prints it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from ti_raytrace_amd import PointQuery, scenes, _native     # noqa: E402

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


def node_counts(ctx, pts, k, dmax, count):
    """mean N_box, N_leaf per query of a COUNT_NODES walk of the same query"""
    n = pts.shape[0]
    counts = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    d2 = torch.empty((n, max(k, 1)), dtype=torch.float32, device=DEV)
    cnt = torch.empty(n, dtype=torch.int32, device=DEV)
    ctx.query_nearest(pts.data_ptr(), n, 3, k, 64, _native.COUNT_NODES, dmax_all=float("inf") if dmax is None else dmax, out_d2=d2.data_ptr() if k else 0,
                      out_count=cnt.data_ptr() if count else 0, counts=counts.data_ptr(), stream=torch.cuda.current_stream(DEV).cuda_stream)
    c = counts.double()
    return float(c[:, 0].mean()), float(c[:, 1].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_rate.txt"))
    a = ap.parse_args()
    n = a.n
    ex = scenes.synthetic(64, 64, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    g = torch.Generator(device=DEV); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    ext = float((hi - lo).max())
    pts = (lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=g)).contiguous()
    q = PointQuery(ex.scene)
    lines = ["# python tools/nearest_rate.py --reps %d   (one MI355X)" % a.reps,
             "# 100k-triangle headline scene (scenes.synthetic), %d queries uniform in the root box.  ms = torch events on the current stream around one call" % n,
             "# (dist2 + prim; count_within: the count), median of %d after 2 warm-up calls; returned = mean entries per query that are not padding (count_within:" % a.reps,
             "# the mean count); ns/neighbour = ms over all returned entries; x closest = ms over the ms of closest() with the same bound in this run; N_box (four per",
             "# node visit) / N_leaf (primitive tests) = means per query of a COUNT_NODES walk.",
             "%-26s %9s %12s %10s %13s %10s %10s %10s" % ("query", "ms", "Mqueries/s", "returned", "ns/neighbour", "x closest", "N_box", "N_leaf")]
    base = {}
    for name, dmax in (("none", None), ("2pct", 0.02 * ext)):
        ms = timed(lambda: q.closest(pts, dmax), a.reps)
        base[name] = ms
        h, cnt = q.closest_counts(pts, dmax)
        cnt = cnt.double()
        found = float((h.prim >= 0).double().mean())
        lines.append("%-26s %9.3f %12.1f %10.3f %13.3f %10.2f %10.1f %10.1f" % ("closest_" + name, ms, n / ms / 1e3, found, ms * 1e6 / max(found * n, 1.0), 1.0,
                                                                                 float(cnt[:, 0].mean()), float(cnt[:, 1].mean())))
        print(lines[-1], flush=True)
    for name, dmax in (("none", None), ("2pct", 0.02 * ext)):
        for k in (1, 4, 16, 64):
            ms = timed(lambda: q.nearest(pts, k, dmax), a.reps)
            returned = float((q.nearest(pts, k, dmax).prim >= 0).double().sum(dim=1).mean())
            nbox, nleaf = node_counts(ctx, pts, k, dmax, False)
            lines.append("%-26s %9.3f %12.1f %10.3f %13.3f %10.2f %10.1f %10.1f" % ("nearest_k%d_%s" % (k, name), ms, n / ms / 1e3, returned,
                                                                                     ms * 1e6 / max(returned * n, 1.0), ms / base[name], nbox, nleaf))
            print(lines[-1], flush=True)
    for pct in (1, 2):
        dmax = 0.01 * pct * ext
        ms = timed(lambda: q.count_within(pts, dmax), a.reps)
        mean = float(q.count_within(pts, dmax).double().mean())
        nbox, nleaf = node_counts(ctx, pts, 0, dmax, True)
        lines.append("%-26s %9.3f %12.1f %10.3f %13.3f %10s %10.1f %10.1f" % ("count_within_%dpct" % pct, ms, n / ms / 1e3, mean, ms * 1e6 / max(mean * n, 1.0), "", nbox, nleaf))
        print(lines[-1], flush=True)
    sub = pts[:1 << 12].contiguous()
    scan = PointQuery(ex.scene, 64, _native.TRAVERSE_EXHAUSTIVE)
    for k in (4, 64):
        a_, b_ = scan.nearest(sub, k, 0.02 * ext, count=True), q.nearest(sub, k, 0.02 * ext, count=True)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in ((a_.dist2, b_.dist2), (a_.prim, b_.prim), (a_.count, b_.count)))
        lines.append("# scan against walk, 4 Ki queries, k = %d, bound 2 %%, with the count: equal bits: %s" % (k, same))
    assert ctx.stats()["stack_overflow"] == 0
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
