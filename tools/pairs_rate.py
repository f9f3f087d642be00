"""Rate of the pair lists on device memory (PointQuery.within / TriangleQuery.pairs: csrc/tirt_pairs.hip) on one GPU, in one process.

    python tools/pairs_rate.py [--reps 5] [--out profiles/pairs_rate.txt]

Scene: the headline synthetic 100k-triangle scene.  Points: 1 Mi points near the surface (within 1 % of the extent of a point of a random scene triangle).
  within at bounds of 1 % and 2 % of the extent beside count_within at the same bound -- the same walk without the fill, so the ratio prices the second
  walk, the scan and the ordering --, with a capacity (one call, no host wait) and without (count, host wait, fill), ordered and not;
  within beside nearest(k=64, count=True) at the largest bound at which no row exceeds 64.
Triangles: pairs(0.0) for the second 100k-triangle mesh of tools/triangle_query_rate.py beside closest(max_distance=0.0), ordered and not.
ms = torch events on the current stream around one call, median of `--reps` after two warm-up calls.  Writes a table to --out and prints it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from ti_raytrace_amd import PointQuery, TriangleQuery, scenes     # noqa: E402
from triangle_query_rate import scene_triangles, timed            # noqa: E402

DEV = torch.device("cuda", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_rate.txt"))
    a = ap.parse_args()
    n = a.n
    ex = scenes.synthetic(64, 64, 4, device_id=0)
    ex.build_scene()
    g = torch.Generator(device=DEV); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    ext = float((hi - lo).max())
    st = torch.from_numpy(scene_triangles(ex.scene)).to(DEV)
    rnd = lambda *shape: torch.rand(shape, device=DEV, generator=g)
    pick = torch.randint(0, st.shape[0], (n,), device=DEV, generator=g)
    w = rnd(n, 3, 1); w = w / w.sum(dim=1, keepdim=True)
    pts = ((st[pick] * w).sum(dim=1) + (rnd(n, 3) - 0.5) * (0.02 * ext)).contiguous()
    other = scenes.synthetic(64, 64, 4, device_id=0, scene_seed=4321)
    other.scene.setup_data_cpu()
    mesh = torch.from_numpy(scene_triangles(other.scene)).to(DEV).contiguous()
    pq, tq = PointQuery(ex.scene), TriangleQuery(ex.scene)
    lines = ["# python tools/pairs_rate.py --reps %d   (one MI355X, one process)" % a.reps,
             "# 100k-triangle headline scene (scenes.synthetic, %d triangles).  points: %d points within 1 %% of the extent of a point of a random scene triangle;" % (st.shape[0], n),
             "# mesh: the %d triangles of a second synthetic scene (seed 4321) over the same box.  ms = torch events on the current stream around one call, median of %d" % (mesh.shape[0], a.reps),
             "# after 2 warm-up calls.  base = the sibling call named in the row; x base = ms / base ms.  capacity = the exact total: one call, no host wait;",
             "# exact = capacity None: the counting call, the host's read of the total, the filling call.  pairs = the total, longest = the longest row.",
             "%-34s %9s %10s %9s %8s %12s %8s" % ("call", "ms", "base", "base ms", "x base", "pairs", "longest")]

    def row(name, ms, base, bms, rs):
        lengths = rs[1:] - rs[:-1]
        lines.append("%-34s %9.3f %10s %9.3f %8.2f %12d %8d" % (name, ms, base, bms, ms / bms, int(rs[-1]), int(lengths.max())))
        print(lines[-1], flush=True)

    for pct in (1, 2):
        bound = 0.01 * pct * ext
        rs = pq.within(pts, bound).row_start
        total = int(rs[-1])
        cms = timed(lambda: pq.count_within(pts, bound), a.reps)
        row("within_%dpct capacity" % pct, timed(lambda: pq.within(pts, bound, capacity=total), a.reps), "count", cms, rs)
        row("within_%dpct capacity unordered" % pct, timed(lambda: pq.within(pts, bound, capacity=total, ordered=False), a.reps), "count", cms, rs)
        row("within_%dpct capacity attributes" % pct, timed(lambda: pq.within(pts, bound, attributes=True, capacity=total), a.reps), "count", cms, rs)
        row("within_%dpct exact" % pct, timed(lambda: pq.within(pts, bound), a.reps), "count", cms, rs)
    # the largest bound of a short ladder at which no row exceeds 64: nearest(k = 64) then returns the same rows
    bound = None
    for f in (0.004, 0.003, 0.002, 0.001, 0.0005):
        if int(pq.count_within(pts, f * ext).max()) <= 64:
            bound = f * ext
            break
    if bound is not None:
        rs = pq.within(pts, bound).row_start
        nms = timed(lambda: pq.nearest(pts, 64, bound, count=True), a.reps)
        row("within_%.2fpct capacity" % (100 * bound / ext), timed(lambda: pq.within(pts, bound, capacity=int(rs[-1])), a.reps), "nearest64", nms, rs)
        row("within_%.2fpct exact" % (100 * bound / ext), timed(lambda: pq.within(pts, bound), a.reps), "nearest64", nms, rs)
    rs = tq.pairs(mesh, 0.0).row_start
    total = int(rs[-1])
    cms = timed(lambda: tq.closest(mesh, 0.0), a.reps)
    row("pairs_0 mesh capacity", timed(lambda: tq.pairs(mesh, 0.0, capacity=total), a.reps), "closest_0", cms, rs)
    row("pairs_0 mesh capacity unordered", timed(lambda: tq.pairs(mesh, 0.0, capacity=total, ordered=False), a.reps), "closest_0", cms, rs)
    row("pairs_0 mesh capacity points", timed(lambda: tq.pairs(mesh, 0.0, points=True, capacity=total), a.reps), "closest_0", cms, rs)
    row("pairs_0 mesh exact", timed(lambda: tq.pairs(mesh, 0.0), a.reps), "closest_0", cms, rs)
    row("count_within_0 mesh", timed(lambda: tq.count_within(mesh, 0.0), a.reps), "closest_0", cms, rs)
    assert ex.scene.ctx.stats()["stack_overflow"] == 0
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
