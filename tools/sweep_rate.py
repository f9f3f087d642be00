"""Rate of the sphere sweep on device memory (ti_raytrace_amd.SweepQuery.cast / .blocked: csrc/tirt_sweep.hip) on one GPU.

    python tools/sweep_rate.py [--runs 5] [--n 1048576] [--out profiles/sweep_rate.txt]

Scene: the headline synthetic 100k-triangle scene.  Query sets of 1 Mi segments each: `camera` (a pinhole at 1.5 extents looking at the scene, d = the
ray to the far side: coherent) and `random` (both end points uniform in the root box, d = p1 - p0), tmax = 1.  Per set: SweepQuery.cast and .blocked at
radii of 0.1 %, 1 % and 5 % of the extent; beside them, in the same run, RayQuery.closest on the same rays (the walk's floor: no radius) and 16 steps of
PointQuery.closest along each segment (what a caller does today: 16 launches, and it tunnels through anything thinner than a step).  Every figure is
host clock around one call with a device sync before and after, after one warm-up call; a run is a process of its own (`--child`), the runs alternate
through all the variants, and the table holds the medians over the runs.  N_box / N_leaf per query come from cast_counts.  Nothing gates on these figures."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
RADII = (0.001, 0.01, 0.05)


def child(n):
    import torch
    from ti_raytrace_amd import PointQuery, RayQuery, SweepQuery, scenes
    dev = torch.device("cuda", 0)
    ex = scenes.synthetic(64, 64, 4, device_id=0)
    ex.build_scene()
    g = torch.Generator(device=dev); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=dev); hi = torch.tensor(ex.scene.maxboundarynp[0], device=dev)
    ext = float((hi - lo).max()); mid = 0.5 * (lo + hi)
    rnd = lambda *shape: torch.rand(shape, device=dev, generator=g)
    p0, p1 = lo + (hi - lo) * rnd(n, 3), lo + (hi - lo) * rnd(n, 3)
    random = torch.cat([p0, p1 - p0], dim=1).contiguous()
    side = int(np.sqrt(n))
    eye = mid + torch.tensor([0.0, 0.0, 1.5 * ext], device=dev)
    ys, xs = torch.meshgrid(torch.linspace(-0.6, 0.6, side, device=dev), torch.linspace(-0.6, 0.6, n // side, device=dev), indexing="ij")
    tgt = mid + torch.stack([xs.reshape(-1) * ext, ys.reshape(-1) * ext, torch.full((side * (n // side),), -0.6 * ext, device=dev)], dim=1)
    camera = torch.cat([eye.expand_as(tgt), tgt - eye], dim=1).contiguous()
    sq, rq, pq = SweepQuery(ex.scene), RayQuery(ex.scene), PointQuery(ex.scene)

    def timed(fn):
        fn(); torch.cuda.synchronize(dev)
        t = time.perf_counter(); fn(); torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3

    def stepped(rays):
        for k in range(16):
            pq.closest(rays[:, 0:3] + rays[:, 3:6] * ((k + 0.5) / 16.0))
    out = {}
    for name, rays in (("camera", camera), ("random", random)):
        out[name + " ray_closest"] = dict(ms=timed(lambda: rq.closest(rays)))
        out[name + " point_x16"] = dict(ms=timed(lambda: stepped(rays)))
        for rad in RADII:
            r = rad * ext
            h, cnt = sq.cast_counts(rays, r, 1.0)
            cnt = cnt.double()
            out["%s cast %g" % (name, rad)] = dict(ms=timed(lambda: sq.cast(rays, r, 1.0)), hit=float((h.prim >= 0).double().mean()),
                                                    start=float((h.t == 0).double().mean()), nbox=float(cnt[:, 0].mean()), nleaf=float(cnt[:, 1].mean()))
            out["%s blocked %g" % (name, rad)] = dict(ms=timed(lambda: sq.blocked(rays, r, 1.0)))
    assert ex.scene.ctx.stats()["stack_overflow"] == 0
    print("SWEEP_RATE " + json.dumps(dict(n=int(rays.shape[0]), tris=int(ex.scene.primitive_count), rows=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_rate.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.n)
    runs = []
    for _ in range(a.runs):                                   # a fresh process per run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n)], stdout=subprocess.PIPE, text=True, check=True, timeout=300)
        runs.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("SWEEP_RATE ")][-1][len("SWEEP_RATE "):]))
    n = runs[0]["n"]
    lines = ["# python tools/sweep_rate.py --runs %d   (one MI355X)" % a.runs,
             "# headline synthetic scene (%d primitives), %d segments per set, tmax = 1; camera: a pinhole 1.5 extents away, random: both ends uniform in the root box." % (runs[0]["tris"], n),
             "# ms = host clock around one call with a device sync before and after, one warm-up call, median of %d runs, each a process of its own;" % a.runs,
             "# ray_closest = RayQuery.closest on the same rays (no radius: the walk's floor); point_x16 = 16 PointQuery.closest calls along each segment (today's way);",
             "# cast R / blocked R = SweepQuery at a radius of R x the extent; hit / start = share of queries with a contact / with T = 0; N_box, N_leaf per query (cast_counts)",
             "%-24s %9s %12s %8s %8s %9s %9s" % ("query", "ms", "Mqueries/s", "hit", "start", "N_box", "N_leaf")]
    for key in runs[0]["rows"]:
        ms = float(np.median([r["rows"][key]["ms"] for r in runs]))
        row = runs[0]["rows"][key]
        extra = "%8.3f %8.3f %9.1f %9.1f" % (row["hit"], row["start"], row["nbox"], row["nleaf"]) if "hit" in row else ""
        lines.append("%-24s %9.3f %12.1f %s" % (key, ms, n / ms / 1e3, extra))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
