"""Rate of the ray queries on device memory (ti_raytrace_amd.RayQuery: csrc/tirt_query.hip) on one GPU, and of the host route.

    python tools/query_rate.py [--reps 20] [--only camera] [--host-reps 3]

Scene: the headline synthetic 100k-triangle scene (camera of a 1024 x 1024 film).  Ray sets: the 1 Mi camera rays of that film (frame 0,
the Debug frame's pixels), 1 Mi and 16 Mi rays with origins uniform in the scene's bounds and uniform directions.  Queries: closest (t +
prim), closest(attributes=True), occluded(tmax=inf), occluded(tmax=0.5 * closest t).  Each is timed with torch events on the current
stream around one call, median of `--reps` after two warm-up calls; the same rays through Context.trace_closest (numpy in, numpy out,
host clock, median of `--host-reps`) for comparison.  One JSON line per measurement.  `--only camera` runs the 1 Mi camera-ray set alone
(for a `rocprofv3 --kernel-trace --stats` split of pack / k_trace / resolve)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ti_raytrace_amd import RayQuery, scenes     # noqa: E402
import oracle_api as oa                          # noqa: E402  (numpy camera rays)

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


def random_rays(ex, n, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    o = lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=g)
    d = torch.randn((n, 3), device=DEV, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o, d], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    W = 1024
    ex = scenes.synthetic(W, W, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    q = RayQuery(ex.scene)
    sets = [("camera_1Mi", lambda: torch.from_numpy(oa.camera_rays(ex.cam, W, W)).to(DEV)),
            ("random_1Mi", lambda: random_rays(ex, 1 << 20, 1)),
            ("random_16Mi", lambda: random_rays(ex, 1 << 24, 2))]
    for name, mk in sets:
        if a.only and not name.startswith(a.only):
            continue
        rays = mk()
        n = rays.shape[0]
        t = q.closest(rays).t
        half = t * 0.5
        torch.cuda.synchronize(DEV)
        kinds = [("closest", lambda: q.closest(rays)),
                 ("closest_attributes", lambda: q.closest(rays, attributes=True)),
                 ("occluded_inf", lambda: q.occluded(rays)),
                 ("occluded_half_t", lambda: q.occluded(rays, half))]
        for kind, fn in kinds:
            ms = timed(fn, a.reps)
            rec = {"rays": name, "n": n, "query": kind, "ms": round(ms, 4), "mrays_s": round(n / ms / 1e3, 1),
                   "hit_fraction": round(float((t < 1e6).float().mean()), 4)}
            if kind == "occluded_half_t":
                rec["occluded_fraction"] = round(float(q.occluded(rays, half).float().mean()), 4)
            print(json.dumps(rec), flush=True)
        if a.host_reps > 0 and n <= (1 << 20):
            host = rays.cpu().numpy()
            ctx.trace_closest(host, 64, 0)
            ms = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter(); ctx.trace_closest(host, 64, 0); ms.append((time.perf_counter() - t0) * 1e3)
            m = float(np.median(ms))
            print(json.dumps({"rays": name, "n": n, "query": "host_trace_closest", "ms": round(m, 3), "mrays_s": round(n / m / 1e3, 1)}), flush=True)
    st = ctx.stats()
    assert st["stack_overflow"] == 0


if __name__ == "__main__":
    main()
