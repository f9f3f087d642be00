"""Cost of the signed distance (ti_raytrace_amd.PointQuery.signed_distance: csrc/tirt_signed_distance.hip, the SIGNED kernels of csrc/tirt_closest_point.hip)
against the unsigned closest point in the same process, on one GPU.

    python tools/signed_distance_rate.py [--reps 5] [--out profiles/signed_distance_rate.txt]

Scenes: a torus of 100k and of 1M triangles (closed, every vertex shared by six triangles: the build has something to find; mesh_report must say closed).
Per scene: the table's build -- tirt_signed_distance_prepare (host clock around the call, which waits; its stack is 4096 entries, so its grid is the
small one that fits their tails) and the lazy build inside the first signed query after tirt_lbvh_build (torch events; stack_size 64, the full grid) --
and, for three sets of 1 Mi queries (uniform in the box; surface samples pushed out by 1 % of the extent; those with max_distance = 2 %), PointQuery.closest
against PointQuery.signed_distance, median of --reps after two warm-up calls each, alternating.  Writes a table to --out and prints it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from ti_raytrace_amd import Example, PointQuery, PT_RGB          # noqa: E402
from ti_raytrace_amd import SceneData as SCD                     # noqa: E402

DEV = torch.device("cuda", 0)


def torus(nu, nv, R=2.0, r=0.75):
    """2 nu nv triangles, outward, every position computed once (float32) and shared"""
    u = 2.0 * np.pi * np.arange(nu) / nu; v = 2.0 * np.pi * np.arange(nv) / nv
    cu, su, cv, sv = np.cos(u)[:, None], np.sin(u)[:, None], np.cos(v)[None, :], np.sin(v)[None, :]
    P = np.stack([(R + r * cv) * cu, (R + r * cv) * su, np.broadcast_to(r * sv, (nu, nv))], axis=2).astype(np.float32).astype(np.float64)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = P[i, j], P[i1, j], P[i1, j1], P[i, j1]
    return np.concatenate([np.stack([a, b, c], axis=2), np.stack([a, c, d], axis=2)], axis=0).reshape(-1, 3, 3)


def timed_pair(f0, f1, reps):
    """medians of two calls timed alternately with torch events"""
    for _ in range(2):
        f0(); f1()
    torch.cuda.synchronize(DEV)
    s = torch.cuda.current_stream(DEV)
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((f0, f1)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); fn(); e1.record(s)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return float(np.median(ms[0])), float(np.median(ms[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sizes", default="224,708")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_distance_rate.txt"))
    a = ap.parse_args()
    n = a.n
    lines = ["# python tools/signed_distance_rate.py --reps %d   (one MI355X)" % a.reps,
             "# torus of 2 k^2 triangles; %d queries per set.  build: tirt_signed_distance_prepare (host clock, waits; stack 4096) and the lazy build inside the first" % n,
             "# signed query after tirt_lbvh_build (torch events around that call of 64 queries less a later one; stack 64).  ms = torch events around one call of",
             "# PointQuery.closest (dist2 + prim) / PointQuery.signed_distance (dist + prim), medians of %d after 2 warm-up calls, alternating; ratio = signed / unsigned time." % a.reps]
    for k in (int(x) for x in a.sizes.split(",")):
        tris = torus(k, k)
        ex = Example.example(32, 32, 4, 0)
        mat = SCD.Material(); mat.type = SCD.MAT_DISNEY; mat.setMetal(0.0); mat.setRough(0.5); mat.setColor([0.8, 0.8, 0.8, 1.0]); mat.alebdoTex = -1
        ex.scene.add_mesh(tris, mat)
        ex.add_sphere_light(pos=(0.0, 0.0, 3.0), radius=0.5, emission=50.0)
        ex.integrator = PT_RGB.PathTrace(32, 32, ex.cam, ex.scene, 64)
        ex.build_scene()
        ctx = ex.scene.ctx
        q = PointQuery(ex.scene)
        g = torch.Generator(device=DEV); g.manual_seed(1)
        lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
        ext = float((hi - lo).max())
        uni = (lo + (hi - lo) * torch.rand((n, 3), device=DEV, generator=g)).contiguous()
        t = torch.from_numpy(tris.astype(np.float32)).to(DEV)[torch.randint(0, tris.shape[0], (n,), device=DEV, generator=g)]
        b = torch.rand((n, 2), device=DEV, generator=g)
        b = torch.where((b.sum(dim=1) > 1.0)[:, None], 1.0 - b, b)
        nrm = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        surf = (t[:, 0] + (t[:, 1] - t[:, 0]) * b[:, 0:1] + (t[:, 2] - t[:, 0]) * b[:, 1:2] + nrm / nrm.norm(dim=1, keepdim=True) * (0.01 * ext)).contiguous()
        few = uni[:64].contiguous()
        prep, lazy = [], []
        for _ in range(a.reps):
            ctx.lbvh_build(); ctx.sync()
            t0 = time.perf_counter(); rep = q.mesh_report(); prep.append((time.perf_counter() - t0) * 1e3)
            ctx.lbvh_build(); ctx.sync()
            s = torch.cuda.current_stream(DEV)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s); q.signed_distance(few); e1.record(s); q.signed_distance(few); e2.record(s)
            e2.synchronize()
            lazy.append(e0.elapsed_time(e1) - e1.elapsed_time(e2))
        assert rep["closed"], rep
        lines.append("")
        lines.append("torus %d x %d: %d triangles, mesh_report %s" % (k, k, tris.shape[0], rep))
        lines.append("  table build: prepare %.3f ms (host clock, median of %d), lazy inside the first signed query %.3f ms" % (float(np.median(prep)), a.reps, float(np.median(lazy))))
        lines.append("  %-26s %12s %12s %14s %14s %8s %8s" % ("set", "unsigned ms", "signed ms", "unsigned Mq/s", "signed Mq/s", "ratio", "inside"))
        print("\n".join(lines[-3:]), flush=True)
        for name, pts, dmax in (("a_uniform", uni, None), ("b_surface_1pct", surf, None), ("c_surface_1pct_max_2pct", surf, 0.02 * ext)):
            mu, ms = timed_pair(lambda: q.closest(pts, dmax), lambda: q.signed_distance(pts, dmax), a.reps)
            h, u = q.signed_distance(pts, dmax), q.closest(pts, dmax)
            assert torch.equal(h.prim, u.prim) and torch.equal(h.dist.abs(), u.dist2.sqrt())
            lines.append("  %-26s %12.3f %12.3f %14.1f %14.1f %8.3f %8.4f" % (name, mu, ms, n / mu / 1e3, n / ms / 1e3, ms / mu, float((h.dist < 0).double().mean())))
            print(lines[-1], flush=True)
        assert ctx.stats()["stack_overflow"] == 0
        del ex, ctx, q
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
