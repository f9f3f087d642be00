"""Cost of the winding number (ti_raytrace_amd.PointQuery.winding_number: csrc/tirt_winding.hip) beside the closest point and the signed distance, on one GPU.

    python tools/winding_rate.py [--procs 5] [--reps 3] [--out profiles/winding_rate.txt]

Scenes: a torus of 100k and of 1M triangles.  Every figure is the median over --procs fresh processes (one per scene and round, each under its own time
limit), and inside a process the median of --reps calls after two warm-up calls: a host clock around the call and a device synchronise.  Per scene: the
moment table's build alone (tirt_lbvh_build, sync, then the clock around tirt_winding_prepare, which waits), and for two sets of 1 Mi queries (uniform in
the scene box; surface samples pushed out by 1 % of the extent) PointQuery.closest, .signed_distance and .winding_number at beta = 2 and 3, with the
child slots examined and the leaves evaluated per query (winding_counts).  Writes a table to --out and prints it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

CHILD_LIMIT = 420      # seconds for one process (one scene)


def child(k, n, reps):
    import torch
    from signed_distance_rate import torus
    from ti_raytrace_amd import Example, PointQuery, PT_RGB
    from ti_raytrace_amd import SceneData as SCD
    dev = torch.device("cuda", 0)
    tris = torus(k, k)
    ex = Example.example(32, 32, 4, 0)
    mat = SCD.Material(); mat.type = SCD.MAT_DISNEY; mat.setMetal(0.0); mat.setRough(0.5); mat.setColor([0.8, 0.8, 0.8, 1.0]); mat.alebdoTex = -1
    ex.scene.add_mesh(tris, mat)
    ex.integrator = PT_RGB.PathTrace(32, 32, ex.cam, ex.scene, 64)
    ex.build_scene()
    ctx = ex.scene.ctx
    q = PointQuery(ex.scene)
    g = torch.Generator(device=dev); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=dev); hi = torch.tensor(ex.scene.maxboundarynp[0], device=dev)
    ext = float((hi - lo).max())
    uni = (lo + (hi - lo) * torch.rand((n, 3), device=dev, generator=g)).contiguous()
    t = torch.from_numpy(tris.astype(np.float32)).to(dev)[torch.randint(0, tris.shape[0], (n,), device=dev, generator=g)]
    b = torch.rand((n, 2), device=dev, generator=g)
    b = torch.where((b.sum(dim=1) > 1.0)[:, None], 1.0 - b, b)
    nrm = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    surf = (t[:, 0] + (t[:, 1] - t[:, 0]) * b[:, 0:1] + (t[:, 2] - t[:, 0]) * b[:, 1:2] + nrm / nrm.norm(dim=1, keepdim=True) * (0.01 * ext)).contiguous()
    del t, b, nrm

    def clock(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(dev); ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))
    out = {"triangles": int(tris.shape[0])}
    build = []
    for _ in range(reps):
        ctx.lbvh_build(); ctx.sync()
        t0 = time.perf_counter(); ctx.winding_prepare(); build.append((time.perf_counter() - t0) * 1e3)
    out["table_build_ms"] = float(np.median(build))
    for name, pts in (("uniform", uni), ("surface_1pct", surf)):
        r = {"closest_ms": clock(lambda: q.closest(pts)), "signed_ms": clock(lambda: q.signed_distance(pts))}
        for beta in (2.0, 3.0):
            r["winding_b%g_ms" % beta] = clock(lambda: q.winding_number(pts, beta))
            _, counts = q.winding_counts(pts, beta)
            c = counts.double().mean(dim=0).cpu().numpy()
            r["winding_b%g_slots" % beta], r["winding_b%g_leaves" % beta] = float(c[0]), float(c[1])
        r["inside_share"] = float((q.winding_number(pts) > 0.5).double().mean())
        out[name] = r
    assert ctx.stats()["stack_overflow"] == 0
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sizes", default="224,708")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_rate.txt"))
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.n, a.reps)
    lines = ["# python tools/winding_rate.py --procs %d --reps %d   (one MI355X)" % (a.procs, a.reps),
             "# torus of 2 k^2 triangles; %d queries per set.  Every figure: the median over %d fresh processes of the median of %d calls (host clock around the call" % (a.n, a.procs, a.reps),
             "# and a device synchronise, after 2 warm-up calls).  table build: tirt_lbvh_build, sync, then the clock around tirt_winding_prepare alone.",
             "# slots / leaves: child slots examined and leaves evaluated per query (COUNT_NODES), means over the set."]
    for k in (int(x) for x in a.sizes.split(",")):
        runs = []
        for p in range(a.procs):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), "--n", str(a.n), "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], flush=True)
                raise SystemExit("winding_rate: process %d of size %d ended with %d: nothing further is started" % (p, k, r.returncode))
            runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print("size %d process %d done" % (k, p), flush=True)

        def med(*path):
            vals = []
            for r in runs:
                for key in path:
                    r = r[key]
                vals.append(r)
            return float(np.median(vals))
        lines += ["", "torus %d x %d: %d triangles; table build %.3f ms" % (k, k, runs[0]["triangles"], med("table_build_ms")),
                  "  %-14s %11s %11s %12s %12s %10s %10s %10s %10s %8s" % ("set", "closest ms", "signed ms", "beta 2 ms", "beta 3 ms", "b2 slots", "b2 leaves", "b3 slots", "b3 leaves", "inside")]
        for name in ("uniform", "surface_1pct"):
            lines.append("  %-14s %11.3f %11.3f %12.3f %12.3f %10.1f %10.1f %10.1f %10.1f %8.4f" % (
                name, med(name, "closest_ms"), med(name, "signed_ms"), med(name, "winding_b2_ms"), med(name, "winding_b3_ms"), med(name, "winding_b2_slots"),
                med(name, "winding_b2_leaves"), med(name, "winding_b3_slots"), med(name, "winding_b3_leaves"), med(name, "inside_share")))
            lines.append("  %-14s %11.1f %11.1f %12.1f %12.1f   Mqueries/s" % ("", *(a.n / med(name, key) / 1e3 for key in ("closest_ms", "signed_ms", "winding_b2_ms", "winding_b3_ms"))))
        print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
