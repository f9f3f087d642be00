"""Frame time of the Debug integrator (ti_raytrace_amd.Debug) on one GPU, and of the route a user had before it.

    python tools/debug_fps.py [--frames 200] [--warmup 10] [--host-frames 10] [--only cornell|synthetic]

Scenes: the headline synthetic 100k-triangle scene at 1024 x 1024 and the Cornell box at 512 x 512, all four views.  Per view:
warm-up, then `--frames` frames, each timed with the host clock around Debug.render() + a device sync: p50 / p99 ms per frame and
Mrays/s (one camera ray per pixel).  The same pixels through the earlier route -- numpy camera rays -> Context.trace_closest (rays
copied to the device, hit records copied back, one sync per call) -> numpy composition of the view -- are timed the same way in the
same process (`--host-frames` frames, albedo and fnormal).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ti_raytrace_amd import Debug, scenes          # noqa: E402
import debug_views as dv                            # noqa: E402  (numpy camera rays and view composition)


def pct(ms):
    ms = np.sort(np.asarray(ms))
    return float(np.percentile(ms, 50)), float(np.percentile(ms, 99))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    cases = [("synthetic", 1024, lambda W: scenes.synthetic(W, W, 4, device_id=0)), ("cornell", 512, lambda W: scenes.cornell_box(W, W, 4, device_id=0))]
    for name, W, mk in cases:
        if a.only and a.only != name:
            continue
        ex = mk(W)
        ex.integrator = Debug.Debug(W, W, ex.cam, ex.scene, 64)
        ex.build_scene()
        ctx, d, n = ex.scene.ctx, ex.integrator, W * W
        for mode in dv.MODES:
            d.mode = mode
            for f in range(a.warmup):
                ex.cam.frame = f
                d.render()
            ctx.sync()
            ms = []
            for f in range(a.frames):
                ex.cam.frame = f
                t0 = time.perf_counter()
                d.render()
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            p50, p99 = pct(ms)
            print(json.dumps({"scene": name, "W": W, "H": W, "route": "Debug.render", "view": mode, "frames": a.frames,
                              "p50_ms": round(p50, 4), "p99_ms": round(p99, 4), "mrays_s": round(n / p50 / 1e3, 1)}), flush=True)
        ctx.stats()                                       # raises on a traversal stack overflow
        for mode in ("albedo", "fnormal"):
            ms = []
            for f in range(a.host_frames + 1):
                t0 = time.perf_counter()
                rays = dv.camera_rays(ex.cam, W, W, 0)
                out, prim, _ = ctx.trace_closest(rays, 64)
                view = dv.compose(ex.scene, rays, out, prim, mode, W, W)
                if f > 0:                                 # (the first call allocates the batch buffers)
                    ms.append((time.perf_counter() - t0) * 1e3)
            p50, p99 = pct(ms)
            d.mode = mode
            ex.cam.frame = 0
            d.render()
            same = dv.same_bits(view, d.hdr.to_numpy())
            print(json.dumps({"scene": name, "W": W, "H": W, "route": "numpy rays + trace_closest + numpy view", "view": mode,
                              "frames": a.host_frames, "p50_ms": round(p50, 3), "p99_ms": round(p99, 3), "mrays_s": round(n / p50 / 1e3, 1),
                              "same_view_as_Debug": same}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
