"""Time of one whole geometry step -- new triangle positions to a finished build -- on one GPU, by three routes.

    python tools/dynamic_rate.py [--reps 20] [--sizes 100000,1000000]

Scene: the synthetic triangle soup of the headline scene (scenes.synthetic) with its sphere light, at 100k and 1M triangles.  A step takes
positions that already exist (float32 [3 * ntri, 3], two alternating sets, made before the clock starts) and ends with the LBVH, the
traversal tree and the scene box of those positions on the device:

  existing_route   a new Scene from the numpy positions: add_mesh, add_shape, setup_data_cpu, setup_data_gpu (the context is kept, which
                   favours this route: a new context per step would add its creation)
  update_numpy     Scene.update_vertices(numpy array)
  update_torch     Scene.update_vertices(torch tensor on the device)

Host clock around each step, bracketed by ctx.sync(); median of --reps steps after two warm-up steps, all in one process.  Also printed:
stats()["ms_build"] of the last build (the share of a step that is the build itself) and the time of Context.vertex_update alone
(validate, scatter, face normals, box, with its two waits).  One JSON line per measurement; the two update routes are asserted to be no
slower than the existing one."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from ti_raytrace_amd import Example, PT_RGB, scenes     # noqa: E402

DEV = torch.device("cuda", 0)


def timed(ctx, fn, reps):
    ms = []
    for k in range(reps + 2):
        ctx.sync()
        t0 = time.perf_counter()
        fn(k)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    W = 64
    for ntri in [int(s) for s in a.sizes.split(",")]:
        ex = scenes.synthetic(W, W, 4, ntri=ntri, device_id=0)
        ex.build_scene()
        sc, ctx = ex.scene, ex.scene.ctx
        base = sc.vertex_np[:, 0:3].copy()
        sets = [base, (base * np.float32(0.97)).astype(np.float32)]
        dev_sets = [torch.from_numpy(p).to(DEV) for p in sets]
        torch.cuda.synchronize(DEV)
        mat, light_shape, light_mat = sc.material_cpu[0], sc.shape_cpu[0], sc.material_cpu[1]

        def existing(k):
            e = Example.example(W, W, 4, 0)
            e.scene._ctx = ctx
            e.scene.add_mesh(sets[k & 1].reshape(-1, 3, 3), mat)
            e.scene.add_shape(light_shape, light_mat)
            e.integrator = PT_RGB.PathTrace(W, W, e.cam, e.scene, 64)
            e.scene.setup_data_cpu()
            e.scene.setup_data_gpu()

        out = {"triangles": ntri, "reps": a.reps}
        out["existing_route_ms"] = timed(ctx, existing, a.reps)
        out["existing_route_ms_build"] = ctx.stats()["ms_build"]
        sc.update_vertices(sets[0])                         # (the scene object of the update routes is `sc`: same context, same topology)
        out["update_numpy_ms"] = timed(ctx, lambda k: sc.update_vertices(sets[k & 1]), a.reps)
        out["update_torch_ms"] = timed(ctx, lambda k: sc.update_vertices(dev_sets[k & 1]), a.reps)
        out["ms_build"] = ctx.stats()["ms_build"]
        out["vertex_update_alone_numpy_ms"] = timed(ctx, lambda k: ctx.vertex_update(0, 3 * ntri, sets[k & 1].ctypes.data, 3), a.reps)
        stream = torch.cuda.current_stream(DEV).cuda_stream
        out["vertex_update_alone_torch_ms"] = timed(ctx, lambda k: ctx.vertex_update(0, 3 * ntri, dev_sets[k & 1].data_ptr(), 3, device=True, stream=stream), a.reps)
        ctx.lbvh_build()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
        assert out["update_numpy_ms"] <= out["existing_route_ms"] and out["update_torch_ms"] <= out["existing_route_ms"], "an update route is slower than the existing one"
        del ex, sc, ctx, dev_sets


if __name__ == "__main__":
    main()
