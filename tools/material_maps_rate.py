"""What roughness, metallic and normal-map textures (Material.roughTex / metalTex / normalTex, csrc/tirt_device.h tex_normal) cost the path tracer on one GPU.

    python tools/material_maps_rate.py [--parent-root <checkout of the parent commit, built>] [--alt-lib <another build of this library>] [--repeats 5] [--steps 8] [--frames-per-step 32] [--out profiles/material_maps_rate.txt]

The headline scene of bench.py (100 000 triangles, 1024 x 1024, scene seed 1234).  A run is bench.py's timed region, as in tools/texture_rate.py: `--steps` x
{render_frames(frames-per-step), update_frame}, a device sync, the host clock around both; ms per step = the run over its steps.  Every run is a process of
its own (one warm-up run, one timed run), and the configurations alternate, `--repeats` rounds, so that all see the same clocks and the same neighbours:
  a   untextured, this library                      a-parent   the same from --parent-root (left out without it)
  c   albedo only: every Disney material points at a procedural 1024 x 1024 texture, every vertex has a uv of its own: k_shade<SF_ALL | SF_TEXTURE>
                                                    c-parent   the same from --parent-root
  d   albedo + roughness + metallic + normal map on every Disney material (four 1024 x 1024 textures): k_shade<SF_ALL | SF_TEXTURE | SF_TEXTURE_PARAM>
  d-alt  d on --alt-lib (TIRT_LIB_PATH; e.g. `make EXTRA=-DSH_MIN_WAVES_MAPS=5 OUT=...`: the other launch bound of the new kernel; left out without it)
a against a-parent and c against c-parent: the old kernels cost what they did (the tool says whether the medians differ by less than the runs' own spread).
d against c: roughness, metallic and a mapped normal change where the paths go and how long they live, so d is another image with another number of rays
than c; each line therefore carries the run's shaded hits and rays, and the time per ray beside the time per step.
Median, minimum and maximum of each; every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, os.path.abspath(a.package_root))
    import numpy as np
    from ti_raytrace_amd import scenes
    from ti_raytrace_amd import SceneData as SCD
    W = H = a.size
    fps, spp = a.frames_per_step, a.steps * a.frames_per_step
    ex = scenes.synthetic(W, H, spp, ntri=a.ntri, device_id=0)
    sc = ex.scene
    textured = a.child in ("c", "d")
    if textured:
        jj, ii = np.meshgrid(np.arange(1024), np.arange(1024))
        img = np.stack([(ii * 7 + jj * 3) % 256, ((ii // 16 + jj // 16) % 2) * 200 + 30, (ii ^ jj) % 256], axis=-1).astype(np.uint8)
        ids = [sc.add_texture(img)]
        if a.child == "d":
            orm = np.stack([(ii + jj) % 256, (ii * 5 + jj * 11) % 256, ((ii // 32 + jj // 8) % 2) * 255], axis=-1).astype(np.uint8)      # .g roughness, .b metallic
            rough2 = np.roll(orm, 97, axis=0)
            n = np.stack([np.sin(ii * 0.13) * 0.35, np.cos(jj * 0.11) * 0.35, np.ones_like(ii, dtype=np.float64)], axis=-1)
            n /= np.linalg.norm(n, axis=2, keepdims=True)
            nm = np.clip(np.rint((n * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
            ids += [sc.add_texture(rough2), sc.add_texture(orm), sc.add_texture(nm)]
        for m in sc.material_cpu:
            if m.type == SCD.MAT_DISNEY:
                m.alebdoTex = ids[0]
                if a.child == "d":
                    m.roughTex, m.metalTex, m.normalTex = ids[1], ids[2], ids[3]
    sc.setup_data_cpu()
    if textured:
        sc.vertex_np[:, 6:8] = np.random.RandomState(1).uniform(0.0, 1.0, (sc.vertex_count, 2)).astype(np.float32)
    ex.integrator.setup_data_cpu(); ex.integrator.setup_data_gpu(); sc.setup_data_gpu()
    sc.total_area(); ex.frame_camera(0.8)                 # (the rest of scenes.synthetic.build_scene, whose packing step the uvs had to follow)
    ctx = sc.ctx
    ms = []
    for _ in range(2):                                    # one warm-up run, one timed
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.set_option("job_frames", spp)
        ctx.sync()
        ctx.stats_reset()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ex.integrator.render_frames(fps); ex.cam.update_frame(fps)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    st = ctx.stats()                                      # raises on a traversal stack overflow; the counts of the timed run
    print(json.dumps({"config": a.child, "ms_per_step": ms[-1], "features": ctx.shade_features()[0],
                      "shaded": int(st["shaded"]), "rays": int(st["rays_closest"]) + int(st["rays_shadow"])}), flush=True)
    ctx.close()


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--frames-per-step", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ntri", type=int, default=100000)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--package-root", default=HERE)
    ap.add_argument("--child", default=None)
    ap.add_argument("--run-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "material_maps_rate.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    parent = [("a-parent", a.parent_root), ("c-parent", a.parent_root)] if a.parent_root else []
    configs = [("a", HERE)] + parent[:1] + [("c", HERE)] + parent[1:] + [("d", HERE)] + ([("d-alt", HERE)] if a.alt_lib else [])
    ms = {name: [] for name, _ in configs}
    feat, work = {}, {}
    say(a, "%d x %d, %d triangles, %d steps of %d frames per run; every run a process of its own (one warm-up, one timed), %d rounds of %s"
        % (a.size, a.size, a.ntri, a.steps, a.frames_per_step, a.repeats, " / ".join(n for n, _ in configs)))
    for _ in range(a.repeats):
        for name, root in configs:
            # (the child of a parent checkout is this file: it uses nothing the parent's package lacks in configurations a and c)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name[0], "--package-root", root, "--steps", str(a.steps),
                   "--frames-per-step", str(a.frames_per_step), "--size", str(a.size), "--ntri", str(a.ntri)]
            env = dict(os.environ); env.pop("TIRT_LIB_PATH", None)
            if name == "d-alt":
                env["TIRT_LIB_PATH"] = os.path.abspath(a.alt_lib)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.run_timeout, env=env)
            if res.returncode != 0:                       # (a fault ends the whole measurement: nothing more is started on the GPU)
                raise SystemExit("%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            ms[name].append(rec["ms_per_step"]); feat[name] = rec["features"]; work[name] = (rec["shaded"], rec["rays"])
            print(json.dumps({"run": name, "ms_per_step": rec["ms_per_step"]}), flush=True)
    med = {}
    for name, _ in configs:
        med[name] = statistics.median(ms[name])
        say(a, "%-9s ms per step: median %.3f  min %.3f  max %.3f  (n = %d, feature word %s; a run shades %d hits and traces %d rays: %.3f ns per ray)"
            % (name, med[name], min(ms[name]), max(ms[name]), len(ms[name]), feat[name], work[name][0], work[name][1], med[name] * 1e6 * a.steps / work[name][1]),
            config=name, ms=ms[name])
    spread = lambda n: max(ms[n]) - min(ms[n])
    for x in ("a", "c"):
        if x + "-parent" in med:
            say(a, "%s / %s-parent = %.4f   (spreads: %s %.3f, %s-parent %.3f ms)" % (x, x, med[x] / med[x + "-parent"], x, spread(x), x, spread(x + "-parent")))
            diff, room = abs(med[x] - med[x + "-parent"]), max(spread(x), spread(x + "-parent"))
            say(a, "%s against %s-parent: the medians differ by %.3f ms, the larger spread is %.3f ms -- %s" % (
                x, x, diff, room, "EQUAL within the runs' own spread" if diff <= room else "NOT equal within the runs' own spread: an old kernel moved"),
                config=x, equal_within_spread=bool(diff <= room))
        else:
            say(a, "%s-parent: not measured (no --parent-root)" % x)
    say(a, "c - a = %.3f ms per step: albedo textures.   d - c = %.3f ms per step (d / c = %.4f): roughness, metallic and normal maps on top (%d frames of %d x %d)"
        % (med["c"] - med["a"], med["d"] - med["c"], med["d"] / med["c"], a.frames_per_step, a.size, a.size))
    if "d-alt" in med:
        say(a, "d-alt / d = %.4f   (spreads: d %.3f, d-alt %.3f ms)" % (med["d-alt"] / med["d"], spread("d"), spread("d-alt")))


if __name__ == "__main__":
    main()
