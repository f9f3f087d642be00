"""What alpha cut-outs (Scene.add_texture(cutout=True), csrc/tirt_internal.h trace_leaf_step<VERIFY, CUTOUT>) cost the path tracer on one GPU.

    python tools/cutout_rate.py [--alt-lib <the parent commit's libtirt.so>] [--repeats 5] [--steps 8] [--frames-per-step 32] [--out profiles/cutout_rate.txt]

The headline scene of bench.py (100 000 triangles, 1024 x 1024, scene seed 1234), measured as tools/material_maps_rate.py measures: a run is `--steps` x
{render_frames(frames-per-step), update_frame}, a device sync, the host clock around both; ms per step = the run over its steps.  Every run is a process of
its own (one warm-up run, one timed run), and the configurations alternate, `--repeats` rounds, so that all see the same clocks and the same neighbours:
  a        untextured, this library                 a-alt   the same on --alt-lib (TIRT_LIB_PATH; left out without it)
  t-off    albedo-textured (every Disney material points at one procedural 1024 x 1024 RGBA texture, every vertex has a uv of its own), the cut-out flag off:
           the parent's behaviour, k_trace's opaque instantiations, camera rays through the candidate lists
  t-nolist t-off with the candidate lists switched off (option "primary_beams" 0): what a scene with cut-outs loses by not using them
  t-255    flag on, every alpha 255: the CUTOUT twins of k_trace, no list pass, the same image and the same rays as t-off -- the price of the test itself
  t-mask   flag on, a checker mask of 16 x 16-texel cells: another image, so each line carries the run's shaded hits and rays, and the time per ray
a against a-alt: the old kernels cost what they did (the tool says whether the medians differ by less than the runs' own spread).
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
    sys.path.insert(0, HERE)
    import ctypes
    import numpy as np
    from ti_raytrace_amd import scenes, _native
    from ti_raytrace_amd import SceneData as SCD
    if os.environ.get("TIRT_LIB_PATH"):
        # an older build lacks the entry points added since; the untextured run calls none of them
        _native._prefer_torch_hip_runtime()          # (as _native.lib() does before it maps the library: one HIP runtime per process)
        old = ctypes.CDLL(_native.LIB_PATH)
        for name in [n for n in _native.SIGNATURES if not hasattr(old, n)]:
            del _native.SIGNATURES[name]
    W = H = a.size
    fps, spp = a.frames_per_step, a.steps * a.frames_per_step
    ex = scenes.synthetic(W, H, spp, ntri=a.ntri, device_id=0)
    sc = ex.scene
    textured = a.child != "a"
    if textured:
        jj, ii = np.meshgrid(np.arange(1024), np.arange(1024))
        alpha = np.where(((ii // 16 + jj // 16) % 2) == 0, 255, 0) if a.child == "t-mask" else np.full_like(ii, 255)
        img = np.stack([(ii * 7 + jj * 3) % 256, ((ii // 16 + jj // 16) % 2) * 200 + 30, (ii ^ jj) % 256, alpha], axis=-1).astype(np.uint8)
        tid = sc.add_texture(img, cutout=True)
        if a.child in ("t-off", "t-nolist"):
            sc.texture_cutout[tid - 1] = 0
        for m in sc.material_cpu:
            if m.type == SCD.MAT_DISNEY:
                m.alebdoTex = tid
    sc.setup_data_cpu()
    if textured:
        sc.vertex_np[:, 6:8] = np.random.RandomState(1).uniform(0.0, 1.0, (sc.vertex_count, 2)).astype(np.float32)
    ex.integrator.setup_data_cpu(); ex.integrator.setup_data_gpu(); sc.setup_data_gpu()
    sc.total_area(); ex.frame_camera(0.8)                 # (the rest of scenes.synthetic.build_scene, whose packing step the uvs had to follow)
    ctx = sc.ctx
    if a.child == "t-nolist":
        ctx.set_option("primary_beams", 0)
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
    print(json.dumps({"config": a.child, "ms_per_step": ms[-1], "features": ctx.shade_features()[0], "list_rays": ctx.primary_beam_stats()["rays"],
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
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--run-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cutout_rate.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = ["a"] + (["a-alt"] if a.alt_lib else []) + ["t-off", "t-nolist", "t-255", "t-mask"]
    ms = {name: [] for name in configs}
    info = {}
    say(a, "%d x %d, %d triangles, %d steps of %d frames per run; every run a process of its own (one warm-up, one timed), %d rounds of %s"
        % (a.size, a.size, a.ntri, a.steps, a.frames_per_step, a.repeats, " / ".join(configs)))
    for _ in range(a.repeats):
        for name in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "a" if name == "a-alt" else name, "--steps", str(a.steps),
                   "--frames-per-step", str(a.frames_per_step), "--size", str(a.size), "--ntri", str(a.ntri)]
            env = dict(os.environ); env.pop("TIRT_LIB_PATH", None)
            if name == "a-alt":
                env["TIRT_LIB_PATH"] = os.path.abspath(a.alt_lib)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.run_timeout, env=env)
            if res.returncode != 0:                       # (a fault ends the whole measurement: nothing more is started on the GPU)
                raise SystemExit("%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            ms[name].append(rec["ms_per_step"]); info[name] = rec
            print(json.dumps({"run": name, "ms_per_step": rec["ms_per_step"]}), flush=True)
    med = {}
    for name in configs:
        med[name] = statistics.median(ms[name])
        r = info[name]
        say(a, "%-9s ms per step: median %.3f  min %.3f  max %.3f  (n = %d, feature word %s, %d camera rays through the lists; a run shades %d hits and traces %d rays: %.3f ns per ray)"
            % (name, med[name], min(ms[name]), max(ms[name]), len(ms[name]), r["features"], r["list_rays"], r["shaded"], r["rays"], med[name] * 1e6 * a.steps / r["rays"]),
            config=name, ms=ms[name])
    spread = lambda n: max(ms[n]) - min(ms[n])
    if "a-alt" in med:
        say(a, "a / a-alt = %.4f   (spreads: a %.3f, a-alt %.3f ms)" % (med["a"] / med["a-alt"], spread("a"), spread("a-alt")))
        diff, room = abs(med["a"] - med["a-alt"]), max(spread("a"), spread("a-alt"))
        say(a, "a against a-alt: the medians differ by %.3f ms, the larger spread is %.3f ms -- %s" % (
            diff, room, "EQUAL within the runs' own spread" if diff <= room else "NOT equal within the runs' own spread: an old kernel moved"),
            config="a", equal_within_spread=bool(diff <= room))
    else:
        say(a, "a-alt: not measured (no --alt-lib)")
    same = info["t-off"]["rays"] == info["t-255"]["rays"] == info["t-nolist"]["rays"] and info["t-off"]["shaded"] == info["t-255"]["shaded"]
    say(a, "t-off, t-nolist and t-255 trace %s" % ("the same rays and shade the same hits" if same else "DIFFERENT numbers of rays: the flag changed an opaque image"), same_work=bool(same))
    total, lists = med["t-255"] - med["t-off"], med["t-nolist"] - med["t-off"]
    say(a, "t-255 - t-off = %.3f ms per step (t-255 / t-off = %.4f): the price of the cut-out test on an opaque image; t-nolist - t-off = %.3f ms of it is the loss of the "
           "candidate lists (%s of the difference), t-255 - t-nolist = %.3f ms the CUTOUT twins themselves"
        % (total, med["t-255"] / med["t-off"], lists, ("%.0f %%" % (100.0 * lists / total)) if abs(total) > 1e-9 else "n/a", med["t-255"] - med["t-nolist"]))
    say(a, "t-mask / t-255 = %.4f per step, %.4f per ray (another image: half the texels are holes)"
        % (med["t-mask"] / med["t-255"], (med["t-mask"] / info["t-mask"]["rays"]) / (med["t-255"] / info["t-255"]["rays"])))


if __name__ == "__main__":
    main()
