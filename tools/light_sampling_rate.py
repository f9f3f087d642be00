"""What choosing emitters by power (PT_RGB.PathTrace(light_sampling="power"); include/tirt.h, "Choosing emitters by power") costs on one GPU.

    python tools/light_sampling_rate.py [--parent-root <checkout of the parent commit, built>] [--repeats 5] [--steps 1] [--frames-per-step 32] [--out profiles/light_sampling_rate.txt]

The method of tools/env_sampling_rate.py: a run is bench.py's timed region -- `--steps` x {render_frames(frames-per-step), update_frame}, a device sync, the host
clock around both --, every run a process of its own (one warm-up run, one timed run), the configurations alternate, `--repeats` rounds:
  a        the headline scene of bench.py (100 000 triangles, 1024 x 1024), this library      a-parent   the same from --parent-root (left out without it)
  l-off    scenes.lamp_and_embers at 1024 x 1024, light_sampling="uniform"                     l-on       the same with "power"
  v-off    the Veach scene through PT_RGB at 1024 x 1024, "uniform"                            v-on       the same with "power"
a against a-parent: a scene without the switch costs what it did (its kernels have equal instruction digests, tools/isa_stats.py).  on against off: ms per step,
rays per run and ns per ray -- the switched-on render aims its shadow rays elsewhere and its paths end elsewhere, so the rays are counted too.
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
    from ti_raytrace_amd import scenes
    W = H = a.size
    fps, spp = a.frames_per_step, a.steps * a.frames_per_step
    mode = "power" if a.child.endswith("-on") else "uniform"
    if a.child == "a":
        ex = scenes.synthetic(W, H, spp, ntri=a.ntri, device_id=0)
    elif a.child.startswith("l-"):
        ex = scenes.lamp_and_embers(W, H, spp, device_id=0, light_sampling=mode)
    else:
        ex = scenes.veach_bdpt(W, H, spp, device_id=0, integrator="pt", light_sampling=mode)
    ex.build_scene()
    ctx = ex.scene.ctx
    ms = []
    for _ in range(2):                                    # one warm-up run, one timed
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.set_option("job_frames", spp)
        ctx.stats_reset()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ex.integrator.render_frames(fps); ex.cam.update_frame(fps)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    st = ctx.stats()                                      # raises on a traversal stack overflow
    print(json.dumps({"config": a.child, "ms_per_step": ms[-1], "rays": int(st["rays_closest"]) + int(st["rays_shadow"]), "features": ctx.shade_features()[0]}), flush=True)
    ctx.close()


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--frames-per-step", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ntri", type=int, default=100000)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=HERE)
    ap.add_argument("--child", default=None)
    ap.add_argument("--run-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "light_sampling_rate.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = [("a", HERE)] + ([("a-parent", a.parent_root)] if a.parent_root else []) + [(n, HERE) for n in ("l-off", "l-on", "v-off", "v-on")]
    ms, rays, feat = {n: [] for n, _ in configs}, {}, {}
    say(a, "%d x %d, %d steps of %d frames per run; every run a process of its own (one warm-up, one timed), %d rounds of %s"
        % (a.size, a.size, a.steps, a.frames_per_step, a.repeats, " / ".join(n for n, _ in configs)))
    for _ in range(a.repeats):
        for name, root in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "a" if name == "a-parent" else name, "--package-root", root, "--steps", str(a.steps),
                   "--frames-per-step", str(a.frames_per_step), "--size", str(a.size), "--ntri", str(a.ntri)]
            env = dict(os.environ); env.pop("TIRT_LIB_PATH", None)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.run_timeout, env=env)
            if res.returncode != 0:                       # (a fault ends the whole measurement: nothing more is started on the GPU)
                raise SystemExit("%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            ms[name].append(rec["ms_per_step"]); rays[name] = rec["rays"]; feat[name] = rec["features"]
            print("%s %.3f ms" % (name, rec["ms_per_step"]), file=sys.stderr, flush=True)
    med = {}
    for name, _ in configs:
        med[name] = statistics.median(ms[name])
        say(a, "%-9s ms per step: median %.3f  min %.3f  max %.3f  (n = %d); %d rays per run, %.4f ns per ray, feature word %d"
            % (name, med[name], min(ms[name]), max(ms[name]), len(ms[name]), rays[name], med[name] * a.steps * 1e6 / max(rays[name], 1), feat[name]), config=name, ms=ms[name])
    if "a-parent" in med:
        say(a, "a / a-parent = %.4f   (spreads: a %.3f, a-parent %.3f ms)" % (med["a"] / med["a-parent"], max(ms["a"]) - min(ms["a"]), max(ms["a-parent"]) - min(ms["a-parent"])))
    else:
        say(a, "a-parent: not measured (no --parent-root)")
    for s, what in (("l", "lamp_and_embers"), ("v", "veach")):
        say(a, "%s: on / off = %.4f in time, %.4f in rays" % (what, med[s + "-on"] / med[s + "-off"], rays[s + "-on"] / max(rays[s + "-off"], 1)))


if __name__ == "__main__":
    main()
