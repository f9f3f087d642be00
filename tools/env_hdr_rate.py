"""What an HDR (RGBE8) environment (Scene.add_env_hdr; include/tirt.h, "HDR environment") costs on one GPU.

    python tools/env_hdr_rate.py [--parent-root <checkout of the parent commit, built>] [--repeats 5] [--frames 32] [--out profiles/env_hdr_rate.txt]

The method of tools/env_sampling_rate.py: a run is `--frames` frames at 1024 x 1024 in one render_frames call between two device syncs, the host clock around
them; every run a process of its own (one warm-up run, one timed run), the configurations alternate, `--repeats` rounds:
  a         the headline scene of bench.py (100 000 triangles), this library     a-parent  the same from --parent-root (left out without it)
  b-ldr     the Teapot scene (glass, sphere light) under env.png x 5             b-hdr     the same image converted: every texel srgb_to_lrgb(8-bit value), encoded
  c-off     scenes.sun_ground under scenes.hdr_sun_sky(), switch off              c-on      the same with env_sampling=True
a against a-parent: a scene without an HDR image costs what it did (its kernels have equal instruction digests, tools/isa_stats.py).  b: ms per step and ns per
ray of the 8-bit and the RGBE8 kernel on one picture.  c: what the sampler costs on an HDR sky.  Median, minimum and maximum of each; every line goes to stdout as
JSON and, as text, to the end of --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def env_png_linear():
    """env.png as linear radiance [h, w, 3] float32: srgb_to_lrgb of each 8-bit value (float64 pow: the conversion is the measurement's input, not under test)"""
    import numpy as np
    from PIL import Image
    from ti_raytrace_amd import scenes
    c = np.asarray(Image.open(scenes.asset("image", "env.png")).convert("RGB"), np.float64) / 255.0
    return np.where(c < 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)


def child(a):
    sys.path.insert(0, os.path.abspath(a.package_root))
    from ti_raytrace_amd import scenes
    W = H = a.size
    if a.child == "a":
        ex = scenes.synthetic(W, H, a.frames, ntri=a.ntri, device_id=0)
    elif a.child in ("b-ldr", "b-hdr"):
        ex = scenes.single_model(W, H, a.frames, device_id=0)
        if a.child == "b-hdr":
            ex.scene.add_env_hdr(env_png_linear(), 5.0)
    else:
        ex = scenes.sun_ground(W, H, a.frames, 0, sky=scenes.hdr_sun_sky(), env_sampling=a.child == "c-on")
    ex.build_scene()
    ctx = ex.scene.ctx
    ms = []
    for _ in range(2):                                    # one warm-up run, one timed
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.set_option("job_frames", a.frames)
        ctx.stats_reset()
        ctx.sync()
        t0 = time.perf_counter()
        ex.integrator.render_frames(a.frames); ex.cam.update_frame(a.frames)
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ntri", type=int, default=100000)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=HERE)
    ap.add_argument("--child", default=None)
    ap.add_argument("--run-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "env_hdr_rate.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = ["a"] + (["a-parent"] if a.parent_root else []) + ["b-ldr", "b-hdr", "c-off", "c-on"]
    ms, rays, feat = {n: [] for n in configs}, {}, {}
    say(a, "%d x %d, one step of %d frames per run; every run a process of its own (one warm-up, one timed), %d rounds of %s"
        % (a.size, a.size, a.frames, a.repeats, " / ".join(configs)))
    for _ in range(a.repeats):
        for name in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "a" if name == "a-parent" else name, "--frames", str(a.frames), "--size", str(a.size),
                   "--ntri", str(a.ntri), "--package-root", a.parent_root if name == "a-parent" else HERE]
            env = dict(os.environ); env.pop("TIRT_LIB_PATH", None)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.run_timeout, env=env)
            if res.returncode != 0:                       # (a fault ends the whole measurement: nothing more is started on the GPU)
                raise SystemExit("%s: exit status %d\n%s" % (name, res.returncode, res.stderr[-2000:]))
            rec = json.loads(res.stdout.strip().splitlines()[-1])
            ms[name].append(rec["ms_per_step"]); rays[name] = rec["rays"]; feat[name] = rec["features"]
    med = {}
    for name in configs:
        med[name] = statistics.median(ms[name])
        say(a, "%-9s ms per step: median %.3f  min %.3f  max %.3f  (n = %d); %d rays per run, %.4f ns per ray, feature word %d"
            % (name, med[name], min(ms[name]), max(ms[name]), len(ms[name]), rays[name], med[name] * 1e6 / max(rays[name], 1), feat[name]), config=name, ms=ms[name])
    if "a-parent" in med:
        say(a, "a / a-parent = %.4f   (spreads: a %.3f, a-parent %.3f ms)" % (med["a"] / med["a-parent"], max(ms["a"]) - min(ms["a"]), max(ms["a-parent"]) - min(ms["a-parent"])))
    else:
        say(a, "a-parent: not measured (no --parent-root)")
    say(a, "b-hdr / b-ldr = %.4f in time, %.4f in rays, %.4f in ns per ray   (spreads: b-ldr %.3f, b-hdr %.3f ms)"
        % (med["b-hdr"] / med["b-ldr"], rays["b-hdr"] / max(rays["b-ldr"], 1), (med["b-hdr"] / max(rays["b-hdr"], 1)) / (med["b-ldr"] / max(rays["b-ldr"], 1)),
           max(ms["b-ldr"]) - min(ms["b-ldr"]), max(ms["b-hdr"]) - min(ms["b-hdr"])))
    say(a, "c-on / c-off = %.4f in time, %.4f in rays" % (med["c-on"] / med["c-off"], rays["c-on"] / max(rays["c-off"], 1)))


if __name__ == "__main__":
    main()
