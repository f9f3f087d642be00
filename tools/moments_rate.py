"""What the path tracer's sample moments (PathTrace(moments=True), csrc/tirt_moments.hip) cost on one GPU.

    python tools/moments_rate.py [--steps 8] [--warmup 1] [--frames-per-step 32] [--repeats 5] [--calls 64] [--out profiles/moments_overhead.txt]
    python tools/moments_rate.py --off-only --package-root <checkout of the parent commit> --label parent ...
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/moments_rate.py --repeats 1 --out ""
    python tools/moments_rate.py --kernel-stats <dir> ...          (no device: one line per kernel of that trace, k_moments' share)

The headline scene of bench.py (100 000 triangles, 1024 x 1024, scene seed 1234) on one context.  A run is bench.py's timed region: `--steps` x
{render_frames(frames-per-step), update_frame}, a device sync, the host clock around both (256 spp with the defaults); ms per step = the run over its
steps.  Moments off and on alternate, `--repeats` runs of each after `--warmup` untimed runs of each, so that both see the same clocks and
the same neighbours on the host: median, minimum and maximum of each, and the ratio of the medians.  Then the interactive loop: `--calls` x {render(),
update_frame(), sync} at one sample per call, ms per call, off and on alternating in the same way.
--off-only measures the off case alone and never touches tirt_moments_*: with --package-root it runs on a checkout that does not have them (the parent
commit), from the same process set-up, so that "off costs nothing" is a comparison of two numbers taken the same way.
What to expect: k_moments reads 12 bytes per pixel-sample (and 32 + 32 bytes per pixel and batch) against a path state of 204 bytes per
pixel-sample that every bounce streams through.
Every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def say(a, text, **rec):
    print(json.dumps(dict(rec, label=a.label, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("[%s] %s\n" % (a.label, text))


def spread(ms):
    return "median %.3f  min %.3f  max %.3f  (n = %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def kernel_stats(a):
    fs = sorted(glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True))
    if not fs:
        raise SystemExit("no *kernel_stats.csv under %s" % a.kernel_stats)
    rows = [(r["Name"].split("(")[0].replace("void tirt::", "").replace("tirt::", ""), int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(fs[0]))]
    total = sum(ns for _, _, ns in rows)
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        if name.startswith("k_moments") or ns >= 0.01 * total:
            say(a, "kernel trace: %-28s calls %6d  total %10.3f ms  %6.2f %% of all kernel time  %9.1f us per call"
                % (name[:28], calls, ns / 1e6, 100.0 * ns / total, ns / 1e3 / max(calls, 1)), kernel=name, calls=calls, total_ms=ns / 1e6)
    if not any(name.startswith("k_moments") for name, _, _ in rows):
        say(a, "kernel trace: no k_moments launch in this trace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames-per-step", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ntri", type=int, default=100000)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--package-root", default=HERE)
    ap.add_argument("--label", default="this checkout")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "moments_overhead.txt"))
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a)
    sys.path.insert(0, os.path.abspath(a.package_root))
    from ti_raytrace_amd import scenes

    W = H = a.size
    fps, spp = a.frames_per_step, a.steps * a.frames_per_step
    ex = scenes.synthetic(W, H, spp, ntri=a.ntri, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    modes = (False,) if a.off_only else (False, True)

    def prepare(on):
        if not a.off_only:
            ctx.moments_enable(on)
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.sync()

    def job(on):
        """bench.py's timed region: ms per step"""
        prepare(on)
        ctx.set_option("job_frames", spp)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ex.integrator.render_frames(fps); ex.cam.update_frame(fps)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def loop(on):
        """one sample per call, the film complete after every call: ms per call"""
        prepare(on)
        ctx.set_option("job_frames", 1)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            ex.integrator.render(); ex.cam.update_frame(); ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    say(a, "%d x %d, %d triangles, %d steps of %d frames (%d spp) per run; %d warm-up + %d timed runs of each, alternating"
        % (W, H, a.ntri, a.steps, fps, spp, a.warmup, a.repeats))
    for what, run, unit in (("render_frames", job, "ms per step"), ("render() loop", loop, "ms per call")):
        if what == "render() loop" and a.calls <= 0:
            continue
        ms = {on: [] for on in modes}
        for r in range(a.warmup + a.repeats):
            for on in modes:
                v = run(on)
                if r >= a.warmup:
                    ms[on].append(v)
        for on in modes:
            say(a, "%-14s moments %-3s %s: %s" % (what, "on" if on else "off", unit, spread(ms[on])), what=what, moments=on, ms=ms[on])
        if not a.off_only:
            ratio = statistics.median(ms[True]) / statistics.median(ms[False])
            say(a, "%-14s on / off = %.4f" % (what, ratio), what=what, ratio=ratio)
    ctx.stats()                                           # raises on a traversal stack overflow
    ctx.close()


if __name__ == "__main__":
    main()
