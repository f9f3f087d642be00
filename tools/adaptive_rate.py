"""What adaptive sampling (PathTrace.render_adaptive, csrc/tirt_adaptive.hip) costs the dense path, and what it buys, on one GPU.

    python tools/adaptive_rate.py [--parent-root <built checkout of the parent commit>] [--repeats 5] [--out profiles/adaptive_rate.txt]
    python tools/adaptive_rate.py --dense-child --package-root <checkout> ...          (what (a) starts, one process per run)

(a) The dense path, no pixel set installed, with the parent commit's library and with this one.  The headline scene of bench.py (100 000 triangles,
1024 x 1024, scene seed 1234): bench.py's timed region -- `--steps` x {render_frames(frames-per-step), update_frame}, a sync, the host clock around both --
after one untimed run, then the interactive loop, `--calls` x {render(), update_frame(), sync}.  One fresh process per run, each importing the package
of its own checkout; the two checkouts alternate, `--repeats` runs of each: median, minimum and maximum of each and the ratio of the medians.  The claim
to support: the medians differ by no more than either's own spread.  Without --parent-root (a) is left out and the file says so.

(b) The Cornell box at `--size`^2 (512), max_samples 64, min_samples 4, passes of 4 frames, thresholds 0.1 / 0.2 / 0.3: wall time (host clock, sync) and
pixel-samples of render_adaptive against the dense 64-frame render (median of `--repeats-b` runs each, after one untimed run), the time of one selection
(tirt_pixel_set_from_moments: three launches and the read-back of the count) on the final records, and the rel-L2 of both films against a dense
`--reference-frames` (1024) film of the same seed sequence.
Every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def spread(ms):
    return "median %.3f  min %.3f  max %.3f  (n = %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def dense_child(a):
    """one process of (a): the job once untimed, once timed; the loop once untimed, once timed; one JSON line"""
    sys.path.insert(0, os.path.abspath(a.package_root))
    from ti_raytrace_amd import scenes
    W = H = a.headline_size
    fps, spp = a.frames_per_step, a.steps * a.frames_per_step
    ex = scenes.synthetic(W, H, spp, ntri=a.ntri, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx

    def rewind():
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.sync()

    def job():
        rewind()
        ctx.set_option("job_frames", spp)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ex.integrator.render_frames(fps); ex.cam.update_frame(fps)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def loop():
        rewind()
        ctx.set_option("job_frames", 1)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            ex.integrator.render(); ex.cam.update_frame(); ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    job(); j = job()
    loop(); l = loop()
    ctx.stats()                                           # raises on a traversal stack overflow
    ctx.close()
    print(json.dumps({"dense_child": True, "job_ms_per_step": j, "loop_ms_per_call": l}), flush=True)


def part_a(a):
    if not a.parent_root:
        say(a, "(a) dense path against the parent commit: not measured (no --parent-root given)")
        return
    roots = (("parent", os.path.abspath(a.parent_root)), ("this", HERE))
    ms = {name: {"job": [], "loop": []} for name, _ in roots}
    say(a, "(a) dense path, no pixel set: %d x %d, %d triangles, %d steps of %d frames per job, %d calls per loop; %d processes of each checkout, alternating"
        % (a.headline_size, a.headline_size, a.ntri, a.steps, a.frames_per_step, a.calls, a.repeats))
    for _ in range(a.repeats):
        for name, root in roots:
            cmd = [sys.executable, os.path.join(HERE, "tools", "adaptive_rate.py"), "--dense-child", "--package-root", root, "--out", "",
                   "--steps", str(a.steps), "--frames-per-step", str(a.frames_per_step), "--calls", str(a.calls), "--headline-size", str(a.headline_size),
                   "--ntri", str(a.ntri)]
            env = dict(os.environ); env.pop("TIRT_LIB_PATH", None)
            pr = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
            if pr.returncode != 0:
                raise SystemExit("dense child of %s failed (%d):\n%s" % (name, pr.returncode, pr.stderr[-2000:]))
            rec = [json.loads(line) for line in pr.stdout.splitlines() if line.startswith("{") and "dense_child" in line][-1]
            ms[name]["job"].append(rec["job_ms_per_step"]); ms[name]["loop"].append(rec["loop_ms_per_call"])
    for what, unit in (("job", "ms per step"), ("loop", "ms per call")):
        for name, _ in roots:
            say(a, "(a) %-4s %-6s %s: %s" % (what, name, unit, spread(ms[name][what])), what=what, checkout=name, ms=ms[name][what])
        mp, mt = statistics.median(ms["parent"][what]), statistics.median(ms["this"][what])
        widest = max(max(v) - min(v) for v in (ms["parent"][what], ms["this"][what]))
        say(a, "(a) %-4s this / parent = %.4f; medians differ by %.3f, the wider of the two spreads (max - min) is %.3f: %s"
            % (what, mt / mp, abs(mt - mp), widest, "within the spread" if abs(mt - mp) <= widest else "NOT within the spread"), what=what, ratio=mt / mp)


def part_b(a):
    import numpy as np
    sys.path.insert(0, HERE)
    from ti_raytrace_amd import scenes
    S, MAX, MIN, PASS = a.size, a.max_samples, 4, 4
    ex = scenes.cornell_box(S, S, MAX, device_id=0, seed=5, aov=False, moments=True)
    ex.build_scene()
    ctx, it = ex.scene.ctx, ex.integrator

    def rewind():
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.sync()

    def rel_l2(film, ref):
        ok = np.isfinite(film).all(axis=2) & np.isfinite(ref).all(axis=2)
        return float(np.sqrt(((film[ok].astype(np.float64) - ref[ok]) ** 2).sum() / (ref[ok].astype(np.float64) ** 2).sum()))

    rewind()
    ctx.set_option("job_frames", a.reference_frames)
    it.render_frames(a.reference_frames)
    ref = it.hdr.to_numpy()
    ctx.set_option("job_frames", MAX)

    def dense():
        rewind()
        t0 = time.perf_counter()
        it.render_frames(MAX)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def adaptive(thr):
        rewind()
        t0 = time.perf_counter()
        res = it.render_adaptive(thr, MAX, MIN, PASS)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, res

    say(a, "(b) Cornell box %d x %d, seed 5, max_samples %d, min_samples %d, passes of %d frames; reference: dense %d frames; %d timed runs of each after one untimed"
        % (S, S, MAX, MIN, PASS, a.reference_frames, a.repeats_b))
    dense()
    d_ms = [dense() for _ in range(a.repeats_b)]
    d_err = rel_l2(it.hdr.to_numpy(), ref)
    say(a, "(b) dense %d frames: ms %s; %d pixel-samples; rel-L2 against the reference %.4f" % (MAX, spread(d_ms), MAX * S * S, d_err),
        what="dense", ms=d_ms, pixel_samples=MAX * S * S, rel_l2=d_err)
    for thr in a.thresholds:
        adaptive(thr)
        runs = [adaptive(thr) for _ in range(a.repeats_b)]
        ms, res = [r[0] for r in runs], runs[-1][1]
        err = rel_l2(it.hdr.to_numpy(), ref)
        sel = []
        for _ in range(9):
            t0 = time.perf_counter()
            count = ctx.pixel_set_from_moments(thr, MIN, MAX + 1)
            sel.append((time.perf_counter() - t0) * 1e3)
        ctx.pixel_set_clear()
        say(a, "(b) threshold %.2f: ms %s = %.3f x dense; %d pixel-samples = %.3f x dense in %d passes, %d pixels at max_samples; rel-L2 %.4f (dense %.4f); "
            "one selection + read-back %.3f ms (median of 9, %d listed), x %d passes = %.1f %% of the call"
            % (thr, spread(ms), statistics.median(ms) / statistics.median(d_ms), res["pixel_samples"], res["pixel_samples"] / float(MAX * S * S), res["passes"],
               res["pixels_at_max"], err, d_err, statistics.median(sel), count, res["passes"] + 1,
               100.0 * statistics.median(sel) * (res["passes"] + 1) / statistics.median(ms)),
            what="adaptive", threshold=thr, ms=ms, result=res, rel_l2=err, select_ms=sel)
    ctx.stats()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=HERE)
    ap.add_argument("--dense-child", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--frames-per-step", type=int, default=32)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--headline-size", type=int, default=1024)
    ap.add_argument("--ntri", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--max-samples", type=int, default=64)
    ap.add_argument("--reference-frames", type=int, default=1024)
    ap.add_argument("--repeats-b", type=int, default=3)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.1, 0.2, 0.3])
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "adaptive_rate.txt"))
    a = ap.parse_args()
    if a.dense_child:
        return dense_child(a)
    part_a(a)
    if not a.skip_b:
        part_b(a)


if __name__ == "__main__":
    main()
