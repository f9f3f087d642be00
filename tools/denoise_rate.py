"""What the denoiser (PathTrace.denoise() / denoise_var(), csrc/tirt_denoise.hip) costs on one GPU.

    python tools/denoise_rate.py [--mode plain|var] [--sizes 512 1024] [--max-levels 5] [--frames 4] [--calls 20] [--repeats 5] [--out profiles/denoise_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/denoise_rate.py --repeats 1 --out ""

The Cornell box at size x size, `--frames` frames with feature buffers, then for levels = 1 .. --max-levels: after one untimed call, `--repeats`
runs of `--calls` x tirt_denoise (--mode var: tirt_denoise_var, on a scene with sample moments) followed by one device sync, the host clock around each run; ms per call = a run over its calls.  The level counts
alternate inside every repeat, so that all see the same clocks and the same neighbours on the host: median, minimum and maximum of each, and the
megapixels per second of the median.  The filter reads 44 B and writes 12 B per pixel outside its scratch; inside it, per level, 25 taps of two
16-byte records and one 16-byte (last level: 12-byte) store -- the bytes per level are printed beside the times, the share of a peak is not claimed.
There is no LDS variant to time (none was built: csrc/tirt_denoise.hip).  Every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["plain", "var"], default="plain")
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--max-levels", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "denoise_rate.txt"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    from ti_raytrace_amd import scenes

    for size in a.sizes:
        ex = scenes.cornell_box(size, size, a.frames, device_id=0, aov=True, moments=a.mode == "var")
        ex.build_scene()
        ctx = ex.scene.ctx
        denoise = ctx.denoise_var if a.mode == "var" else ctx.denoise
        ex.integrator.render_frames(a.frames)
        ctx.sync()
        levels = list(range(1, a.max_levels + 1))
        ms = {l: [] for l in levels}
        for l in levels:                                      # untimed: code objects, the scratch
            denoise(levels=l)
        ctx.sync()
        for _ in range(a.repeats):
            for l in levels:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    denoise(levels=l)
                ctx.sync()
                ms[l].append((time.perf_counter() - t0) * 1e3 / a.calls)
        say(a, "Cornell box %d x %d, %d frames%s; %d repeats of %d calls per level count, alternating" % (size, size, a.frames, ", variance-guided" if a.mode == "var" else "", a.repeats, a.calls))
        npx = size * size
        for l in levels:
            med = statistics.median(ms[l])
            tap_mb = npx * l * 25 * 32 / 1e6
            say(a, "%4d^2 levels %d: ms per call median %.4f  min %.4f  max %.4f  (n = %d)   %.0f Mpixel/s   tap loads %.0f MB per call"
                % (size, l, med, min(ms[l]), max(ms[l]), len(ms[l]), npx / med / 1e3, tap_mb), size=size, levels=l, ms=ms[l])
        if len(levels) > 1:
            per = (statistics.median(ms[levels[-1]]) - statistics.median(ms[levels[0]])) / (levels[-1] - levels[0])
            say(a, "%4d^2 one more level: %.4f ms (medians of levels %d and %d)" % (size, per, levels[0], levels[-1]), size=size, ms_per_level=per)
        ctx.close()


if __name__ == "__main__":
    main()
