"""What the temporal accumulation (PathTrace.temporal_accumulate(), csrc/tirt_temporal.hip) costs on one GPU.

    python tools/temporal_rate.py [--sizes 512 1024] [--frames 2] [--yaw-step 0.02] [--calls 20] [--repeats 5] [--out profiles/temporal_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/temporal_rate.py --repeats 1 --out ""

The Cornell box at size x size with feature buffers, sample moments and the history: one view of `--frames` frames is rendered and accumulated, the
camera yaws by `--yaw-step`, a second view is rendered -- and then, after one untimed call each, `--repeats` runs of `--calls` x
tirt_temporal_accumulate followed by one device sync, the host clock around each run; ms per call = a run over its calls.  (Every call reprojects the
previous call's result from the camera it was made with, which after the first is the current one: the same loads and stores, a near-identity
reprojection.  The first call of every run is the yaw step itself; `--calls 1` times that alone, launch latency included.)  Beside it, alternating in
the same repeats, ONE level of tirt_denoise -- the other gather pass over the film -- as the yardstick.  Medians, minima and maxima, megapixels per
second of the median, and the bytes a call moves per pixel by construction: 76 B of current records in, up to 4 taps x 76 B of history (32 B for a tap
the guides reject), 44 B out, and the 32 B + 32 B copy of the feature records beside the result.  The share of a peak is not claimed.  Every line goes
to stdout as JSON and, as text, to the end of --out.

    python tools/temporal_rate.py --motion [--sizes 512 1024] [--calls 10] [--repeats 5]

times the accumulate with motion records (tirt_motion_enable) on the headline scene (scenes.synthetic, 100k triangles): before every timed call one
object -- the first `--object-tris` triangles -- is moved back or forth by Scene.update_vertices (untimed: it rebuilds and waits), then the host clock
runs around ONE tirt_temporal_accumulate and the device sync behind it: the pixel-centre rays, k_motion_resolve and k_temporal<true>.  Beside it, timed
the same way (one call and its sync, launch latency included, so the three are comparable with each other and not with the batched figures above) and
alternating in the same repeats: the static accumulate on a TWIN context of the same scene and film without motion records (the call as it was
before them: with the records on, a static accumulate also zeroes the 32 B per pixel of the record buffer, which is not part of the yardstick) and
one Debug frame on that twin (tirt_debug_render at frame 0: the same rays and one resolve kernel).  ms per call = a run's timed calls over their number; medians of the repeats."""
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


def motion_mode(a, scenes):
    import numpy as np
    from ti_raytrace_amd import _native
    calls = min(a.calls, 10)
    for size in a.sizes:
        ex = scenes.synthetic(size, size, a.frames, device_id=0, seed=5, aov=True, moments=True, temporal=True, motion=True)
        ex.build_scene()
        it, ctx = ex.integrator, ex.scene.ctx
        it.render_frames(a.frames)
        it.temporal_accumulate()
        twin = scenes.synthetic(size, size, a.frames, device_id=0, seed=5, aov=True, moments=True, temporal=True)
        twin.build_scene()
        twin.integrator.render_frames(a.frames)
        twin.integrator.temporal_accumulate()
        k = 3 * a.object_tris
        home = np.ascontiguousarray(ex.scene.vertex_np[:k, 0:3], np.float32)
        away = (home + np.float32([0.01, 0.0, 0.0])).astype(np.float32)
        state = {"away": False}

        def timed(fn):
            ctx.sync(); twin.scene.ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync(); twin.scene.ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        def with_motion():
            state["away"] = not state["away"]
            ex.scene.update_vertices(away if state["away"] else home)      # untimed; marks the geometry as moved
            return timed(it.temporal_accumulate)

        def static():
            return timed(twin.integrator.temporal_accumulate)

        def debug_frame():
            return timed(lambda: twin.scene.ctx.debug_render(0, 5, _native.DEBUG_NORMAL))

        runs = (("tirt_temporal_accumulate, motion records", with_motion), ("tirt_temporal_accumulate, no motion records", static), ("tirt_debug_render, one frame", debug_frame))
        for _, fn in runs:                                     # untimed: code objects, the scratch, the snapshot
            fn()
        moved_px = int((it.motion_to_numpy()[:, :, 0:3] != 0).any(axis=2).sum()) if with_motion() else 0
        ms = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, fn in runs:
                ms[name].append(sum(fn() for _ in range(calls)) / calls)
        say(a, "headline scene (%d triangles) %d x %d, %d frames per view, %d triangles moved before every call (%d pixels with a record that is not zero); "
            "%d repeats of %d single timed calls, alternating" % (ex.scene.primitive_count, size, size, a.frames, a.object_tris, moved_px, a.repeats, calls))
        for name, _ in runs:
            med = statistics.median(ms[name])
            say(a, "%4d^2 %-42s ms per call median %.4f  min %.4f  max %.4f  (n = %d)"
                % (size, name + ":", med, min(ms[name]), max(ms[name]), len(ms[name])), size=size, what=name, ms=ms[name])
        ctx.close(); twin.scene.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--yaw-step", type=float, default=0.02)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-ms", type=float, default=3.56, help="ms per call of the one-frame loop (tools/moments_rate.py) the cost is set against")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "temporal_rate.txt"))
    ap.add_argument("--motion", action="store_true", help="the accumulate with motion records after a one-object update, on the headline scene")
    ap.add_argument("--object-tris", type=int, default=1000)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    from ti_raytrace_amd import scenes
    if a.motion:
        return motion_mode(a, scenes)

    for size in a.sizes:
        ex = scenes.cornell_box(size, size, a.frames, device_id=0, seed=5, aov=True, moments=True, temporal=True)
        ex.build_scene()
        it, ctx = ex.integrator, ex.scene.ctx
        it.render_frames(a.frames)
        it.temporal_accumulate()
        ex.cam.set_view_point(ex.cam.yaw + a.yaw_step, 0.0, 0.0, ex.cam.scale)
        ctx.film_clear()
        it.seed += 1
        it.render_frames(a.frames)
        ctx.sync()
        share = None

        def accumulate():
            it.temporal_accumulate()

        def one_level():
            ctx.denoise(levels=1)

        runs = (("tirt_temporal_accumulate", accumulate), ("tirt_denoise, 1 level", one_level))
        for _, fn in runs:                                     # untimed: code objects, the scratch; the first accumulate is the yaw step
            fn()
        ctx.sync()
        hist_n = it.accumulated_samples.to_numpy()
        share = float((hist_n > it.samples.to_numpy()).mean())
        ms = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, fn in runs:
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                ctx.sync()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
        say(a, "Cornell box %d x %d, %d frames per view, yaw step %.3f (%.1f %% of the pixels took a history); %d repeats of %d calls, alternating"
            % (size, size, a.frames, a.yaw_step, 100.0 * share, a.repeats, a.calls))
        npx = size * size
        for name, _ in runs:
            med = statistics.median(ms[name])
            extra = ""
            if name.startswith("tirt_temporal"):
                extra = "   %.1f .. %.1f MB per call (76 B in, 32 .. 304 B of taps, 44 B out, 64 B for the copy of the feature records per pixel)   %.1f %% of a %.2f ms one-frame loop call" % (
                    npx * (76 + 32 + 44 + 64) / 1e6, npx * (76 + 304 + 44 + 64) / 1e6, 100.0 * med / a.loop_ms, a.loop_ms)
            else:
                extra = "   %.1f MB of tap loads per call (25 taps x 32 B per pixel)" % (npx * 25 * 32 / 1e6)
            say(a, "%4d^2 %-26s ms per call median %.4f  min %.4f  max %.4f  (n = %d)   %.0f Mpixel/s%s"
                % (size, name + ":", med, min(ms[name]), max(ms[name]), len(ms[name]), npx / med / 1e3, extra), size=size, what=name, ms=ms[name])
        ctx.close()


if __name__ == "__main__":
    main()
