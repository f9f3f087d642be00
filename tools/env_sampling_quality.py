"""What importance sampling of the environment buys: error against a long render at equal frames and at equal time.

    python tools/env_sampling_quality.py [--out profiles/env_sampling_quality.txt] [--reference-frames 4096]

Two scenes at 64 x 48: the Teapot (glass, sphere light, env.png x 5) and scenes.sun_ground (rough metals under a sky with nearly all its light in one texel,
no emitters).  The reference is a switch-off render of --reference-frames frames at another seed.  For 4 / 16 / 64 frames, switch off and on: rel-L2 of the film
against the reference over the pixels finite in both, and the host time of the render; then, at equal time, the switch-off render with as many frames as fit
into the switched-on render's time (frames scaled by the measured times, at least one).  Every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def film(ex, frames, seed, on, runs=2):
    ctx = ex.scene.ctx
    ex.integrator.set_env_sampling(on)
    ex.integrator.seed = seed
    best = None
    for _ in range(runs):                                 # (the last run is the timed one; the reference is not timed and runs once)
        ctx.film_clear()
        ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
        ctx.sync()
        t0 = time.perf_counter()
        ex.integrator.render_frames(frames)
        ctx.sync()
        best = time.perf_counter() - t0
    return ex.integrator.hdr.to_numpy().astype(np.float64), best


def rel_l2(x, ref):
    m = np.isfinite(x).all(axis=2) & np.isfinite(ref).all(axis=2)
    return float(np.sqrt(((x[m] - ref[m]) ** 2).sum() / max((ref[m] ** 2).sum(), 1e-30)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-frames", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "env_sampling_quality.txt"))
    a = ap.parse_args()
    from ti_raytrace_amd import scenes
    W, H = 64, 48
    for name, make in (("teapot", lambda: scenes.single_model(W, H, 64, device_id=0)), ("sun_ground", lambda: scenes.sun_ground(W, H, 64, device_id=0, env_sampling=False))):
        ex = make()
        ex.build_scene()
        ref, _ = film(ex, a.reference_frames, 1000003, False, runs=1)
        say(a, "%s, %d x %d, reference: %d frames, switch off, another seed" % (name, W, H, a.reference_frames))
        for frames in (4, 16, 64):
            off, t_off = film(ex, frames, 1, False)
            on, t_on = film(ex, frames, 1, True)
            eq_frames = max(1, int(round(frames * t_on / t_off)))
            eq, t_eq = film(ex, eq_frames, 1, False)
            say(a, "%-10s %3d frames: rel-L2 off %.4f (%.2f ms)  on %.4f (%.2f ms)  | equal time: off with %d frames %.4f (%.2f ms)"
                % (name, frames, rel_l2(off, ref), t_off * 1e3, rel_l2(on, ref), t_on * 1e3, eq_frames, rel_l2(eq, ref), t_eq * 1e3),
                scene=name, frames=frames, off=rel_l2(off, ref), on=rel_l2(on, ref), equal_time_off=rel_l2(eq, ref), ms=[t_off * 1e3, t_on * 1e3, t_eq * 1e3])
        ex.scene.ctx.close()


if __name__ == "__main__":
    main()
