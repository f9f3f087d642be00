"""What importance sampling of the environment buys under an HDR sky: the summed per-pixel sample variance of scenes.sun_ground under scenes.hdr_sun_sky()
(a sun 250 000 times its sky; Scene.add_env_hdr), switch off and on, and the error of both against a long switched-on render.

    python tools/env_hdr_quality.py [--out profiles/env_hdr_quality.txt] [--frames 256] [--reference-frames 4096]

16 x 12 pixels, `--frames` frames, two seeds: sum over pixels and channels of M2 / (n - 1) from the render's own moment records (what
tests/test_gpu_env_hdr.py prints), and rel-L2 of each film against `--reference-frames` frames at a third seed with the switch on -- the two estimators have one
expectation (include/tirt.h, "Importance sampling of the environment", step 5) and only the switched-on one converges in that many frames under such a sun.
The pattern of tools/env_sampling_quality.py; every line goes to stdout as JSON and, as text, to the end of --out."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def say(a, text, **rec):
    print(json.dumps(dict(rec, text=text)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def render(ex, frames, seed, on):
    from ti_raytrace_amd import PT_RGB
    ctx = ex.scene.ctx
    ex.integrator.set_env_sampling(on)
    ctx.film_clear()
    ctx.pt_rgb_render(0, frames, seed, PT_RGB.MAX_DEPTH, 64, 0)
    W, H = ex.imgSizeX, ex.imgSizeY
    return ctx.film_download(W, H)[0].astype(np.float64), ctx.moments_download(W, H).astype(np.float64)


def rel_l2(x, ref):
    m = np.isfinite(x).all(axis=2) & np.isfinite(ref).all(axis=2)
    return float(np.sqrt(((x[m] - ref[m]) ** 2).sum() / max((ref[m] ** 2).sum(), 1e-30)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reference-frames", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "env_hdr_quality.txt"))
    a = ap.parse_args()
    from ti_raytrace_amd import scenes
    W, H = 16, 12
    ex = scenes.sun_ground(W, H, a.frames, 0, sky=scenes.hdr_sun_sky(), env_sampling=False, moments=True)
    ex.build_scene()
    word = ex.scene.ctx.shade_features()[0]
    ref, _ = render(ex, a.reference_frames, 1000003, True)
    say(a, "sun_ground under hdr_sun_sky(), env_power 20, %d x %d, %d frames; feature word %d (switch off); reference: %d frames, switch on, another seed"
        % (W, H, a.frames, word, a.reference_frames))
    for seed in (11, 111):
        row = {}
        for on in (False, True):
            film, mom = render(ex, a.frames, seed, on)
            m = mom.reshape(-1, 8)
            row[on] = (float((m[:, 4:7] / (m[:, 0:1] - 1.0)).sum()), rel_l2(film, ref), int((m[:, 7] != 0).sum()))
        say(a, "seed %3d: summed per-pixel variance off %.4g  on %.4g  (off / on = %.1f);  rel-L2 against the reference off %.4f  on %.4f;  pixels with a non-finite sample off %d on %d"
            % (seed, row[False][0], row[True][0], row[False][0] / row[True][0], row[False][1], row[True][1], row[False][2], row[True][2]),
            seed=seed, variance_off=row[False][0], variance_on=row[True][0], rel_l2_off=row[False][1], rel_l2_on=row[True][1])
    ex.scene.ctx.close()


if __name__ == "__main__":
    main()
