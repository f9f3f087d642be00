"""What choosing emitters by power buys, and where its expectation can move: variance and region z-scores against the switch-off render.

    python tools/light_sampling_quality.py [--out profiles/light_sampling_quality.txt] [--frames 256]

scenes.lamp_and_embers (a small bright lamp of two entries, 254 dim embers of one entry each) at 16 x 12, the film of tests/test_gpu_light_sampling.py, on its
rough-metal ground and on its rough-dielectric twin; then the Veach scene.  Per scene: the summed per-pixel sample variance (from the moment records) of the switch-off
render, of the switch-off render at another seed and of the switched-on render, the factor off / on, and the z-scores of the mean of four film quarters between
each pair (combined standard errors from the renders' own moments, by the formula of tests/env_sampling_scenes.py, region_stats / z_score).  A quarter here is
EVERY pixel of that quarter of the film; tests/test_gpu_light_sampling.py takes the ground pixels of a quarter only, so its printed z-scores are of other regions.  The dielectric z-scores are the measured size of the limit stated in include/tirt.h
("Choosing emitters by power", LIMIT).  Every line goes to stdout as JSON and, as text, to the end of --out."""
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


def moments(ex, frames, seed, mode):
    ctx = ex.scene.ctx
    ex.integrator.set_light_sampling(mode)
    ctx.film_clear()
    ctx.pt_rgb_render(0, frames, seed, 15, 64, 0)
    return ctx.moments_download(ex.imgSizeX, ex.imgSizeY).reshape(-1, 8).astype(np.float64)


def region(m, px):
    r = m[px]
    n = r[:, 0]
    se = np.sqrt(r[:, 4:7] / (n * (n - 1.0))[:, None]).sum(axis=1) / 3.0      # a pixel's three channels are not independent: their errors add linearly
    return r[:, 1:4].mean(), float(np.sqrt((se ** 2).sum()) / px.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "light_sampling_quality.txt"))
    a = ap.parse_args()
    from ti_raytrace_amd import scenes
    W, H = 16, 12
    ii, jj = np.arange(W * H) // H, np.arange(W * H) % H
    quarters = {"%s-%s" % (x, y): np.where((ii < W // 2 if x == "left" else ii >= W // 2) & (jj < H // 2 if y == "low" else jj >= H // 2))[0]
                for x in ("left", "right") for y in ("low", "high")}
    cases = (("lamp_and_embers, rough metal", lambda: scenes.lamp_and_embers(W, H, 4, 0, metallic=1.0, light_sampling="uniform", seed=11, moments=True)),
             ("lamp_and_embers, rough dielectric", lambda: scenes.lamp_and_embers(W, H, 4, 0, metallic=0.0, light_sampling="uniform", seed=11, moments=True)),
             ("veach", lambda: scenes.veach_bdpt(W, H, 4, device_id=0, integrator="pt", seed=11, moments=True)))
    for name, make in cases:
        ex = make()
        ex.build_scene()
        m = {"off": moments(ex, a.frames, 11, "uniform"), "off2": moments(ex, a.frames, 111, "uniform"), "on": moments(ex, a.frames, 11, "power")}
        active = bool(ex.scene.ctx.shade_features()[0] & 4096)
        fin = np.isfinite(m["off"]).all(axis=1) & np.isfinite(m["off2"]).all(axis=1) & np.isfinite(m["on"]).all(axis=1)
        var = {k: float((v[fin, 4:7] / (v[fin, 0:1] - 1.0)).sum()) for k, v in m.items()}
        say(a, "%s, %d x %d, %d frames, %d emitters, bit 4096 %s: summed per-pixel variance off %.4g, off (another seed) %.4g, on %.4g; off / on = %.2f"
            % (name, W, H, a.frames, ex.scene.light_count, "set" if active else "CLEAR", var["off"], var["off2"], var["on"], var["off"] / max(var["on"], 1e-30)),
            scene=name, variance=var)
        for x, y in (("off", "off2"), ("on", "off"), ("on", "off2")):
            zs = []
            for rname, px in quarters.items():
                px = px[fin[px]]
                if px.size < 8:
                    continue
                p, q = region(m[x], px), region(m[y], px)
                zs.append("%s %+.2f" % (rname, (p[0] - q[0]) / max(np.sqrt(p[1] ** 2 + q[1] ** 2), 1e-30)))
            say(a, "  %s vs %s, z per film quarter: %s" % (x, y, ", ".join(zs)), scene=name, pair=[x, y])
        ex.scene.ctx.close()


if __name__ == "__main__":
    main()
