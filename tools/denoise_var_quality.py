"""What the variance-guided mode of the denoiser (tirt_denoise_var) does to a noisy film, on the CPU alone: the oracle's films and moments through
the numpy restatements of both filters (tests/denoise_expected.py, tests/denoise_var_expected.py).  No device.

    python tools/denoise_var_quality.py [--out profiles/denoise_var_quality.txt]

The Cornell box at 64 x 48 (seed 5, the camera of tests/test_gpu_aov.py), 4 and 16 frames, against the oracle's own 256-frame film: rel-L2 of the
unfiltered film, of tirt_denoise at its defaults, and of tirt_denoise_var over a sweep of sigma_c (the other parameters at their defaults).  The
per-frame samples behind the moments are the oracle's one-frame films (each frame rendered into a zeroed film and scaled back by frame + 1; in f64
here: this is a quality figure, the exact-sample tests use the power-of-two frames only); the records are folded with tests/moments_expected.py."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

SIGMAS = (0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 16.0, 32.0)
W, H, SEED, REF_FRAMES = 64, 48, 5, 256


def inputs(frames_list=(4, 16)):
    """{frames: (hdr, aov, mom)}, and the 256-frame film"""
    import aov_expected as ae
    import moments_expected as me
    from test_film_shapes import make, oracle
    ex = make("cornell", W, H, 0.8)
    orc = oracle(ex, "cornell")
    ref, _ = orc.render(W, H, 0, REF_FRAMES, seed=SEED)
    most = max(frames_list)
    samples = []
    for fr in range(most):
        one, _ = orc.render(W, H, fr, 1, seed=SEED)
        samples.append((one.astype(np.float64) * (fr + 1)).astype(np.float32))
    out = {}
    for frames in frames_list:
        hdr, _ = orc.render(W, H, 0, frames, seed=SEED)
        aov, _, _ = ae.expected(ex, orc, W, H, range(frames), SEED)
        out[frames] = (hdr, aov, me.expected(samples[:frames], W, H))
    return out, ref


def rel_l2(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum() / (b.astype(np.float64) ** 2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "denoise_var_quality.txt"))
    a = ap.parse_args()
    import denoise_expected as de
    import denoise_var_expected as dv
    data, ref = inputs()
    lines = ["Cornell box %d x %d, seed %d: rel-L2 against the oracle's %d-frame film (CPU: oracle films, numpy restatements of the filters)" % (W, H, SEED, REF_FRAMES)]
    for frames, (hdr, aov, mom) in sorted(data.items()):
        lines.append("%2d frames: unfiltered %.4f   tirt_denoise (defaults %s) %.4f" % (frames, rel_l2(hdr, ref), de.DEFAULTS, rel_l2(de.denoise_expected(hdr, aov), ref)))
        for s in SIGMAS:
            lines.append("%2d frames: tirt_denoise_var sigma_c %5.1f (levels 5, sigma_n 0.3, sigma_z 0.1)  %.4f"
                         % (frames, s, rel_l2(dv.denoise_var_expected(hdr, aov, mom, sigma_c=s), ref)))
    lines.append("default sigma_c of tirt_denoise_var: %.1f" % dv.DEFAULTS["sigma_c"])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
