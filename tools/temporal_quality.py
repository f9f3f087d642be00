"""What the temporal accumulation (tirt_temporal_accumulate) buys a viewer that moves its camera, on the CPU alone: the oracle's films, feature and
moment records through the numpy restatements (tests/temporal_expected.py, tests/denoise_var_expected.py).  No device.

    python tools/temporal_quality.py [--out profiles/temporal_quality.txt] [--no-sweep]

An orbit of 8 views of the Cornell box at 64 x 48, a yaw step of 0.02 rad between them, 2 frames per view at seed 5 + view.  At the last view, rel-L2
against the oracle's own 256-frame film of that view: the raw 2-frame film, tirt_denoise_var of it, the accumulated film, and tirt_denoise_var of the
accumulated film -- and the share of pixels that took a history.  Then a sweep of max_history, sigma_n and sigma_z, one at a time about the defaults.

Also the arithmetic of the merge: two record sets of ONE camera (24 x 20, seeds 5 and 6, 2 frames each) merged by the restatement against the
float64 moments of the four samples; the worst deviation of the mean and of M2, each relative to the largest value of its kind on the film.
tests/test_temporal_host.py reads that line and holds the restatement to four times it.

    python tools/temporal_quality.py --motion [--out profiles/motion_quality.txt]

is the sequence for moving geometry (tirt_motion_enable; tests/motion_expected.py): a still camera, the short block of the Cornell box pushed sideways
by MOVE_STEP units per step over 8 steps, 64 x 48, 2 frames per step at seed 5 + step.  At the last step, rel-L2 against the oracle's 256-frame film
of the final geometry: the raw 2-frame film; the history dropped at every step, which is what a geometry update does without motion records (the
accumulated film IS the raw film then; tirt_denoise_var of it beside it); the film accumulated through the motion records; and tirt_denoise_var of
that.  No threshold is set: the file records what was found."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

W, H, SEED, REF_FRAMES, VIEWS, FRAMES, YAW0, STEP = 64, 48, 5, 256, 8, 2, 0.0, 0.02
MERGE_W, MERGE_H = 24, 20
MOVE_STEP = 8.0          # units per step: 0.65 pixels of the 64-wide film at the block's depth, 56 units over the sequence (the block stays inside the room)
SWEEP = {"max_history": (4.0, 8.0, 16.0, 32.0, 64.0), "sigma_n": (0.1, 0.3, 0.6, 1.0), "sigma_z": (0.02, 0.05, 0.1, 0.2, 0.5)}


def rel_l2(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum() / (b.astype(np.float64) ** 2).sum()))


def orbit():
    """[(hdr, aov, mom, Cam)] of the views, and the 256-frame film of the last one"""
    import temporal_expected as te
    from test_film_shapes import make, oracle
    ex = make("cornell", W, H, 0.8)
    orc = oracle(ex, "cornell")
    views = []
    for v in range(VIEWS):
        ex.cam.set_view_point(YAW0 + v * STEP, 0.0, 0.0, ex.cam.scale)
        views.append(te.oracle_view(ex, orc, W, H, SEED + v, FRAMES) + (te.Cam(ex.cam),))
    ref, _ = orc.render(W, H, 0, REF_FRAMES, seed=SEED + VIEWS)
    return views, ref


def run(views, **params):
    """the accumulated (hdr, mom) after all views, and the share of pixels of the last view that took a history"""
    import temporal_expected as te
    hdr, aov, mom, cam = views[0]
    acc_h, acc_m = te.first(hdr, aov, mom)
    share = 0.0
    for k in range(1, len(views)):
        h, a, m, c = views[k]
        acc_h, acc_m, info = te.accumulate(h, a, m, acc_h, views[k - 1][1], acc_m, c, views[k - 1][3], want_info=True, **params)
        share = float(info["history"].mean())
    return acc_h, acc_m, share


def moving_box():
    """[(hdr, aov, mom, motion record)] of the steps, the camera, the 256-frame film of the last geometry, and the mask of the pixels on the block there"""
    import motion_expected as mx
    import temporal_expected as te
    from test_film_shapes import make, oracle
    ex = make("cornell", W, H, 0.8)
    cam = te.Cam(ex.cam)
    rows = np.array(ex.scene.vertex_np, np.float32)
    tris = mx.block_triangles(rows, "translate")
    steps, orc, hits = [], None, None
    for s in range(VIEWS):
        prev = rows
        if s:
            rows = mx.moved_rows(prev, tris, mx.translated(prev, tris, (-MOVE_STEP, 0.0, 0.0)))
            ex.scene.vertex_np = rows
            ex.scene.minboundarynp[0, :] = rows[:, 0:3].min(axis=0); ex.scene.maxboundarynp[0, :] = rows[:, 0:3].max(axis=0)
        orc = oracle(ex, "cornell")
        hits = mx.centre_hits(orc, ex.cam, W, H)
        rec = mx.record(*hits, ex.scene.primitive_np, rows, prev, W, H)
        steps.append(te.oracle_view(ex, orc, W, H, SEED + s, FRAMES) + (rec,))
    ref, _ = orc.render(W, H, 0, REF_FRAMES, seed=SEED + VIEWS)
    on_block = (hits[0] & np.isin(hits[1], tris)).reshape(W, H)
    return steps, cam, ref, on_block


def run_motion(steps, cam, **params):
    """the accumulated (hdr, mom) after all steps through the motion records, and the share of pixels of the last step that took a history"""
    import motion_expected as mx
    import temporal_expected as te
    acc_h, acc_m = te.first(*steps[0][:3])
    share = 0.0
    for k in range(1, len(steps)):
        h, a, m, rec = steps[k]
        acc_h, acc_m, info = mx.accumulate_mv(h, a, m, acc_h, steps[k - 1][1], acc_m, cam, cam, rec, want_info=True, **params)
        share = float(info["history"].mean())
    return acc_h, acc_m, share


def motion_main(a):
    import denoise_var_expected as dv
    steps, cam, ref, on_block = moving_box()
    hdr, aov, mom, _ = steps[-1]
    acc_h, acc_m, share = run_motion(steps, cam)
    both = dv.denoise_var_expected(acc_h, aov, acc_m)
    alone = dv.denoise_var_expected(hdr, aov, mom)
    blk = lambda x: rel_l2(x[on_block], ref[on_block])
    med = lambda x: float(np.median(np.abs(x.astype(np.float64) - ref).sum(axis=2)[on_block]))
    lines = ["Cornell box %d x %d, a still camera, the short block pushed %.1f units in -x per step over %d steps, %d frames per step, seeds %d + step: rel-L2 at the"
             % (W, H, MOVE_STEP, VIEWS, FRAMES, SEED),
             "last step against the oracle's %d-frame film of the final geometry (CPU: oracle films and records, numpy restatements); whole film / the %d pixels on the block"
             % (REF_FRAMES, int(on_block.sum())),
             "raw %d-frame film                                      %.4f / %.4f" % (FRAMES, rel_l2(hdr, ref), blk(hdr)),
             "history dropped at every step (no motion records)     %.4f / %.4f   (the raw film: every accumulate is a first one)" % (rel_l2(hdr, ref), blk(hdr)),
             "  tirt_denoise_var of it                               %.4f / %.4f" % (rel_l2(alone, ref), blk(alone)),
             "accumulated through the motion records                 %.4f / %.4f" % (rel_l2(acc_h, ref), blk(acc_h)),
             "  tirt_denoise_var of it                               %.4f / %.4f" % (rel_l2(both, ref), blk(both)),
             "pixels of the last step with a history                 %.4f / %.4f   (mean samples per pixel behind the accumulated film %.2f / %.2f)"
             % (share, float((acc_m[:, :, 0] > mom[:, :, 0])[on_block].mean()), float(acc_m[:, :, 0].mean()), float(acc_m[:, :, 0][on_block].mean())),
             "median over the block's pixels of |error| summed over r, g, b:  raw %.4f   tirt_denoise_var %.4f   accumulated %.4f   accumulated + tirt_denoise_var %.4f"
             % (med(hdr), med(alone), med(acc_h), med(both)),
             "(rel-L2 on the block is carried by single bright samples: one such sample of an early step stays in the history of the pixel that follows the",
             " block, at 1 / n of its weight, where the raw film of the last step happens to have none)"]
    text = "\n".join(lines)
    print(text)
    out = a.out or os.path.join(HERE, "profiles", "motion_quality.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


def merge_deviation():
    """(mean deviation, M2 deviation, pixels) of the restatement's merge of two record sets of one camera against float64 (see above)"""
    import moments_expected as me
    import temporal_expected as te
    from test_film_shapes import make, oracle
    ex = make("cornell", MERGE_W, MERGE_H, 0.8)
    orc = oracle(ex, "cornell")
    cam = te.Cam(ex.cam)
    a = te.oracle_view(ex, orc, MERGE_W, MERGE_H, SEED, FRAMES)
    b = te.oracle_view(ex, orc, MERGE_W, MERGE_H, SEED + 1, FRAMES)
    _, mom, info = te.accumulate(b[0], b[1], b[2], a[0], a[1], a[2], cam, cam, max_history=1e6, sigma_n=4.0, sigma_z=10.0, want_info=True)
    xs = [me.oracle_sample(orc, MERGE_W, MERGE_H, fr, s) for s in (SEED, SEED + 1) for fr in range(FRAMES)]
    n, mean, m2, _ = me.welford64(xs, MERGE_W, MERGE_H)
    ok = info["history"] & (mom[:, :, 0] == n)
    d_mean = float(np.abs(mom[:, :, 1:4] - mean)[ok].max() / np.abs(mean[ok]).max())
    d_m2 = float(np.abs(mom[:, :, 4:7] - m2)[ok].max() / np.abs(m2[ok]).max())
    return d_mean, d_m2, int(ok.sum()), int(info["history"].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/temporal_quality.txt, with --motion profiles/motion_quality.txt")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--motion", action="store_true", help="the moving-geometry sequence instead of the orbit")
    a = ap.parse_args()
    if a.motion:
        return motion_main(a)
    if a.out is None:
        a.out = os.path.join(HERE, "profiles", "temporal_quality.txt")
    import denoise_var_expected as dv
    import temporal_expected as te
    views, ref = orbit()
    hdr, aov, mom, _ = views[-1]
    acc_h, acc_m, share = run(views)
    lines = ["Cornell box %d x %d, an orbit of %d views %.3f rad of yaw apart, %d frames per view, seeds %d + view: rel-L2 at the last view against the oracle's"
             % (W, H, VIEWS, STEP, FRAMES, SEED),
             "%d-frame film of that view (CPU: oracle films and records, numpy restatements); defaults %s" % (REF_FRAMES, te.DEFAULTS),
             "raw %d-frame film                       %.4f" % (FRAMES, rel_l2(hdr, ref)),
             "tirt_denoise_var of it                  %.4f" % rel_l2(dv.denoise_var_expected(hdr, aov, mom), ref),
             "accumulated film                        %.4f" % rel_l2(acc_h, ref),
             "tirt_denoise_var of the accumulated     %.4f" % rel_l2(dv.denoise_var_expected(acc_h, aov, acc_m), ref),
             "pixels of the last view with a history  %.4f   (mean samples per pixel behind the accumulated film %.2f)" % (share, float(acc_m[:, :, 0].mean()))]
    if not a.no_sweep:
        lines.append("sweep, one parameter at a time about the defaults: accumulated / accumulated + tirt_denoise_var / share with a history")
        for name, values in SWEEP.items():
            for v in values:
                h, m, s = run(views, **{name: v})
                lines.append("  %-11s %6.2f   %.4f   %.4f   %.4f" % (name, v, rel_l2(h, ref), rel_l2(dv.denoise_var_expected(h, aov, m), ref), s))
    d_mean, d_m2, n_ok, n_hist = merge_deviation()
    lines.append("merge arithmetic, %d x %d, one camera, 2 + 2 samples, %d of %d history pixels with n_o == 4, against float64:" % (MERGE_W, MERGE_H, n_ok, n_hist))
    lines.append("merge deviation: mean %.3e  M2 %.3e   (worst absolute deviation / largest value of its kind)" % (d_mean, d_m2))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
