"""Error of the winding number's far-field approximation (ti_raytrace_amd.PointQuery.winding_number: csrc/tirt_winding.hip) against the exact sum in float64.

    python tools/winding_accuracy.py [--out profiles/winding_accuracy.txt]

Meshes: the torus of tests/winding_expected.py, closed and with its window removed, at 2 000 and 100 000 triangles.  Queries: winding_expected.accuracy_queries
(2 000 points uniform in the mesh's box scaled by 1.5, a fixed seed: the queries of tests/test_gpu_winding.py's accuracy test).  Per mesh and beta = 2, 3, 4,
inf: the maximum and mean |w - w64|, the queries on the wrong side of 0.5 among those farther than 2 % of the extent from the surface, and the leaves evaluated
per query.  The 2 000-triangle maxima at beta = 2 are the constants of that test.  Writes a table to --out and prints it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import winding_expected as W                                    # noqa: E402
from ti_raytrace_amd import Example, PointQuery, PT_RGB          # noqa: E402
from ti_raytrace_amd import SceneData as SCD                     # noqa: E402

DEV = torch.device("cuda", 0)


def winding64(p, tris, block=512):
    """the sum of the signed solid angles / 4 pi in float64, a block of triangles at a time"""
    p = np.asarray(p, np.float64)[:, None, :]
    w = np.zeros(p.shape[0])
    for lo in range(0, tris.shape[0], block):
        t = np.asarray(tris[lo:lo + block], np.float32).astype(np.float64)[None]
        a, b, c = t[:, :, 0] - p, t[:, :, 1] - p, t[:, :, 2] - p
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = (a * np.cross(b, c)).sum(axis=2)
        den = la * lb * lc + (a * b).sum(axis=2) * lc + (a * c).sum(axis=2) * lb + (b * c).sum(axis=2) * la
        w += (2.0 * np.arctan2(num, den)).sum(axis=1)
    return w / (4.0 * np.pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_accuracy.txt"))
    ap.add_argument("--sizes", default="40x25,250x200")
    a = ap.parse_args()
    lines = ["# python tools/winding_accuracy.py   (one MI355X)",
             "# torus R = 1, r = 0.4 of 2 nu nv triangles, closed and with a window (a quarter of the ring, the outer two fifths of the tube) removed; 2 000 queries uniform in",
             "# the box scaled by 1.5 (tests/winding_expected.py, accuracy_queries).  error = |w - w64|, w64 the exact sum in float64; wrong = queries farther than 2 % of the",
             "# extent from the surface whose w is on the other side of 0.5 than w64; leaves = leaves evaluated per query (of T).",
             "%-22s %8s %6s %12s %12s %8s %8s %10s" % ("mesh", "T", "beta", "max error", "mean error", "far", "wrong", "leaves")]
    for size in a.sizes.split(","):
        nu, nv = (int(x) for x in size.split("x"))
        closed = W.torus_triangles(nu, nv)
        keep = W.torus_hole(nu, nv, (0, nu // 4), (-(nv // 5), nv // 5))
        for name, tris in (("torus", closed), ("torus_open", closed[keep])):
            ex = Example.example(32, 32, 4, 0)
            mat = SCD.Material(); mat.type = SCD.MAT_DISNEY; mat.setMetal(0.0); mat.setRough(0.5); mat.setColor([0.8, 0.8, 0.8, 1.0]); mat.alebdoTex = -1
            ex.scene.add_mesh(tris, mat)
            ex.integrator = PT_RGB.PathTrace(32, 32, ex.cam, ex.scene, 64)
            ex.build_scene()
            q = PointQuery(ex.scene)
            pts = W.accuracy_queries(tris)
            w64 = winding64(pts, tris)
            p = torch.from_numpy(pts).to(DEV)
            dist = q.closest(p).dist2.sqrt().cpu().numpy()
            t = tris.reshape(-1, 3)
            far = dist > 0.02 * float((t.max(axis=0) - t.min(axis=0)).max())
            for beta in (2.0, 3.0, 4.0, float("inf")):
                w, counts = q.winding_counts(p, beta)
                w = w.cpu().numpy(); leaves = float(counts[:, 1].double().mean())
                err = np.abs(w.astype(np.float64) - w64)
                wrong = int((far & ((w > 0.5) != (w64 > 0.5))).sum())
                lines.append("%-22s %8d %6g %12.4e %12.4e %8d %8d %10.1f" % ("%s %dx%d" % (name, nu, nv), tris.shape[0], beta, err.max(), err.mean(), int(far.sum()), wrong, leaves))
                print(lines[-1], flush=True)
            assert ex.scene.ctx.stats()["stack_overflow"] == 0
            del ex, q
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
