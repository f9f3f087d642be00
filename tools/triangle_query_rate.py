"""Rate of the triangle-distance query on device memory (ti_raytrace_amd.TriangleQuery.closest: csrc/tirt_triangle_query.hip) on one GPU.

    python tools/triangle_query_rate.py [--reps 5] [--out profiles/triangle_query_rate.txt]

Scene: the headline synthetic 100k-triangle scene.  Query sets: 1 Mi small triangles (edges about 0.5 % of the extent) placed (a) uniformly in the root
box and (b) near the surface (around points of random scene triangles, within 1 % of the extent), and (c) a second synthetic 100k-triangle mesh (another
seed) that overlaps the scene.  Per set, without a bound and with max_distance = 2 % of the extent: ms of TriangleQuery.closest (torch events on the
current stream around one call, d2 + prim + code, median of `--reps` after two warm-up calls), Mqueries/s, ms of PointQuery.closest on the same
triangles' 3n vertices in the same run (the kernel the tree already had: the baseline) and the ratio, the share of queries that found something and that
touch (d2 == 0), and the mean N_box / N_leaf per query of a COUNT_NODES walk.  Last: the exhaustive scan on 4 096 queries of set (a), and its bits
against the walk's.  Writes a table to --out and prints it."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from ti_raytrace_amd import PointQuery, TriangleQuery, scenes, _native     # noqa: E402

DEV = torch.device("cuda", 0)
PRIMITIVE_TRI = 1


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(DEV)
    ms = []
    s = torch.cuda.current_stream(DEV)
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(); e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def scene_triangles(scene):
    """[nt, 3, 3] float32 from the scene's host arrays"""
    prim = scene.primitive_np
    first = prim[prim[:, 0] == PRIMITIVE_TRI, 1]
    v = np.asarray(scene.vertex_np, np.float32)
    return np.stack([v[first, 0:3], v[first + 1, 0:3], v[first + 2, 0:3]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangle_query_rate.txt"))
    a = ap.parse_args()
    n = a.n
    ex = scenes.synthetic(64, 64, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    g = torch.Generator(device=DEV); g.manual_seed(1)
    lo = torch.tensor(ex.scene.minboundarynp[0], device=DEV); hi = torch.tensor(ex.scene.maxboundarynp[0], device=DEV)
    ext = float((hi - lo).max())
    st = torch.from_numpy(scene_triangles(ex.scene)).to(DEV)
    rnd = lambda *shape: torch.rand(shape, device=DEV, generator=g)
    shape = (rnd(n, 3, 3) - 0.5) * (0.005 * ext)                              # corners within a cube of 0.5 % of the extent
    uniform = ((lo + (hi - lo) * rnd(n, 1, 3)) + shape).contiguous()
    pick = torch.randint(0, st.shape[0], (n,), device=DEV, generator=g)
    w = rnd(n, 3, 1); w = w / w.sum(dim=1, keepdim=True)
    near = ((st[pick] * w).sum(dim=1, keepdim=True) + (rnd(n, 1, 3) - 0.5) * (0.02 * ext) + shape).contiguous()
    other = scenes.synthetic(64, 64, 4, device_id=0, scene_seed=4321)
    other.scene.setup_data_cpu()
    mesh = torch.from_numpy(scene_triangles(other.scene)).to(DEV).contiguous()
    tq, pq = TriangleQuery(ex.scene), PointQuery(ex.scene)
    lines = ["# python tools/triangle_query_rate.py --reps %d   (one MI355X)" % a.reps,
             "# 100k-triangle headline scene (scenes.synthetic, %d triangles).  uniform / near: %d query triangles with corners in a cube of 0.5 %% of the extent," % (st.shape[0], n),
             "# uniform in the root box / within 1 %% of the extent of a point of a random scene triangle; mesh: the %d triangles of a second synthetic scene (seed 4321)" % mesh.shape[0],
             "# over the same box.  ms = torch events on the current stream around one call (d2 + prim + code), median of %d after 2 warm-up calls; points ms =" % a.reps,
             "# PointQuery.closest on the same triangles' 3n vertices in the same run (the baseline kernel); x points = ms / points ms; found / touch = share of queries",
             "# with prim >= 0 / d2 == 0; N_box (four per node visit) / N_leaf (pair tests) = means per query of a COUNT_NODES walk.",
             "%-16s %9s %12s %10s %9s %8s %8s %10s %10s" % ("query", "ms", "Mqueries/s", "points ms", "x points", "found", "touch", "N_box", "N_leaf")]
    for name, tris in (("uniform", uniform), ("near", near), ("mesh", mesh)):
        m = tris.shape[0]
        verts = tris.reshape(-1, 3)
        for bname, dmax in (("none", None), ("2pct", 0.02 * ext)):
            ms = timed(lambda: tq.closest(tris, dmax), a.reps)
            pms = timed(lambda: pq.closest(verts, dmax), a.reps)
            h, cnt = tq.closest_counts(tris, dmax)
            cnt = cnt.double()
            lines.append("%-16s %9.3f %12.1f %10.3f %9.2f %8.3f %8.3f %10.1f %10.1f" % (name + "_" + bname, ms, m / ms / 1e3, pms, ms / pms, float((h.prim >= 0).double().mean()),
                                                                                          float((h.d2 == 0).double().mean()), float(cnt[:, 0].mean()), float(cnt[:, 1].mean())))
            print(lines[-1], flush=True)
    sub = uniform[:1 << 12].contiguous()
    scan = TriangleQuery(ex.scene, 64, _native.TRAVERSE_EXHAUSTIVE)
    ms = timed(lambda: scan.closest(sub), a.reps)
    a_, b_ = scan.closest(sub, points=True), tq.closest(sub, points=True)
    same = all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a_, b_))
    lines.append("# scan (TRAVERSE_EXHAUSTIVE), 4 096 queries of `uniform`: %.3f ms = %.4f Mqueries/s; all five outputs equal the walk's bits: %s" % (ms, 4096 / ms / 1e3, same))
    assert ctx.stats()["stack_overflow"] == 0
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
