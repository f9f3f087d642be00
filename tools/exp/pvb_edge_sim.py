"""What the camera rays' candidate lists cost under three rules for listing a triangle, counted on the CPU (numpy, float64, no device):

  faces    the four faces of the pixel's pyramid (k_pvb_beam since round 5): a triangle is left out if its three corners lie outside one face
  edges    + the triangle's three edge planes through the eye (option "primary_beams_edges", pvb_beam_triangle_off in csrc/tirt_pvb.h)
  clipped  + nr taken from the triangle's plane clipped by the pyramid instead of from its corners (not built: priced here only)

The model: the headline scene's triangles (scenes.synthetic_triangles), the eye 0.8 box diagonals from the centre on +z, fx = 2 * size / 2.4, the pyramid 0.55
pixels wide, nr = the least projection of the corners on the pixel's axis, bound = 1.5 x the farthest of the five probe hits (infinite if one misses), lists cut at
24 leaves with the overflow rule (the farthest goes, the bound comes in to just below it).  A ray tests every listed leaf whose nr is not beyond its hit so far.
The tree's boxes are left out: the triangle test decides nearly every leaf.  "max over 64" takes 64 random rays of different pixels and stands in for a wave
(a wave's pixels are neighbours, so it overstates the spread).

    python tools/exp/pvb_edge_sim.py [--pixels 400] [--jitters 8] [--seed 1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ti_raytrace_amd.scenes import synthetic_triangles      # noqa: E402

CMAX, WIDEN, REACH, INF = 24, 0.55, 1.5, 1.0e6
CORNERS = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])


def hits(o, d, tri):
    """Moller-Trumbore of rays (d [r, 3]) from o against triangles [n, 3, 3]: t [r, n], inf where there is no hit"""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pv = np.cross(d[:, None, :], e2[None, :, :])
    det = (pv * e1[None]).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - tri[:, 0]
        u = (pv * tv[None]).sum(-1) * inv
        qv = np.cross(tv, e1)
        v = (d[:, None, :] * qv[None]).sum(-1) * inv
        t = (e2 * qv).sum(-1)[None] * inv
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return np.where(ok, t, np.inf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=400)
    ap.add_argument("--jitters", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    tris = np.asarray(synthetic_triangles(), np.float64)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    eye = 0.5 * (lo + hi) + np.array([0.0, 0.0, 0.8 * np.linalg.norm(hi - lo)])
    fx, c0 = 2.0 * a.size / 2.4, 0.5 * a.size

    def direction(u, v):
        d = np.stack([(np.asarray(u, float) - c0) / fx, (np.asarray(v, float) - c0) / fx, -np.ones(np.shape(u))], axis=-1)
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    rel = tris - eye
    film = np.stack([-rel[..., 0] / rel[..., 2] * fx + c0, -rel[..., 1] / rel[..., 2] * fx + c0], axis=-1)      # every triangle is in front of the eye
    fmin, fmax = film.min(1), film.max(1)
    rules = ("faces", "edges", "clipped")
    steps = {r: [] for r in rules}; length = {r: [] for r in rules}; left = {r: [] for r in rules}
    for _ in range(a.pixels):
        i, j = rng.integers(0, a.size, 2)
        # the four faces, for triangles in front of the eye: the rectangle of the corners on the film against the pixel's square
        near = np.flatnonzero((fmax[:, 0] >= i - WIDEN) & (fmin[:, 0] <= i + WIDEN) & (fmax[:, 1] >= j - WIDEN) & (fmin[:, 1] <= j + WIDEN))
        T, R = tris[near], rel[near]
        axis = direction(i, j)
        dq = direction(i + WIDEN * CORNERS[:, 0], j + WIDEN * CORNERS[:, 1])
        probes = np.concatenate([axis[None], direction(i + 0.5 * CORNERS[:, 0], j + 0.5 * CORNERS[:, 1])])
        tp = hits(eye, probes, T).min(axis=1) if near.size else np.full(5, np.inf)
        bound0 = REACH * tp.max() if np.isfinite(tp).all() else INF
        nr_corner = (R @ axis).min(axis=1) if near.size else np.zeros(0)
        # the edge planes: one edge with all four corner directions strictly on the far side from the third corner
        m = np.cross(R, np.roll(R, -1, axis=1))                                     # [n, edge, 3]: cross(ga, gb)
        s = np.sign((m[:, 0] * R[:, 2]).sum(-1))
        side = np.einsum("nek,qk->neq", m, dq) * s[:, None, None]
        off = ((side < 0).all(-1).any(-1)) & (s != 0)
        # nr from the plane clipped by the pyramid: the nearest of the four corner rays' crossings of the plane, if all four cross it in front of the eye
        nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
        with np.errstate(divide="ignore", invalid="ignore"):
            tq = (nrm * R[:, 0]).sum(-1)[:, None] / (nrm @ dq.T)
        depth = tq * (dq @ axis)[None]
        nr_plane = np.where((tq > 0).all(-1) & np.isfinite(tq).all(-1), depth.min(-1), -np.inf)
        jit = rng.uniform(-0.5, 0.5, (a.jitters, 2))
        rays = direction(i + jit[:, 0], j + jit[:, 1])
        th = hits(eye, rays, T) if near.size else np.zeros((a.jitters, 0))
        for rule in rules:
            keep = np.ones(near.size, bool) if rule == "faces" else ~off
            nr = np.maximum(nr_corner, nr_plane) if rule == "clipped" else nr_corner
            bound = bound0
            idx = np.flatnonzero(keep & (nr <= bound))
            idx = idx[np.argsort(nr[idx], kind="stable")]
            if idx.size > CMAX:
                bound = min(bound, nr[idx[CMAX]] * 0.999999)
                idx = idx[:CMAX]
                idx = idx[nr[idx] <= bound]
            length[rule].append(idx.size)
            for r in range(a.jitters):
                best, n = np.inf, 0
                for k in idx:
                    if nr[k] > best:
                        break
                    n += 1
                    best = min(best, th[r, k])
                steps[rule].append(n)
                left[rule].append(not (best <= bound or bound >= INF))      # (a list made without a bound and not cut is complete: a miss on it is a miss)
    print("%d pixels x %d jitters, %d triangles, eye %s, fx %.2f" % (a.pixels, a.jitters, tris.shape[0], np.round(eye, 3).tolist(), fx))
    print("%-8s %18s %12s %22s %22s" % ("rule", "leaf steps per ray", "list length", "max steps over 64 rays", "rays left to k_trace"))
    for rule in rules:
        st = np.array(steps[rule])
        groups = [st[rng.permutation(st.size)[:64]].max() for _ in range(200)]
        print("%-8s %18.2f %12.2f %22.2f %21.2f %%" % (rule, st.mean(), np.mean(length[rule]), np.mean(groups), 100.0 * np.mean(left[rule])))


if __name__ == "__main__":
    main()
