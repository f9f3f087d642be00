"""The Debug integrator's views composed from the CPU oracle (integrator/Debug.py:44-67), in numpy f32.

Camera rays as oracle_api.camera_rays, with the jitter of Camera.py:135-138 for frame != 0 (orc_kat_rand at the dimensions
TM_DIM_JX / TM_DIM_JY = 0 / 1); hits from OracleScene.closest_hit; then the view of each mode, one f32 rounding per source-level
operation.  No transcendental function is on this path, so the device must match these bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_api as oa
from common import same_bits          # noqa: F401  (the tests say dv.same_bits)

MODES = ("albedo", "fnormal", "normal", "gnormal")
INF_VALUE = np.float32(1000000.0)
f = np.float32


def jitter(seed, W, H, frame):
    """(jx, jy) per linear pixel p = i * H + j: tm_rand(seed, p, frame, dim) - 0.5, or zeros at frame 0 (Camera.py:133-137)."""
    n = W * H
    if frame == 0:
        return np.zeros(n, f), np.zeros(n, f)
    L = oa.load()
    rnd = L.orc_kat_rand
    jx = np.fromiter((rnd(seed, p, frame, 0) for p in range(n)), f, n) - f(0.5)
    jy = np.fromiter((rnd(seed, p, frame, 1) for p in range(n)), f, n) - f(0.5)
    return jx, jy


def camera_rays(cam, W, H, frame=0, seed=1):
    """[W*H, 6] rays in linear pixel order, as the device's k_debug_generate makes them."""
    jx, jy = jitter(seed, W, H, frame)
    ii, jj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    ii, jj = ii.reshape(-1).astype(f), jj.reshape(-1).astype(f)
    x = ((ii + jx) - f(cam.cx)) / f(cam.fx)                        # Camera.py:138-139
    y = ((jj + jy) - f(cam.cy)) / f(cam.fy)
    z = np.full_like(x, -1.0)
    M = cam.view_inv_np[0].astype(f)
    w = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] * f(0.0) for r in range(3)]
    n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    inv = f(1.0) / np.sqrt(n2)
    d = np.stack([w[0] * inv, w[1] * inv, w[2] * inv], axis=1).astype(f)
    o = np.broadcast_to(cam.eye_np[0].astype(f), d.shape)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=f)


def closest_hits(orc, rays, threads=None):
    """OracleScene.closest_hit in chunks on a few threads (the oracle call drops the GIL and only reads the scene)."""
    threads = threads or min(16, os.cpu_count() or 1)
    n = rays.shape[0]
    step = max(4096, (n + threads - 1) // threads)
    parts = [rays[s:s + step] for s in range(0, n, step)]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        res = list(pool.map(lambda r: orc.closest_hit(r), parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def sign(x):
    """taichi_glsl sign: 1, -1 or 0 (0 for NaN too)"""
    return (x > 0).astype(f) - (x < 0).astype(f)


def compose(scene, rays, hit, prim, mode, W, H):
    """hdr [W, H, 3] of one view from the oracle's hit records (t, pos, gnormal, normal, tex) + primitive ids."""
    t = hit[:, 0]
    ok = t < INF_VALUE
    out = np.zeros((W * H, 3), f)
    if mode == "albedo":
        mat = scene.primitive_np[np.where(ok, prim, 0), 2]
        val = scene.material_np[mat, 2:5].astype(f)                # get_material_color(material, get_prim_mindex(...))
    else:
        gn, nn = hit[:, 4:7].astype(f), hit[:, 7:10].astype(f)
        n = gn if mode == "gnormal" else nn
        if mode == "fnormal":                                      # faceforward(normal, -direction, gnormal) = sign(dot(i, nref)) * n
            i = -rays[:, 3:6]
            s = sign((i[:, 0] * gn[:, 0] + i[:, 1] * gn[:, 1]) + i[:, 2] * gn[:, 2])
            n = s[:, None] * n
        with np.errstate(invalid="ignore"):
            val = (n + f(1.0)) * f(0.5)
    out[ok] = val[ok]
    return out.reshape(W, H, 3)


def views(ex, orc, W, H, frame, seed, modes=MODES):
    """{mode: hdr} for one frame of an example whose host scene is packed and whose camera is set (orc: its OracleScene,
    LBVH built, smooth normals applied where the example has them)."""
    rays = camera_rays(ex.cam, W, H, frame, seed)
    hit, prim = closest_hits(orc, rays)
    return {m: compose(ex.scene, rays, hit, prim, m, W, H) for m in modes}
