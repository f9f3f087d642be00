"""Scenes and pixel regions of the environment-sampling tests (host side only).  Regions are fixed by geometry, through the CPU oracle: the primitive a
pixel's centre ray meets and, for ground pixels, whether rays towards the sun's part of the sky are blocked."""
import numpy as np

import common
import env_sampling_expected as ee
import oracle_api
import shade_step_cases as cases
from ti_raytrace_amd import PT_RGB, scenes
from ti_raytrace_amd import SceneData as SCD

f = np.float32
SEED = 11
SUN_POWER = 20.0


def sun_direction(dtx=0.0, dty=0.0, at=(11, 1), w=16, h=8):
    """the direction whose lookup falls on the bright texel's centre of weight (tx * w = at.x, ty * h = h - 1 - at.y), moved by (dtx, dty) texels"""
    return ee.direction([f((at[0] + dtx) / w)], [f((h - 1 - at[1] + dty) / h)])[0].astype(np.float64)


def sun_scene(W=16, H=12, seed=SEED, env_sampling=False, before=None, **kw):
    """`before(ex)`: changes to the host scene before it is packed"""
    ex = scenes.sun_ground(W, H, 4, 0, env_power=SUN_POWER, env_sampling=env_sampling, seed=seed, moments=True, **kw)
    if before is not None:
        before(ex)
    ex.scene.setup_data_cpu()
    ex.frame_camera()
    return ex


def cornell_sky(W=16, H=12, seed=SEED, env_sampling=False, env_share=0.5, metallic=False):
    """the Cornell box with its mesh light, the sun sky seen through the open side.  metallic: every Disney material a rough metal, the materials on which
    the reference's sampler draws from its stated pdf (tests/test_env_sampling_host.py) and the sample's density ratio is exactly 1"""
    ex = scenes.cornell_box(W, H, 4, device_id=0, seed=seed, moments=True, env_sampling=env_sampling, env_share=env_share)
    if metallic:
        for m in ex.scene.material_cpu:
            if m.type == SCD.MAT_DISNEY:
                m.setMetal(1.0); m.setRough(0.6)
    ex.scene.add_env(scenes.sun_sky_image(), SUN_POWER)
    common.host_only(ex)
    return ex


def regions_sun(ex):
    """{"lit": pixels, "shadow": pixels, "box": pixels} as linear indices i * H + j of the film: ground pixels from which the sun's texel centre and four
    directions 0.4 texels around it are all free / all blocked, and pixels whose centre ray meets the box"""
    W, H = ex.imgSizeX, ex.imgSizeY
    orc = oracle_api.OracleScene(ex.scene, ex.cam)
    assert orc.lbvh_build() == ex.scene.primitive_count - 1
    rays = oracle_api.camera_rays(ex.cam, W, H)
    out, prim, _ = orc.closest_hit(rays)
    ground, box = (prim >= 0) & (prim < 2), prim >= 2
    pos = rays[:, 0:3].astype(np.float64) + rays[:, 3:6].astype(np.float64) * out[:, 0:1].astype(np.float64) + np.array([0.0, 1e-3, 0.0])
    blocked = np.zeros((5, W * H), bool)
    for k, (dx, dy) in enumerate(((0, 0), (0.4, 0), (-0.4, 0), (0, 0.4), (0, -0.4))):
        d = sun_direction(dx, dy)
        sh = np.concatenate([pos, np.broadcast_to(d, pos.shape)], axis=1).astype(f)
        blocked[k] = orc.closest_hit(sh)[1] >= 0
    orc.close()
    return {"lit": np.where(ground & ~blocked.any(axis=0))[0], "shadow": np.where(ground & blocked.all(axis=0))[0], "box": np.where(box)[0]}


def regions_cornell(ex):
    """three fixed blocks of the film: the floor, the back wall, the left third (wall and tall box)"""
    W, H = ex.imgSizeX, ex.imgSizeY
    ii, jj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    lin = (ii * H + jj)
    return {"floor": lin[W // 4:3 * W // 4, 1:H // 4].reshape(-1), "back": lin[3 * W // 8:5 * W // 8, 3 * H // 8:5 * H // 8].reshape(-1),
            "left": lin[3 * W // 16:3 * W // 8, H // 4:3 * H // 4].reshape(-1)}


def region_stats(mom, pixels):
    """(mean over the region's pixels and the three channels of the per-pixel means, its standard error) from the moment records [W, H, 8]: the pixels are
    independent, a pixel's mean has variance M2 / (n (n - 1)) per channel; the three channels of a pixel are NOT independent, so their errors add linearly"""
    m = mom.reshape(-1, 8)[pixels].astype(np.float64)
    n = m[:, 0]
    assert (n >= 2).all() and (m[:, 7] == 0).all()
    mean = m[:, 1:4].mean()
    se_pix = np.sqrt(m[:, 4:7] / (n * (n - 1.0))[:, None]).sum(axis=1) / 3.0
    return mean, float(np.sqrt((se_pix ** 2).sum()) / pixels.size)


def z_score(a, b):
    return (a[0] - b[0]) / np.sqrt(a[1] ** 2 + b[1] ** 2)
