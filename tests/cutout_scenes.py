"""Scene builders of the alpha cut-out tests (host side only; tests/test_cutout_host.py and tests/test_gpu_cutout.py share them, so the rays whose
excluded share and hole count the CPU test asserts are the rays the GPU test traces)."""
import numpy as np

import common
import shade_step_cases as cases
from ti_raytrace_amd import Example, PT_RGB

f = np.float32
SEED = 11


def rgba(w, h, seed, alpha):
    """[h, w, 4] uint8: random colours, the given alpha plane"""
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 0:3] = np.random.RandomState(seed).randint(0, 256, (h, w, 3))
    out[..., 3] = alpha
    return out


def checker(w, h, cell=1):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // cell) + (yy // cell)) % 2 == 0, 255, 0).astype(np.uint8)


def disc(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = (xx + 0.5 - w / 2.0) ** 2 + (yy + 0.5 - h / 2.0) ** 2
    return np.where(r2 < (0.38 * w) ** 2, 255, 0).astype(np.uint8)


def mask_images():
    """the cut-out masks of the layered scene: (image, wrap) -- an 8 x 8 checker, random alpha 5 x 3 (with texels of exactly 127 and 128), a 1 x 1 fully
    transparent one, a 64 x 64 disc; both wraps"""
    ra = np.random.RandomState(5).randint(0, 256, (3, 5)).astype(np.uint8)
    ra[0, 0], ra[1, 2], ra[2, 4] = 127, 128, 127
    return [(rgba(8, 8, 1, checker(8, 8)), "repeat"), (rgba(5, 3, 2, ra), "clamp"), (rgba(1, 1, 3, np.zeros((1, 1), np.uint8)), "repeat"),
            (rgba(64, 64, 4, disc(64, 64)), "clamp"), (rgba(8, 8, 6, checker(8, 8, 2)), "clamp")]


LAYERS, PER_LAYER = 5, 12


def layered_scene(W=16, H=16):
    """Sixty tilted triangles in five layers across the z axis (z = 0, -1, .. -4, every vertex off its plane by up to 0.25: no flat box), a sphere behind
    them.  Materials, one mesh each: five cut-out textures (mask_images), an opaque-textured one -- a texture with arbitrary top bytes whose flag stays 0
    --, two untextured ones and an emitter whose row names a cut-out texture (the slot is ignored: it stays solid).  Random vertex uvs.  Host side only."""
    ex = Example.example(W, H, 4, 0)
    sc = ex.scene
    r = np.random.RandomState(21)
    cut_ids = [sc.add_texture(img, wrap=wrap, cutout=True) for img, wrap in mask_images()]
    noisy = rgba(7, 4, 9, np.random.RandomState(10).randint(0, 256, (4, 7)).astype(np.uint8))
    opaque_id = sc.add_texture(noisy, wrap="repeat", cutout=True)          # packed with its top bytes ...
    sc.texture_cutout[opaque_id - 1] = 0                                    # ... which nobody is to read: the flag is off
    mats = []
    for k, tid in enumerate(cut_ids):
        m = cases.disney((0.0, 0.3, 1.0)[k % 3], (0.5, 0.2, 0.9)[k % 3], tuple(r.uniform(0.2, 1.0, 3))); m.alebdoTex = tid; mats.append(m)
    m = cases.disney(0.0, 0.5, (0.7, 0.6, 0.5)); m.alebdoTex = opaque_id; mats.append(m)
    mats.append(cases.disney(0.2, 0.4, (0.3, 0.8, 0.4)))
    m = cases.glass(1.5, 5.0); mats.append(m)
    m = cases.emitter((9.0, 8.0, 6.0)); m.alebdoTex = cut_ids[2]; mats.append(m)      # names the fully transparent texture: stays solid
    # which material a triangle gets: the front layers mostly holes, so that many rays end deeper than they would without the masks
    weights = np.array([[4, 2, 3, 2, 1, 0, 0, 0, 0], [3, 2, 3, 2, 1, 1, 0, 0, 0], [2, 2, 2, 2, 1, 1, 1, 1, 0], [2, 1, 1, 2, 1, 1, 2, 1, 1], [1, 1, 1, 1, 1, 2, 2, 1, 2]], np.float64)
    tris = [[] for _ in mats]
    for layer in range(LAYERS):
        order = r.permutation(np.repeat(np.arange(len(mats)), (weights[layer] / weights[layer].sum() * PER_LAYER + 0.5).astype(int)))
        order = np.resize(order, PER_LAYER)
        for k in range(PER_LAYER):
            c = np.array([-1.5 + 1.0 * (k % 4), -1.0 + 1.0 * (k // 4), -float(layer)]) + r.uniform(-0.2, 0.2, 3) * np.array([1, 1, 0.2])
            ang = r.uniform(0, 2 * np.pi)
            p = np.array([[np.cos(ang + 2 * np.pi * j / 3) * r.uniform(0.7, 1.1), np.sin(ang + 2 * np.pi * j / 3) * r.uniform(0.7, 1.1), r.uniform(-0.25, 0.25)] for j in range(3)])
            tris[order[k]].append(c[None, :] + p)
    for m, tl in zip(mats, tris):
        assert tl, "a material of the layered scene owns no triangle"
        sc.add_mesh(np.asarray(tl), m)
    ex.add_sphere_light(pos=(0.1, -0.2, -7.0), radius=1.6, emission=20.0)
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, sc, 64, seed=SEED, aov=True, moments=True)
    common.host_only(ex)
    sc.vertex_np[:, 6:8] = r.uniform(-1.5, 2.5, (sc.vertex_count, 2)).astype(f)
    return ex


def layered_rays(n=20000, seed=3):
    """half from outside (in front of layer 0, aimed through the stack), half from between the layers in every direction"""
    r = np.random.RandomState(seed)
    h = n // 2
    o1 = np.stack([r.uniform(-2.2, 2.2, h), r.uniform(-1.8, 1.8, h), r.uniform(1.0, 3.0, h)], axis=1)
    far = np.stack([r.uniform(-2.2, 2.2, h), r.uniform(-1.8, 1.8, h), np.full(h, -5.0)], axis=1)
    d1 = far - o1
    o2 = np.stack([r.uniform(-2.0, 2.0, n - h), r.uniform(-1.5, 1.5, n - h), r.uniform(-3.8, -0.2, n - h)], axis=1)
    d2 = r.normal(size=(n - h, 3)); d2[:, 2] *= 2.0
    o = np.concatenate([o1, o2]); d = np.concatenate([d1, d2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), f)


def textures_of(sc):
    return [(t.np_img, w) for t, w in sc.textures]


# ---- the Cornell box with a screen in front of its light ---------------------------------------------------------------------------
def quad(a, b, c, d):
    return np.array([[a, b, c], [a, c, d]], np.float64)


SCREEN_N = 8


def screen_mask():
    """16 x 16 texels in 2 x 2 blocks of one alpha each -- one block per quad of the screen: holes on a checker, a few more by hand"""
    a = checker(16, 16, 2)
    a[0:2, 4:6] = 0; a[6:8, 6:8] = 255
    return a


def screen_box(W, H, holes=True, twin=False, general_uv=False):
    """A box of five Disney walls and a quad light under the ceiling, and below the light a screen of 8 x 8 small quads with ONE cut-out material.
    Each quad's three uvs are ONE point, the middle of its 2 x 2 block of texels of one alpha: every lookup on it reads those four texels only, and
    mix(a, a, t) is a exactly for a = 0 and a = 1.  twin: the same scene without the triangles on transparent texels, the material untextured
    and of the looked-up colour -- colour of the opaque texels is one colour.  general_uv: uvs spread over the whole mask instead (no twin exists)."""
    ex = Example.example(W, H, 8, 0)
    sc = ex.scene
    p = lambda x, y, z: (float(x), float(y), float(z))
    walls = [quad(p(0, 0, 0), p(1, 0, 0), p(1, 0, -1), p(0, 0, -1)), quad(p(0, 1, 0), p(0, 1, -1), p(1, 1, -1), p(1, 1, 0)),
             quad(p(0, 0, -1), p(1, 0, -1), p(1, 1, -1), p(0, 1, -1)), quad(p(0, 0, 0), p(0, 0, -1), p(0, 1, -1), p(0, 1, 0)),
             quad(p(1, 0, 0), p(1, 1, 0), p(1, 1, -1), p(1, 0, -1))]
    for k, wq in enumerate(walls):
        sc.add_mesh(wq, cases.disney((0.0, 0.3, 0.0, 0.0, 0.0)[k], (0.5, 0.2, 0.6, 1.0, 0.5)[k], ((0.8, 0.7, 0.6), (0.7, 0.7, 0.7), (0.6, 0.6, 0.8), (0.8, 0.3, 0.3), (0.3, 0.8, 0.3))[k]))
    sc.add_mesh(quad(p(0.3, 0.99, -0.3), p(0.7, 0.99, -0.3), p(0.7, 0.99, -0.7), p(0.3, 0.99, -0.7)), cases.emitter((30.0, 26.0, 18.0)))
    mask = screen_mask()
    colour = np.array([255, 255, 0], np.uint8)          # (channels of 0 and 1: mix(c, c, t) = c * (1 - t) + c * t is c exactly, so the twin's colour is the lookup's)
    img = np.zeros((16, 16, 4), np.uint8); img[..., 0:3] = colour; img[..., 3] = mask
    # quad (i, j) of the screen, i along x, j along -z; image row 0 is the top: v = 0 is the bottom row
    tl, uvl = [], []
    for i in range(SCREEN_N):
        for j in range(SCREEN_N):
            x0, x1 = 0.2 + 0.6 * i / SCREEN_N, 0.2 + 0.6 * (i + 1) / SCREEN_N
            z0, z1 = -0.2 - 0.6 * j / SCREEN_N, -0.2 - 0.6 * (j + 1) / SCREEN_N
            yof = lambda z: 0.6 + 0.3 * (-0.2 - z) / 0.6 + 0.003 * ((i * 3 + j * 5) % 4)      # rising towards the back: the camera sees its underside; no flat boxes
            q = quad(p(x0, yof(z0), z0), p(x1, yof(z0) + 0.004, z0), p(x1, yof(z1), z1), p(x0, yof(z1) + 0.004, z1))
            opaque = mask[15 - (2 * j + 1), 2 * i] == 255
            if twin and not opaque:
                continue
            tl.append(q)
            if general_uv:
                uvl.append(np.array([[i, j], [i + 1, j], [i + 1, j + 1], [i, j], [i + 1, j + 1], [i, j + 1]], np.float64) / SCREEN_N * 1.9 - 0.3)
            else:
                uvl.append(np.tile(np.array([(2 * i + 0.5) / 16.0, (2 * j + 0.5) / 16.0]), (6, 1)))
    m = cases.disney(0.0, 0.5, tuple(colour / 255.0))
    if not twin:
        m.alebdoTex = sc.add_texture(img, wrap="clamp", cutout=holes)
    first = sc.vertex_count
    sc.add_mesh(np.concatenate(tl), m)
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, sc, 64, seed=SEED, aov=True, moments=True)
    common.host_only(ex)
    sc.vertex_np[first:first + 6 * len(tl), 6:8] = np.concatenate(uvl).astype(f)
    return ex
