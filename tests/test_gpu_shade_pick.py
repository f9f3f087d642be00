"""The instantiation of k_shade that tirt_shade_instantiation names for a live context's feature word (include/tirt.h) is one that the context accepts: for every
reachable combination of the three derived bits -- the environment's light sample (1024), RGBE8 texels (2048), emitters chosen by power (4096) --, before and
after a material names a texture; and the choice between a narrow instantiation and the generic one (option "shade_specialize") leaves the film alone.
Which kernel a render launched is not observable from its film; tests/test_shade_pick_host.py holds the choice itself to the selection it replaced."""
import numpy as np
import pytest

import common
import shade_step_cases as cases
from ti_raytrace_amd import _native, scenes, PT_RGB
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu
DERIVED = _native.SF_ENV_SAMPLE | _native.SF_ENV_HDR | _native.SF_LIGHT_POWER      # 7168
# (environment, its light sample, emitters by power): without a lit environment there is no light sample to switch on
REACHABLE = [(env, sample, power) for env in (None, "ldr", "hdr") for sample in (False, True) for power in (False, True) if env or not sample]


def step_rows(ex, n=64):
    """n rows of tirt_kat_shade_step: misses in every kind of direction of shade_step_cases, then hits of the first primitives from above, path states as there"""
    rng = np.random.RandomState(5)
    miss = cases.miss_rows(rng)
    miss = miss[:: miss.shape[0] // (n // 2)][: n // 2]
    k = n - miss.shape[0]
    head, tail, spec = cases.path_state(k, rng)
    o = np.tile(np.float32([0.1, 2.0, 0.2]), (k, 1)); d = cases.unit(np.tile(np.float32([0.1, -1.0, 0.05]), (k, 1))).astype(np.float32)
    hit = cases.pack(head, o, d, np.full(k, 1.5, np.float32), np.full(k, 0.25, np.float32), np.full(k, 0.5, np.float32), np.arange(k) % ex.scene.primitive_count, tail, spec)
    return np.ascontiguousarray(np.concatenate([miss, hit], axis=0))


@pytest.mark.parametrize("env,sample,power", REACHABLE, ids=lambda v: {None: "noenv", True: "on", False: "off"}.get(v, v))
def test_the_named_instantiation_is_one_the_context_accepts(gpu_ctx_ok, env, sample, power):
    ex = common.step_scene(env)
    ctx, sc = common.on_device(ex), ex.scene
    ctx.env_sampling(sample, 0.5)
    ctx.light_sampling(power, 0.25)
    rows = step_rows(ex)
    word, on = ctx.shade_features()
    want = (_native.SF_ENV_SAMPLE if sample else 0) | (_native.SF_ENV_HDR if env == "hdr" else 0) | (_native.SF_LIGHT_POWER if power else 0)
    assert on == 1 and word & DERIVED == want and not word & (_native.SF_TEXTURE | _native.SF_TEXTURE_PARAM), (word, want)
    feat = _native.shade_instantiation(word, 1)
    assert feat == 127 | (word & DERIVED) and _native.shade_instantiation(word, 0) == feat
    assert ctx.kat_shade_step(feat, rows).shape == (64, _native.KAT_STEP_OUT)
    # a Disney row names the uploaded texture as its roughness map (word 7, 1-based): bit 256, which only the instantiations with every texture slot cover
    mats = sc.material_np.copy()
    mats[np.where(mats[:, 0] == SCD.MAT_DISNEY)[0][0], 7] = 1.0
    ctx.material_upload(mats)
    word = ctx.shade_features()[0]
    assert word & _native.SF_TEXTURE_PARAM and word & DERIVED == want, (word, want)
    feat = _native.shade_instantiation(word, 1)
    assert feat == 511 | (word & DERIVED) and _native.shade_instantiation(word, 0) == feat
    assert ctx.kat_shade_step(feat, rows).shape == (64, _native.KAT_STEP_OUT)


def test_cornell_box_gets_the_mesh_light_kernel_or_the_generic_one_and_one_film(gpu_ctx_ok):
    ex = scenes.cornell_box(16, 16, 2, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    word = ctx.shade_features()[0]
    assert word == _native.SF_LIGHT_TRI == 4
    assert _native.shade_instantiation(word, 1) == 4 and _native.shade_instantiation(word, 0) == 127
    films = []
    for specialize in (1, 0):
        ctx.set_option("shade_specialize", specialize)
        assert ctx.shade_features() == (word, specialize)
        ctx.film_clear()
        ctx.pt_rgb_render(0, 2, 3, PT_RGB.MAX_DEPTH, 64, 0)
        films.append(ctx.film_download(16, 16)[0])
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32)) and np.isfinite(films[0]).all() and films[0].sum() > 0
