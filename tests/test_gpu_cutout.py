"""Alpha cut-outs on the device (include/tirt.h, "Alpha cut-outs").  The oracle knows nothing of textures, so every comparison is with the numpy
restatement (tests/cutout_expected.py; tests/test_cutout_host.py shows it is the oracle where nothing is cut out and caps the rays it excludes at 1 %)
or with a TWIN scene, the same scene without the triangles that lie on transparent texels.  Every result is exact: bit-identical to its expectation, or
a stated error code."""
import numpy as np
import pytest
import torch

import aov_expected
import common
import cutout_expected as ce
import cutout_scenes as cs
import oracle_api
import texture_expected as te
from ti_raytrace_amd import _native, PT_RGB, PT_Spec, RayQuery
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu
f = np.float32
SEED = cs.SEED
EXH = _native.TRAVERSE_EXHAUSTIVE
DEV = torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def on_device(ex):
    ex.integrator.setup_data_cpu(); ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
    return ex.scene.ctx


def render(ex, calls, frames=8, flags=0):
    ctx = ex.scene.ctx
    ctx.film_clear()
    per = frames // calls
    for k in range(calls):
        ctx.pt_rgb_render(k * per, per, SEED, PT_RGB.MAX_DEPTH, 64, flags)
    W, H = ex.imgSizeX, ex.imgSizeY
    return ctx.film_download(W, H)[0], ctx.aov_download(W, H), ctx.moments_download(W, H)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------
def test_alpha_lookup_equals_the_restatement(gpu_ctx_ok):
    sizes = [(1, 1), (2, 2), (5, 3), (64, 64)]
    textures = []
    for wrap in (0, 1):
        for (w, h) in sizes:
            a = np.random.RandomState(11 * w + h + wrap).randint(0, 256, (h, w)).astype(np.uint8)
            a.reshape(-1)[::3] = (127, 128)[wrap]; a.reshape(-1)[1::5] = (128, 127)[wrap]          # texels of exactly 127 and 128
            textures.append((ce.pack_rgba(cs.rgba(w, h, 3 * w + h + wrap, a)), wrap))              # uploaded together: the offsets matter
    ctx = _native.Context(0)
    ctx.texture_upload(textures)
    r = np.random.RandomState(4)
    for t, (img, wrap) in enumerate(textures):
        w, h = img.shape
        uv = r.uniform(-2.0, 3.0, (3000, 2)).astype(f)
        uv[:400, 0] = (r.randint(-2 * w, 3 * w, 400) / f(w)).astype(f)                              # on texel boundaries, one axis, the other, both
        uv[200:600, 1] = (r.randint(-2 * h, 3 * h, 400) / f(h)).astype(f)
        special = np.array([-0.25, 0.0, 1.0, 1.75, 0.5, 1.0 / 3.0, -0.0, np.inf, -np.inf, np.nan, 1.0 / 64.0, 63.0 / 64.0], f)
        uv = np.concatenate([uv, np.stack(np.meshgrid(special, special, indexing="ij"), axis=-1).reshape(-1, 2)], axis=0)
        rows = np.zeros((uv.shape[0], 3), np.uint32)
        rows[:, 0] = t
        rows.view(f)[:, 1:3] = uv
        got = ctx.kat_texture_alpha(rows)
        al = ce.tex_alpha(img, wrap, uv[:, 0], uv[:, 1])
        want = np.stack([al, (al >= ce.CUTOFF).astype(f)], axis=1)
        bad = np.where((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, "texture %d (%s, wrap %d): %d rows differ, first uv %s got %s want %s" % (
            t, img.shape, wrap, bad.size, uv[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
        if w * h > 1:
            assert 0.05 < want[:, 1].mean() < 0.95
        # the RGB lookup does not see the top byte
        assert np.array_equal(bits(ctx.kat_texture(rows)[:, 0:3]), bits(te.tex_albedo(img, wrap, uv[:, 0], uv[:, 1])))
    with pytest.raises(_native.TirtError, match="texture number"):
        ctx.kat_texture_alpha(np.array([[len(textures), 0, 0]], np.uint32))
    ctx.texture_upload([])
    with pytest.raises(_native.TirtError, match="no textures"):
        ctx.kat_texture_alpha(np.zeros((1, 3), np.uint32))
    ctx.close()


# ---- 2. the layered scene -----------------------------------------------------------------------------------------------------------
def test_layered_scene_equals_the_restatement(gpu_ctx_ok):
    ex = cs.layered_scene()
    sc = ex.scene
    ctx = on_device(ex)
    word, _ = ctx.shade_features()
    assert word & _native.SF_CUTOUT and word & _native.SF_TEXTURE
    rays = cs.layered_rays()
    leaf = ce.leaf_indices(ctx.lbvh_download(sc.primitive_count, False, False, True)[2])
    vertex = ctx.vertex_download(sc.vertex_count)
    args = (vertex, sc.primitive_np, sc.material_np, sc.shape_np, cs.textures_of(sc))
    on = ce.closest_hit(*args, sc.texture_cutout, rays, leaf)
    off = ce.closest_hit(*args, [0] * len(sc.textures), rays, leaf)
    k = on["kept"]
    assert (~k).mean() <= 0.01
    deeper = k & ((on["t"] > off["t"]) | ((on["prim"] < 0) & (off["prim"] >= 0)))
    assert deeper.mean() >= 0.25                                          # the test cannot pass by never meeting a hole
    want = ce.hit_record(vertex, sc.primitive_np, rays, on)
    rt = torch.from_numpy(rays).to(DEV)
    for flags in (0, EXH):
        rec, prim, _ = ctx.trace_closest(rays, 64, flags)
        assert np.array_equal(prim[k], on["prim"][k]), (flags, int((prim[k] != on["prim"][k]).sum()))
        got = rec[:, [0, 1, 2, 3, 10, 11]]
        assert np.array_equal(bits(got[k]), bits(want[k])), flags
        h = RayQuery(sc, 64, flags).closest(rt, attributes=True)
        torch.cuda.synchronize(DEV)
        assert np.array_equal(h.prim.cpu().numpy(), prim) and np.array_equal(bits(h.record.cpu().numpy()), bits(rec)), flags
        t, sprim, _ = ctx.trace_shadow(rays, 64, flags)
        assert np.array_equal(bits(t[k]), bits(on["t"][k])) and np.array_equal(sprim[k], on["prim"][k]), flags
        q = RayQuery(sc, 64, flags)
        for tm in (None, (on["t"] * f(0.5)).astype(f), on["t"].copy(), np.nextafter(on["t"], f(np.inf)).astype(f), off["t"].copy()):
            got = q.occluded(rt) if tm is None else q.occluded(rt, torch.from_numpy(tm).to(DEV))
            torch.cuda.synchronize(DEV)
            exp = (on["t"] < ce.INF_VALUE) & ((on["t"] < tm) if tm is not None else True)
            assert np.array_equal(got.cpu().numpy()[k], exp[k]), flags
    # the opposite flags: the restatement with none is what the device gives with none
    ctx.texture_cutout([0] * len(sc.textures))
    assert ctx.shade_features()[0] == word & ~_native.SF_CUTOUT
    rec, prim, _ = ctx.trace_closest(rays, 64, 0)
    assert np.array_equal(prim[k], off["prim"][k]) and np.array_equal(bits(rec[k, 0]), bits(off["t"][k]))
    ctx.close()


# ---- 3. the film against a twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(24, 20), (13, 7)])
def test_film_equals_the_twin_without_the_transparent_triangles(gpu_ctx_ok, oracle_lib, W, H):
    ex = cs.screen_box(W, H)
    twin = cs.screen_box(W, H, twin=True)
    assert twin.scene.primitive_count < ex.scene.primitive_count - 40
    ctx = on_device(ex)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_TRI | _native.SF_TEXTURE | _native.SF_CUTOUT
    got = render(ex, 2)
    ctx2 = on_device(twin)
    assert ctx2.shade_features()[0] == _native.SF_LIGHT_TRI
    want = render(twin, 2)
    for name, a, b in zip(("film", "aov", "moments"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    orc = oracle_api.OracleScene(twin.scene, twin.cam)
    assert orc.lbvh_build() == twin.scene.primitive_count - 1
    ref, _ = orc.render(W, H, 0, 8, seed=SEED)
    assert common.same_bits(want[0], ref)
    assert common.same_bits(want[1], aov_expected.expected(twin, orc, W, H, range(8), SEED)[0])          # the twin's feature records are the oracle's hits'
    # the shadow on the floor shows the holes: the floor pixels (by the twin's pixel-centre hits) hold the twin's values, and with the flag off -- a solid
    # screen under the light -- they hold less light than the twin's
    _, fprim, _ = orc.closest_hit(oracle_api.camera_rays(twin.cam, W, H))
    floor = np.isin(fprim, (0, 1)).reshape(W, H)
    assert floor.sum() >= 5
    assert np.array_equal(bits(got[0][floor]), bits(want[0][floor]))
    ctx.texture_cutout([0])
    solid = render(ex, 2)
    assert float(solid[0][floor].sum()) < float(want[0][floor].sum())
    ctx.close(); ctx2.close()


# ---- 4. general alpha is self-consistent -------------------------------------------------------------------------------------------------
def test_general_alpha_is_self_consistent_and_the_records_are_the_restated_hits(gpu_ctx_ok, oracle_lib):
    W, H = 24, 20
    ex = cs.screen_box(W, H, general_uv=True)
    sc = ex.scene
    ctx = on_device(ex)
    one = render(ex, 1)
    two = render(ex, 2)
    ctx.set_option("overlap_lanes", 1)
    single = render(ex, 4)
    ctx.set_option("overlap_lanes", 4)
    ctx.pixel_set_upload(np.arange(W * H, dtype=np.int32))
    listed = render(ex, 2)
    ctx.pixel_set_clear()
    counted = render(ex, 1, flags=_native.COUNT_NODES)
    for name, other in (("two calls", two), ("one lane", single), ("pixel set", listed), ("count nodes", counted)):
        assert same(one, other), name
    ctx.texture_cutout([0])
    assert not np.array_equal(bits(render(ex, 1)[0]), bits(one[0]))       # the holes matter
    ctx.texture_cutout([1])
    # frame 0 (rays through the pixel centres): coverage, depth and albedo = the restated hits
    rays = oracle_api.camera_rays(ex.cam, W, H)
    leaf = ce.leaf_indices(ctx.lbvh_download(sc.primitive_count, False, False, True)[2])
    textures = cs.textures_of(sc)
    hit = ce.closest_hit(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, textures, sc.texture_cutout, rays, leaf)
    k = hit["kept"]
    assert (~k).mean() <= 0.01
    ok = hit["prim"] >= 0
    hp = np.where(ok, hit["prim"], 0)
    tu, tv = te.hit_uv(sc.vertex_np, sc.primitive_np, hp, hit["u"], hit["v"])
    albedo = np.where(ok[:, None], te.albedo_at(sc.material_np, textures, sc.primitive_np[hp, 2], tu, tv), f(0.0)).astype(f)
    ctx.film_clear()
    ctx.pt_rgb_render(0, 1, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    aov = ctx.aov_download(W, H).reshape(-1, _native.AOV_WORDS)
    assert np.array_equal(aov[k, _native.AOV_ALPHA], ok[k].astype(f))
    assert np.array_equal(bits(aov[k, _native.AOV_DEPTH]), bits(np.where(ok, hit["t"], f(0.0))[k]))
    assert np.array_equal(bits(aov[k, 0:3]), bits(albedo[k]))
    ctx.debug_render(0, SEED, _native.DEBUG_ALBEDO)
    dbg = ctx.film_download(W, H)[0].reshape(-1, 3)
    assert np.array_equal(bits(dbg[k]), bits(albedo[k]))
    ctx.close()


# ---- 5. lifecycle -------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals(gpu_ctx_ok, oracle_lib):
    W, H = 13, 7
    ex = cs.screen_box(W, H, general_uv=True)
    sc = ex.scene
    textures = cs.textures_of(sc)
    spec = PT_Spec.PathTrace(W, H, ex.cam, sc, 64, seed=SEED)
    spec.setup_data_cpu(); spec.setup_data_gpu()
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, sc, 64, seed=SEED, aov=True, moments=True, temporal=True)
    ctx = on_device(ex)
    word = ctx.shade_features()[0]
    assert word == _native.SF_LIGHT_TRI | _native.SF_TEXTURE | _native.SF_CUTOUT
    holes = render(ex, 1)
    # BDPT and the spectral integrators refuse
    for call in (lambda: ctx.bdpt_rgb_render(0, 1, SEED), lambda: ctx.pt_spec_render(0, 1, SEED), lambda: ctx.bdpt_spec_render(0, 1, SEED)):
        with pytest.raises(_native.TirtError, match="albedo texture"):
            call()
    # wrong count or flag values are refused and change nothing
    for bad in ([1, 0], [], [2], [-1]):
        with pytest.raises(_native.TirtError, match="differs|neither"):
            ctx.texture_cutout(bad)
    assert ctx.shade_features()[0] == word and same(render(ex, 1), holes)
    # a texture upload clears the flags and bit 512: the next render is the opaque film
    ctx.texture_upload(textures)
    assert ctx.shade_features()[0] == word & ~_native.SF_CUTOUT
    opaque = render(ex, 1)
    assert not np.array_equal(bits(opaque[0]), bits(holes[0]))
    tri = ctx.wide_tree_download(sc.primitive_count)["tri"]
    assert not tri[:, 7].view(np.uint32).any()                            # no record of an opaque scene carries a tag
    ctx.texture_cutout([0])
    assert same(render(ex, 1), opaque)
    # flags set after a build take effect without a rebuild; the records carry the tags
    ctx.texture_cutout([1])
    assert ctx.shade_features()[0] == word and same(render(ex, 1), holes)
    dl = ctx.wide_tree_download(sc.primitive_count)
    tags = dl["tri"][:, 7].view(np.uint32)[dl["prim_slot"]]
    screen = sc.primitive_np[:, 2] == sc.material_np.shape[0] - 1
    assert np.array_equal(tags, np.where(screen, 1, 0).astype(np.uint32))
    # a material upload that takes the texture away, and gives it back
    m = sc.material_np.copy(); m[-1, 1] = -1.0
    ctx.material_upload(m)
    assert ctx.shade_features()[0] == _native.SF_LIGHT_TRI
    assert not ctx.wide_tree_download(sc.primitive_count)["tri"][:, 7].view(np.uint32).any()
    ctx.material_upload(sc.material_np)
    assert ctx.shade_features()[0] == word and same(render(ex, 1), holes)
    # no list pass runs on a scene with cut-outs
    ctx.set_option("primary_beams_min_frames", 1)
    ctx.stats_reset()
    assert same(render(ex, 1), holes)
    st = ctx.primary_beam_stats()
    assert st["rays"] == 0 and st["list_builds"] == 0
    ctx.texture_cutout([0])
    ctx.stats_reset()
    assert same(render(ex, 1), opaque)
    assert ctx.primary_beam_stats()["rays"] == 8 * W * H
    ctx.texture_cutout([1])
    ctx.set_option("primary_beams_min_frames", 16)
    # tirt_vertex_update followed by a rebuild keeps the cut-outs: moving there and back gives the first film
    pos, nrm = sc.vertex_np[:, 0:3].copy(), sc.vertex_np[:, 3:6].copy()
    sc.update_vertices(np.ascontiguousarray(pos + f(0.01)), nrm)
    assert ctx.shade_features()[0] == word
    moved = render(ex, 1)
    assert not np.array_equal(bits(moved[0]), bits(holes[0]))
    ctx.texture_cutout([0]); solid_moved = render(ex, 1); ctx.texture_cutout([1])
    assert not np.array_equal(bits(moved[0]), bits(solid_moved[0]))
    sc.update_vertices(pos, nrm)
    assert same(render(ex, 1), holes)
    # render_adaptive and temporal_accumulate run on a cut-out scene
    ctx.film_clear()
    res = ctx.pt_rgb_render_adaptive(0, SEED, 0.05, 16, min_samples=4, pass_frames=4)
    assert res["passes"] >= 1 and res["pixel_samples"] >= 4 * W * H
    assert np.isfinite(ctx.film_download(W, H)[0]).all()
    ctx.pixel_set_clear()
    assert same(render(ex, 1), holes)
    ctx.temporal_accumulate()
    hdr, mom = ctx.temporal_download(W, H)
    assert np.isfinite(hdr).all() and float(hdr.sum()) > 0.0
    ctx.close()
