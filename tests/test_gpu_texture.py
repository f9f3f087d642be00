"""Albedo textures on the device (include/tirt.h, "Albedo textures on materials").  The oracle knows nothing of textures, so every comparison is with the
numpy restatement (tests/texture_expected.py) or with a TWIN scene: the same geometry, untextured, each material's colour the restated lookup at the uv
its hits have -- tests/test_texture_host.py shows why that is the same: a shading step sees one colour per hit, and a uv of exactly (0, 0) reads texel
(0, 0) with weight exactly 1.  Every result is exact: bit-identical to its expectation, or a stated error code."""
import numpy as np
import pytest

import common
import oracle_api
import shade_step_cases as cases
import texture_expected as te
from ti_raytrace_amd import _native, Example, PT_RGB, PT_Spec
from ti_raytrace_amd import SceneData as SCD
from ti_raytrace_amd import Texture as TX

pytestmark = pytest.mark.gpu
f = np.float32
SEED = 11


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def packed(rgb):
    t = TX.Texture(); t.load_array(rgb)
    return t.np_img


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


# ---- 1. the lookup ----------------------------------------------------------------------------------------------------------------
def test_lookup_equals_the_restatement(gpu_ctx_ok, oracle_lib):
    sizes = [(1, 1), (2, 2), (5, 3), (64, 64)]
    textures = [(packed(image(w, h, 3 * w + h + wrap)), wrap) for wrap in (0, 1) for (w, h) in sizes]      # uploaded together: the offsets matter
    ctx = _native.Context(0)
    ctx.texture_upload(textures)
    r = np.random.RandomState(4)
    n = 3000
    uv = r.uniform(-2.0, 3.0, (n, 2)).astype(f)
    special = np.array([-0.25, 0.0, 1.0, 1.75, 0.25, 0.5, 0.75, 1.0 / 3.0, 0.2, 0.4, 0.6, 0.8, -0.0, np.inf, -np.inf, np.nan, 1.0 / 64.0, 63.0 / 64.0], f)
    grid = np.stack(np.meshgrid(special, special, indexing="ij"), axis=-1).reshape(-1, 2)
    uv = np.concatenate([uv, grid], axis=0)
    for t, (img, wrap) in enumerate(textures):
        rows = np.zeros((uv.shape[0], 3), np.uint32)
        rows[:, 0] = t
        rows.view(f)[:, 1:3] = uv
        got = ctx.kat_texture(rows)
        c = te.tex_albedo(img, wrap, uv[:, 0], uv[:, 1])
        want = np.concatenate([c, te.srgb_to_lrgb(c)], axis=1)
        bad = np.where((bits(got) != bits(want)).any(axis=1))[0]
        assert bad.size == 0, "texture %d (%s, wrap %d): %d rows differ, first uv %s got %s want %s" % (
            t, img.shape, wrap, bad.size, uv[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
    with pytest.raises(_native.TirtError, match="texture number"):
        ctx.kat_texture(np.array([[len(textures), 0, 0]], np.uint32))
    ctx.texture_upload([])
    with pytest.raises(_native.TirtError, match="no textures"):
        ctx.kat_texture(np.zeros((1, 3), np.uint32))
    ctx.close()


# ---- 2. one shading step with general uvs ---------------------------------------------------------------------------------------
def step_scene():
    """192 triangles with random uvs, each with its own textured Disney or glass material (8 textures of several sizes, both wrap modes), two untextured
    ones, a sphere light and a mesh light"""
    ex = Example.example(cases.FILM_W, cases.FILM_H, 4, 0)
    r = np.random.RandomState(8)
    tex_ids = [ex.scene.add_texture(image(w, h, 50 + k), wrap="repeat" if k % 2 else "clamp")
               for k, (w, h) in enumerate([(1, 1), (2, 2), (5, 3), (64, 64), (3, 7), (16, 4), (2, 9), (8, 8)])]
    from ti_raytrace_amd import scenes
    tri = scenes.synthetic_triangles(194, 31, 0.25)
    for k in range(194):
        if k % 5 == 4:
            m = cases.glass((1.0, 1.3, 2.4)[k % 3], (0.01, 5.0, 300.0)[(k // 3) % 3], tuple(r.uniform(0.2, 1.0, 3)))
        else:
            m = cases.disney(cases.METALLIC[k % 3], cases.ROUGHNESS[k % 5], tuple(r.uniform(0.0, 1.0, 3)))
        m.alebdoTex = tex_ids[k % len(tex_ids)] if k < 192 else (0 if k == 192 else -1)
        ex.scene.add_mesh(tri[k:k + 1], m, cases.tilted_normals(tri[k:k + 1], r) if k % 7 == 3 else None)
    ex.scene.add_mesh(np.array([[[-0.5, 1.6, -0.5], [0.5, 1.6, -0.5], [0.0, 1.6, 0.6]]]), cases.emitter((30.0, 28.0, 20.0)))
    ex.add_sphere_light(pos=(0.0, 3.0, 0.0), radius=0.75, emission=50.0)
    ex.scene.material_cpu[-2].alebdoTex = 3          # an emitter ignores its slot
    ex.integrator = PT_RGB.PathTrace(cases.FILM_W, cases.FILM_H, ex.cam, ex.scene, 64)
    common.host_only(ex)
    uv = r.uniform(-1.5, 2.5, (ex.scene.vertex_count, 2)).astype(f)
    ex.scene.vertex_np[:, 6:8] = uv
    return ex


def test_shading_step_equals_the_oracle_on_the_twin(gpu_ctx_ok, oracle_lib):
    ex = step_scene()
    sc = ex.scene
    textures = [(t.np_img, w) for t, w in sc.textures]
    r = np.random.RandomState(12)
    ntri = 195
    # one barycentric point per triangle, 40 path states and directions each
    bu = r.uniform(0.0, 1.0, ntri); bv = r.uniform(0.0, 1.0, ntri) * (1.0 - bu)
    bu, bv = bu.astype(f), bv.astype(f)
    reps = 40
    prim = np.repeat(np.arange(ntri), reps)
    n = prim.size
    vi = sc.primitive_np[prim, 1]
    pos = sc.vertex_np[vi, 0:3].astype(np.float64) * (1.0 - bu[prim] - bv[prim])[:, None] + sc.vertex_np[vi + 1, 0:3] * bu[prim][:, None] + sc.vertex_np[vi + 2, 0:3] * bv[prim][:, None]
    d = cases.unit(r.normal(size=(n, 3))).astype(f)
    head, tail, spec = cases.path_state(n, r)
    rows = cases.pack(head, (pos - d.astype(np.float64)).astype(f), d, np.ones(n, f), bu[prim], bv[prim], prim, tail, spec)
    # the twin: every triangle's material gets the restated lookup at the triangle's point
    u, v = te.hit_uv(sc.vertex_np, sc.primitive_np, np.arange(ntri), bu, bv)
    mat_of = sc.primitive_np[:ntri, 2]
    assert np.unique(mat_of).size == ntri
    twin = te.twin_materials(sc.material_np, textures, {int(m): (u[k], v[k]) for k, m in enumerate(mat_of)})
    assert int((twin[:, 2:5] != sc.material_np[:, 2:5]).any(axis=1).sum()) == 192
    base = sc.material_np
    try:
        sc.material_np = twin
        orc = oracle_api.OracleScene(sc, ex.cam)
        assert orc.lbvh_build() == sc.primitive_count - 1
        want = orc.kat_shade_step(rows)
    finally:
        sc.material_np = base
    ex.integrator.setup_data_gpu(); sc.setup_data_gpu()
    ctx = sc.ctx
    word, _ = ctx.shade_features()
    assert word == _native.SF_GLASS | _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPHERE | _native.SF_TEXTURE
    got = ctx.kat_shade_step(255, rows)
    report = cases.first_differences(got, want, rows, ex)
    assert not report, "\n".join(report)
    assert int((want.view(np.int32)[:, 3] == 1).sum()) > 5000 and int((want.view(np.int32)[:, 16] == 1).sum()) > 500      # (the rows shade and sample lights)
    for feat in (128, _native.SF_ALL):                  # 128 alone is no instantiation; 127 does not cover a textured scene
        with pytest.raises(_native.TirtError, match="instantiation|cover"):
            ctx.kat_shade_step(feat, rows[:4])
    # the records carry the uvs, and only here
    rec = ctx.shade_table_download(0, sc.primitive_count)
    vi = sc.primitive_np[:ntri, 1]
    assert np.array_equal(rec[:ntri, 7], np.concatenate([sc.vertex_np[vi, 6:8], sc.vertex_np[vi + 1, 6:8]], axis=1))
    assert np.array_equal(rec[:ntri, 2, 3], sc.vertex_np[vi + 2, 6]) and np.array_equal(rec[:ntri, 3, 3], sc.vertex_np[vi + 2, 7])
    assert not rec[ntri:, 7].any()
    # the twin on the device: untextured, bit 128 clear, and the generic kernel gives the same words
    ctx.texture_upload([])
    ctx.material_upload(twin)
    assert ctx.shade_features()[0] == word & ~_native.SF_TEXTURE
    assert not ctx.shade_table_download(0, sc.primitive_count)[:, 7].any()
    assert not cases.first_differences(ctx.kat_shade_step(_native.SF_ALL, rows), want, rows, ex)
    with pytest.raises(_native.TirtError, match="needs uploaded textures"):
        ctx.kat_shade_step(255, rows[:4])
    ctx.close()


# ---- 3 - 5. films ---------------------------------------------------------------------------------------------------------------
def quad(a, b, c, d):
    return np.array([[a, b, c], [a, c, d]], np.float64)


QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float64)
BOX_TEXTURES = [(1, 1), (2, 2), (5, 3), (64, 64), (7, 4)]


def box_scene(W, H, uv_scale, textured=True, colours=None):
    """a Cornell-like box: five Disney walls, each with its own texture of its own size, an untextured glass tetrahedron and a quad light.  uv_scale 0: every uv (0, 0).
    textured False: the twin, whose wall colours are `colours`"""
    ex = Example.example(W, H, 8, 0)
    sc = ex.scene
    p = lambda x, y, z: (float(x), float(y), float(z))
    walls = [quad(p(0, 0, 0), p(1, 0, 0), p(1, 0, -1), p(0, 0, -1)), quad(p(0, 1, 0), p(0, 1, -1), p(1, 1, -1), p(1, 1, 0)),
             quad(p(0, 0, -1), p(1, 0, -1), p(1, 1, -1), p(0, 1, -1)), quad(p(0, 0, 0), p(0, 0, -1), p(0, 1, -1), p(0, 1, 0)),
             quad(p(1, 0, 0), p(1, 1, 0), p(1, 1, -1), p(1, 0, -1))]
    for k, wq in enumerate(walls):
        m = cases.disney((0.0, 0.3, 1.0, 0.0, 0.0)[k], (0.5, 0.2, 0.001, 1.0, 0.5)[k], (0.8, 0.7, 0.6) if colours is None else colours[k])
        if textured:
            w, h = BOX_TEXTURES[k]
            m.alebdoTex = sc.add_texture(image(w, h, 70 + k), wrap="clamp" if k == 2 else "repeat")
        sc.add_mesh(wq, m)
    a, b, c, d = np.array([0.3, 0.05, -0.3]), np.array([0.7, 0.05, -0.35]), np.array([0.5, 0.05, -0.7]), np.array([0.5, 0.55, -0.45])
    sc.add_mesh(np.array([[a, c, b], [a, b, d], [b, c, d], [c, a, d]]), cases.glass(1.5, 5.0))
    sc.add_mesh(quad(p(0.35, 0.99, -0.35), p(0.65, 0.99, -0.35), p(0.65, 0.99, -0.65), p(0.35, 0.99, -0.65)), cases.emitter((17.0, 12.0, 4.0)))
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, sc, 64, seed=SEED, aov=True, moments=True)
    common.host_only(ex)
    uvs = np.zeros((sc.vertex_count, 2), f)
    for k in range(5):
        uvs[6 * k:6 * k + 6] = (QUAD_UV * uv_scale * (1.0 + 0.37 * k) - 0.21 * k * (uv_scale != 0)).astype(f)
    sc.vertex_np[:, 6:8] = uvs
    return ex


def on_device(ex):
    ex.integrator.setup_data_cpu(); ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
    return ex.scene.ctx


def render(ex, calls, frames=8):
    ctx = ex.scene.ctx
    ctx.film_clear()
    per = frames // calls
    for k in range(calls):
        ctx.pt_rgb_render(k * per, per, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    W, H = ex.imgSizeX, ex.imgSizeY
    return ctx.film_download(W, H)[0], ctx.aov_download(W, H), ctx.moments_download(W, H)


@pytest.mark.parametrize("W,H", [(24, 20), (13, 7)])
def test_film_with_zero_uvs_equals_the_twin(gpu_ctx_ok, oracle_lib, W, H):
    ex = box_scene(W, H, 0.0)
    textures = [(t.np_img, w) for t, w in ex.scene.textures]
    colours = [te.tex_albedo(img, wrap, np.zeros(1, f), np.zeros(1, f))[0] for img, wrap in textures]
    for (img, _), c in zip(textures, colours):                                   # texel (0, 0) itself
        assert c.tolist() == [f((int(img[0, 0]) >> s) & 255) / f(255) for s in (16, 8, 0)]
    twin = box_scene(W, H, 0.0, textured=False, colours=[tuple(float(x) for x in c) for c in colours])
    assert np.array_equal(twin.scene.material_np[:, 2:], te.twin_materials(ex.scene.material_np, textures, {k: (0.0, 0.0) for k in range(5)})[:, 2:])
    ctx = on_device(ex)
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI | _native.SF_TEXTURE
    got = render(ex, 2)
    ctx2 = on_device(twin)
    assert ctx2.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI
    want = render(twin, 2)
    for name, a, b in zip(("film", "aov", "moments"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    assert float(got[0].sum()) > 0.0 and np.unique(got[1][..., 0]).size > 4
    orc = oracle_api.OracleScene(twin.scene, twin.cam)
    assert orc.lbvh_build() == twin.scene.primitive_count - 1
    ref, _ = orc.render(W, H, 0, 8, seed=SEED)
    assert common.same_bits(got[0], ref)
    ctx.close(); ctx2.close()


def test_general_uvs_are_self_consistent_and_the_albedo_is_the_lookup(gpu_ctx_ok, oracle_lib):
    W, H = 24, 20
    ex = box_scene(W, H, 1.7)
    sc = ex.scene
    textures = [(t.np_img, w) for t, w in sc.textures]
    ctx = on_device(ex)
    one = render(ex, 1)
    four = render(ex, 4)
    ctx.set_option("overlap_lanes", 1)
    single = render(ex, 4)
    ctx.set_option("overlap_lanes", 4)
    ctx.pixel_set_upload(np.arange(W * H, dtype=np.int32))                      # every pixel, through the LIST instantiation
    listed = render(ex, 2)
    ctx.pixel_set_clear()
    for other in (four, single, listed):
        for name, a, b in zip(("film", "aov", "moments"), one, other):
            assert np.array_equal(bits(a), bits(b)), name
    # the textures matter: the untextured scene gives another film
    ctx.texture_upload([])
    flat = render(ex, 1)
    assert not np.array_equal(bits(flat[0]), bits(one[0]))
    ctx.texture_upload(textures)
    # albedo of frame 0 (rays through the pixel centres) = the restated lookup at the oracle's hits
    orc = oracle_api.OracleScene(sc, ex.cam)
    assert orc.lbvh_build() == sc.primitive_count - 1
    out, prim, _, bary = orc.closest_hit(oracle_api.camera_rays(ex.cam, W, H), uv=True)
    hit = out[:, 0] < cases.INF_VALUE
    want = np.zeros((W * H, 3), f)
    hp = prim[hit]
    u, v = te.hit_uv(sc.vertex_np, sc.primitive_np, hp, bary[hit, 0], bary[hit, 1])
    want[hit] = te.albedo_at(sc.material_np, textures, sc.primitive_np[hp, 2], u, v)
    assert int(hit.sum()) > W * H // 2 and np.unique(want[hit], axis=0).shape[0] > 100      # (surface detail, not five flat colours)
    ctx.film_clear()
    ctx.pt_rgb_render(0, 1, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    aov = ctx.aov_download(W, H).reshape(-1, _native.AOV_WORDS)
    assert np.array_equal(bits(aov[:, 0:3]), bits(want))
    ctx.debug_render(0, SEED, _native.DEBUG_ALBEDO)
    dbg = ctx.film_download(W, H)[0].reshape(-1, 3)
    assert np.array_equal(bits(dbg), bits(want))
    ctx.close()


def test_a_slot_far_below_zero_is_untextured(gpu_ctx_ok, oracle_lib):
    """slot values that the conversion to int saturates (-3e9, -inf) are below 1 like -1: the host accepts the rows, and k_shade, k_aov and the Debug albedo
    view treat those materials as untextured -- the film, its records and the view equal those of the same rows with -1, bit for bit"""
    W, H = 13, 7
    ex = box_scene(W, H, 1.7)
    sc = ex.scene
    ctx = on_device(ex)
    results = []
    for slots in ((-3.0e9, -np.inf), (-1.0, -1.0)):
        m = sc.material_np.copy()
        m[0, 1], m[2, 1] = slots
        ctx.material_upload(m)
        assert ctx.shade_features()[0] & _native.SF_TEXTURE            # (the other walls keep their textures)
        got = render(ex, 1)
        ctx.debug_render(0, SEED, _native.DEBUG_ALBEDO)
        results.append(got + (ctx.film_download(W, H)[0],))
    for name, a, b in zip(("film", "aov", "moments", "debug albedo"), *results):
        assert np.array_equal(bits(a), bits(b)), name
    flat = np.unique(results[0][3].reshape(-1, 3), axis=0)
    assert any(np.array_equal(row, sc.material_np[k, 2:5]) for row in flat for k in (0, 2))      # one of the two walls is in view, in its material colour
    ctx.close()


def test_refusals_and_lifecycle(gpu_ctx_ok, oracle_lib):
    W, H = 13, 7
    ex = box_scene(W, H, 1.7)
    sc = ex.scene
    textures = [(t.np_img, w) for t, w in sc.textures]
    spec = PT_Spec.PathTrace(W, H, ex.cam, sc, 64, seed=SEED)
    spec.setup_data_cpu(); spec.setup_data_gpu()                                # (the spectral tables; the film is created again below)
    ctx = on_device(ex)
    textured = render(ex, 1)
    for call in (lambda: ctx.bdpt_rgb_render(0, 1, SEED), lambda: ctx.pt_spec_render(0, 1, SEED), lambda: ctx.bdpt_spec_render(0, 1, SEED)):
        with pytest.raises(_native.TirtError, match="albedo texture.*count 0"):
            call()
    # a material row may not name a texture that is not there
    with pytest.raises(_native.TirtError, match="names texture"):
        ctx.texture_upload(textures[:2])
    bad = sc.material_np.copy(); bad[0, 1] = 9
    with pytest.raises(_native.TirtError, match="names texture 9 of 5"):
        ctx.material_upload(bad)
    again = render(ex, 1)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(textured, again))          # the refused calls changed nothing
    # cleared: the untextured film, records without uvs, and the other integrators work again
    ctx.texture_upload([])
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI
    flat = render(ex, 1)
    assert not ctx.shade_table_download(0, sc.primitive_count)[:, 7].any()
    plain = box_scene(W, H, 1.7, textured=False)
    ctx2 = on_device(plain)
    want = render(plain, 1)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(flat, want))
    ctx2.close()
    ctx.film_clear(); ctx.bdpt_rgb_render(0, 1, SEED); ctx.sync()
    ctx.film_clear(); ctx.pt_spec_render(0, 1, SEED); ctx.sync()
    assert np.isfinite(ctx.film_download(W, H)[0]).all()
    # a texture upload after a render takes effect on the next render
    ctx.texture_upload(textures)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(render(ex, 1), textured))
    other = [(packed(image(img.shape[0], img.shape[1], 90 + k)), wrap) for k, (img, wrap) in enumerate(textures)]
    ctx.texture_upload(other)
    assert not np.array_equal(bits(render(ex, 1)[0]), bits(textured[0]))
    ctx.texture_upload(textures)
    # moving the vertices keeps the uvs: the records of the moved scene carry them, and moving back gives the first film
    pos, nrm = sc.vertex_np[:, 0:3].copy(), sc.vertex_np[:, 3:6].copy()
    sc.update_vertices(np.ascontiguousarray(pos + f(0.01)), nrm)
    rec = ctx.shade_table_download(0, sc.primitive_count)
    assert np.array_equal(rec[:10, 7], np.concatenate([sc.vertex_np[0:30:3, 6:8], sc.vertex_np[1:30:3, 6:8]], axis=1)) and rec[:10, 7].any()
    assert np.array_equal(sc.vertex_np[:, 6:8], ctx.vertex_download(sc.vertex_count)[:, 6:8])
    sc.update_vertices(pos, nrm)          # (with the normals the scene had: without them the device makes face normals of its own, in float32)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(render(ex, 1), textured))
    ctx.close()
