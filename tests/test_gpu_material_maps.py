"""Roughness, metallic and normal-map textures on the device (include/tirt.h, "Roughness, metallic and normal-map textures on materials").  The oracle
knows nothing of textures, so every comparison is with the numpy restatement (tests/material_maps_expected.py) or with a TWIN scene: the same geometry,
untextured, each material's words 5 and 6 (and colour) the restated lookups at the uv its hits have, and -- for hits at a vertex, where the oracle's
interpolation returns that vertex's normal exactly -- the restated unnormalised mapped normal as that vertex's normal.  Every result is exact:
bit-identical to its expectation, or a stated error code.

What a twin cannot do: reproduce a mapped normal at a hit with general barycentrics.  There the device normalises (T * n.x + B * n.y) + N * n.z with N the
normalised interpolation, and a twin interpolates three vertex normals and normalises that: two different sequences of roundings, equal only at a vertex.
So films are held to the oracle where the normal maps are named and their triangles' uvs are all (0, 0) (det == 0: the normal stays, every lookup reads
texel (0, 0) with weight exactly 1), and films with mapped normals (det != 0) to the restatement at the pixel-centre hits and to themselves."""
import numpy as np
import pytest

import common
import material_maps_expected as me
import oracle_api
import shade_step_cases as cases
import texture_expected as te
from ti_raytrace_amd import _native, Example, PT_RGB, PT_Spec
from ti_raytrace_amd import SceneData as SCD
from ti_raytrace_amd import Texture as TX

pytestmark = pytest.mark.gpu
f = np.float32
SEED = 11
MAPS = _native.SHADE_INSTANTIATION_MAPS          # 511


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def packed(rgb):
    t = TX.Texture(); t.load_array(rgb)
    return t.np_img


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def same(a, b):
    """bit for bit, NaN where the other has NaN"""
    a, b = np.ascontiguousarray(a, f), np.ascontiguousarray(b, f)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def textures_of(sc):
    return [(t.np_img, w) for t, w in sc.textures]


# ---- the scene of tests 1 and 2 ---------------------------------------------------------------------------------------------------
N_GENERAL, N_VERTEX, N_DEGENERATE = 120, 80, 4          # triangles hit at a general point / at a vertex / with degenerate uvs (hit at a vertex too)
N_TRI = N_GENERAL + N_VERTEX + N_DEGENERATE
TEX_SIZES = [(1, 1), (2, 2), (5, 3), (64, 64), (3, 7), (16, 4), (2, 9), (8, 8)]


def step_scene():
    """204 triangles with random uvs in [-1.5, 2.5], each with its own Disney or glass material: the first 120 with roughness and metallic textures (every
    other one an albedo texture too), the others also with a normal map; the last four have degenerate uvs.  Then an untextured triangle, a sphere whose
    material names all three maps, a mesh light whose material names them too (ignored) and a sphere light.  8 textures, both wrap modes."""
    ex = Example.example(cases.FILM_W, cases.FILM_H, 4, 0)
    sc = ex.scene
    r = np.random.RandomState(8)
    tex_ids = [sc.add_texture(image(w, h, 150 + k), wrap="repeat" if k % 2 else "clamp") for k, (w, h) in enumerate(TEX_SIZES)]
    from ti_raytrace_amd import scenes
    tri = scenes.synthetic_triangles(N_TRI + 1, 31, 0.25)
    for k in range(N_TRI + 1):
        if k % 5 == 4:
            m = cases.glass((1.0, 1.3, 2.4)[k % 3], (0.01, 5.0, 300.0)[(k // 3) % 3], tuple(r.uniform(0.2, 1.0, 3)))
        else:
            m = cases.disney(cases.METALLIC[k % 3], cases.ROUGHNESS[k % 5], tuple(r.uniform(0.0, 1.0, 3)))
        if k < N_TRI:
            m.roughTex, m.metalTex = tex_ids[k % 8], tex_ids[(k + 3) % 8]
            if m.type == SCD.MAT_GLASS and k % 2:
                m.roughTex, m.metalTex = 99, 1.0e9                  # a glass row's words 7 and 8 are ignored, whatever they hold
            if k % 2:
                m.alebdoTex = tex_ids[(k + 1) % 8]
            if k >= N_GENERAL:
                m.normalTex = tex_ids[(k + 5) % 8]
        sc.add_mesh(tri[k:k + 1], m, cases.tilted_normals(tri[k:k + 1], r) if k % 7 == 3 else None)
    sphere = SCD.Shape(); sphere.type = SCD.SHPAE_SPHERE; sphere.pos = [0.3, -0.2, 0.1]; sphere.setRadius(0.2)
    m = cases.disney(0.3, 0.2, (0.6, 0.5, 0.4)); m.roughTex, m.metalTex, m.normalTex = tex_ids[2], tex_ids[5], tex_ids[3]
    sc.add_shape(sphere, m)
    sc.add_mesh(np.array([[[-0.5, 1.6, -0.5], [0.5, 1.6, -0.5], [0.0, 1.6, 0.6]]]), cases.emitter((30.0, 28.0, 20.0)))
    sc.material_cpu[-1].roughTex, sc.material_cpu[-1].metalTex, sc.material_cpu[-1].normalTex = 3, 77, 1000          # an emitter ignores its slots
    ex.add_sphere_light(pos=(0.0, 3.0, 0.0), radius=0.75, emission=50.0)
    ex.integrator = PT_RGB.PathTrace(cases.FILM_W, cases.FILM_H, ex.cam, sc, 64)
    common.host_only(ex)
    uv = r.uniform(-1.5, 2.5, (sc.vertex_count, 2)).astype(f)
    first = 3 * (N_GENERAL + N_VERTEX)
    uv[first + 3:first + 6] = uv[first:first + 3] = uv[first]                       # all three equal, twice
    for k in (2, 3):                                                               # collinear, exactly (quarters add without rounding), twice
        t0 = (np.rint(uv[first + 3 * k] * 4) / 4).astype(f)
        uv[first + 3 * k:first + 3 * k + 3] = [t0, t0 + np.array([0.5, 1.0], f), t0 + np.array([0.25, 0.5], f)]
    sc.vertex_np[:, 6:8] = uv
    return ex


@pytest.fixture(scope="module")
def step(gpu_ctx_ok, oracle_lib):
    """the scene on the device, shared by the known-answer and the shading-step test (neither changes it)"""
    ex = step_scene()
    ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
    yield ex
    ex.scene.ctx.close()


# ---- 1. known answers --------------------------------------------------------------------------------------------------------------
def test_material_maps_equal_the_restatement(step):
    sc = step.scene
    ctx = sc.ctx
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPHERE | _native.SF_TEXTURE | _native.SF_TEXTURE_PARAM
    r = np.random.RandomState(3)
    nprim = N_TRI + 2                                                       # the triangles, the untextured one and the sphere
    assert sc.primitive_np[N_TRI + 1, 0] == SCD.PRIMITIVE_SHAPE
    reps = 6
    prim = np.concatenate([np.repeat(np.arange(nprim), reps), np.repeat(np.arange(nprim), 3)])
    bu = r.uniform(0.0, 1.0, nprim * reps); bv = r.uniform(0.0, 1.0, nprim * reps) * (1.0 - bu)
    bu = np.concatenate([bu, np.tile([0.0, 1.0, 0.0], nprim)]).astype(f)      # ... and the three vertices
    bv = np.concatenate([bv, np.tile([0.0, 0.0, 1.0], nprim)]).astype(f)
    rows = np.zeros((prim.size, 3), np.uint32)
    rows[:, 0] = prim
    rows.view(f)[:, 1], rows.view(f)[:, 2] = bu, bv
    got = ctx.kat_material_maps(rows)
    textures = textures_of(sc)
    want = me.maps_at(sc.material_np, textures, sc.vertex_np, sc.primitive_np, prim, bu, bv)
    bad = np.where(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
    assert bad.size == 0, "%d rows differ, first: prim %d (u, v) = (%s, %s) got %s want %s" % (
        bad.size, prim[bad[0]], bu[bad[0]], bv[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
    # the rows cover what they should: mapped normals that differ from the interpolated ones, degenerate uvs and the sphere that keep theirs
    N = me.hit_normal(sc.vertex_np, sc.primitive_np, prim, bu, bv)
    mapped = (bits(want[:, 4:7]) != bits(N)).any(axis=1)
    vertex_group = (prim >= N_GENERAL) & (prim < N_GENERAL + N_VERTEX)
    assert mapped[vertex_group].all() and not mapped[~vertex_group].any()
    assert np.isfinite(want[prim <= N_TRI]).all() and np.abs(np.linalg.norm(want[vertex_group, 4:7].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    glassy = sc.material_np[sc.primitive_np[prim, 2], 0] == SCD.MAT_GLASS
    assert np.array_equal(want[glassy, 2:4], sc.material_np[sc.primitive_np[prim[glassy], 2]][:, [6, 5]])      # a glass row keeps extinction and ior
    plain = ~glassy & (prim < N_TRI)
    assert (want[plain, 2:4] != sc.material_np[sc.primitive_np[prim[plain], 2]][:, [6, 5]]).any(axis=1).mean() > 0.9
    assert not want[prim == N_TRI + 1, 0:2].any() and not want[prim == N_TRI + 1, 4:7].any()                  # the sphere: uv 0, no normal here
    with pytest.raises(_native.TirtError, match="prim outside"):
        ctx.kat_material_maps(np.array([[sc.primitive_count, 0, 0]], np.uint32))


# ---- 2. one shading step against the oracle, on the twin ---------------------------------------------------------------------------
def test_shading_step_equals_the_oracle_on_the_twin(step):
    ex = step
    sc = ex.scene
    ctx = sc.ctx
    textures = textures_of(sc)
    r = np.random.RandomState(12)
    # one point per triangle: general barycentrics on the first 120, one of the three vertices on the others; 40 path states and directions each
    bu = r.uniform(0.0, 1.0, N_TRI + 1); bv = r.uniform(0.0, 1.0, N_TRI + 1) * (1.0 - bu)
    corner = r.randint(0, 3, N_TRI + 1)
    at_vertex = (np.arange(N_TRI + 1) >= N_GENERAL) & (np.arange(N_TRI + 1) < N_TRI)
    bu = np.where(at_vertex, (corner == 1).astype(f), bu).astype(f)
    bv = np.where(at_vertex, (corner == 2).astype(f), bv).astype(f)
    reps = 40
    prim = np.repeat(np.arange(N_TRI + 1), reps)
    vi = sc.primitive_np[prim, 1]
    pos = sc.vertex_np[vi, 0:3].astype(np.float64) * (1.0 - bu[prim] - bv[prim])[:, None] + sc.vertex_np[vi + 1, 0:3] * bu[prim][:, None] + sc.vertex_np[vi + 2, 0:3] * bv[prim][:, None]
    d = cases.unit(r.normal(size=(prim.size, 3))).astype(f)
    o, t = (pos - d.astype(np.float64)).astype(f), np.ones(prim.size, f)
    # ... and 80 rays at the sphere, from twice its radius towards its centre
    ns, centre, radius = 80, np.array([0.3, -0.2, 0.1]), 0.2
    sd = cases.unit(r.normal(size=(ns, 3)))
    prim = np.concatenate([prim, np.full(ns, N_TRI + 1)])
    o = np.concatenate([o, (centre + 2.0 * radius * sd).astype(f)]); d = np.concatenate([d, (-sd).astype(f)]); t = np.concatenate([t, np.full(ns, radius, f)])
    n = prim.size
    head, tail, spec = cases.path_state(n, r)
    rows = cases.pack(head, o, d, t, np.concatenate([bu[prim[:-ns]], np.zeros(ns, f)]), np.concatenate([bv[prim[:-ns]], np.zeros(ns, f)]), prim, tail, spec)
    # the twin: every material gets the restated lookups at its triangle's point, every triangle hit at a vertex the restated Nraw as that vertex's normal
    tris = np.arange(N_TRI + 1)
    tu, tv = te.hit_uv(sc.vertex_np, sc.primitive_np, tris, bu, bv)
    mat_of = sc.primitive_np[:N_TRI + 1, 2]
    assert np.unique(mat_of).size == N_TRI + 1
    twin = te.twin_materials(sc.material_np, textures, {int(m): (tu[k], tv[k]) for k, m in enumerate(mat_of)})
    rough, metal = me.rough_metal_at(sc.material_np, textures, mat_of, tu, tv)
    twin[mat_of, 6], twin[mat_of, 5] = rough, metal
    sphere_mat = sc.primitive_np[N_TRI + 1, 2]
    sr, sm = me.rough_metal_at(sc.material_np, textures, np.array([sphere_mat]), np.zeros(1, f), np.zeros(1, f))          # a shape's uv is 0
    twin[sphere_mat, 6], twin[sphere_mat, 5] = sr[0], sm[0]
    twin[:, 7:10] = 0.0
    changed = (twin[mat_of, 5:7] != sc.material_np[mat_of, 5:7]).any(axis=1)
    is_glass = sc.material_np[mat_of, 0] == SCD.MAT_GLASS
    assert not changed[is_glass].any() and changed[:N_TRI][~is_glass[:N_TRI]].mean() > 0.9
    N = me.hit_normal(sc.vertex_np, sc.primitive_np, tris, bu, bv)
    raw, mapped = me.normal_at(sc.material_np, textures, sc.vertex_np, sc.primitive_np, tris, tu, tv, N, raw=True)
    assert mapped[N_GENERAL:N_GENERAL + N_VERTEX].all() and not mapped[:N_GENERAL].any() and not mapped[N_GENERAL + N_VERTEX:].any()
    assert int((is_glass & mapped).sum()) >= 10                                   # glass rows that carry a normal map
    twin_vertex = sc.vertex_np.copy()
    for k in np.where(mapped)[0]:
        twin_vertex[sc.primitive_np[k, 1] + corner[k], 3:6] = raw[k]
    base_m, base_v = sc.material_np, sc.vertex_np
    try:
        sc.material_np, sc.vertex_np = twin, twin_vertex
        orc = oracle_api.OracleScene(sc, ex.cam)
        assert orc.lbvh_build() == sc.primitive_count - 1
        want = orc.kat_shade_step(rows)
    finally:
        sc.material_np, sc.vertex_np = base_m, base_v
    got = ctx.kat_shade_step(MAPS, rows)
    report = cases.first_differences(got, want, rows, ex)
    assert not report, "\n".join(report)
    assert int((want.view(np.int32)[:, 3] == 1).sum()) > 5000 and int((want.view(np.int32)[:, 16] == 1).sum()) > 500      # (the rows shade and sample lights)
    # the mapped normals matter: without them (the twin's materials on the scene's own vertex normals) the oracle answers otherwise
    try:
        sc.material_np = twin
        flat = oracle_api.OracleScene(sc, ex.cam)
        assert flat.lbvh_build() == sc.primitive_count - 1
        assert cases.first_differences(got, flat.kat_shade_step(rows), rows, ex)
    finally:
        sc.material_np = base_m
    for feat in (256, 255, _native.SF_ALL):                  # 256 alone is no instantiation; 255 and 127 do not cover this scene
        with pytest.raises(_native.TirtError, match="instantiation|cover"):
            ctx.kat_shade_step(feat, rows[:4])
    # the records carry the uvs under bit 256 as under bit 128
    rec = ctx.shade_table_download(0, sc.primitive_count)
    vi = sc.primitive_np[:N_TRI, 1]
    assert np.array_equal(rec[:N_TRI, 7], np.concatenate([sc.vertex_np[vi, 6:8], sc.vertex_np[vi + 1, 6:8]], axis=1))
    assert np.array_equal(rec[:N_TRI, 2, 3], sc.vertex_np[vi + 2, 6]) and np.array_equal(rec[:N_TRI, 3, 3], sc.vertex_np[vi + 2, 7])


# ---- 3. films -------------------------------------------------------------------------------------------------------------------------
def quad(a, b, c, d):
    return np.array([[a, b, c], [a, c, d]], np.float64)


QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float64)
BOX_TEXTURES = [(1, 1), (2, 2), (5, 3), (8, 8), (7, 4), (3, 3)]
FLAT_NORMAL = np.full((1, 1, 3), 128, np.uint8); FLAT_NORMAL[..., 2] = 255          # the "flat" texel of a normal map: 2 * 128 / 255 - 1 is not 0


def box_scene(W, H, uv_scale, maps="all", twin_of=None, flat_normal_maps=False):
    """a Cornell-like box: five Disney walls, each with its own roughness, metallic, normal-map and (three of them) albedo texture, a glass tetrahedron with a
    normal map, a quad light.  uv_scale 0: every uv (0, 0).  maps "albedo": only the albedo textures; "none": untextured.  twin_of: the untextured twin of
    that scene for uvs of 0 -- colour, metallic and roughness the restated lookups at uv (0, 0).  flat_normal_maps: every normal map the 1 x 1 image (128, 128, 255)"""
    ex = Example.example(W, H, 8, 0)
    sc = ex.scene
    p = lambda x, y, z: (float(x), float(y), float(z))
    walls = [quad(p(0, 0, 0), p(1, 0, 0), p(1, 0, -1), p(0, 0, -1)), quad(p(0, 1, 0), p(0, 1, -1), p(1, 1, -1), p(1, 1, 0)),
             quad(p(0, 0, -1), p(1, 0, -1), p(1, 1, -1), p(0, 1, -1)), quad(p(0, 0, 0), p(0, 0, -1), p(0, 1, -1), p(0, 1, 0)),
             quad(p(1, 0, 0), p(1, 1, 0), p(1, 1, -1), p(1, 0, -1))]
    tid = []
    if maps != "none" and twin_of is None:
        tid = [sc.add_texture(image(w, h, 170 + k), wrap="clamp" if k == 2 else "repeat") for k, (w, h) in enumerate(BOX_TEXTURES)]
        if flat_normal_maps:
            tid.append(sc.add_texture(FLAT_NORMAL))
    for k, wq in enumerate(walls):
        m = cases.disney((0.0, 0.3, 1.0, 0.0, 0.0)[k], (0.5, 0.2, 0.001, 1.0, 0.5)[k], (0.8, 0.7, 0.6))
        if tid:
            if k < 3:
                m.alebdoTex = tid[k]
            if maps == "all":
                m.roughTex, m.metalTex, m.normalTex = tid[(k + 1) % 6], tid[(k + 2) % 6], (tid[6] if flat_normal_maps else tid[(k + 3) % 6])
        sc.add_mesh(wq, m)
    a, b, c, d = np.array([0.3, 0.05, -0.3]), np.array([0.7, 0.05, -0.35]), np.array([0.5, 0.05, -0.7]), np.array([0.5, 0.55, -0.45])
    g = cases.glass(1.5, 5.0)
    if tid and maps == "all":
        g.roughTex, g.metalTex, g.normalTex = 50, 60, (tid[6] if flat_normal_maps else tid[4])          # glass: words 7, 8 ignored, the normal map honoured
    sc.add_mesh(np.array([[a, c, b], [a, b, d], [b, c, d], [c, a, d]]), g)
    sc.add_mesh(quad(p(0.35, 0.99, -0.35), p(0.65, 0.99, -0.35), p(0.65, 0.99, -0.65), p(0.35, 0.99, -0.65)), cases.emitter((17.0, 12.0, 4.0)))
    ex.integrator = PT_RGB.PathTrace(W, H, ex.cam, sc, 64, seed=SEED, aov=True, moments=True)
    common.host_only(ex)
    uvs = np.zeros((sc.vertex_count, 2), f)
    for k in range(5):
        uvs[6 * k:6 * k + 6] = (QUAD_UV * uv_scale * (1.0 + 0.37 * k) - 0.21 * k * (uv_scale != 0)).astype(f)
    if uv_scale != 0:
        uvs[30:42] = np.random.RandomState(5).uniform(0.0, 1.0, (12, 2)).astype(f)                    # the tetrahedron
    sc.vertex_np[:, 6:8] = uvs
    if twin_of is not None:
        src, textures = twin_of.scene.material_np, textures_of(twin_of.scene)
        twin = te.twin_materials(src, textures, {k: (0.0, 0.0) for k in range(src.shape[0])})
        mats = np.arange(src.shape[0])
        rough, metal = me.rough_metal_at(src, textures, mats, np.zeros(mats.size, f), np.zeros(mats.size, f))
        twin[:, 6], twin[:, 5] = rough, metal
        twin[:, 7:10] = 0.0
        sc.material_np = twin
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
    """every uv (0, 0): each lookup reads texel (0, 0) with weight 1, each normal map is named and meets det == 0 -- film, feature buffers and moment records
    of the new instantiation equal the untextured twin's, and the film the oracle's on the twin"""
    ex = box_scene(W, H, 0.0)
    twin = box_scene(W, H, 0.0, twin_of=ex)
    assert (twin.scene.material_np[:5, 5:7] != ex.scene.material_np[:5, 5:7]).any(axis=1).all()          # every wall's metallic or roughness is a texel's
    assert np.array_equal(twin.scene.material_np[5:, 5:7], ex.scene.material_np[5:, 5:7])               # glass and the emitter keep their words
    assert np.array_equal(twin.scene.vertex_np, ex.scene.vertex_np)
    ctx = on_device(ex)
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI | _native.SF_TEXTURE | _native.SF_TEXTURE_PARAM
    one, two = render(ex, 1), render(ex, 2)
    ctx.pixel_set_upload(np.arange(W * H, dtype=np.int32))                      # every pixel, through the LIST instantiation
    listed = render(ex, 4)
    ctx.pixel_set_clear()
    ctx2 = on_device(twin)
    assert ctx2.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI
    want = render(twin, 2)
    for got in (one, two, listed):
        for name, a, b in zip(("film", "aov", "moments"), got, want):
            assert np.array_equal(bits(a), bits(b)), name
    assert float(one[0].sum()) > 0.0
    orc = oracle_api.OracleScene(twin.scene, twin.cam)
    assert orc.lbvh_build() == twin.scene.primitive_count - 1
    ref, _ = orc.render(W, H, 0, 8, seed=SEED)
    assert common.same_bits(one[0], ref)
    # the maps matter: the same scene without them gives another film
    m = ex.scene.material_np.copy(); m[:, 7:10] = 0.0
    ctx.material_upload(m)
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI | _native.SF_TEXTURE
    assert not np.array_equal(bits(render(ex, 1)[0]), bits(one[0]))
    ctx.close(); ctx2.close()


def frame0_expectation(ex):
    """(hit mask, N' [W*H, 3], N [W*H, 3]) at the pixel-centre hits of frame 0, from the oracle's hits and the restatement; misses: 0"""
    sc = ex.scene
    W, H = ex.imgSizeX, ex.imgSizeY
    textures = textures_of(sc)
    orc = oracle_api.OracleScene(sc, ex.cam)
    assert orc.lbvh_build() == sc.primitive_count - 1
    out, prim, _, bary = orc.closest_hit(oracle_api.camera_rays(ex.cam, W, H), uv=True)
    hit = out[:, 0] < cases.INF_VALUE
    hp = prim[hit]
    assert (sc.primitive_np[hp, 0] == SCD.PRIMITIVE_TRI).all()
    tu, tv = te.hit_uv(sc.vertex_np, sc.primitive_np, hp, bary[hit, 0], bary[hit, 1])
    N = me.hit_normal(sc.vertex_np, sc.primitive_np, hp, bary[hit, 0], bary[hit, 1])
    assert np.array_equal(bits(N), bits(out[hit, 7:10]))                          # the oracle's shading normal is the restated interpolation
    want, plain = np.zeros((W * H, 3), f), np.zeros((W * H, 3), f)
    want[hit] = me.normal_at(sc.material_np, textures, sc.vertex_np, sc.primitive_np, hp, tu, tv, N)
    plain[hit] = N
    return hit, want, plain


@pytest.mark.parametrize("flat", [False, True])
def test_general_maps_are_self_consistent_and_the_normal_is_the_mapped_one(gpu_ctx_ok, oracle_lib, flat):
    """det != 0 on every triangle.  flat: every normal map the constant (128, 128, 255) -- still not the interpolated normal"""
    W, H = 24, 20
    ex = box_scene(W, H, 1.7, flat_normal_maps=flat)
    sc = ex.scene
    p, t = me.tri_rows(sc.vertex_np, sc.primitive_np, np.arange(14))
    d1, d2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    assert (d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1] != 0).all()
    ctx = on_device(ex)
    assert ctx.shade_features()[0] & _native.SF_TEXTURE_PARAM
    one = render(ex, 1)
    two = render(ex, 2)
    ctx.set_option("overlap_lanes", 1)
    single = render(ex, 4)
    ctx.set_option("overlap_lanes", 4)
    ctx.pixel_set_upload(np.arange(W * H, dtype=np.int32))
    listed = render(ex, 2)
    ctx.pixel_set_clear()
    for other in (two, single, listed):
        for name, a, b in zip(("film", "aov", "moments"), one, other):
            assert np.array_equal(bits(a), bits(b)), name
    # the maps matter
    m = sc.material_np.copy(); m[:, 7:10] = 0.0
    ctx.material_upload(m)
    assert not np.array_equal(bits(render(ex, 1)[0]), bits(one[0]))
    ctx.material_upload(sc.material_np)
    # normal of frame 0 (rays through the pixel centres) = the restated N' at the oracle's hits, in the feature buffer and in the Debug views
    hit, want, plain = frame0_expectation(ex)
    moved = (bits(want) != bits(plain)).any(axis=1)
    assert int(hit.sum()) > W * H // 2 and int(moved.sum()) > int(hit.sum()) * 0.9
    ctx.film_clear()
    ctx.pt_rgb_render(0, 1, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    aov = ctx.aov_download(W, H).reshape(-1, _native.AOV_WORDS)
    first = (want * f(1.0) + np.zeros_like(want) * f(0.0)).astype(f)              # the running mean's first step, value * 1 + 0 * 0: a component of -0 becomes +0
    assert np.array_equal(bits(aov[:, 3:6]), bits(first))
    ctx.debug_render(0, SEED, _native.DEBUG_NORMAL)
    dbg = ctx.film_download(W, H)[0].reshape(-1, 3)
    view = np.where(hit[:, None], (want + f(1.0)) * f(0.5), f(0.0)).astype(f)
    assert np.array_equal(bits(dbg), bits(view))
    ctx.debug_render(0, SEED, _native.DEBUG_GNORMAL)                               # the geometric normal is untouched: the view of the scene without textures
    gn = ctx.film_download(W, H)[0].copy()
    ctx.texture_upload([])
    ctx.debug_render(0, SEED, _native.DEBUG_GNORMAL)
    assert np.array_equal(bits(gn), bits(ctx.film_download(W, H)[0]))
    ctx.debug_render(0, SEED, _native.DEBUG_NORMAL)
    assert np.array_equal(bits(ctx.film_download(W, H)[0].reshape(-1, 3)), bits(np.where(hit[:, None], (plain + f(1.0)) * f(0.5), f(0.0)).astype(f)))
    ctx.close()


# ---- 4. nothing else moved ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maps,word", [("albedo", 128), ("none", 0)])
def test_other_scenes_keep_their_feature_word_and_film(gpu_ctx_ok, oracle_lib, maps, word):
    """an albedo-only textured scene and an untextured one: the feature word they had, and the film the oracle gives (on the twin, for the textured one)"""
    W, H = 24, 20
    ex = box_scene(W, H, 0.0, maps=maps)
    assert not ex.scene.material_np[:, 7:10].any()
    ctx = on_device(ex)
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI | word
    got = render(ex, 2)
    twin = box_scene(W, H, 0.0, twin_of=ex) if maps == "albedo" else ex
    assert np.array_equal(twin.scene.material_np[:, 5:7], ex.scene.material_np[:, 5:7])
    orc = oracle_api.OracleScene(twin.scene, twin.cam)
    assert orc.lbvh_build() == twin.scene.primitive_count - 1
    ref, _ = orc.render(W, H, 0, 8, seed=SEED)
    assert common.same_bits(got[0], ref)
    with pytest.raises(_native.TirtError, match="cover|textures"):              # and the new instantiation is not theirs to ask for without textures
        if maps == "none":
            ctx.kat_shade_step(MAPS, np.zeros((1, 23), np.uint32))
        else:
            ctx.kat_shade_step(_native.SF_ALL, np.zeros((1, 23), np.uint32))
    ctx.close()


# ---- 5. refusals and lifecycle --------------------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle(gpu_ctx_ok, oracle_lib):
    W, H = 13, 7
    ex = box_scene(W, H, 1.7)
    sc = ex.scene
    textures = textures_of(sc)
    T = len(textures)
    spec = PT_Spec.PathTrace(W, H, ex.cam, sc, 64, seed=SEED)
    spec.setup_data_cpu(); spec.setup_data_gpu()                                # (the spectral tables; the film is created again below)
    ctx = on_device(ex)
    mapped = render(ex, 1)
    only_maps = sc.material_np.copy(); only_maps[:, 1] = -1.0                   # no albedo texture: bit 256 alone still refuses
    for table, message in ((sc.material_np, "albedo texture.*count 0"), (only_maps, "roughness, metallic or normal-map texture.*count 0")):
        ctx.material_upload(table)
        assert bool(ctx.shade_features()[0] & 128) == (table is sc.material_np) and ctx.shade_features()[0] & 256
        for call in (lambda: ctx.bdpt_rgb_render(0, 1, SEED), lambda: ctx.pt_spec_render(0, 1, SEED), lambda: ctx.bdpt_spec_render(0, 1, SEED)):
            with pytest.raises(_native.TirtError, match=message):
                call()
    ctx.material_upload(sc.material_np)
    # a slot beyond T fails in each word, in each of the three upload entries; an emitter's and a glass row's ignored slots are ignored
    assert me.refused_slots(sc.material_np, T) == []
    for word in (1, 7, 8, 9):
        bad = sc.material_np.copy(); bad[3, word] = T + 1
        assert me.refused_slots(bad, T) == [(3, word)]
        with pytest.raises(_native.TirtError, match="material 3 names texture %d of %d" % (T + 1, T)):
            ctx.material_upload(bad)
        with pytest.raises(_native.TirtError, match="material 3 names texture %d of %d" % (T + 1, T)):
            ctx.scene_upload(sc.vertex_np, sc.primitive_np, bad, sc.shape_np, sc.light_np, sc.light_count, sc.minboundarynp, sc.maxboundarynp)
        need = sc.material_np.copy(); need[3, word] = T                          # names the last texture: uploading one fewer is refused
        ctx.material_upload(need)
        assert (3, word) in me.refused_slots(need, T - 1)                         # (among other rows that name the last texture)
        with pytest.raises(_native.TirtError, match="names texture %d of %d" % (T, T - 1)):
            ctx.texture_upload(textures[:T - 1])
        ctx.material_upload(sc.material_np)
    again = render(ex, 1)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(mapped, again))          # the refused calls changed nothing
    ignored = sc.material_np.copy()
    assert ignored[5, 0] == SCD.MAT_GLASS and ignored[6, 0] == SCD.MAT_LIGHT and ignored[5, 7] == 50 and ignored[5, 8] == 60
    ignored[6, 1], ignored[6, 7:10] = 40, (41, 42, 43)
    assert me.refused_slots(ignored, T) == []
    ctx.material_upload(ignored)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(render(ex, 1), mapped))
    ignored[5, 9] = T + 1                                                        # ... but a glass row's normal map is honoured
    with pytest.raises(_native.TirtError, match="material 5 names texture %d of %d uploaded in word 9" % (T + 1, T)):
        ctx.material_upload(ignored)
    ctx.material_upload(sc.material_np)
    # cleared: bit 256 goes, the records carry no uvs, the film is the untextured scene's, and the other integrators work again
    ctx.texture_upload([])
    assert ctx.shade_features()[0] == _native.SF_GLASS | _native.SF_LIGHT_TRI
    flat = render(ex, 1)
    assert not ctx.shade_table_download(0, sc.primitive_count)[:, 7].any()
    plain = box_scene(W, H, 1.7, maps="none")
    ctx2 = on_device(plain)
    want = render(plain, 1)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(flat, want))
    ctx2.close()
    ctx.film_clear(); ctx.bdpt_rgb_render(0, 1, SEED); ctx.sync()
    ctx.film_clear(); ctx.pt_spec_render(0, 1, SEED); ctx.sync()
    assert np.isfinite(ctx.film_download(W, H)[0]).all()
    ctx.texture_upload(textures)
    assert ctx.shade_features()[0] & 256
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(render(ex, 1), mapped))
    # moving the vertices keeps the uvs: the film after it equals a fresh scene's
    pos, nrm = sc.vertex_np[:, 0:3].copy(), sc.vertex_np[:, 3:6].copy()
    moved_pos = pos.copy(); moved_pos[30:42] += f(0.05)                           # the tetrahedron
    sc.update_vertices(np.ascontiguousarray(moved_pos), nrm)
    rec = ctx.shade_table_download(0, sc.primitive_count)
    assert np.array_equal(rec[:10, 7], np.concatenate([sc.vertex_np[0:30:3, 6:8], sc.vertex_np[1:30:3, 6:8]], axis=1)) and rec[:10, 7].any()
    assert np.array_equal(sc.vertex_np[:, 6:8], ctx.vertex_download(sc.vertex_count)[:, 6:8])
    after = render(ex, 1)
    fresh = box_scene(W, H, 1.7)
    fresh.scene.vertex_np[:, 0:3] = moved_pos                                    # (the tetrahedron stays inside the walls: the scene box and the camera are the same)
    ctx3 = on_device(fresh)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after, render(fresh, 1)))
    assert not np.array_equal(bits(after[0]), bits(mapped[0]))
    ctx3.close()
    ctx.close()
