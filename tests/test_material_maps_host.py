"""Roughness, metallic and normal-map textures on the host: the material row's slots, map_Pr / map_Pm / norm in both OBJ parsers, the slot rules restated on
host tables, and the numpy restatement of the device functions (tests/material_maps_expected.py) checked against what it must satisfy by construction."""
import os

import numpy as np
import pytest

import material_maps_expected as me
import texture_expected as te
from ti_raytrace_amd import _native, ObjLoader, Scene
from ti_raytrace_amd import SceneData as SCD
from ti_raytrace_amd import Texture as TX

f = np.float32
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "material_maps_obj")


def packed(rgb):
    t = TX.Texture(); t.load_array(rgb)
    return t.np_img


# ---- the row ------------------------------------------------------------------------------------------------------------------
def test_slots_land_in_row_words_7_to_9():
    m = SCD.Material()
    assert (m.roughTex, m.metalTex, m.normalTex) == (0, 0, 0)
    m.type = SCD.MAT_DISNEY; m.setMetal(0.25); m.setRough(0.75); m.setColor([0.1, 0.2, 0.3]); m.alebdoTex = 4
    m.roughTex, m.metalTex, m.normalTex = 1, 2, 3
    rows = np.full((2, SCD.MAT_VEC_SIZE), 9.0, f)
    m.fillStruct(rows, 1)
    assert rows[1].tolist() == [0.0, 4.0] + [float(f(x)) for x in (0.1, 0.2, 0.3)] + [0.25, 0.75, 1.0, 2.0, 3.0]
    assert (rows[0] == 9.0).all()
    SCD.Material().fillStruct(rows, 0)
    assert not rows[0].any()                                              # the defaults: every slot 0


def test_host_feature_word_never_has_the_texture_bits():
    mats = np.zeros((2, SCD.MAT_VEC_SIZE), f)
    mats[0] = [SCD.MAT_DISNEY, 1, 0.5, 0.5, 0.5, 0, 0.5, 1, 1, 1]
    mats[1] = [SCD.MAT_LIGHT, 0, 5, 5, 5, 0, 0, 0, 0, 0]
    prim = np.array([[SCD.PRIMITIVE_TRI, 0, 0], [SCD.PRIMITIVE_TRI, 3, 1]], np.int32)
    word = _native.shade_features_host(mats, prim, np.zeros((1, SCD.SHA_VEC_SIZE), f), np.array([1], np.int32), 1)
    assert word & (128 | 256) == 0 and word & _native.SF_LIGHT_TRI


# ---- MTL ----------------------------------------------------------------------------------------------------------------------
def test_the_three_statements_through_both_parsers():
    path = os.path.join(FIX, "quad.obj")
    a = ObjLoader.Wavefront(path).materials
    b = ObjLoader.Wavefront(path, native=False).materials
    assert list(a) == list(b) == ["mapped", "orm", "glassy", "plain", "lamp"]
    for name in a:
        assert a[name].maps == b[name].maps, name
        assert a[name].texture is None and b[name].texture is None           # map_Ke and refl are keywords the loader does not know: still skipped
        assert np.array_equal(a[name].vertices, b[name].vertices)
    p = lambda n: os.path.join(FIX, n)
    assert a["mapped"].maps == [p("rough.png"), p("orm map.png"), p("normal.png")]      # options skipped, the blank in the name kept
    assert a["orm"].maps == [p("orm map.png"), p("orm map.png"), p("normal.png")]       # map_Bump -bm 0.8: the option and its number are skipped
    assert a["glassy"].maps == [p("rough.png"), None, p("normal.png")]                  # bump
    assert a["plain"].maps == [None, None, None]
    assert a["lamp"].maps == [p("rough.png"), None, p("normal.png")]


def test_a_statement_without_a_file_is_an_error(tmp_path):
    obj = tmp_path / "m.obj"
    obj.write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl a\nf 1/1 2/1 3/1\n")
    for key in ("map_Pr", "map_Pm", "norm", "map_Bump", "bump"):
        for native in (True, False):
            (tmp_path / "m.mtl").write_text("newmtl a\n%s\n" % key)
            with pytest.raises(Exception, match=key):
                ObjLoader.Wavefront(str(obj), native=native)
            (tmp_path / "m.mtl").write_text("newmtl a\nmap_unknown\n%s -bm 2 x.png\n" % key)      # an unknown keyword, even an empty one, is skipped
            maps = ObjLoader.Wavefront(str(obj), native=native).materials["a"].maps
            assert [m for m in maps if m] == [os.path.join(str(tmp_path), "x.png")]


def test_add_obj_fills_the_slots_and_uploads_each_file_once():
    sc = Scene.Scene(device_id=0)
    sc.add_obj(os.path.join(FIX, "quad.obj"))
    slots = [(m.alebdoTex, m.roughTex, m.metalTex, m.normalTex) for m in sc.material_cpu]
    # rough.png = 1, "orm map.png" = 2, normal.png = 3; the glass material takes no roughness map, the emitter nothing
    assert slots == [(-1, 1, 2, 3), (-1, 2, 2, 3), (-1, 0, 0, 3), (-1, 0, 0, 0), (-1, 0, 0, 0)]
    assert [int(m.type) for m in sc.material_cpu] == [0, 0, 1, 0, 2]
    assert len(sc.textures) == 3
    assert [(t.wid, t.hgt, w) for t, w in sc.textures] == [(8, 4, 1), (5, 3, 1), (6, 6, 1)]
    sc.setup_data_cpu()
    assert sc.material_np[:, 7:10].tolist() == [[1, 2, 3], [2, 2, 3], [0, 0, 3], [0, 0, 0], [0, 0, 0]]
    assert sc.vertex_np[1, 6:8].tolist() == [2.5, 0.0]
    assert me.refused_slots(sc.material_np, 3) == [] and me.feature_bits(sc.material_np, 3) == 256


# ---- the slot rules on host tables -----------------------------------------------------------------------------------------------
def test_slot_rules_on_host_tables():
    mats = np.zeros((5, SCD.MAT_VEC_SIZE), f)
    mats[0] = [SCD.MAT_DISNEY, 0, 0.1, 0.2, 0.3, 0.0, 0.5, 1, 2, 3]
    mats[1] = [SCD.MAT_LIGHT, 9, 9, 9, 9, 0, 0, 9, 9, 9]                # an emitter ignores its slots, however large
    mats[2] = [SCD.MAT_GLASS, -1, 0.9, 0.9, 0.9, 1.5, 5, 9, 9, 2]       # glass ignores 7 and 8 and honours 9
    mats[3] = [SCD.MAT_DISNEY, -1, 0.5, 0.5, 0.5, 0.3, 0.2, -3.0e9, np.nan, -np.inf]
    mats[4] = [SCD.MAT_DISNEY, -1, 0.5, 0.5, 0.5, 0.3, 0.2, 0, 0, 0]
    T = 3
    assert [[me.material_map(m, w, T) for w in (7, 8, 9)] for m in mats] == [[0, 1, 2], [-1, -1, -1], [-1, -1, 1], [-1, -1, -1], [-1, -1, -1]]
    assert all(me.material_map(m, w, 0) == -1 for m in mats for w in (7, 8, 9))
    assert me.refused_slots(mats, T) == [] and me.refused_slots(mats, 0) == []
    assert me.refused_slots(mats, 2) == [(0, 9)]                           # row 0's normal map names texture 3 of 2
    assert me.refused_slots(mats, 1) == [(0, 8), (0, 9), (2, 9)]
    for word in (1, 7, 8, 9):
        bad = mats.copy(); bad[4, word] = T + 1
        assert me.refused_slots(bad, T) == [(4, word)]
        bad[4, word] = 3.0e9                                               # saturates
        assert me.refused_slots(bad, T) == [(4, word)]
    assert me.feature_bits(mats, T) == 256 and me.feature_bits(mats[1:2], T) == 0 and me.feature_bits(mats[2:3], T) == 256
    assert me.feature_bits(mats[3:], T) == 0 and me.feature_bits(mats, 0) == 0
    alb = mats[4:5].copy(); alb[0, 1] = 2
    assert me.feature_bits(alb, T) == 128


# ---- the restatement, against what holds by construction ----------------------------------------------------------------------------
def frames(n, seed):
    r = np.random.RandomState(seed)
    p = r.uniform(-2.0, 2.0, (n, 3, 3)).astype(f)
    t = r.uniform(-1.5, 2.5, (n, 3, 2)).astype(f)
    N = me.normalized(r.normal(size=(n, 3)).astype(f))
    return r, p, t, N


def test_a_texel_of_exactly_0_0_1_gives_the_normal_back():
    _, p, t, N = frames(500, 1)
    n = np.tile(np.array([0, 0, 1], f), (500, 1))
    raw, ok = me.normal_raw_of(n, N, p, t)
    assert ok.all()
    assert np.array_equal(raw, N)                                          # (T * 0 + B * 0) + N * 1
    assert np.array_equal(me.normalized(raw).view(np.uint32), me.normalized(N).view(np.uint32))


def test_degenerate_uvs_leave_the_normal_alone():
    r, p, t, N = frames(300, 2)
    n = r.uniform(-1, 1, (300, 3)).astype(f)
    same = t.copy(); same[:, 1] = same[:, 0]; same[:, 2] = same[:, 0]                      # all three equal
    line = (np.rint(t * 4) / 4).astype(f); line[:, 1] = line[:, 0] + np.array([0.5, 1.0], f); line[:, 2] = line[:, 0] + np.array([0.25, 0.5], f)      # collinear, exactly: quarters add without rounding
    nan = t.copy(); nan[:, 2, 0] = np.nan
    inf = t.copy(); inf[:, 1, 1] = np.inf
    for uv in (same, line, nan, inf):
        raw, ok = me.normal_raw_of(n, N, p, uv)
        assert not ok.any() and np.array_equal(raw, N)
    # a tangent parallel to the normal: T - N * dot(N, T) vanishes, normalized() makes NaN of it, the normal stays
    t2 = np.tile(np.array([[0, 0], [1, 0], [0, 1]], f), (4, 1, 1))
    p2 = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f), (4, 1, 1))
    N2 = np.tile(np.array([1, 0, 0], f), (4, 1))
    raw, ok = me.normal_raw_of(n[:4], N2, p2, t2)
    assert not ok.any() and np.array_equal(raw, N2)


def test_the_frame_is_orthonormal_and_follows_the_uv_axes():
    r, p, t, N = frames(400, 3)
    # an axis-aligned quad's triangle: u along +x, v along +y, normal +z -> T = x, B = cross(N, T) = y, and Nraw = n
    p2 = np.tile(np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], f), (400, 1, 1))
    t2 = np.tile(np.array([[0, 0], [1, 0], [0, 1]], f), (400, 1, 1))
    N2 = np.tile(np.array([0, 0, 1], f), (400, 1))
    n = r.uniform(-1, 1, (400, 3)).astype(f)
    raw, ok = me.normal_raw_of(n, N2, p2, t2)
    assert ok.all() and np.array_equal(raw, n)
    # in general: |N'| = 1 and dot(N', N) = n.z / |n| to rounding
    n[:, 2] = np.abs(n[:, 2]) + f(0.2)
    raw, ok = me.normal_raw_of(n, N, p, t)
    Np = me.normalized(raw[ok]).astype(np.float64)
    assert ok.sum() > 390
    assert np.abs(np.linalg.norm(Np, axis=1) - 1.0).max() < 1e-6
    want = n[ok, 2].astype(np.float64) / np.linalg.norm(n[ok].astype(np.float64), axis=1)
    assert np.abs((Np * N[ok].astype(np.float64)).sum(axis=1) - want).max() < 2e-5


def test_roughness_and_metallic_are_the_green_and_blue_channels():
    rgb = np.random.RandomState(4).randint(0, 256, (3, 5, 3)).astype(np.uint8)
    tex = [(packed(rgb), 0)]
    mats = np.zeros((3, SCD.MAT_VEC_SIZE), f)
    mats[0] = [SCD.MAT_DISNEY, 0, 0.1, 0.2, 0.3, 0.25, 0.75, 1, 1, 0]
    mats[1] = [SCD.MAT_DISNEY, 0, 0.1, 0.2, 0.3, 0.25, 0.75, 0, 1, 0]
    mats[2] = [SCD.MAT_GLASS, 0, 0.9, 0.9, 0.9, 1.5, 5.0, 1, 1, 0]
    z = np.zeros(3, f)
    rough, metal = me.rough_metal_at(mats, tex, np.array([0, 1, 2]), z, z)
    t00 = rgb[2, 0].astype(f) / f(255)                                    # uv (0, 0) reads texel (0, 0), the image's bottom-left, with weight exactly 1
    assert rough.tolist() == [t00[1], f(0.75), f(5.0)] and metal.tolist() == [t00[2], t00[2], f(1.5)]


def test_maps_at_on_a_small_table():
    """the eight words of the known-answer entry on two triangles and a sphere"""
    vertex = np.zeros((6, 9), f)
    vertex[0:3, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]; vertex[0:3, 3:6] = [0, 0, 2]; vertex[0:3, 6:8] = [[0, 0], [1, 0], [0, 1]]
    vertex[3:6, 0:3] = [[0, 0, 1], [1, 0, 1], [0, 1, 1]]; vertex[3:6, 3:6] = [0, 0, 1]
    prim = np.array([[SCD.PRIMITIVE_TRI, 0, 0], [SCD.PRIMITIVE_TRI, 3, 0], [SCD.PRIMITIVE_SHAPE, 0, 0]], np.int32)
    rgb = np.zeros((1, 1, 3), np.uint8); rgb[0, 0] = (255, 51, 204)
    mats = np.zeros((1, SCD.MAT_VEC_SIZE), f); mats[0] = [SCD.MAT_DISNEY, 0, 0.1, 0.2, 0.3, 0.25, 0.75, 1, 1, 1]
    out = me.maps_at(mats, [(packed(rgb), 1)], vertex, prim, np.array([0, 1, 2]), np.full(3, 0.25, f), np.full(3, 0.5, f))
    assert out[:, 0:2].tolist() == [[0.25, 0.5], [0.0, 0.0], [0.0, 0.0]]
    assert (out[:, 2] == f(51) / f(255)).all() and (out[:, 3] == f(204) / f(255)).all() and not out[:, 7].any()
    n = (np.array([255, 51, 204], f) / f(255) * f(2) - f(1)).astype(f)
    assert np.array_equal(out[0, 4:7], me.normalized(n[None, :])[0])       # T = x, B = y, N = z
    assert out[1, 4:7].tolist() == [0, 0, 1]                               # zero det: the vertex uvs are all (0, 0)
    assert out[2, 4:7].tolist() == [0, 0, 0]                               # a shape has no normal without a ray
