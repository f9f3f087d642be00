"""Albedo textures on the host: the numpy restatement of tex_albedo (tests/texture_expected.py) against float64, its index and wrap rules, the two facts the
GPU tests rest on -- a shading step sees one colour per hit; a uv of exactly (0, 0) reads texel (0, 0) with weight exactly 1 --, and map_Kd through
both OBJ parsers and Scene.add_texture.  No device."""
import os

import numpy as np
import pytest

import texture_expected as te
from ti_raytrace_amd import ObjLoader, Scene
from ti_raytrace_amd import SceneData as SCD
from ti_raytrace_amd import Texture as TX

f = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "texture_obj")


def packed(rgb):
    """(h, w, 3) uint8, row 0 the top -> the [w, h] packed image of Texture.load_array"""
    t = TX.Texture(); t.load_array(rgb)
    return t.np_img


def random_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def lookup64(rgb, wrap, u, v):
    """bilinear lookup in float64 straight from the (h, w, 3) image: texel (x, y) is rgb[h - 1 - y, x]"""
    h, w = rgb.shape[:2]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    if wrap:
        u, v = u - np.floor(u), v - np.floor(v)
    x, y = np.clip(u * w, 0.0, w - 1.0), np.clip(v * h, 0.0, h - 1.0)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    wx, wy = (x - x0)[:, None], (y - y0)[:, None]
    at = lambda xi, yi: rgb[h - 1 - yi, xi].astype(np.float64) / 255.0
    return (at(x0, y0) * (1 - wx) + at(x1, y0) * wx) * (1 - wy) + (at(x0, y1) * (1 - wx) + at(x1, y1) * wx) * wy


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (5, 3), (64, 64)])
@pytest.mark.parametrize("wrap", [0, 1])
def test_restatement_against_float64(w, h, wrap):
    rgb = random_image(w, h, 10 * w + h)
    r = np.random.RandomState(w + 7 * wrap)
    u, v = r.uniform(-2.0, 3.0, 4000).astype(f), r.uniform(-2.0, 3.0, 4000).astype(f)
    got = te.tex_albedo(packed(rgb), wrap, u, v)
    want = lookup64(rgb, wrap, u, v)
    assert got.dtype == f and got.shape == (4000, 3)
    # float32 against float64: u * w carries 2^-24 relative, i.e. up to 3 * 64 * 2^-24 of a texel at |u| <= 3, w <= 64, times a colour step of at most 1;
    # the three mixes add a few ulp of values <= 1
    assert np.abs(got - want).max() <= 3 * 64 * 2.0 ** -24 + 8 * 2.0 ** -24


def test_texels_are_read_where_x_h_plus_y_says():
    """5 x 3, 15 distinct texels: texel centres... the integer points (x / w, y / h) read texel (x, y) = image row h - 1 - y, column x, exactly"""
    w, h = 5, 3
    rgb = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            rgb[h - 1 - y, x] = (10 * x + 1, 20 * y + 2, 16 * x + y)
    img = packed(rgb)
    assert img.shape == (w, h)
    for y in range(h):
        for x in range(w):
            assert img.reshape(-1)[x * h + y] == ((10 * x + 1) << 16) | ((20 * y + 2) << 8) | (16 * x + y)
            # u * w lands on x exactly when x / w * w rounds back to x in float32: true for these
            u, v = f(x) / f(w), f(y) / f(h)
            if f(u * f(w)) == f(x) and f(v * f(h)) == f(y):
                c = te.tex_albedo(img, 0, np.array([u]), np.array([v]))[0]
                assert c.tolist() == [f(10 * x + 1) / f(255), f(20 * y + 2) / f(255), f(16 * x + y) / f(255)], (x, y)


def test_clamp_against_repeat_and_texel_borders():
    rgb = random_image(4, 2, 3)
    img = packed(rgb)
    tex = lambda x, y: rgb[2 - 1 - y, x].astype(f) / f(255)
    one = lambda wrap, u, v: te.tex_albedo(img, wrap, np.array([u], f), np.array([v], f))[0]
    # clamp: u < 0 reads column 0, u >= 1 the last column; repeat: -0.25 -> 0.75 (column 3 of 4), 1 -> 0, 1.75 -> 0.75
    assert one(0, -0.25, 0.0).tolist() == tex(0, 0).tolist()
    assert one(0, 0.0, 0.0).tolist() == tex(0, 0).tolist()
    assert one(0, 1.0, 0.0).tolist() == tex(3, 0).tolist()
    assert one(0, 1.75, 0.0).tolist() == tex(3, 0).tolist()
    assert one(1, -0.25, 0.0).tolist() == tex(3, 0).tolist()
    assert one(1, 0.0, 0.0).tolist() == tex(0, 0).tolist()
    assert one(1, 1.0, 0.0).tolist() == tex(0, 0).tolist()
    assert one(1, 1.75, 0.0).tolist() == tex(3, 0).tolist()
    # exact texel borders: u = k / 4 is texel k with weight exactly 1 in both modes (k < 4)
    for wrap in (0, 1):
        for k in range(4):
            assert one(wrap, k / 4.0, 0.5).tolist() == tex(k, 1).tolist(), (wrap, k)
    # half way between texels 1 and 2 of row 0
    mid = one(0, 1.5 / 4.0, 0.0)
    assert mid.tolist() == (tex(1, 0) * f(0.5) + tex(2, 0) * f(0.5)).tolist()


@pytest.mark.parametrize("wrap", [0, 1])
def test_non_finite_uv_counts_as_zero_and_zero_is_texel_zero(wrap):
    for (w, h) in ((1, 1), (2, 2), (5, 3), (64, 64)):
        rgb = random_image(w, h, w)
        img = packed(rgb)
        t00 = rgb[h - 1, 0].astype(f) / f(255)
        zero = te.tex_albedo(img, wrap, np.zeros(1, f), np.zeros(1, f))[0]
        assert zero.view(np.uint32).tolist() == t00.view(np.uint32).tolist()          # texel (0, 0), weight exactly 1: a * (1 - 0) + b * 0
        for bad in (np.nan, np.inf, -np.inf):
            with np.errstate(all="raise"):                                                # (the restatement casts no NaN)
                got = te.tex_albedo(img, wrap, np.array([bad, 0.0, bad], f), np.array([0.0, bad, bad], f))
            assert (got.view(np.uint32) == t00.view(np.uint32)[None, :]).all()


def test_zero_uv_survives_the_barycentric_sum():
    """(0 * a + 0 * b) + 0 * c is +0 for every finite a, b, c a hit record can carry"""
    vertex = np.zeros((3, 9), f)
    prim = np.array([[SCD.PRIMITIVE_TRI, 0, 0]], np.int32)
    r = np.random.RandomState(1)
    bu, bv = r.uniform(-0.1, 1.1, 1000).astype(f), r.uniform(-0.1, 1.1, 1000).astype(f)
    u, v = te.hit_uv(vertex, prim, np.zeros(1000, int), bu, bv)
    assert not u.view(np.uint32).any() and not v.view(np.uint32).any()


def test_a_shading_step_sees_one_colour_per_hit():
    """the twin construction: a material whose colour is the looked-up one answers albedo_at with that colour wherever it is hit"""
    rgb = random_image(5, 3, 2)
    textures = [(packed(rgb), 1)]
    mats = np.zeros((3, SCD.MAT_VEC_SIZE), f)
    mats[0] = [SCD.MAT_DISNEY, 1, 0.1, 0.2, 0.3, 0, 0.5, 0, 0, 0]
    mats[1] = [SCD.MAT_LIGHT, 1, 9, 9, 9, 0, 0, 0, 0, 0]          # an emitter ignores its slot
    mats[2] = [SCD.MAT_GLASS, -1, 0.9, 0.9, 0.9, 1.5, 5, 0, 0, 0]
    assert [te.texture_of(m, 1) for m in mats] == [0, -1, -1]
    assert [te.texture_of(m, 0) for m in mats] == [-1, -1, -1]
    assert te.texture_of(np.array([0, 2, 0, 0, 0, 0, 0, 0, 0, 0], f), 1) == -1 and te.texture_of(np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0], f), 3) == -1
    uv = (f(0.3), f(1.7))
    twin = te.twin_materials(mats, textures, {0: uv})
    assert (twin[:, 1] == -1).all() and np.array_equal(twin[1:, 2:5], mats[1:, 2:5])
    want = te.tex_albedo(textures[0][0], 1, np.array([uv[0]]), np.array([uv[1]]))[0]
    assert twin[0, 2:5].tolist() == want.tolist()
    got = te.albedo_at(mats, textures, np.array([0, 0, 1, 2]), np.array([uv[0], 0.0, 0.5, 0.5], f), np.array([uv[1], 0.0, 0.5, 0.5], f))
    assert got[0].tolist() == twin[0, 2:5].tolist() and got[2].tolist() == [9, 9, 9] and got[3].tolist() == mats[2, 2:5].tolist()
    assert np.array_equal(te.albedo_at(twin, [], np.array([0, 0]), np.zeros(2, f), np.ones(2, f)), np.stack([twin[0, 2:5]] * 2))


# ---- map_Kd ---------------------------------------------------------------------------------------------------------------------
def test_map_kd_through_both_parsers():
    path = os.path.join(FIX, "quad.obj")
    a = ObjLoader.Wavefront(path).materials
    b = ObjLoader.Wavefront(path, native=False).materials
    assert list(a) == list(b) == ["first", "second", "plain", "lamp"]
    for name in a:
        assert a[name].texture == b[name].texture, name
        assert a[name].vertex_format == b[name].vertex_format and np.array_equal(a[name].vertices, b[name].vertices)
    assert a["first"].texture == os.path.join(FIX, "checker.png")
    assert a["second"].texture == os.path.join(FIX, "sub dir.png")          # the options in front of the name are skipped, the name keeps its blank
    assert a["plain"].texture is None
    assert a["first"].vertex_format == "T2F_V3F" and a["lamp"].vertex_format == "V3F"


def test_add_obj_uploads_what_map_kd_names():
    sc = Scene.Scene(device_id=0)
    sc.add_obj(os.path.join(FIX, "quad.obj"))
    assert [m.alebdoTex for m in sc.material_cpu] == [1, 2, -1, -1]          # 1-based ids; an emitter's map_Kd is ignored
    assert len(sc.textures) == 2
    (t0, w0), (t1, w1) = sc.textures
    assert (t0.wid, t0.hgt, w0) == (5, 3, 1) and (t1.wid, t1.hgt, w1) == (2, 2, 1)
    sc.setup_data_cpu()
    assert sc.material_np[:, 1].tolist() == [1.0, 2.0, -1.0, -1.0]
    assert sc.vertex_np[1, 6:9].tolist() == [2.5, 0.0, 0.0]                  # the vt of the second corner rides in columns 6, 7
    # ids are shared per path, and a second OBJ naming the same image adds none
    assert sc.add_texture(os.path.join(FIX, "checker.png")) == 1
    assert sc.add_texture(os.path.join(FIX, ".", "checker.png")) == 1
    assert sc.add_texture(os.path.join(FIX, "checker.png"), wrap="clamp") == 3
    assert sc.add_texture(np.zeros((2, 3, 3), np.uint8)) == 4 and sc.add_texture(np.zeros((2, 3, 3), np.uint8)) == 5
    assert sc.textures[3][0].np_img.shape == (3, 2)
    with pytest.raises(ValueError, match="wrap"):
        sc.add_texture(np.zeros((2, 3, 3), np.uint8), wrap="mirror")
    with pytest.raises(ValueError, match="uint8"):
        sc.add_texture(np.zeros((2, 3, 3), np.float32))


def test_a_missing_image_is_an_error_that_names_it(tmp_path):
    obj = tmp_path / "m.obj"
    obj.write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nusemtl a\nf 1/1 2/1 3/1\n")
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nd 1\nmap_Kd nowhere.png\n")
    sc = Scene.Scene(device_id=0)
    with pytest.raises(FileNotFoundError, match="nowhere.png"):
        sc.add_obj(str(obj))
    with pytest.raises(FileNotFoundError, match="absent.png"):
        sc.add_texture(str(tmp_path / "absent.png"))
    for native in (True, False):
        (tmp_path / "m.mtl").write_text("newmtl a\nmap_Kd -clamp on\n")          # an option and no file name
        assert ObjLoader.Wavefront(str(obj), native=native).materials["a"].texture == os.path.join(str(tmp_path), "on")
        (tmp_path / "m.mtl").write_text("newmtl a\nmap_Kd\n")
        with pytest.raises(Exception, match="map_Kd"):
            ObjLoader.Wavefront(str(obj), native=native)
