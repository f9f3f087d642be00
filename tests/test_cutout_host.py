"""Alpha cut-outs without a device (include/tirt.h, "Alpha cut-outs"): the numpy restatement against a float64 lookup and against the oracle, the share of
rays it excludes, the packing of Scene.add_texture(cutout=True) and the map_d statement of both OBJ / MTL parsers."""
import os

import numpy as np
import pytest

import cutout_expected as ce
import cutout_scenes as cs
import oracle_api
import texture_expected as te
from ti_raytrace_amd import Example, ObjLoader, Scene
from ti_raytrace_amd import SceneData as SCD

f = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
OBJ_DIR = os.path.join(HERE, "golden", "cutout_obj")


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------
def alpha64(img, wrap, u, v):
    """the bilinear lookup of the alpha channel in float64, from the definition"""
    w, h = img.shape
    u, v = np.asarray(u, np.float64).copy(), np.asarray(v, np.float64).copy()
    u[~np.isfinite(u)] = 0.0; v[~np.isfinite(v)] = 0.0
    if wrap == 1:
        u, v = u - np.floor(u), v - np.floor(v)
    x, y = np.clip(u * w, 0.0, w - 1.0), np.clip(v * h, 0.0, h - 1.0)
    lx, ly = np.floor(x), np.floor(y)
    a = (255 - ((img.astype(np.int64) >> 24) & 255)) / 255.0
    at = lambda xi, yi: a[np.clip(xi.astype(int), 0, w - 1), np.clip(yi.astype(int), 0, h - 1)]
    wx, wy = x - lx, y - ly
    return (at(lx, ly) * (1 - wx) + at(lx + 1, ly) * wx) * (1 - wy) + (at(lx, ly + 1) * (1 - wx) + at(lx + 1, ly + 1) * wx) * wy


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (5, 3), (64, 64)])
@pytest.mark.parametrize("wrap", [0, 1])
def test_tex_alpha_against_float64(size, wrap):
    w, h = size
    r = np.random.RandomState(7 * w + h + wrap)
    img = ce.pack_rgba(cs.rgba(w, h, 3, r.randint(0, 256, (h, w)).astype(np.uint8)))
    uv = r.uniform(-2.0, 3.0, (4000, 2)).astype(f)
    got = ce.tex_alpha(img, wrap, uv[:, 0], uv[:, 1])
    want = alpha64(img, wrap, uv[:, 0], uv[:, 1])
    lx, ly, wlr, wbt = ce.coords(img.shape, wrap, uv[:, 0], uv[:, 1])
    edge = (wlr < 1e-4) | (wlr > 1 - 1e-4) | (wbt < 1e-4) | (wbt > 1 - 1e-4)
    # |error|: four roundings of values <= 1 and the coordinate's own rounding times the largest alpha step (1 per texel)
    tol = 8 * 2.0 ** -24 + max(w, h) * 3.0 * 2.0 ** -22
    worst = lambda sel: float(np.abs(got[sel] - want[sel]).max()) if sel.any() else 0.0
    assert worst(~edge) <= tol
    assert worst(edge) <= tol + 2e-4          # within 1e-4 of a texel boundary the two may sit on either side of it: a neighbouring texel enters with weight < 1e-4
    assert got.dtype == f and (got >= 0).all() and (got <= 1).all()
    nf = np.array([np.inf, -np.inf, np.nan], f)
    assert np.array_equal(bits(ce.tex_alpha(img, wrap, nf, nf)), bits(ce.tex_alpha(img, wrap, np.zeros(3, f), np.zeros(3, f))))
    # the RGB lookup does not see the top byte
    plain = (img.view(np.uint32) & 0x00FFFFFF).view(np.int32)
    assert np.array_equal(bits(te.tex_albedo(img, wrap, uv[:, 0], uv[:, 1])), bits(te.tex_albedo(plain, wrap, uv[:, 0], uv[:, 1])))
    assert (ce.tex_alpha(plain, wrap, uv[:, 0], uv[:, 1]) == 1.0).all()


def test_alpha_127_and_128_straddle_the_cutoff():
    for a, keep in ((127, False), (128, True)):
        img = ce.pack_rgba(cs.rgba(1, 1, 0, np.full((1, 1), a, np.uint8)))
        al = ce.tex_alpha(img, 1, np.array([0.3], f), np.array([0.6], f))
        assert al[0] == f(a) / f(255.0) and bool(al[0] >= ce.CUTOFF) == keep


# ---- the restatement is the oracle where nothing is cut out ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layered():
    ex = cs.layered_scene()
    orc = oracle_api.OracleScene(ex.scene, ex.cam)
    assert orc.lbvh_build() == ex.scene.primitive_count - 1
    leaf = ce.leaf_indices(orc.lbvh_get()[2])
    rays = cs.layered_rays()
    return ex, orc, leaf, rays


def restate(ex, flags, rays, leaf, textures=None):
    sc = ex.scene
    return ce.closest_hit(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, cs.textures_of(sc) if textures is None else textures, flags, rays, leaf)


def assert_equals_oracle(hit, orc, rays):
    out, prim, _, bary = orc.closest_hit(rays, uv=True)
    k = hit["kept"]
    assert np.array_equal(hit["prim"][k], prim[k])
    assert np.array_equal(bits(hit["t"][k]), bits(out[k, 0]))
    assert np.array_equal(bits(hit["u"][k]), bits(bary[k, 0])) and np.array_equal(bits(hit["v"][k]), bits(bary[k, 1]))


def test_flags_off_is_the_oracle(layered):
    ex, orc, leaf, rays = layered
    hit = restate(ex, [0] * len(ex.scene.textures), rays, leaf)
    assert not hit["ties"].any()
    assert_equals_oracle(hit, orc, rays)
    assert int((hit["prim"] >= 0).sum()) > rays.shape[0] * 3 // 4


def test_all_alphas_255_is_the_oracle(layered):
    ex, orc, leaf, rays = layered
    solid = [((img.view(np.uint32) & 0x00FFFFFF).view(np.int32), w) for img, w in cs.textures_of(ex.scene)]
    hit = restate(ex, ex.scene.texture_cutout, rays, leaf, textures=solid)
    assert_equals_oracle(hit, orc, rays)


def test_excluded_share_and_holes(layered):
    ex, orc, leaf, rays = layered
    sc = ex.scene
    assert sc.texture_cutout == [1, 1, 1, 1, 1, 0]
    on = restate(ex, sc.texture_cutout, rays, leaf)
    off = restate(ex, [0] * len(sc.textures), rays, leaf)
    assert np.array_equal(on["kept"], off["kept"])                       # (the exclusion looks at candidates before the alpha rule)
    assert (~on["kept"]).mean() <= 0.01, (~on["kept"]).mean()
    assert not on["ties"].any()
    deeper = on["kept"] & ((on["t"] > off["t"]) | ((on["prim"] < 0) & (off["prim"] >= 0)))
    assert deeper.mean() >= 0.25, deeper.mean()
    assert not (on["t"] < off["t"]).any()
    # the emitter that names the fully transparent texture stays solid, the sphere behind the layers is reached through the holes
    emit = np.where(sc.material_np[:, 0] == SCD.MAT_LIGHT)[0]
    prim_mat = sc.primitive_np[:, 2]
    tri_emit = np.where(np.isin(prim_mat, emit) & (sc.primitive_np[:, 0] == SCD.PRIMITIVE_TRI))[0]
    assert np.isin(on["prim"], tri_emit).sum() > 50
    sphere = np.where(sc.primitive_np[:, 0] != SCD.PRIMITIVE_TRI)[0]
    assert np.isin(on["prim"], sphere).sum() > np.isin(off["prim"], sphere).sum() + 100
    # nothing ends on the 1 x 1 transparent material
    gone = np.where(prim_mat == 2)[0]
    assert np.isin(off["prim"], gone).sum() > 100 and not np.isin(on["prim"], gone).any()


def test_screen_rays_excluded_share():
    """the pixel-centre rays of the general-uv screen scene (tests/test_gpu_cutout.py compares the feature buffers with the restatement there)"""
    W, H = 24, 20
    ex = cs.screen_box(W, H, general_uv=True)
    sc = ex.scene
    rays = oracle_api.camera_rays(ex.cam, W, H)
    orc = oracle_api.OracleScene(sc, ex.cam)
    assert orc.lbvh_build() == sc.primitive_count - 1
    leaf = ce.leaf_indices(orc.lbvh_get()[2])          # (rays through shared edges tie: the equal-distance rule needs the leaves' indices)
    hit = ce.closest_hit(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, cs.textures_of(sc), sc.texture_cutout, rays, leaf)
    assert (~hit["kept"]).mean() <= 0.01
    assert_equals_oracle(ce.closest_hit(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, cs.textures_of(sc), [0], rays, leaf), orc, rays)
    screen = np.where(sc.primitive_np[:, 2] == sc.material_np.shape[0] - 1)[0]
    off = ce.closest_hit(sc.vertex_np, sc.primitive_np, sc.material_np, sc.shape_np, cs.textures_of(sc), [0], rays, leaf)
    assert np.isin(off["prim"], screen).sum() >= np.isin(hit["prim"], screen).sum() + 8 >= 16      # the screen is in view, and it has holes


# ---- Scene.add_texture(cutout=True) ---------------------------------------------------------------------------------------------------
def test_add_texture_cutout_packing(tmp_path):
    from PIL import Image
    sc = Scene.Scene()
    img = cs.rgba(5, 3, 1, np.random.RandomState(2).randint(0, 256, (3, 5)).astype(np.uint8))
    tid = sc.add_texture(img, wrap="clamp", cutout=True)
    tex, flag = sc.textures[tid - 1]
    assert flag == 0 and sc.texture_cutout == [1] and tex.np_img.shape == (5, 3) and tex.np_img.dtype == np.int32
    assert np.array_equal(tex.np_img, ce.pack_rgba(img))
    x, y = 3, 1                                                           # texel (x, y): image row h - 1 - y
    r, g, b, a = (int(c) for c in img[3 - 1 - y, x])
    assert int(np.uint32(tex.np_img[x, y])) == ((255 - a) << 24) | (r << 16) | (g << 8) | b
    # the default is what it was: RGB arrays only, top byte 0, and a 4-channel array is refused
    with pytest.raises(ValueError):
        sc.add_texture(img)
    with pytest.raises(ValueError):
        sc.add_texture(img[..., 0:3], cutout=True)
    t2 = sc.add_texture(np.ascontiguousarray(img[..., 0:3]))
    assert sc.texture_cutout == [1, 0] and not (sc.textures[t2 - 1][0].np_img.view(np.uint32) >> 24).any()
    assert np.array_equal(sc.textures[t2 - 1][0].np_img, (tex.np_img.view(np.uint32) & 0x00FFFFFF).view(np.int32))
    # a file: the flag is part of the id cache's key
    path = str(tmp_path / "leaf.png")
    Image.fromarray(img, "RGBA").save(path)
    a_id, b_id = sc.add_texture(path, cutout=True), sc.add_texture(path)
    assert a_id != b_id and sc.add_texture(path, cutout=True) == a_id and sc.add_texture(path) == b_id
    assert sc.texture_cutout == [1, 0, 1, 0]
    assert np.array_equal(sc.textures[a_id - 1][0].np_img, ce.pack_rgba(img))
    assert not (sc.textures[b_id - 1][0].np_img.view(np.uint32) >> 24).any()


# ---- map_d -------------------------------------------------------------------------------------------------------------------------------
def png(name):
    from PIL import Image
    return Image.open(os.path.join(OBJ_DIR, name))


def test_both_parsers_read_map_d():
    path = os.path.join(OBJ_DIR, "cutouts.obj")
    nat, py = ObjLoader.Wavefront(path), ObjLoader.Wavefront(path, native=False)
    assert list(nat.materials) == list(py.materials) == ["same_file", "other_file", "mask_only", "plain", "lamp"]
    for name in nat.materials:
        assert nat.materials[name].opacity == py.materials[name].opacity, name
        assert nat.materials[name].texture == py.materials[name].texture, name
    m = nat.materials
    assert m["same_file"].opacity == os.path.join(OBJ_DIR, "leaf rgba.png") == m["same_file"].texture      # options skipped, a name with a space
    assert m["other_file"].opacity == os.path.join(OBJ_DIR, "mask_grey.png") and m["other_file"].texture == os.path.join(OBJ_DIR, "colour.png")
    assert m["mask_only"].opacity == os.path.join(OBJ_DIR, "mask_grey.png") and m["mask_only"].texture is None
    assert m["plain"].opacity is None and m["lamp"].opacity == os.path.join(OBJ_DIR, "mask_grey.png")


def test_add_obj_makes_cutout_textures():
    ex = Example.example(8, 8, 1, 0)
    sc = ex.scene
    sc.add_obj(os.path.join(OBJ_DIR, "cutouts.obj"))
    mats = sc.material_cpu
    rgba_img = np.asarray(png("leaf rgba.png").convert("RGBA"), np.uint8)
    grey = np.asarray(png("mask_grey.png").convert("L"), np.uint8)
    colour = np.asarray(png("colour.png").convert("RGB"), np.uint8)
    tex = lambda m: sc.textures[m.alebdoTex - 1][0].np_img
    # the same file as map_Kd: that texture, with its own alpha
    assert np.array_equal(tex(mats[0]), ce.pack_rgba(rgba_img)) and sc.texture_cutout[mats[0].alebdoTex - 1] == 1
    # another file of the same size: its grey value joins the map_Kd image's RGB
    assert np.array_equal(tex(mats[1]), ce.pack_rgba(np.concatenate([colour, grey[..., None]], axis=2))) and sc.texture_cutout[mats[1].alebdoTex - 1] == 1
    # map_d alone: RGB is Kd rounded to 8 bits (0.25 0.5 1.0 -> 64 128 255)
    want = np.concatenate([np.broadcast_to(np.array([64, 128, 255], np.uint8), grey.shape + (3,)), grey[..., None]], axis=2)
    assert np.array_equal(tex(mats[2]), ce.pack_rgba(want)) and sc.texture_cutout[mats[2].alebdoTex - 1] == 1
    # an ordinary map_Kd stays what it was; an emitter gets no texture
    assert sc.texture_cutout[mats[3].alebdoTex - 1] == 0 and not (tex(mats[3]).view(np.uint32) >> 24).any()
    assert mats[4].type == SCD.MAT_LIGHT and mats[4].alebdoTex == -1
    assert len(sc.textures) == 4 and sc.texture_cutout == [1, 1, 1, 0]


def test_map_d_of_another_size_is_refused():
    ex = Example.example(8, 8, 1, 0)
    with pytest.raises(ValueError, match="one size"):
        ex.scene.add_obj(os.path.join(OBJ_DIR, "bad_size.obj"))
