"""HDR environment, host side (include/tirt.h, "HDR environment"): the Radiance reader and the float encoder of ti_raytrace_amd/Texture.py against files and
an encoder written here (no code shared with the package), and the properties of the numpy restatement (tests/env_hdr_expected.py) the device tests rely on."""
import math

import numpy as np
import pytest

import env_hdr_expected as eh
import env_sampling_expected as ee
from ti_raytrace_amd import Scene, Texture, scenes

f = np.float32


# ---- a test-side writer of Radiance pictures: rgbe [h, w, 4] uint8, row 0 the top ------------------------------------------------------
def rle_component(vals):
    """new-style runs of one component: a run of equal bytes >= 3 long as (128 + n, byte), n <= 127; everything else as literals of at most 128 bytes"""
    out, lit, i, n = bytearray(), bytearray(), 0, len(vals)

    def flush():
        for k in range(0, len(lit), 128):
            part = lit[k:k + 128]
            out.append(len(part)); out.extend(part)
        del lit[:]
    while i < n:
        j = i
        while j < n and vals[j] == vals[i] and j - i < 127:
            j += 1
        if j - i >= 3:
            flush()
            out.append(128 + (j - i)); out.append(vals[i])
        else:
            lit.extend(vals[i:j])
        i = j
    flush()
    return bytes(out)


def hdr_bytes(rgbe, rle, header=b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", res=None):
    h, w = rgbe.shape[:2]
    body = bytearray(header + b"\n" + (res if res is not None else b"-Y %d +X %d\n" % (h, w)))
    for row in rgbe:
        if rle:
            body.extend(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                body.extend(rle_component([int(x) for x in row[:, c]]))
        else:
            body.extend(row.astype(np.uint8).tobytes())
    return bytes(body)


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def expected_texels(rgbe):
    """[w, h] packed, y = 0 the bottom row; E == 0 texels are the all-zero word"""
    h, w = rgbe.shape[:2]
    out = np.zeros((w, h), np.int64)
    for i in range(h):
        for j in range(w):
            r, g, b, e = (int(x) for x in rgbe[i, j])
            out[j, h - 1 - i] = 0 if e == 0 else (e << 24) | (r << 16) | (g << 8) | b
    return out.astype(np.uint32).view(np.int32)


def picture(w, h, seed):
    rgbe = np.random.RandomState(seed).randint(2, 256, (h, w, 4)).astype(np.uint8)        # (mantissas from 2: 1 1 1 n would be an old-style run)
    return rgbe


def load(path):
    t = Texture.Texture(); t.load_hdr(path)
    return t


def test_flat_and_rle_files_decode_to_the_same_texels(tmp_path):
    rgbe = picture(16, 8, 1)
    rgbe[2, 3:9, 0] = 77; rgbe[5, :, 3] = 130; rgbe[0, 0] = (9, 8, 7, 0)                   # runs, a whole-row run, an E == 0 texel with mantissas
    a, b = load(write(tmp_path, "flat.hdr", hdr_bytes(rgbe, False))), load(write(tmp_path, "rle.hdr", hdr_bytes(rgbe, True)))
    want = expected_texels(rgbe)
    assert a.format == b.format == Texture.FORMAT_RGBE8 and (a.wid, a.hgt) == (16, 8)
    assert np.array_equal(a.np_img, want) and np.array_equal(b.np_img, want)
    assert a.np_img[0, 7] == 0                                                              # canonical black
    # the #?RGBE signature and further header lines
    c = load(write(tmp_path, "rgbe.hdr", hdr_bytes(rgbe, True, header=b"#?RGBE\n# a comment\nEXPOSURE=1.0\nFORMAT=32-bit_rle_rgbe\n")))
    assert np.array_equal(c.np_img, want)


@pytest.mark.parametrize("w,h,rle", [(8, 3, True), (8, 3, False), (3, 2, False), (1, 1, False)])
def test_small_widths(tmp_path, w, h, rle):
    rgbe = picture(w, h, 10 + w)
    t = load(write(tmp_path, "s.hdr", hdr_bytes(rgbe, rle)))
    assert (t.wid, t.hgt) == (w, h) and np.array_equal(t.np_img, expected_texels(rgbe))


def test_rle_with_a_maximal_run_a_full_literal_and_a_run_to_the_end(tmp_path):
    w = 300
    rgbe = picture(w, 2, 3)
    rgbe[0, 0:127, 0] = 200                       # a run of 127, the longest a count byte holds
    rgbe[0, 127, 0] = 201
    rgbe[0, 290:300, 1] = 55                      # a run that ends exactly at the scanline's end
    # component 2 of row 0: no three equal neighbours anywhere -> literals of 128, 128 and 44 bytes
    rgbe[0, :, 2] = (np.arange(w) % 2) * 7 + 10
    data = hdr_bytes(rgbe, True)
    assert bytes([128 + 127, 200]) in data and bytes([128 + 10, 55]) in data
    comp = rle_component([int(x) for x in rgbe[0, :, 2]])
    assert comp[0] == 128 and comp[129] == 128 and comp[258] == 44 and len(comp) == 303
    t = load(write(tmp_path, "r.hdr", data))
    assert np.array_equal(t.np_img, expected_texels(rgbe))


def test_reader_refusals(tmp_path):
    rgbe = picture(16, 4, 5)
    good_flat, good_rle = hdr_bytes(rgbe, False), hdr_bytes(rgbe, True)
    cases = {
        "signature": (b"P6\n" + good_flat, "RADIANCE"),
        "xyze": (hdr_bytes(rgbe, False, header=b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n"), "xyze"),
        "no format": (hdr_bytes(rgbe, False, header=b"#?RADIANCE\n"), "FORMAT"),
        "orientation +Y": (hdr_bytes(rgbe, False, res=b"+Y 4 +X 16\n"), r"\+Y 4 \+X 16"),
        "orientation X first": (hdr_bytes(rgbe, False, res=b"+X 16 -Y 4\n"), r"\+X 16 -Y 4"),
        "truncated flat": (good_flat[:-5], "truncated"),
        "truncated rle": (good_rle[:-3], "truncated"),
        "truncated header": (b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe", "truncated"),
        "no scanlines": (good_flat[:good_flat.index(b"+X 16\n") + 6], "truncated"),
    }
    old = rgbe.copy(); old[1, 4] = (1, 1, 1, 5)
    cases["old-style run"] = (hdr_bytes(old, False), "old-style")
    # a run overrunning the scanline: the first component of the first scanline claims 127 + 127 > 16
    head = good_rle[:good_rle.index(b"+X 16\n") + 6]
    cases["overrun run"] = (head + bytes([2, 2, 0, 16, 128 + 10, 1, 128 + 10, 2]) + bytes(200), "overruns")
    cases["overrun literal"] = (head + bytes([2, 2, 0, 16, 12]) + bytes(range(1, 13)) + bytes([9]) + bytes(200), "overrun")
    cases["marker width"] = (head + bytes([2, 2, 0, 17]) + bytes(200), "width 17")
    for name, (data, match) in cases.items():
        with pytest.raises(ValueError, match=match):
            load(write(tmp_path, "bad.hdr", data))
    with pytest.raises(OSError):
        load(str(tmp_path / "missing.hdr"))


# ---- the encoder ------------------------------------------------------------------------------------------------------------------
def decoded_image(t):
    """[h, w, 3] float64 of a Texture's RGBE8 texels, row 0 the top"""
    return eh.decode(t.np_img).astype(np.float64).transpose(1, 0, 2)[::-1]


def test_encoder_truncates_within_its_step():
    r = np.random.RandomState(2)
    x = (10.0 ** r.uniform(-30, 30, (9, 7, 3))) * (r.rand(9, 7, 3) < 0.9)
    x[0, 0] = 0.0; x[1, 1] = (1e-3, 5.0, 0.0); x[2, 2] = 2.0 ** -135; x[3, 3] = (2.0 ** -136, 2.0 ** -140, 0.0)
    for dtype in (np.float64, np.float32):
        a = x.astype(dtype)
        t = Texture.Texture(); t.load_array_float(a)
        assert t.format == Texture.FORMAT_RGBE8 and (t.wid, t.hgt) == (7, 9)
        assert np.array_equal(t.np_img, eh.encode(a))                                      # the stated encoder, restated with Python integers
        d, a64 = decoded_image(t), a.astype(np.float64)
        assert (d <= a64).all()
        m = a64.max(axis=2)
        big = m >= 2.0 ** -127                                                              # E not clamped at 1: the largest mantissa is 128 .. 255
        top = np.take_along_axis(d, a64.argmax(axis=2)[..., None], axis=2)[..., 0]
        assert ((m[big] - top[big]) / m[big] < 2.0 ** -7).all()
        step = 2.0 ** (np.floor(np.log2(np.where(big, m, 1.0))) - 7)                        # one unit of the shared exponent
        assert ((a64 - d)[big] < step[big][:, None]).all()
        assert t.np_img[0, 8] == 0 and t.np_img[3, 5] == 0                                  # zero and below 2^-135: black
        assert t.np_img[2, 6].view(np.uint32) == 0x01010101                                  # 2^-135 itself in every channel: mantissa 1 at E = 1


def test_encoder_is_exact_for_powers_of_two():
    ks = np.arange(-135, 127)                     # every power a texel can hold: 2^127 would need E = 256 and is clamped to 255 * 2^119
    a = np.zeros((1, ks.size, 3)); a[0, :, 1] = 2.0 ** ks.astype(np.float64)
    t = Texture.Texture(); t.load_array_float(a)
    assert np.array_equal(decoded_image(t), a)
    a32 = np.zeros((1, 3, 3), f); a32[0, :, 0] = (1.0, 0.5, 1024.0); a32[0, :, 2] = (0.25, 0.5, 24.0)       # (24 = 3 units of 1024's mantissa step 8)
    t.load_array_float(a32)
    assert np.array_equal(decoded_image(t), a32.astype(np.float64))


def test_encoder_refusals_and_clamp():
    t = Texture.Texture()
    for bad in (-1.0, np.nan, np.inf):
        a = np.ones((2, 2, 3)); a[1, 0, 2] = bad
        with pytest.raises(ValueError):
            t.load_array_float(a)
    for arr in (np.ones((2, 2, 3), np.uint8), np.ones((2, 2, 4)), np.ones((2, 3)), np.ones((0, 2, 3))):
        with pytest.raises(ValueError):
            t.load_array_float(arr)
    a = np.full((1, 1, 3), 1e300)
    t.load_array_float(a)
    assert t.np_img[0, 0].view(np.uint32) == 0xFFFFFFFF and np.isfinite(eh.decode(t.np_img)).all()


def test_texture_carries_the_format_and_scene_dispatches():
    t = Texture.Texture()
    assert t.format == Texture.FORMAT_RGB8
    t.load_array_float(scenes.hdr_sun_sky())
    assert t.format == Texture.FORMAT_RGBE8
    t.load_black(4, 4)
    assert t.format == Texture.FORMAT_RGB8 and not t.np_img.any()
    t.load_array_float(scenes.hdr_sun_sky()); t.load_array(np.zeros((2, 2, 3), np.uint8))
    assert t.format == Texture.FORMAT_RGB8
    calls = []

    class Ctx:
        def env_upload(self, img, power): calls.append(("rgb8", power))
        def env_upload_hdr(self, img, power): calls.append(("rgbe8", power))
    t.setup_data_gpu(Ctx(), 2.0)
    t.load_array_float(scenes.hdr_sun_sky()); t.setup_data_gpu(Ctx(), 3.0)
    assert calls == [("rgb8", 2.0), ("rgbe8", 3.0)]
    sc = Scene.Scene.__new__(Scene.Scene); sc.env = Texture.Texture(); sc.env_power = 0.0
    sc.add_env_hdr(scenes.hdr_sun_sky(), 4.0)
    assert sc.env.format == Texture.FORMAT_RGBE8 and sc.env_power == 4.0 and (sc.env.wid, sc.env.hgt) == (16, 8)
    with pytest.raises(ValueError):
        sc.add_env_hdr(np.zeros((2, 2, 3), np.uint8), 1.0)
    with pytest.raises(ValueError):
        sc.add_env(scenes.hdr_sun_sky(), 1.0)                                              # add_env stays what it is


def test_add_env_hdr_reads_a_file(tmp_path):
    rgbe = picture(16, 8, 8)
    sc = Scene.Scene.__new__(Scene.Scene); sc.env = Texture.Texture(); sc.env_power = 0.0
    sc.add_env_hdr(write(tmp_path, "sky.hdr", hdr_bytes(rgbe, True)), 2.5)
    assert sc.env.format == Texture.FORMAT_RGBE8 and np.array_equal(sc.env.np_img, expected_texels(rgbe))


def test_hdr_sun_sky():
    img = scenes.hdr_sun_sky()
    assert img.shape == (8, 16, 3) and img.dtype == f
    assert (img[1, 11] == f(5000.0)).all() and int((img == f(0.02)).sum()) == 3 * (16 * 8 - 1)
    t = Texture.Texture(); t.load_array_float(img)
    d = decoded_image(t)
    assert (d[1, 11] == 4992.0).all()                                                       # 5000 = 156.25 * 2^5 truncates to 156 * 2^5
    assert d[1, 11, 0] / d[0, 0, 0] > 2.0e5                                                 # a ratio 8 bits times one power cannot hold


# ---- the restatement's properties ----------------------------------------------------------------------------------------------------
def images():
    r = np.random.RandomState(4)
    out = {"sun": eh.encode(scenes.hdr_sun_sky())}
    for name, (w, h) in (("1x1", (1, 1)), ("3x2", (3, 2)), ("17x5", (17, 5))):
        out[name] = eh.pack(r.randint(0, 256, (w, h)), r.randint(0, 256, (w, h)), r.randint(1, 256, (w, h)), r.randint(100, 150, (w, h)))
    return out


@pytest.mark.parametrize("k", [-100, 100, -7, 1])
def test_table_does_not_depend_on_a_common_exponent_shift(k):
    for name, img in images().items():
        q = eh.cell_q(img)
        shifted = eh.shift_exponents(img, k)
        assert not np.array_equal(shifted, img) and eh.e_max(shifted) != eh.e_max(img)
        assert np.array_equal(eh.cell_q(shifted), q), name
        assert 0 < int(q.max()) <= 2 ** 24, (name, int(q.max()))
    # the scale uses the table's 24 bits: where the brightest cell is not dimmed by its neighbours or by cos(el) the largest q lies in (2^22, 2^24].  Every mantissa
    # in 192 .. 255 at one exponent byte: lum >= 0.75 * 2^(E_max - 128), cos(el) = 0.98 in the two middle rows of 8, so q >= 0.73 * 2^24
    r = np.random.RandomState(6)
    bright = eh.pack(r.randint(192, 256, (16, 8)), r.randint(192, 256, (16, 8)), r.randint(192, 256, (16, 8)), np.full((16, 8), 140))
    for img in (bright, eh.shift_exponents(bright, k)):
        assert 2 ** 22 < int(eh.cell_q(img).max()) <= 2 ** 24


def test_table_bounds_at_the_ends_of_the_exponent_range():
    """exponent bytes down to 1 (denormal channels) and up to 255 (sums of channels overflow to +Inf: the clamp gives 2^24); q never exceeds 2^24"""
    w, h = 16, 8
    e = (np.arange(w * h).reshape(w, h) * 2 + 1) % 256
    e[e == 0] = 1
    r = np.random.RandomState(9)
    img = eh.pack(r.randint(0, 256, (w, h)), r.randint(0, 256, (w, h)), r.randint(1, 256, (w, h)), e)
    d = eh.decode(img)
    assert np.isfinite(d).all() and (d[e == 1] < 2.0 ** -126).all() and (d[e == 1] > 0).any()      # denormals are kept
    q = eh.cell_q(img)
    assert int(q.max()) <= 2 ** 24 and eh.e_max(img) == 255
    low = eh.pack([[255]], [[255]], [[255]], [[1]])
    assert int(eh.cell_q(low)[0, 0]) > 2 ** 22                                              # E_max = 1: the scale 2^151 is no float32, ldexp applies it
    tab = eh.table(eh.encode(scenes.hdr_sun_sky()))
    assert tab["total"] > 0 and eh.table(np.zeros((4, 2), np.int32)) is None


def test_lookup_of_a_constant_power_of_two_is_that_power():
    """the twin behind the film tests: (1 - t) + t == 1 weights a constant 2^k image back to 2^k, and srgb_to_lrgb(1) == 1 with the project's pow"""
    r = np.random.RandomState(3)
    tx, ty = r.uniform(-0.2, 1.2, 2000).astype(f), r.uniform(-0.2, 1.2, 2000).astype(f)
    for k in (0, 3, -2):
        img = eh.encode(np.full((4, 6, 3), 2.0 ** k))
        assert (eh.lookup(img, tx, ty) == f(2.0 ** k)).all()
    white = np.full((6, 4), 0xFFFFFF, np.int32)
    assert (ee.env_radiance(white, tx, ty) == f(1.0)).all() and ee.srgb_to_lrgb(np.ones(1, f))[0] == f(1.0)
    assert (eh.lookup_8bit(white, tx, ty) == f(1.0)).all()
    assert math.frexp(1.0) == (0.5, 1)
