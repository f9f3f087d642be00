"""HDR environment on the device (include/tirt.h, "HDR environment").  The lookup, the sampling table and one shading step of every new instantiation of k_shade
are held to the numpy restatement (tests/env_hdr_expected.py over tests/env_sampling_expected.py) bit for bit; films are held to the oracle through a twin the
oracle can render (a constant 2^k RGBE8 image with power p against an all-white 8-bit image with power p * 2^k), to the switch-off render by their own sample
moments, and to the 8-bit kernels' bits once the 8-bit image is back."""
import numpy as np
import pytest

import common
import env_hdr_expected as eh
import env_sampling_expected as ee
import env_sampling_scenes as es
import oracle_api
import shade_step_cases as cases
from ti_raytrace_amd import _native, PT_RGB, Texture, scenes
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu
f = np.float32
SEED = es.SEED
W, H = 16, 12
HDR, SAMPLE = _native.SF_ENV_HDR, _native.SF_ENV_SAMPLE


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def packed8(rgb):
    t = Texture.Texture(); t.load_array(rgb)
    return t.np_img


def random_rgbe(w, h, seed, e_lo=100, e_hi=150):
    r = np.random.RandomState(seed)
    img = eh.pack(r.randint(0, 256, (w, h)), r.randint(0, 256, (w, h)), r.randint(0, 256, (w, h)), r.randint(e_lo, e_hi, (w, h)))
    if w * h > 4:
        img.reshape(-1)[r.randint(0, w * h, 2)] = 0                                         # black texels among them
    return img


def exponent_ramp():
    """16 x 8: exponent bytes 1, 3, .., 255 -- denormal channels at the low end, sums of channels beyond FLT_MAX at the high end"""
    r = np.random.RandomState(12)
    e = 1 + 2 * np.arange(128).reshape(16, 8)
    return eh.pack(r.randint(0, 256, (16, 8)), r.randint(0, 256, (16, 8)), r.randint(1, 256, (16, 8)), e)


IMAGES = {"1x1": lambda: random_rgbe(1, 1, 1), "3x2": lambda: random_rgbe(3, 2, 2), "17x5": lambda: random_rgbe(17, 5, 3),
          "sun": lambda: eh.encode(scenes.hdr_sun_sky()), "ramp": exponent_ramp}


def coordinates(w, h, seed=5, n_random=3000):
    """about 4 000 rows of (tx, ty): random ones around [0, 1]^2, every texel edge and centre, 0, 1, below 0, above 1, infinities and NaN"""
    r = np.random.RandomState(seed)
    rows = [r.uniform(-0.1, 1.1, (n_random, 2))]
    gx = np.concatenate([np.arange(w + 1) / w, (np.arange(w) + 0.5) / w]); gy = np.concatenate([np.arange(h + 1) / h, (np.arange(h) + 0.5) / h])
    grid = np.stack(np.meshgrid(gx, gy, indexing="ij"), axis=-1).reshape(-1, 2)
    rows.append(grid[r.permutation(grid.shape[0])[:800]])
    rows.append(np.stack([gx, np.full(gx.size, 0.37)], axis=1)); rows.append(np.stack([np.full(gy.size, 0.61), gy], axis=1))
    sp = [0.0, 1.0, -0.0, -0.5, 1.5, -1e30, 1e30, np.inf, -np.inf, np.nan, 1e-45, 1.0 - 2.0 ** -24]
    rows.append(np.array([(a, b) for a in sp for b in sp]))
    return np.ascontiguousarray(np.concatenate(rows).astype(f))


def on_device(ex):
    ex.integrator.setup_data_cpu(); ex.integrator.setup_data_gpu(); ex.scene.setup_data_gpu()
    return ex.scene.ctx


# ---- 1. the lookup ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_lookup_equals_the_restatement(gpu_ctx_ok, name):
    img = IMAGES[name]()
    xy = coordinates(*img.shape)
    ctx = _native.Context(0)
    ctx.env_upload_hdr(img, 1.0)
    assert ctx.env_format() == (1, eh.e_max(img))
    got = ctx.kat_env_lookup(xy)
    want = eh.lookup(img, xy[:, 0], xy[:, 1])
    nan_rows = np.isnan(xy).any(axis=1)
    assert np.isnan(want[nan_rows]).all() and np.isfinite(want[~nan_rows]).all()
    bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (name, int(bad.any(axis=1).sum()), xy[bad.any(axis=1)][:4], got[bad.any(axis=1)][:4], want[bad.any(axis=1)][:4])
    if name == "ramp":
        assert ((got > 0) & (got < f(2.0 ** -126))).any()                                   # denormal results come out as denormals
    ctx.close()


@pytest.mark.parametrize("name", ["7x5", "sun8"])
def test_lookup_entry_on_an_8bit_image(gpu_ctx_ok, name):
    """the entry is honest: on an 8-bit image it gives the existing restatement of the miss branch's value, env_sampling_expected.env_radiance.  That function
    states finite (tx, ty) (it goes through tex_albedo, whose rule for a coordinate that is not finite the miss branch does not have: there an infinity is clamped
    and a NaN gives NaN); lookup_8bit restates the miss branch's texture2D for every row"""
    img = packed8(np.random.RandomState(3).randint(0, 256, (5, 7, 3)).astype(np.uint8)) if name == "7x5" else packed8(scenes.sun_sky_image())
    xy = coordinates(*img.shape)
    ctx = _native.Context(0)
    ctx.env_upload(img, 1.0)
    assert ctx.env_format() == (0, 0)
    got = ctx.kat_env_lookup(xy)
    fin = np.isfinite(xy).all(axis=1)
    assert fin.sum() > 3000 and np.array_equal(bits(got[fin]), bits(ee.env_radiance(img, xy[fin, 0], xy[fin, 1])))
    nan = np.isnan(xy).any(axis=1)
    assert common.same_bits(got, eh.lookup_8bit(img, xy[:, 0], xy[:, 1])) and np.isnan(got[nan]).all() and np.isfinite(got[~nan]).all()
    ctx.close()


# ---- 2. the table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_table_equals_the_restatement(gpu_ctx_ok, name):
    img = IMAGES[name]()
    want = eh.table(img, 2.0)
    ctx = _native.Context(0)
    ctx.env_upload_hdr(img, 2.0)
    assert ctx.env_table_download() is None and ctx.shade_features()[0] & (HDR | SAMPLE) == HDR
    ctx.env_sampling(True, 0.5)
    got = ctx.env_table_download()
    assert got is not None and (got["w"], got["h"]) == img.shape and got["active"] and ctx.shade_features()[0] & (HDR | SAMPLE) == HDR | SAMPLE
    for key in ("q", "row_sums", "marginal"):
        assert np.array_equal(got[key], want[key]), (name, key, int((got[key] != want[key]).sum()))
    assert int(got["q"].max()) <= 1 << 24
    # a common shift of the exponent bytes: the same table to the bit
    for k in (-100, 100):
        shifted = eh.shift_exponents(img, k)
        if np.array_equal(shifted, img):
            continue                                                                        # (the ramp fills the range: no room to shift)
        ctx.env_upload_hdr(shifted, 2.0)
        assert ctx.env_format() == (1, eh.e_max(shifted))
        again = ctx.env_table_download()
        for key in ("q", "row_sums", "marginal"):
            assert np.array_equal(again[key], got[key]), (name, k, key)
    ctx.close()


@pytest.mark.parametrize("name", ["17x5", "sun"])
def test_sample_and_pdf_over_the_hdr_table(gpu_ctx_ok, name):
    img = IMAGES[name]()
    tab = eh.table(img)
    ctx = _native.Context(0)
    ctx.env_sampling(True, 0.5)
    ctx.env_upload_hdr(img, 1.0)
    r = np.random.RandomState(7)
    top = f(1.0) - f(2.0 ** -24)
    rr = np.concatenate([np.array([[0, 0], [0, top], [top, 0], [top, top]], f), (r.randint(0, 1 << 24, (1500, 2)).astype(f) / f(1 << 24)).astype(f)])
    got = ctx.kat_env_sample(rr)
    i, j, tx, ty, d = ee.sample(tab, rr[:, 0], rr[:, 1])
    li, lj, _, _, p = ee.pdf(tab, d)
    gi = got.view(np.int32)
    assert np.array_equal(gi[:, 0], i) and np.array_equal(gi[:, 1], j) and np.array_equal(bits(got[:, 2:4]), bits(np.stack([tx, ty], axis=1)))
    assert np.array_equal(bits(got[:, 4:7]), bits(d)) and np.array_equal(bits(got[:, 7]), bits(p)) and np.array_equal(gi[:, 8], li) and np.array_equal(gi[:, 9], lj)
    dirs = r.normal(size=(1500, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs = np.concatenate([[[0, 1, 0], [0, -1, 0], [-1, 0, 0], [1, 0, 0]], dirs]).astype(f)
    gp = ctx.kat_env_pdf(dirs)
    wi, wj, wtx, wty, wp = ee.pdf(tab, dirs)
    assert np.array_equal(gp.view(np.int32)[:, 0], wi) and np.array_equal(gp.view(np.int32)[:, 1], wj) and np.array_equal(bits(gp[:, 4]), bits(wp))
    if name == "sun":
        assert (np.bincount(j * 16 + i, minlength=128).argmax() // 16) in (5, 6)          # most samples land in the sun's cells (row 6 from the bottom and its neighbour)
    ctx.close()


# ---- 3. one shading step, per new instantiation -------------------------------------------------------------------------------------------
STEP_STRIDE = {"env_only": 29, "generic": 37}
FORCED = 60


def step_sky():
    """12 x 6 linear radiance over five decades with one hot texel"""
    r = np.random.RandomState(8)
    sky = (10.0 ** r.uniform(-3.0, 2.0, (6, 12, 3))).astype(f)
    sky[1, 7] = 3000.0
    return eh.encode(sky)


@pytest.mark.parametrize("name", sorted(STEP_STRIDE))
def test_one_shading_step_of_every_hdr_instantiation(gpu_ctx_ok, name):
    """Rows of tests/shade_step_cases.py (every STEP_STRIDE-th plus rows that force e_pdf <= 0), on the scene with its environment replaced by an RGBE8 image.
    k_shade<127 | 2048> and <511 | 2048>: miss rows are radiance + (L * throughput) * env_power of the restated lookup, directions that are not finite included;
    hit rows are the 8-bit sibling's bits on the scene with its 8-bit image (they never read the image).  <127 | 1024 | 2048> and <511 | 1024 | 2048>: every word
    of every row with a finite direction is env_sampling_expected.step_on with the RGBE8 lookup and table in the 8-bit ones' place.  The scenes name no texture, so
    the kernels with every texture slot must give the generic twins' words; they run with one unused texture uploaded."""
    ex, orc, rows = cases.build(name)
    ctx, sc = on_device(ex), ex.scene
    try:
        rec = np.zeros((sc.primitive_count, 32), f)
        _native.check(_native.lib().tirt_shade_table_download(ctx.handle, 0, rec.reshape(-1), rec.size))
        lrec = np.zeros((max(sc.light_count, 1), 32), f)
        if sc.light_count:
            _native.check(_native.lib().tirt_shade_table_download(ctx.handle, 1, lrec.reshape(-1), lrec.size))
        forced = ee.behind_shading_normal(rows, rec, sc.material_np)
        pick = np.union1d(np.arange(0, rows.shape[0], STEP_STRIDE[name]), forced[::max(1, forced.size // FORCED)])
        rows = np.ascontiguousarray(rows[pick])
        rf = rows.view(f)
        with np.errstate(invalid="ignore"):
            miss = ~(rf[:, 11] < f(1000000.0))
        fin = np.isfinite(rf[:, 8:11]).all(axis=1)
        assert miss.sum() > 50 and (~miss).sum() > 500 and (miss & ~fin).sum() > 10
        word8 = ctx.shade_features()[0]
        assert word8 == cases.SCENES[name][1] and not word8 & HDR
        sibling = ctx.kat_shade_step(_native.SF_ALL, rows)                                  # the 8-bit kernel on the 8-bit image
        with pytest.raises(_native.TirtError, match="2048"):
            ctx.kat_shade_step(_native.SF_ALL | HDR, rows[:1])                              # an RGBE8 kernel on 8-bit texels
        img, power, share = step_sky(), sc.env_power, 0.5
        ctx.env_upload_hdr(img, power)
        assert ctx.shade_features()[0] == word8 | HDR
        with pytest.raises(_native.TirtError, match="2048"):
            ctx.kat_shade_step(_native.SF_ALL, rows[:1])                                    # and the other way round
        ctx.texture_upload([(np.full((2, 2), 0x808080, np.int32), 0)])
        want_miss = eh.miss_term(img, power, rows[miss])
        for feat in (_native.SF_ALL | HDR, _native.SHADE_INSTANTIATION_MAPS | HDR):
            got = ctx.kat_shade_step(feat, rows)
            assert common.same_bits(got[miss, 0:3], want_miss), (feat, "miss rows")
            assert np.array_equal(bits(got[miss, 3:]), bits(sibling[miss, 3:]))
            assert np.array_equal(bits(got[~miss]), bits(sibling[~miss])), (feat, "hit rows")
        assert np.isfinite(want_miss).any() and not common.same_bits(sibling[miss, 0:3], want_miss)
        # with the table
        ctx.env_sampling(True, share)
        assert ctx.shade_features()[0] == word8 | HDR | SAMPLE
        tab = eh.table(img, power)
        frows = np.ascontiguousarray(rows[fin])
        off = orc.kat_shade_step(frows)
        with eh.radiance_patch():
            want, full, branch = ee.step_on(frows, off, rec, sc.material_np, sc.light_count, img, power, tab, share, lrec)
        counts = {b: int((branch == b).sum()) for b in np.unique(branch)}
        print(name, counts)
        assert full.all()
        for b in ("miss_spec", "miss_mis", "env_taken"):
            assert counts.get(b, 0) > 0, (b, counts)
        for feat in (_native.SF_ALL | SAMPLE | HDR, _native.SHADE_INSTANTIATION_MAPS | SAMPLE | HDR):
            got = ctx.kat_shade_step(feat, frows)
            report = cases.first_differences(got, want, frows, ex)
            assert not report, "%d\n%s" % (feat, "\n".join(report))
        with pytest.raises(_native.TirtError, match="2048"):
            ctx.kat_shade_step(_native.SF_ALL | SAMPLE, frows[:1])
    finally:
        # (ex and orc are the per-process cache's of tests/shade_step_cases.py, which other files use: the 8-bit image back, no textures, the switch off)
        ctx.env_sampling(False, 0.5)
        ctx.texture_upload([])
        ctx.env_upload(sc.env.np_img, sc.env_power)
    assert ctx.shade_features()[0] == cases.SCENES[name][1]


# ---- 4. films against the oracle through an exact twin -------------------------------------------------------------------------------------
FRAMES = 4
P = 1.5
WHITE = np.full((4, 8, 3), 255, np.uint8)


def twin_scene(kind, Wf, Hf, power):
    if kind == "teapot":
        ex = scenes.single_model(Wf, Hf, FRAMES, device_id=0, seed=SEED, aov=True, moments=True)
        ex.scene.add_env(WHITE, power)
    else:
        ex = scenes.sun_ground(Wf, Hf, FRAMES, 0, env_power=power, sky=WHITE, env_sampling=False, seed=SEED, aov=True, moments=True)
    ex.build_scene()
    return ex


def records(ctx, Wf, Hf, calls):
    ctx.film_clear()
    begin = 0
    for n in calls:
        ctx.pt_rgb_render(begin, n, SEED, PT_RGB.MAX_DEPTH, 64, 0)
        begin += n
    assert begin == FRAMES
    return ctx.film_download(Wf, Hf)[0], ctx.aov_download(Wf, Hf), ctx.moments_download(Wf, Hf)


def same_records(a, b, what):
    for x, y, part in zip(a, b, ("film", "features", "moments")):
        assert np.array_equal(bits(x), bits(y)), (what, part, int((bits(x) != bits(y)).sum()))


@pytest.mark.parametrize("kind", ["teapot", "sun_ground"])
@pytest.mark.parametrize("Wf,Hf", [(24, 20), (13, 7)])
def test_films_of_a_constant_sky_equal_the_8bit_twin_and_the_oracle(gpu_ctx_ok, kind, Wf, Hf):
    """An RGBE8 image of constant 2^k with power P against an all-white 8-bit image with power P * 2^k, k = 0, 3, -2: the lookup of either is its constant
    exactly ((1 - t) + t == 1 in float32, srgb_to_lrgb(1) == 1: tests/test_env_hdr_host.py), and the two powers of two meet in one exact product.  Switch off:
    film, feature records and moment records are the same bits, and the 8-bit film is the oracle's.  Switch on: the 8-bit twin's table is rint(cos(el) * 2^24)
    while the constant 2^k has mantissa 128 (a channel reaches only HALF of 2^(E_max - 128)) and its table is rint(cos(el) * 2^23) -- the two tables are not
    equal, so the switched-on twin is RGBE8 against RGBE8: 2^k with power P against 2^0 with power P * 2^k, whose tables ARE equal by the exponent shift."""
    for k in (0, 3, -2):
        ex = twin_scene(kind, Wf, Hf, P * 2.0 ** k)
        ctx = ex.scene.ctx
        word = ctx.shade_features()[0]
        assert word & _native.SF_ENV and not word & (HDR | SAMPLE) and ctx.env_format() == (0, 0)
        ldr = records(ctx, Wf, Hf, (FRAMES,))
        orc = oracle_api.OracleScene(ex.scene, ex.cam)
        assert orc.lbvh_build() == ex.scene.primitive_count - 1
        if kind == "teapot":
            orc.process_normal(ex.scene.vertex_index_np)
        want, _ = orc.render(Wf, Hf, 0, FRAMES, seed=SEED)
        orc.close()
        assert common.same_bits(ldr[0], want) and np.isfinite(want).any() and want.sum() > 0
        const = eh.encode(np.full((4, 8, 3), 2.0 ** k))
        ctx.env_upload_hdr(const, P)
        assert ctx.shade_features()[0] == word | HDR
        same_records(records(ctx, Wf, Hf, (1, FRAMES - 1)), ldr, (kind, k, "off"))
        # switch on
        ctx.env_sampling(True, 0.5)
        assert ctx.shade_features()[0] == word | HDR | SAMPLE
        tab = ctx.env_table_download()
        on = records(ctx, Wf, Hf, (FRAMES,))
        # (the Teapot is all glass: no vertex takes a light sample and every miss follows a specular vertex, so its switched-on film is the switched-off one)
        assert np.array_equal(bits(on[0]), bits(ldr[0])) == (kind == "teapot") and np.array_equal(bits(on[1]), bits(ldr[1]))
        ctx.env_upload_hdr(eh.encode(np.full((4, 8, 3), 1.0)), P * 2.0 ** k)
        tab1 = ctx.env_table_download()
        assert np.array_equal(tab1["row_sums"], tab["row_sums"]) and np.array_equal(tab1["marginal"], tab["marginal"])
        same_records(records(ctx, Wf, Hf, (1, FRAMES - 1)), on, (kind, k, "on"))
        ctx.set_option("merge_paths", 0)                                                    # every call a batch of its own
        same_records(records(ctx, Wf, Hf, (2, 1, 1)), on, (kind, k, "on, every call a batch"))
        ctx.env_sampling(False, 0.5)
        ctx.env_upload_hdr(const, P)
        same_records(records(ctx, Wf, Hf, (2, 1, 1)), ldr, (kind, k, "off, every call a batch"))
        ctx.close()


# ---- 5. the two estimators agree -------------------------------------------------------------------------------------------------------
N_FRAMES = 256
Z_MAX = 4.0
CORNELL_POWER = 0.01           # the sun's texel at 50, about the 8-bit sun scene's 20: the box's own light stays visible beside it


def render(ex, frames, seed=SEED):
    ctx = ex.scene.ctx
    ctx.film_clear()
    ctx.pt_rgb_render(0, frames, seed, PT_RGB.MAX_DEPTH, 64, 0)
    return ctx.film_download(ex.imgSizeX, ex.imgSizeY)[0], ctx.moments_download(ex.imgSizeX, ex.imgSizeY)


def cornell_hdr_sky(Wf=W, Hf=H):
    ex = scenes.cornell_box(Wf, Hf, 4, device_id=0, seed=SEED, moments=True)
    ex.scene.add_env_hdr(scenes.hdr_sun_sky(), CORNELL_POWER)
    common.host_only(ex)
    return ex


def agree(moms, reg, what):
    worst = 0.0
    names = sorted(moms)
    for x in range(len(names)):
        for y in range(x + 1, len(names)):
            for rname, px in reg.items():
                z = es.z_score(es.region_stats(moms[names[x]], px), es.region_stats(moms[names[y]], px))
                print("%s, %s vs %s, %s: z = %+.2f" % (what, names[x], names[y], rname, z))
                worst = max(worst, abs(z))
    return worst


def test_sun_scene_under_the_hdr_sky_agrees_with_the_switch_off_render(gpu_ctx_ok):
    """scenes.sun_ground under scenes.hdr_sun_sky() (a sun 250 000 times its sky), rough metals: region means with the switch on and off agree within 4 combined
    standard errors, by the criterion of tests/test_gpu_env_sampling.py (region_stats also asserts n >= 2 and that no sample was non-finite)."""
    ex = es.sun_scene(W, H, metallic=1.0, sky=scenes.hdr_sun_sky())
    assert ex.scene.env.format == Texture.FORMAT_RGBE8
    reg = es.regions_sun(ex)
    assert min(v.size for v in reg.values()) >= 8, {k: v.size for k, v in reg.items()}
    ctx = on_device(ex)
    assert ctx.shade_features()[0] & (HDR | SAMPLE) == HDR
    moms = {}
    _, moms["off"] = render(ex, N_FRAMES)
    ctx.env_sampling(True, 0.5)
    assert ctx.shade_features()[0] & (HDR | SAMPLE) == HDR | SAMPLE
    film, moms["on"] = render(ex, N_FRAMES)
    assert np.isfinite(film).all()
    var = {k: float((m.reshape(-1, 8)[:, 4:7] / (m.reshape(-1, 8)[:, 0:1] - 1.0)).sum()) for k, m in moms.items()}
    print("HDR sun scene, summed per-pixel variance:", var)
    assert agree(moms, reg, "HDR sun scene") <= Z_MAX


def test_cornell_under_the_hdr_sky_agrees_with_the_switch_off_render(gpu_ctx_ok):
    ex = cornell_hdr_sky()
    reg = es.regions_cornell(ex)
    assert min(v.size for v in reg.values()) >= 4
    ctx = on_device(ex)
    assert ctx.shade_features()[0] & (HDR | SAMPLE) == HDR
    moms = {}
    _, moms["off"] = render(ex, N_FRAMES)
    ctx.env_sampling(True, 0.5)
    _, moms["on"] = render(ex, N_FRAMES)
    assert agree(moms, reg, "cornell + HDR sky") <= Z_MAX


# ---- 6. lifecycle ------------------------------------------------------------------------------------------------------------------------
def test_an_8bit_upload_after_an_hdr_upload_returns_to_the_old_bits(gpu_ctx_ok):
    fresh = es.sun_scene(W, H)
    assert not on_device(fresh).shade_features()[0] & HDR
    want = render(fresh, 8)[0]
    ex = es.sun_scene(W, H)
    ctx = on_device(ex)
    ctx.env_upload_hdr(eh.encode(scenes.hdr_sun_sky()), 3.0)
    assert ctx.shade_features()[0] & HDR and ctx.env_format()[0] == 1
    other = render(ex, 8)[0]
    assert not np.array_equal(bits(other), bits(want))
    ctx.env_upload(ex.scene.env.np_img, ex.scene.env_power)
    assert not ctx.shade_features()[0] & HDR and ctx.env_format() == (0, 0)
    assert np.array_equal(bits(render(ex, 8)[0]), bits(want))
    # the same with the switch on: the 8-bit table is rebuilt from the 8-bit texels
    ctx.env_sampling(True, 0.5)
    on8 = render(ex, 8)[0]
    ctx.env_upload_hdr(eh.encode(scenes.hdr_sun_sky()), 3.0)
    assert np.array_equal(ctx.env_table_download()["q"], eh.table(eh.encode(scenes.hdr_sun_sky()))["q"])
    ctx.env_upload(ex.scene.env.np_img, ex.scene.env_power)
    assert np.array_equal(ctx.env_table_download()["q"], ee.table(ex.scene.env.np_img)["q"])
    assert np.array_equal(bits(render(ex, 8)[0]), bits(on8))


def test_power_zero_with_an_hdr_image_is_a_black_environment(gpu_ctx_ok):
    films = []
    for sky in (scenes.hdr_sun_sky(), None):
        ex = scenes.sun_ground(W, H, 4, 0, env_power=0.0, sky=sky, env_sampling=True, seed=SEED, moments=True)
        ex.build_scene()
        ctx = ex.scene.ctx
        assert ex.scene.env.format == Texture.FORMAT_RGB8 and ctx.env_format() == (0, 0)   # setup_data_cpu loads the black image
        assert not ctx.shade_features()[0] & (_native.SF_ENV | HDR | SAMPLE)
        films.append(render(ex, 4)[0])
    assert np.array_equal(bits(films[0]), bits(films[1]))
    # the C entry itself: power 0 with lit texels is lit (the 8-bit rule) and renders what a black image renders
    ctx.env_upload_hdr(eh.encode(scenes.hdr_sun_sky()), 0.0)
    assert ctx.shade_features()[0] & (_native.SF_ENV | HDR | SAMPLE) == _native.SF_ENV | HDR and ctx.env_table_download() is None
    assert np.array_equal(bits(render(ex, 4)[0]), bits(films[1]))


def test_the_switch_around_an_hdr_upload_keeps_or_rebuilds_the_table(gpu_ctx_ok):
    img, other = eh.encode(scenes.hdr_sun_sky()), random_rgbe(5, 3, 21)
    ctx = _native.Context(0)
    ctx.env_sampling(True, 0.25)
    ctx.env_upload_hdr(img, 2.0)                                                            # switched on before the upload: the upload builds
    assert np.array_equal(ctx.env_table_download()["row_sums"], eh.table(img)["row_sums"])
    ctx.env_sampling(True, 0.75)                                                            # the share alone: the table stands
    assert np.array_equal(ctx.env_table_download()["row_sums"], eh.table(img)["row_sums"]) and ctx.shade_features()[0] & SAMPLE
    ctx.env_sampling(False, 0.5)
    assert ctx.env_table_download() is None and ctx.shade_features()[0] & (HDR | SAMPLE) == HDR
    ctx.env_upload_hdr(other, 2.0)                                                          # uploaded with the switch off, then switched on: the switch builds
    assert ctx.env_table_download() is None
    ctx.env_sampling(True, 0.5)
    assert np.array_equal(ctx.env_table_download()["row_sums"], eh.table(other)["row_sums"])
    ctx.env_upload_hdr(np.zeros((4, 2), np.int32), 2.0)                                     # black: lit by its power, no table
    assert ctx.env_table_download() is None and ctx.shade_features()[0] & (HDR | SAMPLE) == HDR and ctx.env_format() == (1, 0)
    bad = img.copy(); bad[2, 2] = 0x00010000
    with pytest.raises(_native.TirtError, match="texel 18 "):
        ctx.env_upload_hdr(bad, 2.0)
    assert ctx.env_format() == (1, 0)                                                       # a refused upload changes nothing
    ctx.close()


@pytest.mark.parametrize("sampling", [False, True])
def test_pixel_set_gives_the_dense_film(gpu_ctx_ok, sampling):
    """the LIST twins of the RGBE8 kernels"""
    ex = cornell_hdr_sky()
    ctx = on_device(ex)
    ctx.env_sampling(sampling, 0.5)
    assert ctx.shade_features()[0] & (HDR | SAMPLE) == HDR | (SAMPLE if sampling else 0)
    dense, _ = render(ex, 8)
    px = np.arange(W * H, dtype=np.int32)[::3]
    ctx.film_clear()
    ctx.pixel_set_upload(px)
    ctx.pt_rgb_render(0, 8, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    ctx.pixel_set_clear()
    part = ctx.film_download(W, H)[0]
    assert np.array_equal(bits(part.reshape(-1, 3)[px]), bits(dense.reshape(-1, 3)[px])) and dense.sum() > 0
    rest = np.setdiff1d(np.arange(W * H), px)
    assert (part.reshape(-1, 3)[rest] == 0).all()


def test_textured_twin_equals_the_untextured_scene(gpu_ctx_ok):
    """a constant roughness map in place of the row's roughness: k_shade<511 | 2048> and <511 | 1024 | 2048> give the films of <127 | 2048> and <127 | 1024 | 2048>"""
    films = {}
    for textured in (False, True):
        def before(ex):
            ex.scene.material_cpu[0].setRough(float(f(128.0) / f(255.0)))
            if textured:
                ex.scene.material_cpu[0].roughTex = ex.scene.add_texture(np.full((2, 2, 3), 128, np.uint8))
        ex = es.sun_scene(W, H, sky=scenes.hdr_sun_sky(), before=before)
        ctx = on_device(ex)
        for sampling in (False, True):
            ctx.env_sampling(sampling, 0.5)
            word = ctx.shade_features()[0]
            assert word & HDR and bool(word & SAMPLE) == sampling and bool(word & _native.SF_TEXTURE_PARAM) == textured
            films[textured, sampling] = render(ex, 8)[0]
    for sampling in (False, True):
        assert np.array_equal(bits(films[False, sampling]), bits(films[True, sampling])) and films[False, sampling].sum() > 0


# ---- 7. nothing else moved ----------------------------------------------------------------------------------------------------------------
def test_scenes_with_8bit_images_never_get_the_bit(gpu_ctx_ok):
    for ex in (es.sun_scene(W, H), es.cornell_sky(W, H), es.sun_scene(W, H, env_sampling=True)):
        ctx = on_device(ex)
        assert not ctx.shade_features()[0] & HDR and ctx.env_format() == (0, 0)
