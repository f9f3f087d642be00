"""Emitters chosen by power on the device (include/tirt.h, "Choosing emitters by power").  The table, the pick and one shading step of every new instantiation
are held to the numpy restatement (tests/light_sampling_expected.py) bit for bit; the switch-off renders to the oracle; the switched-on renders to the switch-off
renders by their own sample moments, and to themselves for determinism.

Measured on the MI355X, 16 x 12, 256 frames, seed 11 (profiles/light_sampling_quality.txt): see the figures there; no factor is asserted here."""
import numpy as np
import pytest

import common
from common import on_device, step_scene
import cutout_scenes as cs
import env_sampling_expected as ee
import env_sampling_scenes as es
import light_sampling_expected as le
import oracle_api
import shade_step_cases as cases
from ti_raytrace_amd import _native, Example, PT_RGB, scenes
from ti_raytrace_amd import SceneData as SCD

pytestmark = pytest.mark.gpu
f = np.float32
SEED = es.SEED
W, H = 16, 12
BIT = _native.SF_LIGHT_POWER
ENV = _native.SF_ENV_SAMPLE
TOP = float(f(1.0) - f(2.0 ** -24))
NAN_TRI = np.array([[(0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0.25, 0.25, 0.25)]])      # collinear: Heron's product is negative in float32, the area NaN


def bits(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


def render(ex, frames, calls=(None,), seed=SEED, clear=True):
    ctx = ex.scene.ctx
    if clear:
        ctx.film_clear()
    parts = [frames] if calls == (None,) else list(calls)
    begin = 0
    for n in parts:
        ctx.pt_rgb_render(begin, n, seed, PT_RGB.MAX_DEPTH, 64, 0)
        begin += n
    return ctx.film_download(ex.imgSizeX, ex.imgSizeY)[0], ctx.moments_download(ex.imgSizeX, ex.imgSizeY)


def emitter(e):
    m = SCD.Material(); m.type = SCD.MAT_LIGHT; m.setColor([float(e), float(e), float(e)]); m.alebdoTex = -1
    return m


def list_scene(emissions, sizes, spheres=(), extra=None):
    """a ground quad under one emissive right triangle per entry of `emissions` (leg sizes[k], its own material), then `spheres` (pos, radius, emission)"""
    ex = Example.example(8, 8, 4, 0)
    g = 4.0
    ex.scene.add_mesh(cs.quad((-g, 0, -g), (-g, 0, g), (g, 0, g), (g, 0, -g)), cases.disney(1.0, 0.6, (0.7, 0.7, 0.7)))
    side = int(np.ceil(np.sqrt(len(emissions))))
    for k, (e, s) in enumerate(zip(emissions, sizes)):
        x, z = -3.0 + 6.0 * (k % side) / side, -3.0 + 6.0 * (k // side) / side
        ex.scene.add_mesh(np.array([[(x, 2.0, z), (x + s, 2.0, z), (x, 2.0, z + s)]]), emitter(e))
    if extra is not None:
        ex.scene.add_mesh(extra, emitter(3.0))
    for pos, radius, e in spheres:
        ex.add_sphere_light(pos=pos, radius=radius, emission=e)
    ex.integrator = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, moments=True)
    ex.scene.setup_data_cpu()
    ex.frame_camera()
    return ex


def random_list(n, seed):
    r = np.random.RandomState(seed)
    return np.exp2(r.uniform(-6, 6, n)), r.uniform(0.02, 0.3, n)


LISTS = {
    "1": lambda: list_scene(*random_list(1, 1)), "2": lambda: list_scene(*random_list(2, 2)), "3": lambda: list_scene(*random_list(3, 3)),
    "64": lambda: list_scene(*random_list(64, 64)), "65": lambda: list_scene(*random_list(65, 65)), "1000": lambda: list_scene(*random_list(1000, 1000)),
    "zero-first": lambda: list_scene([0.0, 0.0, 2.0, 3.0, 1.0, 5.0], [0.2] * 6), "zero-last": lambda: list_scene([2.0, 3.0, 1.0, 5.0, 0.0, 0.0], [0.2] * 6),
    "zero-middle": lambda: list_scene([2.0, 0.0, 0.0, 5.0, 0.0, 1.0], [0.2, 0.1, 0.3, 0.2, 0.2, 0.1]),
    "equal": lambda: list_scene([3.0] * 5, [0.25] * 5),
    "one-big": lambda: list_scene([2.0 ** -4, 2.0 ** 20, 2.0 ** -4, 2.0 ** -4], [0.25] * 4),
    "nan-area": lambda: list_scene([2.0, 4.0], [0.2, 0.1], extra=NAN_TRI),
    "mix": lambda: list_scene(*random_list(7, 7), spheres=(((0.0, 3.0, 0.0), 0.4, 6.0), ((2.0, 1.5, 1.0), 0.05, 300.0))),
}


def randoms(tab, u):
    """0, 1 - 2^-24, every prefix boundary -1 / 0 / +1 in units of 2^-24 (mapped through the share), the share's own edges, and random ones"""
    total = tab["total"]
    ks = [0, (1 << 24) - 1]
    for c in tab["prefix"][:-1]:
        kb = -((-int(c) << 24) // total)                                   # the first k with floor(k * total / 2^24) >= c
        ks += [max(kb - 1, 0), min(kb, (1 << 24) - 1), min(kb + 1, (1 << 24) - 1)]
    r2 = (np.array(ks, np.float64) / (1 << 24)).astype(f)
    r = (f(u) + (r2 * f(f(1.0) - f(u))).astype(f)).astype(f)
    rnd = np.random.RandomState(5).randint(0, 1 << 24, 2000).astype(f) / f(1 << 24)
    edge = np.array([0.0, TOP, u, np.nextafter(f(u), f(0)), np.nextafter(f(u), f(1)), u * 0.5, 1.0], f)
    return np.minimum(np.concatenate([r, rnd.astype(f), edge]), f(1.0)).astype(f)


# ---- 1. the table and the pick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LISTS))
def test_table_and_pick_equal_the_restatement(gpu_ctx_ok, name):
    ex = LISTS[name]()
    ctx = on_device(ex)
    n = ex.scene.light_count
    assert ctx.light_table_download() is None and not ctx.shade_features()[0] & BIT            # mode 0: no table
    lrec = ctx.shade_table_download(1, n)
    em, area = le.record_lists(lrec)
    host_em, host_area = le.scene_lists(ex.scene)
    assert np.array_equal(bits(em), bits(host_em)) and common.same_bits(area, host_area)
    if name == "nan-area":
        assert np.isnan(area[2])
    for u in (0.0, 0.25, TOP):
        ctx.light_sampling(True, u)
        want = le.table(em, area, u)
        got = ctx.light_table_download()
        assert got is not None and got["count"] == n and got["active"] and ctx.shade_features()[0] & BIT
        assert got["e_max"] == want["e_max"]
        for key in ("q", "prefix"):
            assert np.array_equal(got[key], want[key]), (name, u, key)
        assert np.array_equal(bits(got["P"]), bits(want["P"])), (name, u)
        r = randoms(want, u)
        gi, gp = ctx.kat_light_pick(r)
        wi, wp, uni = le.pick(want, r)
        assert np.array_equal(gi, wi), (name, u, r[gi != wi][:4], gi[gi != wi][:4], wi[gi != wi][:4])
        assert np.array_equal(bits(gp), bits(wp)), (name, u)
        assert uni.any() == (u > 0)
        assert (want["q"][wi[~uni]] > 0).all()                                                  # the integer inverse never answers with a weightless entry
        # the spare word of every emitter's shading record holds its entry's P, every other primitive's is 0
        rec = ctx.shade_table_download(0, ex.scene.primitive_count)
        tri = rec[:, 1, 3].view(np.int32) == 1
        spare = np.where(tri, rec[:, 4, 3], rec[:, 2, 0])
        phit = np.zeros(ex.scene.primitive_count, f); phit[ex.scene.light_np[:n]] = want["P"]
        assert np.array_equal(bits(spare), bits(phit))
        # the light records are what they were: quads 6 and 7 zero, the rest untouched
        assert np.array_equal(bits(ctx.shade_table_download(1, n)), bits(lrec)) and (lrec[:, 6:8] == 0).all()
    if name == "equal":
        assert len(set(want["q"].tolist())) == 1
    if name == "one-big":
        assert want["q"][[0, 2, 3]].tolist() == [1, 1, 1] and want["q"][1] >= 1 << 23                 # 2^24 times the rest: they live on the floor of 1
    if name.startswith("zero") or name == "nan-area":
        assert (want["q"] == 0).any()
    if name == "mix":
        assert (lrec[:, 2, 3].view(np.int32) == 1).sum() == 2 and (lrec[:, 2, 3].view(np.int32) == -1).sum() == 7
    with pytest.raises(_native.TirtError, match="outside"):
        ctx.kat_light_pick(np.array([1.5], f))
    ctx.light_sampling(False, 0.0)
    assert ctx.light_table_download() is None and not ctx.shade_features()[0] & BIT
    rec = ctx.shade_table_download(0, ex.scene.primitive_count)
    assert (rec[:, 4, 3] == 0).all() and (rec[rec[:, 1, 3].view(np.int32) != 1][:, 2, 0] == 0).all()      # written back to 0
    with pytest.raises(_native.TirtError, match="no table"):
        ctx.kat_light_pick(np.array([0.5], f))


def test_black_emitters_leave_the_bit_clear(gpu_ctx_ok):
    ex = list_scene([0.0, 0.0], [0.2, 0.2])
    ctx = on_device(ex)
    ctx.light_sampling(True, 0.0)
    got = ctx.light_table_download()
    assert got is not None and not got["active"] and (got["q"] == 0).all() and (got["P"] == 0).all() and not ctx.shade_features()[0] & BIT
    with pytest.raises(_native.TirtError, match="4096"):
        ctx.kat_shade_step(127 | BIT, np.zeros((1, 23), np.uint32))


# ---- 2. one shading step per new instantiation -------------------------------------------------------------------------------------------
STRIDE = 11
FORCED = 150
U_STEP, P_ENV = 0.25, 0.5
BRANCHES = ("light_power", "light_uniform", "light_not_facing", "light_pdf0", "emitter_spec", "emitter_mis")
_step = {}


def step_rows():
    """every STRIDE-th row of the cases of the scene plus FORCED rows that force e_pdf <= 0, finite directions only; built once, on the scene without environment"""
    if "rows" not in _step:
        ex = step_scene(None)
        orc = oracle_api.OracleScene(ex.scene, ex.cam)
        assert orc.lbvh_build() == ex.scene.primitive_count - 1
        rng = np.random.RandomState(2024)
        rows = np.ascontiguousarray(np.concatenate([cases.real_hit_rows(ex, orc, rng), cases.synthetic_hit_rows(ex, orc, rng, repeats=1), cases.miss_rows(rng)], axis=0))
        _step["rows_all"], _step["orc"], _step["host"] = rows, orc, ex
    return _step["rows_all"], _step["orc"], _step["host"]


@pytest.mark.parametrize("feat", _native.SHADE_INSTANTIATIONS_POWER)
def test_one_shading_step_equals_the_restatement(gpu_ctx_ok, feat):
    """The restatement is a change to the step of the SIBLING instantiation (the same word without bit 4096), which tests/test_gpu_shade_step.py,
    test_gpu_env_sampling.py and test_gpu_env_hdr.py hold to the oracle's step; for 127 | 4096 and 511 | 4096 the sibling's step is compared with the oracle's here as
    well (the oracle has neither the environment's light sample nor RGBE8 texels: the other six siblings have no oracle answer on any scene).
    Every word of every row is compared; the rows the choice by power changes -- an emitter hit that is not behind a specular vertex, every light sample -- are
    restated from the table, the records and the oracle's Disney evaluation.  uniform_share 0.25, so both branches of the choice occur."""
    env = "hdr" if feat & 2048 else ("ldr" if feat & 1024 else None)
    rows_all, orc, _ = step_rows()
    ex = step_scene(env)
    ctx, sc = on_device(ex), ex.scene
    ctx.env_sampling(bool(feat & 1024), P_ENV)
    ctx.light_sampling(True, U_STEP)
    word = ctx.shade_features()[0]
    assert word & BIT and bool(word & ENV) == bool(feat & 1024) and bool(word & 2048) == bool(feat & 2048) and not word & (128 | 256)
    n = sc.light_count
    lrec = ctx.shade_table_download(1, n)
    tab = le.table(*le.record_lists(lrec), U_STEP)
    rec = ctx.shade_table_download(0, sc.primitive_count).reshape(-1, 32)
    phit = np.zeros(sc.primitive_count, f); phit[sc.light_np[:n]] = tab["P"]
    if "pick" not in _step:
        forced = ee.behind_shading_normal(rows_all, rec, sc.material_np)
        assert forced.size >= 20, forced.size
        pick = np.union1d(np.arange(0, rows_all.shape[0], STRIDE), forced[::max(1, forced.size // FORCED)])
        rows = np.ascontiguousarray(rows_all[pick])
        _step["pick"] = np.ascontiguousarray(rows[np.isfinite(rows.view(f)[:, 8:11]).all(axis=1)])
    rows = _step["pick"]
    sibling = feat & ~BIT
    base = ctx.kat_shade_step(sibling, rows)
    if feat in (127 | BIT, 511 | BIT):               # the siblings the oracle has an answer for (no material of the scene names the uploaded texture)
        assert not cases.first_differences(base, orc.kat_shade_step(rows), rows, ex)
    p_env = P_ENV if feat & 1024 else 0.0
    if p_env not in _step:
        want, branch, over = le.step_on(rows, np.zeros((rows.shape[0], 28), f), rec, sc.material_np, tab, lrec.reshape(-1, 32), phit, p_env, with_mask=True)
        _step[p_env] = (want, branch, over)
    want0, branch, over = _step[p_env]
    want = np.where(over, want0, base[:, :28]).astype(f)
    got = ctx.kat_shade_step(feat, rows)
    counts = {b: int((branch == b).sum()) for b in np.unique(branch)}
    print("k_shade<%d>" % feat, counts)
    report = cases.first_differences(got, want, rows, ex)
    assert not report, "\n".join(report)
    for b in BRANCHES:
        assert counts.get(b, 0) > 0, (b, counts)
    # the choice matters: some light sample names another emitter than the sibling's uniform choice did
    lp = np.isin(branch, ("light_power", "light_uniform"))
    assert (got.view(np.uint32)[lp, 17:26] != base.view(np.uint32)[lp, 17:26]).any()
    em = branch == "emitter_mis"
    assert (got.view(np.uint32)[em, 0:3] != base.view(np.uint32)[em, 0:3]).any()
    ctx.light_sampling(False, 0.0)
    with pytest.raises(_native.TirtError, match="4096"):
        ctx.kat_shade_step(feat, rows[:1])


# ---- 3. switch off ------------------------------------------------------------------------------------------------------------------------
def lamp(w=W, h=H, light_sampling="uniform", n_embers=62, before=None, **kw):
    ex = scenes.lamp_and_embers(w, h, 4, 0, n_embers=n_embers, light_sampling=light_sampling, seed=SEED, moments=True, **kw)
    if before is not None:
        before(ex)
    ex.scene.setup_data_cpu()
    ex.frame_camera()
    return ex


def test_switch_off_equals_the_oracle(gpu_ctx_ok):
    """Film, feature records and moment records with the switch off -- never switched on, and switched off again after a switched-on render -- are the same bits,
    and they are the oracle's: the film its render, the feature records tests/aov_expected.py over its hits, the moment records Welford's update
    (tests/moments_expected.py) over its exact one-frame samples; the shading records are the same bits too, spare words 0."""
    import aov_expected as ae
    import moments_expected as me
    ex = lamp()
    ctx = on_device(ex)
    ctx.aov_enable(True)
    nprim = ex.scene.primitive_count

    def records(frames):
        ctx.film_clear()
        for begin, n in frames:
            ctx.pt_rgb_render(begin, n, SEED, PT_RGB.MAX_DEPTH, 64, 0)
        return ctx.film_download(W, H)[0], ctx.moments_download(W, H), ctx.aov_download(W, H)
    whole, exact = [(0, 8)], [(fr, 1) for fr in me.EXACT_FRAMES]
    never, never_exact = records(whole), records(exact)
    rec_never, lrec_never = ctx.shade_table_download(0, nprim), ctx.shade_table_download(1, ex.scene.light_count)
    assert (rec_never[:, 4, 3] == 0).all()
    ctx.light_sampling(True, 0.0)
    assert ctx.shade_features()[0] & BIT
    on = records(whole)
    assert not np.array_equal(bits(on[0]), bits(never[0])) and np.array_equal(bits(on[2]), bits(never[2]))
    assert (ctx.shade_table_download(0, nprim)[ex.scene.light_np, 4, 3] > 0).all()
    ctx.light_sampling(False, 0.0)
    assert not ctx.shade_features()[0] & BIT
    again, again_exact = records(whole), records(exact)
    for k, what in enumerate(("film", "moments", "features")):
        assert np.array_equal(bits(again[k]), bits(never[k])), what
        assert np.array_equal(bits(again_exact[k]), bits(never_exact[k])), what
    assert np.array_equal(bits(ctx.shade_table_download(0, nprim)), bits(rec_never))
    assert np.array_equal(bits(ctx.shade_table_download(1, ex.scene.light_count)), bits(lrec_never))
    orc = oracle_api.OracleScene(ex.scene, ex.cam)
    assert orc.lbvh_build() == nprim - 1
    want, _ = orc.render(W, H, 0, 8, seed=SEED)
    want_aov, hits, _ = ae.expected(ex, orc, W, H, range(8), SEED)
    want_mom = me.expected([me.oracle_sample(orc, W, H, fr, SEED) for fr in me.EXACT_FRAMES], W, H)
    orc.close()
    assert common.same_bits(again[0], want)
    assert hits > 0 and common.same_bits(again[2], want_aov, nan_payload=not np.isnan(want_aov).any())
    assert not np.isnan(again_exact[1]).any() and (again_exact[1] == want_mom).all()


def test_a_spot_or_laser_on_the_list_keeps_today_s_kernels(gpu_ctx_ok):
    ex = common.spot_laser_scene(W, H, device_id=0)
    common.host_only(ex)
    ctx = on_device(ex)
    ctx.moments_enable(True)
    off, off_mom = render(ex, 4)
    ctx.light_sampling(True, 0.25)
    word = ctx.shade_features()[0]
    assert not word & BIT and word & _native.SF_LIGHT_SPOT_LASER and ctx.light_table_download() is None
    on, on_mom = render(ex, 4)
    assert np.array_equal(bits(on), bits(off)) and np.array_equal(bits(on_mom), bits(off_mom))
    assert (ctx.shade_table_download(0, ex.scene.primitive_count)[:, 4, 3] == 0).all()


# ---- 4. determinism and plumbing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(24, 20), (13, 7), (1, 1)])
def test_film_does_not_depend_on_how_the_frames_are_submitted(gpu_ctx_ok, w, h):
    ex = lamp(w, h, "power", light_uniform_share=0.125)
    ctx = on_device(ex)
    assert ctx.shade_features()[0] & BIT and ex.integrator.light_sampling == ("power", 0.125) and ex.integrator.light_sampling_active
    base, base_mom = render(ex, 8)
    assert np.isfinite(base).all() and (base.sum() > 0 or w == 1)
    split, split_mom = render(ex, 8, calls=(2, 6))
    assert np.array_equal(bits(split), bits(base)) and np.array_equal(bits(split_mom), bits(base_mom))
    for lanes in (1, 4):
        ctx.set_option("overlap_lanes", lanes)
        for beams in (0, 1):
            ctx.set_option("primary_beams", beams)
            film, mom = render(ex, 8)
            assert np.array_equal(bits(film), bits(base)) and np.array_equal(bits(mom), bits(base_mom)), (lanes, beams)
    # tiles of another size, two ranks' films put together
    if w * h > 1:
        whole = np.zeros_like(base)
        for rank in (0, 1):
            ctx.film_create(w, h, rank, 2, 10)
            assert ctx.shade_features()[0] & BIT                                                # tirt_film_create keeps the switch
            ctx.pt_rgb_render(0, 8, SEED, PT_RGB.MAX_DEPTH, 64, 0)
            whole += ctx.film_download(w, h)[0]
        assert np.array_equal(bits(whole), bits(base))


def test_a_render_builds_the_table_by_itself(gpu_ctx_ok):
    """no tirt_shade_features, no download before the first switched-on render: tirt_pt_rgb_render builds the table with the light records and picks the twin"""
    ex = lamp(light_sampling="power")
    ctx = on_device(ex)
    first, first_mom = render(ex, 8)
    assert ctx.shade_features()[0] & BIT
    again, again_mom = render(ex, 8)
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first_mom), bits(again_mom)) and first.sum() > 0
    ctx.light_sampling(False, 0.0)                       # and back: the very next render is the uniform one, without a query in between
    off, _ = render(ex, 8)
    ctx.light_sampling(True, 0.0)
    back, _ = render(ex, 8)
    assert not np.array_equal(bits(off), bits(first)) and np.array_equal(bits(back), bits(first))
    ex_off = lamp()
    on_device(ex_off)
    assert np.array_equal(bits(render(ex_off, 8)[0]), bits(off))


def test_pixel_set_gives_the_dense_film(gpu_ctx_ok):
    ex = lamp(light_sampling="power")
    ctx = on_device(ex)
    dense, _ = render(ex, 8)
    px = np.arange(W * H, dtype=np.int32)[::3]
    ctx.film_clear()
    ctx.pixel_set_upload(px)
    ctx.pt_rgb_render(0, 8, SEED, PT_RGB.MAX_DEPTH, 64, 0)
    ctx.pixel_set_clear()
    part = ctx.film_download(W, H)[0]
    assert np.array_equal(bits(part.reshape(-1, 3)[px]), bits(dense.reshape(-1, 3)[px]))
    assert (part.reshape(-1, 3)[np.setdiff1d(np.arange(W * H), px)] == 0).all()


def test_textured_twin_equals_the_untextured_scene(gpu_ctx_ok):
    """a constant roughness map (green 128) in place of the row's roughness 128 / 255: k_shade<511 | 4096> gives k_shade<127 | 4096>'s film"""
    films = []
    for textured in (False, True):
        def before(ex):
            ex.scene.material_cpu[0].setRough(float(f(128.0) / f(255.0)))
            if textured:
                ex.scene.material_cpu[0].roughTex = ex.scene.add_texture(np.full((2, 2, 3), 128, np.uint8))
        ex = lamp(light_sampling="power", before=before)
        ctx = on_device(ex)
        word = ctx.shade_features()[0]
        assert word & BIT and bool(word & _native.SF_TEXTURE_PARAM) == textured
        films.append(render(ex, 8)[0])
    assert np.array_equal(bits(films[0]), bits(films[1])) and films[0].sum() > 0


def test_with_a_cutout_sheet_and_with_env_sampling(gpu_ctx_ok):
    """a cut-out sheet under the lamp (k_trace's CUTOUT twins and the unchanged shadow ray), then the environment's light sample beside the choice by power:
    both render, deterministically, under the words that say so"""
    def add_sheet(ex):
        sc = ex.scene
        img = np.zeros((8, 8, 4), np.uint8); img[..., 0:3] = 200; img[..., 3] = cs.checker(8, 8, 2)
        m = cases.disney(1.0, 0.6, (0.8, 0.8, 0.8)); m.alebdoTex = sc.add_texture(img, wrap="clamp", cutout=True)
        ex.sheet_first = sc.vertex_count
        sc.add_mesh(cs.quad((-0.8, 1.2, -0.8), (0.8, 1.2, -0.8), (0.8, 1.2, 0.8), (-0.8, 1.2, 0.8)), m)
    ex = lamp(light_sampling="power", before=add_sheet)
    ex.scene.vertex_np[ex.sheet_first:ex.sheet_first + 6, 6:8] = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], f)
    ctx = on_device(ex)
    word = ctx.shade_features()[0]
    assert word & BIT and word & _native.SF_CUTOUT
    a, _ = render(ex, 8)
    b, _ = render(ex, 8, calls=(3, 5))
    assert np.array_equal(bits(a), bits(b)) and np.isfinite(a).all() and a.sum() > 0
    ex = lamp(light_sampling="power", before=lambda ex: ex.scene.add_env(scenes.sun_sky_image(), 2.0), env_sampling=True)
    ctx = on_device(ex)
    assert ctx.shade_features()[0] & (BIT | ENV) == BIT | ENV
    a, _ = render(ex, 8)
    b, _ = render(ex, 8, calls=(5, 3))
    assert np.array_equal(bits(a), bits(b)) and np.isfinite(a).all() and a.sum() > 0
    ctx.light_sampling(False, 0.0)
    c, _ = render(ex, 8)
    assert not np.array_equal(bits(a), bits(c)) and ctx.shade_features()[0] & (BIT | ENV) == ENV


def test_other_integrators_do_not_read_the_switch(gpu_ctx_ok):
    ex = scenes.veach_bdpt(W, H, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    films = []
    for on in (False, True, False):
        ctx.light_sampling(on, 0.0)
        assert bool(ctx.shade_features()[0] & BIT) == on
        ctx.film_clear()
        ctx.bdpt_rgb_render(0, 2, SEED)
        films.append(ctx.film_download(W, H)[0])
    # (BDPT splats with atomics: two runs of ONE setting agree to rel-L2 1e-5, tests/test_gpu_bdpt.py; the switch must change no more than a rerun does)
    m = np.isfinite(films[0]).all(axis=2) & np.isfinite(films[1]).all(axis=2) & np.isfinite(films[2]).all(axis=2)
    assert m.mean() > 0.9 and common.rel_l2(films[2][m], films[0][m]) <= 1e-5 and common.rel_l2(films[1][m], films[0][m]) <= 1e-5
    ex = scenes.sky_dome(W, H, 4, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    films = []
    for on in (False, True):
        ctx.light_sampling(on, 0.0)
        ctx.film_clear()
        ex.integrator.render_frames(2)
        films.append(ex.integrator.hdr.to_numpy().copy())
    assert np.array_equal(bits(films[0]), bits(films[1])) and np.isfinite(films[0]).any()


# ---- 5. agreement ---------------------------------------------------------------------------------------------------------------------------
FRAMES = 256
Z_MAX = 4.0


def regions(ex):
    """four fixed blocks of the film, by geometry: ground pixels (the centre ray meets primitive 0 or 1) in the four quarters of the film"""
    orc = oracle_api.OracleScene(ex.scene, ex.cam)
    assert orc.lbvh_build() == ex.scene.primitive_count - 1
    _, prim, _ = orc.closest_hit(oracle_api.camera_rays(ex.cam, W, H))
    orc.close()
    ground = (prim >= 0) & (prim < 2)
    ii = np.arange(W * H) // H
    jj = np.arange(W * H) % H
    return {"%s-%s" % (a, b): np.where(ground & (ii < W // 2 if a == "left" else ii >= W // 2) & (jj < H // 2 if b == "low" else jj >= H // 2))[0]
            for a in ("left", "right") for b in ("low", "high")}


@pytest.mark.parametrize("metallic", [1.0, 0.0], ids=["metal", "dielectric"])
def test_lamp_and_embers_agrees_with_the_switch_off_render_and_is_less_noisy(gpu_ctx_ok, metallic):
    """scenes.lamp_and_embers with its 254 embers, 16 x 12 x 256 frames.  On the rough metal (the reference's sampler draws from the pdf it states, so on and off
    have one expectation) every region of on agrees with off and with off at another seed within 4 combined standard errors, the margin of
    tests/test_gpu_env_sampling.py, and the summed per-pixel variance drops.  On the rough dielectric the z-scores are printed (include/tirt.h, LIMIT) and only the
    variance ordering is asserted."""
    ex = lamp(n_embers=254, metallic=metallic)
    reg = {k: v for k, v in regions(ex).items() if v.size >= 8}
    assert len(reg) >= 2, {k: v.size for k, v in regions(ex).items()}
    ctx = on_device(ex)
    moms = {}
    _, moms["off"] = render(ex, FRAMES)
    _, moms["off2"] = render(ex, FRAMES, seed=SEED + 100)
    ctx.light_sampling(True, 0.0)
    assert ctx.shade_features()[0] & BIT
    film, moms["on"] = render(ex, FRAMES)
    assert np.isfinite(film).all()
    var = {k: float((m.reshape(-1, 8)[:, 4:7] / (m.reshape(-1, 8)[:, 0:1] - 1.0)).sum()) for k, m in moms.items()}
    tag = "metal" if metallic else "dielectric"
    print("lamp_and_embers (%s): summed per-pixel variance %s, off / on = %.2f" % (tag, var, var["off"] / var["on"]))
    worst = 0.0
    for a, b in (("off", "off2"), ("on", "off"), ("on", "off2")):
        for name, px in reg.items():
            z = es.z_score(es.region_stats(moms[a], px), es.region_stats(moms[b], px))
            print("lamp_and_embers (%s), %s vs %s, %s (%d px): z = %+.2f" % (tag, a, b, name, px.size, z))
            worst = max(worst, abs(z))
    if metallic:
        assert worst <= Z_MAX, worst
    assert var["on"] < var["off"] and var["on"] < var["off2"], var


# ---- 6. lifecycle -----------------------------------------------------------------------------------------------------------------------------
def test_table_follows_vertices_materials_and_scene_uploads(gpu_ctx_ok):
    ex = lamp(light_sampling="power")
    ctx, sc = on_device(ex), ex.scene
    n = sc.light_count

    def device_table():
        return ctx.light_table_download(), le.table(*le.record_lists(ctx.shade_table_download(1, n)), 0.0)
    got, want = device_table()
    assert got["active"] and np.array_equal(got["prefix"], want["prefix"])
    before = got["q"].copy()
    # update_vertices that grows the lamp (vertices 6..11: its two triangles) by 3 in x and z
    lamp_first = int(sc.primitive_np[sc.light_np[0], 1])
    pos = sc.vertex_np[lamp_first:lamp_first + 6, 0:3].copy()
    pos[:, 0] *= 3.0; pos[:, 2] *= 3.0
    sc.update_vertices(pos, first_vertex=lamp_first)
    assert ctx.shade_features()[0] & BIT
    got, want = device_table()
    host = le.table(*le.scene_lists(sc), 0.0)
    assert np.array_equal(got["prefix"], want["prefix"]) and np.array_equal(got["q"], host["q"]) and np.array_equal(bits(got["P"]), bits(host["P"]))
    assert not np.array_equal(got["q"], before) and (got["q"][2:] <= before[2:]).all() and got["q"][2:].sum() < before[2:].sum()
    rec = ctx.shade_table_download(0, sc.primitive_count)
    assert np.array_equal(bits(rec[sc.light_np[:n], 4, 3]), bits(host["P"]))
    film, _ = render(ex, 4)
    assert np.isfinite(film).all() and film.sum() > 0
    # a material upload that blacks every emitter turns the feature off; the old colours turn it on again
    mats = sc.material_np.copy()
    black = mats.copy(); black[black[:, 0] == SCD.MAT_LIGHT, 2:5] = 0
    ctx.material_upload(black)
    assert not ctx.shade_features()[0] & BIT and not ctx.light_table_download()["active"]
    assert (ctx.shade_table_download(0, sc.primitive_count)[:, 4, 3] == 0).all()
    ctx.material_upload(mats)
    assert ctx.shade_features()[0] & BIT and np.array_equal(ctx.light_table_download()["q"], host["q"])
    # scene re-upload: another list, the switch persists
    ex2 = lamp(light_sampling="uniform", n_embers=9)
    s2 = ex2.scene
    ctx.scene_upload(s2.vertex_np, s2.primitive_np, s2.material_np, s2.shape_np, s2.light_np, s2.light_count, s2.minboundarynp, s2.maxboundarynp)
    got = ctx.light_table_download()
    host2 = le.table(*le.scene_lists(s2), 0.0)
    assert ctx.shade_features()[0] & BIT and got["count"] == 11 and np.array_equal(got["q"], host2["q"]) and np.array_equal(bits(got["P"]), bits(host2["P"]))
    # tirt_film_create keeps the switch
    ctx.film_create(W, H, 0, 1, 4096)
    assert ctx.shade_features()[0] & BIT
    ex.integrator.set_light_sampling("uniform")
    assert not ctx.shade_features()[0] & BIT and ex.integrator.light_sampling == ("uniform", 0.0)
    with pytest.raises(ValueError):
        ex.integrator.set_light_sampling("power", 1.0)
    with pytest.raises(ValueError):
        ex.integrator.set_light_sampling("brightest")
