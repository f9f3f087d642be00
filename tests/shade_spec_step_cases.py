"""Input rows for the known-answer tests of one PT_Spec shading step (tests/test_shade_spec_step_host.py, tests/test_gpu_shade_spec_step.py): four scenes under
PT_Spec.PathTrace and, per scene, about 1e5 rows of (seed, pixel, frame, bounce, ray, hit record, four-channel path state) built deterministically from a seed.  The
scenes, the hit records and the miss directions are those of tests/shade_step_cases.py (its helpers build words 0..14); the state and the spectral extras are here.

Row layout (include/tirt.h, tirt_kat_shade_spec_step; 32-bit words, integers as themselves):
   0 seed  1 pixel  2 frame  3 bounce  4 last_bounce  5..7 origin  8..10 direction  11 t  12 u  13 v  14 prim  15..18 throughout[4]  19..22 radiance[4]
"""
import numpy as np

import oracle_api
import shade_step_cases as rgb
from ti_raytrace_amd import _native, PT_Spec
from ti_raytrace_amd import SceneData as SCD

IN_WORDS = _native.KAT_SPEC_STEP_IN
OUT_WORDS = _native.KAT_SPEC_STEP_OUT
INF_VALUE = rgb.INF_VALUE
MAX_DEPTH = PT_Spec.MAX_DEPTH
FILM_W, FILM_H = rgb.FILM_W, rgb.FILM_H
TM_DIM_SPEC_LAMBDA = 4000            # tirt_math.h / oracle.c: the dimension of the path's hero wavelength
BRANCH_WORD = OUT_WORDS              # orc_kat_shade_spec_step's word behind the device's 29

# output fields: name -> (first word, words, is float)
OUT_FIELDS = [("radiance", 0, 4, True), ("shaded", 4, 1, False), ("want_next", 5, 1, False), ("next_o", 6, 3, True), ("next_d", 9, 3, True),
              ("next_thr", 12, 4, True), ("want_shadow", 16, 1, False), ("sh_o", 17, 3, True), ("sh_d", 20, 3, True), ("sh_c", 23, 4, True),
              ("sh_expect", 27, 1, False), ("sh_dist", 28, 1, True)]


# ---- scenes: the four of shade_step_cases.py with a black material added, under the spectral integrator ------------------------------
def black_patch(ex, centre):
    """three triangles of a black Disney material (reflect_spec of the RGB -> spectrum table's darkest cell; a throughput that becomes 0 in every channel)"""
    tri = rgb.scenes.synthetic_triangles(3, 33, 0.3) + np.asarray(centre)[None, None, :]
    ex.scene.add_mesh(tri, rgb.disney(0.0, 0.5, (0.0, 0.0, 0.0)))


def spectral(ex):
    ex.integrator = PT_Spec.PathTrace(FILM_W, FILM_H, ex.cam, ex.scene, 64)
    return ex


def grid_sphere():
    ex = rgb.grid_sphere(); black_patch(ex, (0.3, 0.2, -0.2))
    return spectral(ex)


def grid_mesh():
    ex = rgb.grid_mesh(); black_patch(ex, (0.3, 0.2, -0.2))
    return spectral(ex)


def generic():
    ex = rgb.generic()
    tri = rgb.scenes.synthetic_triangles(3, 33, 0.3) * 200.0 + np.array([278.0, 270.0, -280.0])[None, None, :]
    ex.scene.add_mesh(tri, rgb.disney(0.0, 0.5, (0.0, 0.0, 0.0)))
    return spectral(ex)


def sky_only():
    """no emitter at all: PT_Spec's environment is the analytic sky (the image of shade_step_cases.env_only stays: it sets the feature word's bit, nothing reads it)"""
    ex = rgb.env_only(); black_patch(ex, (0.3, 0.2, -0.2))
    return spectral(ex)


SF = _native
# name: (constructor, feature word of the scene, instantiations of k_shade_spec it runs on)
SCENES = {
    "grid_sphere": (grid_sphere, SF.SF_LIGHT_SPHERE, (SF.SF_LIGHT_SPHERE, SF.SF_ALL)),
    "grid_mesh": (grid_mesh, SF.SF_LIGHT_TRI, (SF.SF_LIGHT_TRI, SF.SF_ALL)),
    "generic": (generic, SF.SF_GLASS | SF.SF_ENV | SF.SF_LIGHT_TRI | SF.SF_LIGHT_SPHERE | SF.SF_LIGHT_SPOT_LASER, (SF.SF_ALL,)),
    "sky_only": (sky_only, SF.SF_ENV | SF.SF_NO_LIGHT, (SF.SF_ALL,)),
}


def host_scene(name, build_table=oracle_api.spec_table_build):
    """the scene packed on the host with its camera and spectral tables (no device unless build_table is a context's), and its oracle with the tree built and
    the same tables.  build_table: the oracle's generator of the RGB -> spectrum table on the CPU; a context's spec_table_build on the GPU (bit-identical:
    tests/test_gpu_spectral.py)"""
    ex = SCENES[name][0]()
    rgb.common.host_only(ex)
    ex.integrator.setup_data_cpu()
    ex.integrator.setup_tables(build_table)
    orc = oracle_api.OracleScene(ex.scene, ex.cam)
    assert orc.lbvh_build() == ex.scene.primitive_count - 1
    orc.set_spectral(ex.integrator.tables())
    return ex, orc


# ---- rows ---------------------------------------------------------------------------------------------------------------------
SPECIAL = rgb.SPECIAL


def spec_state(n, rng):
    """(head[n, 5] uint32, state[n, 8] float32): seed, pixel, frame as shade_step_cases.path_state draws them (so that the hero wavelength covers [360, 460)),
    bounce, last_bounce for PT_Spec's depth / throughout4, radiance4 with the SPECIAL values planted per channel, rows whose channels 0..2 of the throughput are 0
    while channel 3 is not and the reverse, and rows with a NaN in exactly one of the channels 0, 1, 2 (the continuation test looks at those three through maxf)"""
    head, _, _ = rgb.path_state(n, rng)
    head[:, 3] = np.arange(n) % MAX_DEPTH
    head[:, 4] = head[:, 3] == MAX_DEPTH - 1
    st = np.zeros((n, 8), np.float32)
    st[:, 0:4] = rng.uniform(0.0, 1.5, (n, 4))
    st[:, 4:8] = rng.uniform(0.0, 3.0, (n, 4)) * (rng.rand(n, 1) < 0.7)
    for cols, frac in ((slice(0, 4), 0.15), (slice(4, 8), 0.03)):
        sel = np.where(rng.rand(n) < frac)[0]
        block = st[:, cols]
        block[sel, rng.randint(0, 4, sel.size)] = SPECIAL[rng.randint(0, SPECIAL.size, sel.size)]
        st[:, cols] = block
    kind = rng.rand(n)
    only3 = kind < 0.03                              # channels 0..2 zero (either sign), channel 3 alive
    st[only3, 0:3] = np.where(rng.rand(int(only3.sum()), 3) < 0.5, 0.0, -0.0)
    st[only3, 3] = rng.uniform(0.1, 1.5, int(only3.sum()))
    no3 = (kind >= 0.03) & (kind < 0.06)             # channel 3 zero, channels 0..2 alive
    st[no3, 0:3] = rng.uniform(0.1, 1.5, (int(no3.sum()), 3))
    st[no3, 3] = 0.0
    one_nan = np.where((kind >= 0.06) & (kind < 0.10))[0]      # NaN in exactly one of the channels 0, 1, 2; the two others positive, zero or negative
    st[one_nan, 0:4] = rng.choice(np.array([0.0, -0.0, 0.7, -0.3, 1.0e-42], np.float32), (one_nan.size, 4))
    st[one_nan, rng.randint(0, 3, one_nan.size)] = np.nan
    return head, st


def respec(rows, rng):
    """rows built by the helpers of shade_step_cases.py (words 0..14 are what this layout has too) with the spectral head and state in words 0..4 and 15..22"""
    rows = np.ascontiguousarray(rows[:, :IN_WORDS]).copy()
    head, st = spec_state(rows.shape[0], rng)
    rows[:, 0:5] = head
    rows.view(np.float32)[:, 15:23] = st
    return rows


def real_hit_rows(ex, orc, rng, n_second=12000):
    first = respec(rgb.rows_from_rays(orc, rgb.random_and_bundled_rays(ex, rng), rng), rng)
    # second-bounce rays: the continuation the oracle's spectral step gives the first hits with a camera path's state (they start at offset_ray points)
    plain = first.copy()
    plain.view(np.float32)[:, 15:19] = 1.0; plain.view(np.float32)[:, 19:23] = 0.0; plain[:, 3] = 0; plain[:, 4] = 0
    step = orc.kat_shade_spec_step(plain)
    go = np.where(step.view(np.int32)[:, 5] == 1)[0][:n_second]
    second = respec(rgb.rows_from_rays(orc, np.ascontiguousarray(step[go, 6:12]), rng), rng)
    return np.concatenate([first, second], axis=0)


def emitter_edge_rows(ex, orc, rng, per_prim=100):
    """hits on every surface emitter with the zero vector as direction: fCosTheta = dot(direction, normal) is a sum of products with 0, exactly +-0 whatever the
    normal -- the arm `fCosTheta < 0` must not take --, at t = 1, tiny and huge, on the corners, an edge and the inside of the primitive"""
    sc = ex.scene
    light = np.where(sc.material_np[sc.primitive_np[:, 2], 0] == SCD.MAT_LIGHT)[0]
    light = [int(p) for p in light if sc.primitive_np[p, 0] == SCD.PRIMITIVE_TRI or int(sc.shape_np[sc.primitive_np[p, 1], 0]) == SCD.SHPAE_SPHERE]
    n = len(light) * per_prim
    if n == 0:
        return np.zeros((0, IN_WORDS), np.uint32)
    prim = np.repeat(np.asarray(light, np.int32), per_prim)
    d = np.zeros((n, 3), np.float32)
    d[1::4] = -0.0                                                       # (+0, +0, +0) and (-0, -0, -0) and mixed
    d[2::4, 1] = -0.0
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    t = rng.choice(np.array([1.0, 1.0e-30, 1.0e-3, 9.9e5], np.float32), n)
    u = rng.choice(np.array([0.0, 0.25, 1.0 / 3.0, 1.0], np.float32), n)
    v = np.where(u == 1.0, 0.0, rng.choice(np.array([0.0, 0.25, 1.0 / 3.0], np.float32), n)).astype(np.float32)
    head, st = spec_state(n, rng)
    rows = np.zeros((n, IN_WORDS), np.uint32)
    f = rows.view(np.float32)
    rows[:, 0:5] = head
    f[:, 5:8] = o; f[:, 8:11] = d; f[:, 11] = t; f[:, 12] = u; f[:, 13] = v
    rows[:, 14] = prim.view(np.uint32)
    f[:, 15:23] = st
    return rows


def sun_rows(ex, rng, per_direction=150):
    """misses along the sun direction itself, its float neighbours on both sides in every component, and the direction a rounding longer and shorter: the dot
    product with sun_dir is then 1, just below, or above 1 (acos of it NaN); the zenith, the horizon, below it and the zero vector come with miss_rows"""
    sun = ex.integrator.sky.sun_dir_np[0].astype(np.float32)
    dirs = [sun.copy(), -sun, sun * np.float32(1.0 + 2.0 ** -22), sun * np.float32(1.0 - 2.0 ** -22), sun * np.float32(1.0e3), sun * np.float32(1.0e-3)]
    for k in range(3):
        for toward in (np.inf, -np.inf):
            d = sun.copy(); d[k] = np.nextafter(d[k], np.float32(toward)); dirs.append(d)
    d = np.repeat(np.asarray(dirs, np.float32), per_direction, axis=0)
    n = d.shape[0]
    head, st = spec_state(n, rng)
    rows = np.zeros((n, IN_WORDS), np.uint32)
    f = rows.view(np.float32)
    rows[:, 0:5] = head
    f[:, 5:8] = rng.uniform(-2.0, 2.0, (n, 3)); f[:, 8:11] = d
    f[:, 11] = rng.choice(np.array([1.0e6, 2.0e6, np.inf, np.nan, 3.0e38], np.float32), n)
    rows[:, 14] = 0xffffffff
    f[:, 15:23] = st
    return rows


_cache = {}


def build(name, seed=2024, build_table=oracle_api.spec_table_build):
    """(ex, orc, rows[n, 23] uint32) for one scene; cached per process"""
    key = (name, seed)
    if key not in _cache:
        ex, orc = host_scene(name, build_table)
        rng = np.random.RandomState(seed)
        nprim = ex.scene.primitive_count
        synthetic = respec(rgb.synthetic_hit_rows(ex, orc, rng, repeats=max(1, 60000 // (nprim * 120))), rng)
        rows = np.concatenate([real_hit_rows(ex, orc, rng), synthetic, emitter_edge_rows(ex, orc, rng), respec(rgb.miss_rows(rng), rng), sun_rows(ex, rng)], axis=0)
        _cache[key] = (ex, orc, np.ascontiguousarray(rows))
    return _cache[key]


def hero_lambda(orc, rows):
    """the hero wavelength of every row, as the step computes it (float32)"""
    f = np.float32
    r = np.array([orc.L.orc_kat_rand(int(a), int(b), int(c), TM_DIM_SPEC_LAMBDA) for a, b, c in rows[:, 0:3]], f)
    return (f(360.0) + f(100.0) * r).astype(f)


def describe(rows, out_want, k, ex):
    """one line about row k for a failure report: branch word, material row, hit record"""
    f = rows.view(np.float32)
    br = int(out_want.view(np.uint32)[k, BRANCH_WORD]) if out_want.shape[1] > BRANCH_WORD else 0
    names = "+".join(n for n, b in oracle_api.SSB.items() if br & b) or "-"
    prim = int(rows.view(np.int32)[k, 14])
    mat = ex.scene.material_np[ex.scene.primitive_np[prim, 2]].tolist() if (f[k, 11] < INF_VALUE and 0 <= prim < ex.scene.primitive_count) else None
    return "row %d branch %s prim %d t %r uv (%r, %r) dir %s head %s state %s material %s" % (
        k, names, prim, float(f[k, 11]), float(f[k, 12]), float(f[k, 13]), f[k, 8:11].tolist(), rows[k, 0:5].tolist(), f[k, 15:23].tolist(), mat)


def first_differences(got, want, rows, ex, limit=8):
    """[] if the 29 words agree on every row (integers equal, floats bit-identical, NaN exactly where `want` has NaN); else a report of the first rows"""
    gi, wi = got.view(np.uint32)[:, :OUT_WORDS], want.view(np.uint32)[:, :OUT_WORDS]
    eq = gi == wi
    fcols = np.zeros(OUT_WORDS, bool)
    for _, first, words, is_float in OUT_FIELDS:
        if is_float:
            fcols[first:first + words] = True
    both_nan = np.isnan(got[:, :OUT_WORDS]) & np.isnan(want[:, :OUT_WORDS]) & fcols[None, :]
    bad = ~(eq | both_nan)
    report = []
    for k in np.where(bad.any(axis=1))[0][:limit]:
        fields = [name for name, first, words, _ in OUT_FIELDS if bad[k, first:first + words].any()]
        detail = "; ".join("%s got %s want %s" % (name, got[k, first:first + words].tolist() if fl else gi[k, first:first + words].view(np.int32).tolist(),
                                                   want[k, first:first + words].tolist() if fl else wi[k, first:first + words].view(np.int32).tolist())
                           for name, first, words, fl in OUT_FIELDS if name in fields)
        report.append(describe(rows, want, int(k), ex) + " :: " + detail)
    if report:
        report.insert(0, "%d of %d rows differ" % (int(bad.any(axis=1).sum()), got.shape[0]))
    return report
