"""The per-pixel bound on BDPT films (tests/bdpt_bound_expected.py) and the oracle's contribution record it is made from, held to the oracle alone (CPU):
the record is complete and in order; the oracle's own film, other summation orders and a pairwise tree lie inside the bound; the cases where at most two
contributions meet are the same bits in every order; a contribution lost, doubled or moved to the next pixel is outside it; and the cases
tests/test_gpu_bdpt_bound.py holds the device to exercise what they are there for (every connection strategy, long and short sums, hardly a pixel excluded)."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import bdpt_bound_expected as bb
import oracle_api as oa
from common import cornell_glass_wall, duplicate_code_scene, host_only, same_bits, spot_laser_scene
from test_film_shapes import make, oracle

SEED = 7
# kind: cornell / veach / prism through test_film_shapes.make; glass, spot_laser, duplicates and spec_spot_laser are built below.  scale: the camera's distance
# in scene diagonals; the two films of a handful of pixels look from inside the box (as test_film_shapes.ROWS does for its narrow films), where every
# direction meets a wall.
Case = namedtuple("Case", "name kind W H frames scale spec seed", defaults=(SEED,))
CASES = [
    Case("cornell_24x20", "cornell", 24, 20, 3, 0.8, False),
    Case("cornell_13x7", "cornell", 13, 7, 3, 0.8, False),                    # 91 items a frame: ragged against 64-lane waves, 128-item resolve groups, 256-thread connect blocks
    Case("cornell_3x2x40", "cornell", 3, 2, 40, 0.4, False),                  # 240 items over six targets: the splats of neighbouring items meet, runs cross item boundaries
    # From eight diagonals away the whole box lies in the centre pixel: no eye ray but that pixel's meets anything, and every light-tracing splat of all 49 items of
    # a frame lands on it -- the only way to a run of more than 32 equal targets in k_bd_resolve's list (an item has at most 20 connections, and its e >= 2 ones go
    # to its own pixel).  ONE_TARGET exempts it from the short-sum guard below: nothing but that pixel is lit.
    Case("cornell_far_7x7", "cornell", 7, 7, 4, 8.0, False),
    Case("cornell_1x1", "cornell", 1, 1, 8, 0.4, False, 9),                  # (seed 9: three of its 24 sums are of eight or more; seed 7 has none above seven)
    Case("veach_24x20", "veach", 24, 20, 2, 0.8, False),                      # glass, smooth normals, two emissive meshes
    Case("glass_wall_16x12", "glass", 16, 12, 3, 0.8, False),
    Case("spot_laser_16x12", "spot_laser", 16, 12, 3, 0.8, False),
    # 40 clusters of small triangles in a cube of side 2 (the device test pages the traversal stack on them: trace_lds_depth 12).  Nearly every ray misses:
    # from 0.3 diagonals, with seed 2, 87 of 9 216 sums get anything and the longest is of three.  The case is there for the stack; SPARSE exempts it from
    # the long-sum guard below, which no film of this scene meets (seeds 1 .. 7, 16 x 12 .. 48 x 48, 0.15 .. 0.8 diagonals tried: at most four).
    Case("duplicates_32x32", "duplicates", 32, 32, 3, 0.3, False, 2),
    Case("prism_16x12", "prism", 16, 12, 3, 0.8, True),
    Case("spec_spot_laser_16x12", "spec_spot_laser", 16, 12, 3, 0.8, True),
    # The green wall of the box emits (and is on the light list): from 0.4 diagonals most eye sub-paths of every length end on an emitter, which is what the l == 0
    # strategies (k_bd_emitted) need -- the cases above give (6, 0) two contributions and (7, 0) ten.  tests/bdpt_records_expected.py counts what these add.
    Case("emitter_wall_24x20", "emitter_wall", 24, 20, 20, 0.4, False),
    Case("spec_emitter_wall_24x20", "spec_emitter_wall", 24, 20, 20, 0.4, True),
    # a sphere emitter inside the box: the l == 1 connections that end on one (the cases above reach a sphere 37 times in RGB)
    Case("sphere_light_16x12", "sphere_light", 16, 12, 4, 0.8, False),
    Case("spec_sphere_light_16x12", "spec_sphere_light", 16, 12, 4, 0.8, True),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
TEETH = ("cornell_24x20", "veach_24x20")
SPARSE = ("duplicates_32x32",)
ONE_TARGET = ("cornell_far_7x7",)


def emitter_wall(ex, emission=(1.5, 4.0, 1.5)):
    """the box's green wall becomes an emitter AFTER add_obj has read it as a surface: the material's row, and its triangles onto the light list where add_obj would have
    put them (in primitive order)"""
    from ti_raytrace_amd import SceneData as SCD
    sc = ex.scene
    (index,) = [k for k, m in enumerate(sc.material_cpu) if m.type == SCD.MAT_DISNEY and tuple(np.round(m.color[:3], 3)) == (0.0, 1.0, 0.0)]
    sc.material_cpu[index].type = SCD.MAT_LIGHT
    sc.material_cpu[index].setColor(list(emission))
    for first, ntri, mat, _ in sc._prim_mat:
        if mat == index:
            sc.light_cpu.extend(range(first, first + ntri)); sc.light_count += ntri
    sc.light_cpu.sort()
    assert sc.light_count == len(sc.light_cpu) == len(set(sc.light_cpu)) and sc.light_count > 2


@functools.lru_cache(maxsize=None)
def _spec_table(res, xyz, d65):
    return oa.spec_table_build(res, np.frombuffer(xyz, np.float32), np.frombuffer(d65, np.float32))


def spec_table(res, xyz, d65):
    """the Rgb2Spec table from the oracle, built once for all the spectral cases of a session (it depends on the observer and the illuminant alone)"""
    xyz, d65 = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(d65, np.float32)
    scale, coeff = _spec_table(int(res), xyz.tobytes(), d65.tobytes())
    return scale.copy(), coeff.copy()


def build(case, device_id=None):
    """(example, oracle scene) of a case, packed on the host or built on a device"""
    from ti_raytrace_amd import BDPT_RGB, BDPT_SPEC
    W, H = case.W, case.H
    if case.kind in ("cornell", "veach", "prism"):
        ex = make(case.kind, W, H, case.scale, device_id=device_id, integrator="bdpt")
        return ex, oracle(ex, case.kind)
    if case.kind == "glass":
        ex = cornell_glass_wall(W, H, device_id=device_id, integrator="bdpt")
    elif case.kind == "spot_laser":
        ex = spot_laser_scene(W, H, device_id=device_id, integrator="bdpt")
    elif case.kind == "duplicates":
        ex = duplicate_code_scene(W=W, H=H, device_id=device_id)
        ex.integrator = BDPT_RGB.BDPT(W, H, ex.cam, ex.scene, 64)
    elif case.kind == "spec_spot_laser":
        ex = spot_laser_scene(W, H, device_id=device_id)
        ex.integrator = BDPT_SPEC.BDPT(W, H, ex.cam, ex.scene, 64)
    elif case.kind in ("emitter_wall", "spec_emitter_wall", "sphere_light", "spec_sphere_light"):
        from ti_raytrace_amd import scenes
        ex = scenes.cornell_box(W, H, 4, device_id=device_id)
        if case.kind.endswith("sphere_light"):
            ex.add_sphere_light(pos=(278.0, 300.0, -280.0), radius=60.0, emission=30.0)
        else:
            emitter_wall(ex)
        ex.integrator = (BDPT_SPEC if case.spec else BDPT_RGB).BDPT(W, H, ex.cam, ex.scene, 64)
    else:
        raise ValueError(case.kind)
    if device_id is None:
        ex.scene.setup_data_cpu(); ex.integrator.setup_data_cpu()
        if case.spec:
            ex.integrator.setup_tables(spec_table)
    else:
        ex.build_scene()
        ex.scene.total_area()
    ex.frame_camera(case.scale)
    o = oa.OracleScene(ex.scene, ex.cam)
    o.lbvh_build()
    if case.spec:
        o.set_spectral(ex.integrator.tables())
    return ex, o


def oracle_render(o, ex, case, frame_begin=0, frames=None, record=True, **kw):
    frames = case.frames if frames is None else frames
    if case.spec:
        return o.bdpt_spec_render(ex.cam, case.W, case.H, frame_begin, frames, seed=case.seed, stack_size=1024, record=record, **kw)
    return o.bdpt_render(ex.cam, case.W, case.H, frame_begin, frames, seed=case.seed, record=record, **kw)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """(film, stats, records) of a case from the oracle, computed once and shared (nothing may write to them)"""
    case = BY_NAME[name]
    ex, o = build(case)
    film, st, _, rec = oracle_render(o, ex, case)
    film.setflags(write=False); rec.setflags(write=False)
    return film, st, rec


def pairwise_film(records, W, H, frames):
    """the film when every (frame, pixel)'s contributions are summed as a balanced binary tree in fp32"""
    rec = records[np.argsort(records["frame"].astype(np.int64) * (W * H) + records["q"], kind="stable")]
    key = rec["frame"].astype(np.int64) * (W * H) + rec["q"]
    val = rec["r"].astype(np.float32)
    first = np.r_[True, key[1:] != key[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(key)), 0))
    rank = np.arange(len(key)) - start
    with np.errstate(invalid="ignore", over="ignore"):
        while len(rank) and rank.max() > 0:
            odd = np.nonzero(rank & 1)[0]
            val[odd - 1] += val[odd]                   # (an odd rank's left neighbour has the even rank before it and the same key)
            keep = (rank & 1) == 0
            val, key, rank = val[keep], key[keep], rank[keep] >> 1
    rad = np.zeros((frames, W * H, 3), np.float32)
    rad[key // (W * H), key % (W * H)] = val
    hdr = np.zeros((W, H, 3), np.float32)
    for f in range(frames):
        hdr = bb.blend(hdr, rad[f].reshape(W, H, 3), f)
    return hdr


def shuffled(records, rng):
    """the records of every frame in a random order: a random order of the contributions to every pixel"""
    return np.argsort(records["frame"].astype(np.float64) + rng.random_sample(len(records)) * 0.5, kind="stable")


# ---- the record ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_IDS)
def test_the_recorder_changes_no_bit_and_the_record_is_complete_and_ordered(name):
    case = BY_NAME[name]
    W, H, frames = case.W, case.H, case.frames
    film, st, rec = recorded(name)
    ex, o = build(case)
    plain, pst, state = oracle_render(o, ex, case, record=False)
    assert same_bits(plain, film) and pst == st, "the film or the stats change with the recorder on"
    again, ast, _ = oracle_render(o, ex, case, record=False)          # (and a state that once recorded goes back to not recording: _bdpt turns it off)
    assert same_bits(again, film) and ast == st
    vfilm, vst, _, vrec, vex = oracle_render(o, ex, case, vertices=True)          # the vertex export (and the write masks it reads) only listens too
    assert same_bits(vfilm, film) and vst == st and vrec.tobytes() == rec.tobytes() and len(vex) == W * H * frames, "the film, the stats or the records change with the vertex export on"
    vfilm, vst, _, vex2 = oracle_render(o, ex, case, record=False, vertices=True)
    assert same_bits(vfilm, film) and vst == st and vex2.tobytes() == vex.tobytes()
    assert rec.dtype == oa.BD_RECORD and len(rec) > 0
    assert (np.diff(rec["frame"]) >= 0).all() and rec["frame"].min() == 0 and rec["frame"].max() == frames - 1
    for f in range(frames):
        assert (np.diff(rec["p"][rec["frame"] == f]) >= 0).all(), "records out of the oracle's pixel order"
    assert ((rec["e"] >= 1) & (rec["e"] <= 7) & (rec["l"] >= 0) & (rec["l"] <= 6) & (rec["e"] + rec["l"] - 2 <= 5) & (rec["e"] + rec["l"] >= 2)).all()
    assert ((rec["e"] == 1) | (rec["p"] == rec["q"])).all(), "only the light-tracing strategy (e == 1) lands on another pixel"
    # summed one after the other in fp32, in the record's order, the record IS the oracle's radiance plane of every frame and its film
    got, rad = bb.replay(rec, W, H, frames)
    assert same_bits(got, film), "%d pixel-channels differ" % int((got.view(np.uint32) != film.view(np.uint32)).sum())
    hdr, state = np.zeros((W, H, 3), np.float32), None
    for f in range(frames):               # frame by frame with the state carried over: every frame's plane through the film it leaves
        hdr, _, state, r1 = oracle_render(o, ex, case, frame_begin=f, frames=1, hdr=hdr, state=state)
        assert same_bits(r1["r"], rec["r"][rec["frame"] == f]) and np.array_equal(r1["q"], rec["q"][rec["frame"] == f])
        assert same_bits(hdr, bb.replay(rec[rec["frame"] <= f], W, H, f + 1)[0]), f
    assert same_bits(hdr, film)


def test_a_buffer_too_small_is_not_overrun_and_the_count_is_what_was_needed():
    case = BY_NAME["cornell_13x7"]
    film, st, rec = recorded(case.name)
    ex, o = build(case)
    cap = len(rec) // 3
    buf = np.zeros(cap + 4, oa.BD_RECORD)
    buf["frame"][cap:] = -77
    state = o.L.orc_bdpt_create(case.W, case.H, np.ascontiguousarray(ex.cam.view_np[0].reshape(-1), np.float32))
    o.L.orc_bdpt_record(state, buf.ctypes.data, cap)
    hdr, _, _ = o.bdpt_render(ex.cam, case.W, case.H, 0, case.frames, seed=case.seed, state=state)
    assert o.L.orc_bdpt_record_count(state) == len(rec)
    assert (buf["frame"][cap:] == -77).all() and np.array_equal(buf[:cap], rec[:cap]) and same_bits(hdr, film)
    o.L.orc_bdpt_record(state, None, 0)                    # no buffer: counted only
    o.bdpt_render(ex.cam, case.W, case.H, 0, 1, seed=case.seed, state=state)
    assert o.L.orc_bdpt_record_count(state) == int((rec["frame"] == 0).sum())
    o.L.orc_bdpt_destroy(state)


# ---- the bound ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_IDS)
def test_the_oracle_and_every_other_order_lie_inside_the_bound(name):
    case = BY_NAME[name]
    W, H, frames = case.W, case.H, case.frames
    film, _, rec = recorded(name)
    rng = np.random.RandomState(11)
    worst = 0.0
    for k in range(1, frames + 1):             # after every frame; after the first one the n <= 2 values are the oracle's bits in any order
        part = rec[rec["frame"] < k]
        own, _ = bb.replay(part, W, H, k)
        films = [own, pairwise_film(part, W, H, k)]
        if k in (1, frames):
            films += [bb.replay(part, W, H, k, order=shuffled(part, rng))[0] for _ in range(20)]
        for i, got in enumerate(films):
            info = bb.assert_film_within(got, part, W, H, k, what="%s, order %d" % (name, i))
            worst = max(worst, info["ratio"])
    assert same_bits(own, film)
    print("%s: largest error / bound %.3f, bound / value (median) %.2e" % (name, worst, info["rel_bound"]))
    # what the bound is as a share of a pixel's value: every frame of the running mean adds at most 3 u, the sums gamma(n - 1) with the longest n at the most
    longest = int(bb.planes(rec, W, H, frames)[2].max())
    assert info["rel_bound"] < (3 * frames + max(longest, 20)) * bb.U, "the typical bound is wider than its own terms explain"


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_cases_exercise_what_they_are_there_for(name):
    case = BY_NAME[name]
    W, H, frames = case.W, case.H, case.frames
    film, st, rec = recorded(name)
    R, A, n, bad = bb.planes(rec, W, H, frames)
    Hx, E, exact0, excluded = bb.film_bound(rec, W, H, frames)
    lit = n > 0
    short = float((n[lit] <= 2).mean())
    print("%s: %d records, %d not zero; lit (frame, pixel-channel)s %d, n <= 2: %.1f %%, n >= 8: %d, largest n %d; excluded %d of %d; negative values %d"
          % (name, len(rec), int((rec["r"] != 0).any(axis=1).sum()), int(lit.sum()), 100 * short, int((n >= 8).sum()), int(n.max()), int(excluded.sum()), excluded.size,
             int((rec["r"] < 0).sum())))
    assert lit.sum() > 0
    if name in SPARSE:
        assert n.max() >= 3, "not even a sum of three"
    else:
        assert (n >= 8).sum() > 0, "no long sum"
    if name in ONE_TARGET:
        centre = (case.W // 2) * case.H + case.H // 2
        assert (rec["q"][(rec["r"] != 0).any(axis=1)] == centre).all(), "a contribution beside the centre pixel"
        assert (n.reshape(frames, -1).max(axis=1) >= 40).any(), "no frame whose contributions can make a run of more than 32"
    else:
        assert short >= 0.30, "too few sums of at most two contributions: %.3f" % short
    assert excluded.mean() <= 0.01, "more than 1 %% of the pixel-channels are excluded"
    if name in ("cornell_24x20", "veach_24x20"):
        assert not excluded.any()
    assert st["rays_shadow"] > 0 and st["rays_closest"] > 0
    if name == "cornell_24x20":
        nz = rec[(rec["r"] != 0).any(axis=1)]
        pairs = set(zip(nz["e"].tolist(), nz["l"].tolist()))
        carrying = {(e, l) for e in range(1, 8) for l in range(1, 7) if not (e == 1 and l == 1) and 0 <= e + l - 2 <= 5}
        assert len(carrying) == 20 and carrying <= pairs, "ray-carrying pairs without a contribution: %s" % sorted(carrying - pairs)
        assert len({e for e, l in pairs if l == 0}) >= 3, sorted(p for p in pairs if p[1] == 0)


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TEETH)
def test_a_contribution_lost_doubled_or_moved_is_outside_the_bound(name):
    """frame 0, every contribution that is not zero, one at a time: the film summed in the oracle's order without it, with it twice, and with it on the next pixel
    instead, checked as the device's film is (bits where n <= 2, the interval elsewhere) -- on the pixels the change touches, the others being the oracle's."""
    case = BY_NAME[name]
    W, H = case.W, case.H
    _, _, rec = recorded(name)
    rec = rec[rec["frame"] == 0]
    rec = rec[(rec["r"] != 0).any(axis=1)]
    Hx, E, exact0, excluded = (a.reshape(W * H, 3) for a in bb.film_bound(rec, W, H, 1))
    want = bb.replay(rec, W, H, 1)[0].reshape(W * H, 3)
    val = rec["r"].astype(np.float32)
    where = {}
    for k, q in enumerate(rec["q"].tolist()):
        where.setdefault(q, []).append(k)

    def total(ks):
        s = np.zeros(3, np.float32)
        for k in ks:
            s = s + val[k]
        return s

    def flagged(changes):
        return any(bb.violations(total(ks), want[q], Hx[q], E[q], exact0[q], excluded[q]).any() for q, ks in changes)

    hits = {"lost": 0, "doubled": 0, "moved": 0}
    for k, q in enumerate(rec["q"].tolist()):
        ks = where[q]
        at = ks.index(k)
        without = ks[:at] + ks[at + 1:]
        q2 = q + 1 if q + 1 < W * H else q - 1
        there = where.get(q2, [])
        hits["lost"] += flagged([(q, without)])
        hits["doubled"] += flagged([(q, ks[:at] + [k, k] + ks[at + 1:])])
        hits["moved"] += flagged([(q, without), (q2, sorted(there + [k]))])
    share = {m: hits[m] / len(rec) for m in hits}
    print("%s frame 0, %d contributions: flagged %s" % (name, len(rec), {m: "%.1f %%" % (100 * s) for m, s in share.items()}))
    assert not flagged([(q, ks) for q, ks in where.items()]), "the unchanged list is flagged"
    assert min(share.values()) >= 0.95, share
