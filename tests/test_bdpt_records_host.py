"""tests/bdpt_records_expected.py held to the oracle alone (CPU): the oracle's own list and vertex export pass their comparisons, the export changes no bit and does
not depend on how the frames are cut into calls, single planted defects are each rejected -- with a note, per defect, of whether the film's rounding bound
(bdpt_bound_expected.assert_film_within) would have seen it --, and the cases together meet the coverage floors tests/test_gpu_bdpt_records.py asserts on the
device, so that they are a condition chosen here and not a measurement made there.

(The device's own too-small record buffer is exercised where there is a device: tests/test_gpu_bdpt_records.py.)"""
import functools

import numpy as np
import pytest

import bdpt_bound_expected as bb
import bdpt_records_expected as br
import oracle_api as oa
from test_bdpt_bound_host import BY_NAME, CASE_IDS, CASES, build, oracle_render


@functools.lru_cache(maxsize=None)
def exported(name):
    """(scene example, records, vertex export) of a case from the oracle, computed once and shared (nothing may write to them)"""
    case = BY_NAME[name]
    ex, o = build(case)
    _, _, _, rec, vex = oracle_render(o, ex, case, vertices=True)
    rec.setflags(write=False); vex.setflags(write=False)
    return ex, rec, vex


def device_like(rec, rng=None, zeros=0.25):
    """what a correct device would write: the non-zero records and some of the zero ones (the connections whose ray met its target and still gave nothing), in any order"""
    rng = rng or np.random.RandomState(5)
    keep = br.nonzero(rec) | (rng.random_sample(len(rec)) < zeros)
    out = rec[keep].copy()
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_oracles_own_list_and_vertices_pass_and_do_not_depend_on_the_calls(name):
    case = BY_NAME[name]
    ex, rec, vex = exported(name)
    nz = br.compare_records(device_like(rec), rec, case.W, case.H, name)
    assert len(nz) == int(br.nonzero(rec).sum()) > 0
    assert len(br.compare_records(rec.copy(), rec, case.W, case.H, name)) == len(nz)
    assert len(vex) == case.W * case.H * case.frames and (np.diff(vex["frame"]) >= 0).all()
    rows, verts = br.as_device_vertices(vex)
    assert br.compare_vertices(rows, verts, vex, name) > 13 * len(vex)
    # depths as the loops bound them, the tail slot is a surface's, and a slot below the depth has been stored in this frame, position and all (slot 0 aside: no prim)
    assert ((vex["eye_depth"] >= 1) & (vex["eye_depth"] <= 7) & (vex["light_depth"] >= 1) & (vex["light_depth"] <= 6)).all()
    act = br.active_slots(vex["eye_depth"], vex["tail"], vex["light_depth"])
    assert ((vex["mask"] & oa.BVF["pos"]) != 0)[act].all() and (vex["v"]["type"][act] != 0).all()
    tail = vex["tail"] != 0
    assert (vex["v"]["type"][tail, vex["eye_depth"][tail]] == br.VERTEX_SURFACE).all()
    # frame by frame with the state carried: the same export
    ex2, o = build(case)
    hdr, state = None, None
    for f in range(min(case.frames, 4)):
        hdr, _, state, v1 = oracle_render(o, ex2, case, frame_begin=f, frames=1, hdr=hdr, state=state, record=False, vertices=True)
        assert v1.tobytes() == vex[vex["frame"] == f].tobytes(), f
    o.L.orc_bdpt_destroy(state)


def film_sees(full, rec, case):
    """would assert_film_within have rejected the film that the oracle's own order makes of the changed list?"""
    W, H, frames = case.W, case.H, case.frames
    try:
        bb.assert_film_within(bb.replay(full, W, H, frames)[0], rec, W, H, frames)
    except AssertionError:
        return True
    return False


def ulp(x):
    return (x.view(np.uint32) ^ np.uint32(1)).view(np.float32)


def plant(kind, rec, i, W, H):
    """the oracle's full list with one defect at record i"""
    full = rec.copy()
    if kind == "dropped":
        full = np.delete(full, i)
    elif kind == "doubled":
        full = np.insert(full, i, full[i])
    elif kind == "moved":
        full["q"][i] = full["q"][i] + 1 if full["q"][i] + 1 < W * H else full["q"][i] - 1
    elif kind == "e_l_swapped":
        full["e"][i], full["l"][i] = rec["l"][i], rec["e"][i]
    elif kind == "one_ulp":
        ch = int(np.argmax(np.abs(full["r"][i])))
        full["r"][i, ch:ch + 1] = ulp(full["r"][i, ch:ch + 1].copy())
    elif kind == "zero_given_a_value":
        full["r"][i] = np.float32(1.0e-3)
    else:
        raise ValueError(kind)
    return full


RECORD_DEFECTS = ("dropped", "doubled", "moved", "e_l_swapped", "one_ulp", "zero_given_a_value")


@pytest.mark.parametrize("name", ["cornell_24x20", "spec_spot_laser_16x12"])
def test_a_single_planted_defect_in_the_records_is_rejected(name):
    """Per kind of defect, at 24 records spread over the list and at the 8 dimmest non-zero ones (against the bound of the pixel they land on): the record comparison
    rejects every one.  Printed beside it: how many of them the film's rounding bound would have seen -- a dim contribution dropped or doubled, any single ulp, and
    an (e, l) swap that moves nothing are invisible to it by construction."""
    case = BY_NAME[name]
    W, H, frames = case.W, case.H, case.frames
    ex, rec, vex = exported(name)
    nz = np.nonzero(br.nonzero(rec))[0]
    zero = np.nonzero(~br.nonzero(rec))[0]
    _, E, _, _ = bb.film_bound(rec, W, H, frames)
    with np.errstate(invalid="ignore"):
        visible = np.nanmax(np.abs(rec["r"][nz]) / E.reshape(-1, 3)[rec["q"][nz]], axis=1)
    spread = nz[np.linspace(0, len(nz) - 1, 24).astype(int)]
    dimmest = nz[np.argsort(visible)[:8]]
    assert not film_sees(rec, rec, case)
    for kind in RECORD_DEFECTS:
        where = zero[np.linspace(0, len(zero) - 1, 32).astype(int)] if kind == "zero_given_a_value" else np.r_[spread, dimmest]
        if kind == "e_l_swapped":
            where = where[rec["e"][where] != rec["l"][where]]              # (a swap of equal numbers is no defect; the film does not know strategies: no swap changes a sum)
        seen = 0
        for i in where:
            full = plant(kind, rec, int(i), W, H)
            dev = full[br.nonzero(full)]
            with pytest.raises(AssertionError):
                br.compare_records(dev, rec, W, H, "%s, %s at record %d" % (name, kind, i))
            seen += film_sees(full, rec, case)
        print("%s: %-20s rejected by the records %d / %d, seen by the film's bound %d / %d" % (name, kind, len(where), len(where), seen, len(where)))
        if kind in ("one_ulp", "e_l_swapped"):
            assert seen == 0, "the film's bound is not supposed to see a %s" % kind


@pytest.mark.parametrize("name", ["glass_wall_16x12", "emitter_wall_24x20"])
def test_a_single_planted_defect_in_the_vertices_is_rejected(name):
    """one field of one vertex off by one ulp (every field in turn), a depth off by one, the tail bit flipped, and `delta` flipped on an eye vertex that lies on an emitter
    (the one the oracle did not store in this frame: k_bd_delta's).  The film has no say here: a vertex shows in it only through the contributions it changes,
    and the `delta` of such a vertex decides whether its l == 1 connection is made at all and enters the MIS weights around it."""
    ex, rec, vex = exported(name)
    rows, verts = br.as_device_vertices(vex)
    br.compare_vertices(rows, verts, vex, name)
    act = br.active_slots(vex["eye_depth"], vex["tail"], vex["light_depth"])
    planted = 0
    for f in br.FIELDS:
        marked = act & ((vex["mask"] & oa.BVF[f]) != 0) if f != "delta" else act
        i, s = np.argwhere(marked)[len(np.argwhere(marked)) // 2]
        bad = verts.copy()
        if bad[f].dtype == np.float32:
            x = bad[f][i, s].reshape(-1)
            x[:1] = ulp(x[:1].copy())
            bad[f][i, s] = x.reshape(bad[f][i, s].shape)
        else:
            bad[f][i, s] += 1
        with pytest.raises(AssertionError):
            br.compare_vertices(rows, bad, vex, "%s, %s off at item %d slot %d" % (name, f, i, s))
        planted += 1
    on_emitter = np.argwhere(act[:, :7] & (vex["v"]["type"][:, :7] == br.VERTEX_LIGHT))
    assert len(on_emitter) > 0
    stale = [(i, s) for i, s in on_emitter if not vex["mask"][i, s] & oa.BVF["delta"]]
    assert len(stale) == len(on_emitter), "the oracle stores delta on an eye vertex that ended on an emitter"
    for i, s in stale[:: max(1, len(stale) // 8)]:
        bad = verts.copy()
        bad["delta"][i, s] ^= 1
        with pytest.raises(AssertionError):
            br.compare_vertices(rows, bad, vex, "%s, delta flipped at item %d slot %d" % (name, i, s))
        planted += 1
    for field in ("eye_depth", "light_depth", "tail"):
        bad = rows.copy()
        bad[field][len(bad) // 2] ^= 1
        with pytest.raises(AssertionError):
            br.compare_vertices(bad, verts, vex, "%s, %s changed" % (name, field))
        planted += 1
    print("%s: %d planted vertex defects, all rejected; %d eye vertices on an emitter, delta stored in this frame on none of them" % (name, planted, len(on_emitter)))


@pytest.mark.parametrize("spec", [False, True], ids=["rgb", "spec"])
def test_the_cases_meet_the_coverage_floors_in_the_oracle(spec):
    """what tests/test_gpu_bdpt_records.py asserts of the records matched on the device, of the oracle's own: the cases were chosen here, on the CPU, to meet it"""
    title = "BDPT_SPEC" if spec else "BDPT_RGB"
    strategies, eye, light, origin = {}, {}, {}, {}
    for c in CASES:
        if c.spec != spec:
            continue
        ex, rec, vex = exported(c.name)
        nz = rec[br.nonzero(rec)]
        br.add_counts(strategies, br.strategy_counts(nz))
        for total, part in zip((eye, light, origin), br.kind_counts(br.end_kinds(nz, vex, ex.scene, c.seed, c.spec))):
            br.add_counts(total, part)
    print(br.strategy_table(strategies, title))
    print(br.kind_table(eye, light, origin, title))
    br.assert_floors(strategies, eye, light, origin, title)
