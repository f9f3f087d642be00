"""Every contribution BDPT_RGB / BDPT_SPEC evaluates on the device, and every sub-path vertex it is made from, held to the oracle's BIT FOR BIT
(tests/bdpt_records_expected.py has the rules; tests/test_bdpt_records_host.py holds them to the oracle alone and shows which planted defects the film's
rounding bound of tests/test_gpu_bdpt_bound.py cannot see).  No tolerance anywhere; a NaN equals any NaN.

The device writes its contribution records through tirt_bdpt_record_enable (k_bd_resolve after bd_splat_target and BEFORE the pairwise pre-sum, k_bd_emitted for
l == 0) and hands out a batch's vertices through tirt_bdpt_vertices_download; the film is made by the same atomics as always and is held to its bound here too.
Every render runs under the 0xFF poison (option "bdpt_state_fill" 2): a vertex field the device failed to write cannot equal the oracle's by accident.

Cases: tests/test_bdpt_bound_host.py::CASES.  Among them, for k_bd_resolve's grouping: cornell_13x7 (91 items against 128-item groups), cornell_far_7x7 (every
splat of a frame on one pixel: runs of more than 32 lanes), cornell_1x1 (one item), cornell_3x2x40 (runs that cross item boundaries) -- the pre-sum must not
show in the records.

Coverage, asserted (test_every_strategy_and_every_kind_of_end_vertex_is_matched_at_least_100_times): over the RGB cases and again over the SPEC cases, the
non-zero records matched on the device number at least 100
  * for each of the 26 strategies (e, l) with 0 <= e + l - 2 <= 5 except (1, 1);
  * for each kind of eye end vertex eye[e - 1]: lens, Disney surface, emitter;
  * for each kind of light end vertex: none (l == 0), triangle emitter and sphere emitter (l == 1: the point the connection samples), Disney surface (l >= 2);
  * for each kind of emitter the light sub-path of an l >= 2 record began on: triangle, sphere, spot, laser.
Not asserted, because the oracle produces a non-zero record of the kind on no input: a GLASS end vertex at either end (delta: connect_path refuses it), and a
SPOT or a LASER as the light end of an l == 1 connection -- Scene.sample_li / sample_light may choose one, but the connection counts only if its shadow ray's
closest hit is the chosen primitive, and no ray ever hits a spot or a laser (SceneData.py:43-44; spot_laser_16x12 and spec_spot_laser_16x12 choose them in a
quarter of their l == 1 connections and none is non-zero).  They reach the film through the light sub-path alone, which the last table counts.

Wall time of this file on an MI355X: 2.8 s for its 34 tests, the slowest 0.3 s (tests/test_gpu_bdpt_bound.py beside it: 1.7 s for 17)."""
import functools

import numpy as np
import pytest

import bdpt_bound_expected as bb
import bdpt_records_expected as br
from ti_raytrace_amd._native import TirtError
from test_bdpt_bound_host import BY_NAME, CASE_IDS, CASES, oracle_render
from test_gpu_bdpt_bound import ONE_BATCH, Device

pytestmark = pytest.mark.gpu


def options(name):
    return (("trace_lds_depth", 12),) if name.startswith("duplicates") else ()


def with_vertices(d):
    """the oracle's vertex export of the whole case beside its record (which must not change for it)"""
    _, _, _, rec, d.vex = oracle_render(d.o, d.ex, d.case, vertices=True)
    assert rec.tobytes() == d.rec.tobytes()
    return d


@functools.lru_cache(maxsize=None)
def device(name):
    """one context per case for the tests that leave it as they found it (one batch, one lane, whole film)"""
    return with_vertices(Device(name, options=options(name)))


def record_run(d, frame_begin, frames, want, what):
    """render with the record on; the device's list against `want`; returns the oracle's non-zero records, all matched"""
    c = d.case
    d.ctx.bdpt_record_enable(c.W * c.H * frames * len(br.STRATEGIES))
    d.render(frame_begin, frames)
    got, need = d.ctx.bdpt_record_download()
    d.ctx.bdpt_record_enable(-1)
    assert need == len(got), (what, need, len(got))
    return br.compare_records(got, want, c.W, c.H, "%s %s" % (c.name, what))


def one_batch(d):
    d.ctx.set_option("bdpt_batch_items", ONE_BATCH); d.ctx.set_option("overlap_lanes", 1)
    d.ctx.film_clear(); d.ctx.stats_reset()


@functools.lru_cache(maxsize=None)
def matched_in_one_call(name):
    d = device(name)
    one_batch(d)
    nz = record_run(d, 0, d.case.frames, d.rec, "one call")
    d.check(d.case.frames, what="one call, record on")            # the film still goes through the atomics
    return nz


@pytest.mark.parametrize("name", CASE_IDS)
def test_device_records_are_the_oracles_frame_by_frame_and_in_one_call(gpu_ctx_ok, name):
    d = device(name)
    c, rec = d.case, d.rec
    one_batch(d)
    n = 0
    for f in range(c.frames):
        n += len(record_run(d, f, 1, rec[rec["frame"] == f], "frame %d" % f))
        d.check(f + 1, what="frame by frame, record on, frame %d" % f)
    nz = matched_in_one_call(name)
    assert n == len(nz) == int(br.nonzero(rec).sum())
    print("%s: %d oracle records, %d not zero, all matched; film within its bound with the record on" % (name, len(rec), len(nz)))


@pytest.mark.parametrize("name", ["cornell_24x20", "veach_24x20"])
def test_batches_bounded_rays_and_tiles_give_the_same_set(gpu_ctx_ok, name):
    d = Device(name)
    c, rec = d.case, d.rec
    d.ctx.set_option("bdpt_batch_items", c.W * c.H * 2); d.ctx.set_option("overlap_lanes", 4)         # batches of two frames
    d.ctx.film_clear()
    record_run(d, 0, c.frames, rec, "batches")
    d.check(c.frames, what="batches, record on")
    if c.frames > 2:
        with pytest.raises(TirtError):
            d.ctx.bdpt_vertices_download()                  # more than one batch: refused
    else:
        assert len(d.ctx.bdpt_vertices_download()[0]) == c.W * c.H * c.frames          # (veach: its two frames are one batch)
    one_batch(d)
    d.ctx.set_option("bdpt_bounded", 0)                     # connection rays as full closest-hit queries
    record_run(d, 0, c.frames, rec, "bdpt_bounded 0")
    d.check(c.frames, what="bdpt_bounded 0, record on")
    d.ctx.set_option("bdpt_bounded", 1)
    total = 0
    for rank in range(2):
        d.ctx.film_create(c.W, c.H, rank, 2, 64)
        with pytest.raises(TirtError):
            d.ctx.bdpt_vertices_download()                  # nothing rendered into this film
        own = bb.owned_records(rec, rank, 2, 64)
        total += len(own)
        d.ctx.film_clear()
        record_run(d, 0, c.frames, own, "rank %d of 2" % rank)
        d.check(c.frames, own, "rank %d of 2, record on" % rank)
    assert total == len(rec)


def test_a_record_buffer_too_small_is_not_overrun_and_the_count_is_what_was_needed(gpu_ctx_ok):
    d = device("cornell_13x7")
    c = d.case
    one_batch(d)
    full = int(br.nonzero(d.rec).sum())
    cap = full // 3
    d.ctx.bdpt_record_enable(cap)
    d.render(0, c.frames)
    buf = np.zeros(cap + 4, br.oa.BD_RECORD)
    buf["frame"][cap:] = -77
    got, need = d.ctx.bdpt_record_download(out=buf)           # (the host buffer has room for four more than the device kept)
    assert need >= full and len(got) == cap and (buf["frame"][cap:] == -77).all(), (need, full, len(got), cap)
    few, need2 = d.ctx.bdpt_record_download(capacity=5)
    assert need2 == need and few.tobytes() == got[:5].tobytes()
    again, need2 = d.ctx.bdpt_record_download(capacity=need)            # asking for all that was needed returns what was kept
    assert need2 == need and again.tobytes() == got.tobytes()
    # what was kept is part of the oracle's list
    ko = br.keys(d.rec)
    at = {int(k): i for i, k in enumerate(ko)}
    twin = d.rec[[at[int(k)] for k in br.keys(got)]]
    assert np.array_equal(twin["q"], got["q"]) and br.bits_equal(twin["r"], got["r"]).all()
    d.check(c.frames, what="record buffer too small")
    d.ctx.bdpt_record_enable(-1)
    with pytest.raises(TirtError):
        d.ctx.bdpt_record_download()


@pytest.mark.parametrize("name", CASE_IDS)
def test_device_vertices_are_the_oracles_one_frame_per_call(gpu_ctx_ok, name):
    d = device(name)
    c = d.case
    one_batch(d)
    hdr, state, compared = None, None, 0
    for f in range(c.frames):
        hdr, _, state, vex = oracle_render(d.o, d.ex, c, frame_begin=f, frames=1, hdr=hdr, state=state, record=False, vertices=True)
        d.render(f, 1)
        rows, verts = d.ctx.bdpt_vertices_download()
        assert len(rows) == c.W * c.H and (rows["frame"] == f).all() and sorted(rows["pixel"].tolist()) == list(range(c.W * c.H))
        compared += br.compare_vertices(rows, verts, vex, "%s frame %d" % (name, f))
        assert vex.tobytes() == d.vex[d.vex["frame"] == f].tobytes(), "the oracle's vertices depend on how the frames are cut into calls"
    d.o.L.orc_bdpt_destroy(state)
    light_eye = int(((d.vex["v"]["type"][:, :7] == br.VERTEX_LIGHT) & br.active_slots(d.vex["eye_depth"], d.vex["tail"], d.vex["light_depth"])[:, :7]).sum())
    print("%s: %d (slot, field) pairs equal; %d eye vertices on an emitter (their delta is an earlier frame's)" % (name, compared, light_eye))


def test_every_strategy_and_every_kind_of_end_vertex_is_matched_at_least_100_times(gpu_ctx_ok):
    for spec in (False, True):
        title = "BDPT_SPEC" if spec else "BDPT_RGB"
        strategies, eye, light, origin = {}, {}, {}, {}
        for c in CASES:
            if c.spec != spec:
                continue
            nz = matched_in_one_call(c.name)
            d = device(c.name)
            br.add_counts(strategies, br.strategy_counts(nz))
            for total, part in zip((eye, light, origin), br.kind_counts(br.end_kinds(nz, d.vex, d.ex.scene, c.seed, c.spec))):
                br.add_counts(total, part)
        print(br.strategy_table(strategies, title))
        print(br.kind_table(eye, light, origin, title))
        br.assert_floors(strategies, eye, light, origin, title)
