"""What the motion records can be held to without a device: the numpy restatement (tests/motion_expected.py) on a known answer -- a fronto-parallel plane
moved by a whole number of pixels --, against temporal_expected.accumulate where nothing moved, on the oracle's Cornell films with one box translated and
the other rotated (the conditions tests/test_gpu_motion.py relies on, and the region the moved box uncovered), and the snapshot rule as a state machine."""
import types

import numpy as np
import pytest

import motion_expected as mx
import temporal_expected as te
from common import same_bits
from test_film_shapes import make, oracle

f = np.float32
W, H, SEED = 24, 20, 5


# ---- known answer ------------------------------------------------------------------------------------------------------------------------------
def narrow_camera(w, h, fx):
    """eye at the origin, looking down -z, identity view.  With fx = 2^16 every |x|, |y| <= 2^-13: x*x + y*y + 1 rounds to 1, so the normalised pixel-centre
    direction is (x, y, -1) exactly, and every product below is a product with a power of two"""
    eye4 = np.eye(4, dtype=f).reshape(1, 4, 4)
    return types.SimpleNamespace(view_np=eye4, view_inv_np=eye4.copy(), eye_np=np.zeros((1, 3), f), fx=float(fx), fy=float(fx), cx=w / 2, cy=h / 2)


@pytest.mark.parametrize("k", [1, 3, -2])
def test_a_plane_moved_by_k_pixels_takes_the_history_k_pixels_away(k):
    """A plane z = -z0 facing the camera, moved in x by s = k * z0 / fx between the views: the point pixel (i, j) sees now was seen by pixel (i - k, j).
    D = P(snapshot) - P(current) = (-s, 0, 0).  X = (x z0, y z0, -z0) exactly, X + D = ((i - cx - k) / fx * z0, ..), and fi = i - k exactly: the tap
    (i - k, j) has weight 1, the other three weight 0."""
    w, h, fx, z0 = 16, 8, 65536.0, 64.0
    cam = narrow_camera(w, h, fx)
    s = f(k) * f(z0) / f(fx)
    aov = np.zeros((w, h, 8), f)
    aov[:, :, 5] = 1.0; aov[:, :, 6] = z0; aov[:, :, 7] = 1.0      # normal (0, 0, 1), depth z0, every ray hit: the guides agree
    ii, jj = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    ramp = (1 + ii + w * jj).astype(f)                             # 1 .. 128: another count on every pixel
    mom_h = np.zeros((w, h, 8), f); mom_h[:, :, 0] = ramp; mom_h[:, :, 1:4] = 0.5; mom_h[:, :, 4:7] = 0.25
    hdr_h = np.full((w, h, 3), 0.5, f)
    mom_c = np.zeros((w, h, 8), f); mom_c[:, :, 0] = 2.0; mom_c[:, :, 1:4] = 0.25
    hdr_c = np.full((w, h, 3), 0.25, f)
    motion = np.zeros((w, h, 8), f); motion[:, :, 0] = -s; motion[:, :, 3] = 1.0
    hdr, mom, info = mx.accumulate_mv(hdr_c, aov, mom_c, hdr_h, aov, mom_h, cam, cam, motion, max_history=1024.0, want_info=True)
    src = ii - k
    inside = (src >= 0) & (src < w)
    assert inside.sum() == (w - abs(k)) * h
    assert np.array_equal(info["history"], inside)
    assert np.array_equal(info["tap_i0"][inside], src[inside]) and np.array_equal(info["tap_j0"][inside], jj[inside])
    want_n = ramp[np.clip(src, 0, w - 1), jj] + f(2.0)
    assert np.array_equal(mom[:, :, 0][inside], want_n[inside])
    assert same_bits(mom[~inside], mom_c[~inside], True) and same_bits(hdr[~inside], hdr_c[~inside], True)
    # the shift the other way round reads the other neighbour: the sign of the record is not a convention one can get wrong unnoticed
    motion[:, :, 0] = s
    _, mom_r, info_r = mx.accumulate_mv(hdr_c, aov, mom_c, hdr_h, aov, mom_h, cam, cam, motion, max_history=1024.0, want_info=True)
    inside_r = (ii + k >= 0) & (ii + k < w)
    assert np.array_equal(info_r["history"], inside_r) and np.array_equal(mom_r[:, :, 0][inside_r], (ramp[np.clip(ii + k, 0, w - 1), jj] + f(2.0))[inside_r])
    # and a record of zeros is the static accumulation, bit for bit
    motion[:] = 0
    a = mx.accumulate_mv(hdr_c, aov, mom_c, hdr_h, aov, mom_h, cam, cam, motion, max_history=1024.0)
    b = te.accumulate(hdr_c, aov, mom_c, hdr_h, aov, mom_h, cam, cam, max_history=1024.0)
    assert same_bits(a[0], b[0], True) and same_bits(a[1], b[1], True)


# ---- the oracle's Cornell films with a box moved ------------------------------------------------------------------------------------------------
def cornell_case(case, w=W, h=H):
    """view 0 of the box as it stands and view 1 after the move of `case` (mx.CASES), same camera: records, centre hits, vertex rows and the triangles moved"""
    ex = make("cornell", w, h, 0.8)
    cam = te.Cam(ex.cam)
    orc0 = oracle(ex, "cornell")
    rows0 = np.array(ex.scene.vertex_np, f)
    v0 = te.oracle_view(ex, orc0, w, h, SEED)
    hits0 = mx.centre_hits(orc0, ex.cam, w, h)
    tris, new = mx.move(case, rows0, ex.cam, w)
    rows1 = mx.moved_rows(rows0, tris, new)
    ex.scene.vertex_np = rows1
    ex.scene.minboundarynp[0, :] = rows1[:, 0:3].min(axis=0); ex.scene.maxboundarynp[0, :] = rows1[:, 0:3].max(axis=0)
    orc1 = oracle(ex, "cornell")
    v1 = te.oracle_view(ex, orc1, w, h, SEED + 1)
    hits1 = mx.centre_hits(orc1, ex.cam, w, h)
    rec = mx.record(*hits1, ex.scene.primitive_np, rows1, rows0, w, h)
    return types.SimpleNamespace(cam=cam, v0=v0, v1=v1, hits0=hits0, hits1=hits1, rows0=rows0, rows1=rows1, tris=tris, rec=rec, primitive_np=ex.scene.primitive_np)


@pytest.fixture(scope="module", params=sorted(mx.CASES))
def moved(request):
    return request.param, cornell_case(request.param)


def test_the_records_of_a_moved_box(moved):
    case, c = moved
    hit, prim, u, v = c.hits1
    on_box = (hit & np.isin(prim, c.tris)).reshape(W, H)
    rec = c.rec
    assert on_box.sum() >= 8 and (rec[:, :, 3] == hit.reshape(W, H)).all() and (rec[:, :, 7] == 0).all()
    assert (rec[~on_box][:, [0, 1, 2, 4, 5, 6]] == 0).all()        # rows that did not move: snapshot - current is 0 exactly
    d = rec[on_box][:, 0:3]
    if case == "translate":
        shift = (c.rows1[3 * c.tris[0], 0:3] - c.rows0[3 * c.tris[0], 0:3]).astype(np.float64)
        assert np.abs(d + shift).max() <= 1e-4 * np.abs(shift).max() + 1e-4 and (rec[on_box][:, 4:7] == 0).all()
        px = np.abs(shift).max() * c.cam.fx / (c.cam.eye_np[0, 2] - c.rows0[3 * c.tris, 2].mean())
        print("translate: %.2f units, %.2f pixels at the box's depth, %d pixels on the box" % (np.abs(shift).max(), px, on_box.sum()))
        assert 1.2 <= px <= 1.8
    else:
        assert (np.abs(rec[on_box][:, 4:7]).max(axis=1) > 0).sum() >= on_box.sum() // 2 and (d[:, 1] == 0).all()        # dN is there; y stays


def test_the_moves_satisfy_what_the_device_test_relies_on(moved):
    """at least half the film takes history, at least one pixel is rejected, at least one pixel's tap differs from the static reprojection's"""
    case, c = moved
    h_mv, m_mv, i_mv = mx.accumulate_mv(*c.v1, *c.v0, c.cam, c.cam, c.rec, want_info=True)
    h_st, m_st, i_st = te.accumulate(*c.v1, *c.v0, c.cam, c.cam, want_info=True)
    zero = mx.accumulate_mv(*c.v1, *c.v0, c.cam, c.cam, np.zeros_like(c.rec), want_info=True)
    assert same_bits(zero[0], h_st, True) and same_bits(zero[1], m_st, True)
    for key in ("history", "rejected", "off_film", "capped"):
        assert np.array_equal(zero[2][key], i_st[key]), key
    taps_differ = (i_mv["tap_i0"] != zero[2]["tap_i0"]) | (i_mv["tap_j0"] != zero[2]["tap_j0"])
    print("%s: history %d of %d (static %d), rejected %d, pixels whose first tap differs from the static reprojection's %d"
          % (case, i_mv["history"].sum(), W * H, i_st["history"].sum(), i_mv["rejected"].sum(), taps_differ.sum()))
    assert i_mv["history"].sum() >= W * H // 2 and i_mv["rejected"].sum() >= 1 and taps_differ.sum() >= 1
    assert not same_bits(m_mv, m_st, True)
    # pixels on the moved box keep their history with the records and mostly lose it without
    on_box = (c.hits1[0] & np.isin(c.hits1[1], c.tris)).reshape(W, H)
    assert i_mv["history"][on_box].sum() > i_st["history"][on_box].sum() or case == "rotate"


def test_what_the_box_uncovered_takes_no_history(moved):
    """Pixels whose centre ray met the box before the move and meets something behind it now: their record is zero (what they see did not move), the
    static reprojection lands on the history of the BOX, and the depth or the normal test must refuse it.  Held on the pixels whose 3 x 3 neighbourhood was
    all box before the move: at the silhouette a pixel's two jittered samples may have met the wall already, and then it has a history to take."""
    case, c = moved
    was = (c.hits0[0] & np.isin(c.hits0[1], c.tris)).reshape(W, H)
    now = (c.hits1[0] & np.isin(c.hits1[1], c.tris)).reshape(W, H)
    core = was.copy()
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            core &= np.roll(np.roll(was, di, axis=0), dj, axis=1)
    uncovered = was & ~now
    _, _, info = mx.accumulate_mv(*c.v1, *c.v0, c.cam, c.cam, c.rec, want_info=True)
    print("%s: uncovered %d, of them inside the old silhouette %d, with a history %d / %d" %
          (case, uncovered.sum(), (uncovered & core).sum(), info["history"][uncovered].sum(), info["history"][uncovered & core].sum()))
    if case == "translate":                                        # (the rotation uncovers a sliver along the silhouette alone)
        assert (uncovered & core).sum() >= 1 and not info["history"][uncovered].any()
    assert (c.rec[uncovered][:, 0:3] == 0).all()
    assert not info["history"][uncovered & core].any()


# ---- the snapshot rule ---------------------------------------------------------------------------------------------------------------------------
def test_two_updates_then_one_accumulate_use_the_last_accumulated_view():
    r = np.random.RandomState(1)
    rows = [r.uniform(-1, 1, (9, 9)).astype(f) for _ in range(5)]
    m = mx.SnapshotModel(rows[0])
    m.update(rows[1])                                              # no history yet: nothing to keep
    assert not m.valid and not m.moved and m.accumulate() == ("first", None)
    assert m.accumulate() == ("static", None)
    m.update(rows[2]); m.update(rows[3])
    assert m.valid and m.moved
    how, snap = m.accumulate()
    assert how == "motion" and same_bits(snap, rows[1], True) and same_bits(m.rows, rows[3], True)
    assert m.accumulate() == ("static", None)
    m.update(rows[4])
    how, snap = m.accumulate()
    assert how == "motion" and same_bits(snap, rows[3], True)
    for clear in (m.reset, m.upload):                              # both empty the history and clear the mark
        m.update(rows[0]); clear()
        assert not m.valid and not m.moved and m.accumulate() == ("first", None)
    off = mx.SnapshotModel(rows[0], motion=False)                  # without motion records an update empties the history
    off.accumulate(); off.update(rows[1])
    assert not off.valid and off.accumulate() == ("first", None)
