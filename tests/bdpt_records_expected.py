"""BDPT's contributions and sub-path vertices, one by one and bit for bit -- plain numpy, no tolerance anywhere; a NaN equals any NaN (common.same_bits).

The device and the oracle compute every contribution from the same tirt_math.h with contraction off; what differs between them is the ORDER in which a
pixel's contributions are added, which is why a film can only be held to a rounding bound (tests/bdpt_bound_expected.py).  The lists of the numbers added do
not have that problem: the oracle writes one record per (frame, source pixel p, strategy (e, l)) with a target on the film (oracle.c, orc_bd_record), the device
writes one per contribution it EVALUATES (include/tirt.h, tirt_bdpt_record_enable) -- the connections whose ray met what it was aimed at and the eye sub-paths
that ended on an emitter; the connections it does not evaluate are zero in the oracle's list.  So the two lists are compared as sets, keyed by (frame, p, e, l):

  * the keys of each list are unique;
  * every device record is the oracle's record of its key: same q, same three values;
  * every oracle record with a value that is not zero (or not finite) has a device record;
  * (hence) a device record outside the oracle's non-zero set is all zero and is one of the oracle's zero records;
  * no record of either list has a target off the film, and only e == 1 lands on another pixel than its own.

The sub-path vertices (tirt_bdpt_vertices_download against orc_bd_vertices): depths and the tail bit equal; on every slot below the sub-path's depth, and the
tail slot, every field the oracle STORED in this frame (its write mask) is the device's bits, and `delta` is compared on every such slot whatever the mask
says -- the device's k_bd_delta claims to reproduce what earlier frames left there.

Used by tests/test_bdpt_records_host.py (these functions held to the oracle alone, planted defects, the coverage floors) and tests/test_gpu_bdpt_records.py."""
import numpy as np

import oracle_api as oa

VERTEX_LIGHT, VERTEX_LENS, VERTEX_SURFACE = 1, 2, 3
MAT_DISNEY, MAT_GLASS, MAT_LIGHT = 0, 1, 2
PRIMITIVE_TRI, SHAPE_SPHERE, SHAPE_SPOT, SHAPE_LASER = 1, 1, 3, 4
BD_EYE_MAX, BD_LIGHT_MAX, BD_MAX_DEPTH = 7, 6, 5
FIELDS = ("pos", "prim", "snormal", "mat", "normal", "fpdf", "beta", "rpdf", "wo", "type", "delta")
# the (e, l) the connection loops admit (BDPT_RGB.py:615-637): 0 <= e + l - 2 <= 5 and not (1, 1)
STRATEGIES = [(e, l) for e in range(1, BD_EYE_MAX + 1) for l in range(0, BD_LIGHT_MAX + 1) if 0 <= e + l - 2 <= BD_MAX_DEPTH and not (e == 1 and l == 1)]
assert len(STRATEGIES) == 26
EYE_KINDS = ("lens", "disney", "emitter")
LIGHT_KINDS = ("none", "triangle", "sphere", "spot", "laser", "disney")
ORIGIN_KINDS = ("triangle", "sphere", "spot", "laser")
FLOOR = 100


def keys(rec):
    """(frame, p, e, l) as one int64"""
    return (rec["frame"].astype(np.int64) << 40) | (rec["p"].astype(np.int64) << 8) | (rec["e"].astype(np.int64) << 4) | rec["l"].astype(np.int64)


def nonzero(rec):
    """records with a value that is not zero (a NaN or an infinity is not zero)"""
    return (rec["r"] != 0).any(axis=1)


def bits_equal(a, b):
    """elementwise: the same 32 bits, or both NaN"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _show(rec, n=6):
    return [(int(r["frame"]), int(r["p"]), int(r["q"]), int(r["e"]), int(r["l"]), [float(x) for x in r["r"]]) for r in rec[:n]]


def well_formed(rec, W, H, what):
    """what holds for either list on its own"""
    k = keys(rec)
    u, cnt = np.unique(k, return_counts=True)
    assert (cnt == 1).all(), "%s: %d keys (frame, p, e, l) more than once: %s" % (what, int((cnt > 1).sum()), _show(rec[np.isin(k, u[cnt > 1])]))
    ok = (rec["q"] >= 0) & (rec["q"] < W * H) & (rec["p"] >= 0) & (rec["p"] < W * H)
    assert ok.all(), "%s: records off the film: %s" % (what, _show(rec[~ok]))
    el = set(zip(rec["e"].tolist(), rec["l"].tolist()))
    assert el <= set(STRATEGIES), "%s: strategies the loops do not admit: %s" % (what, sorted(el - set(STRATEGIES)))
    own = (rec["e"] == 1) | (rec["p"] == rec["q"])
    assert own.all(), "%s: an e >= 2 contribution on another pixel than its own: %s" % (what, _show(rec[~own]))


def compare_records(dev, orc, W, H, what=""):
    """the device's list against the oracle's (module docstring).  Returns the oracle's non-zero records, all of which the device has matched bit for bit --
    what the coverage tables count."""
    assert dev.dtype == oa.BD_RECORD and orc.dtype == oa.BD_RECORD
    well_formed(orc, W, H, what + " (oracle)")
    well_formed(dev, W, H, what + " (device)")
    ko, kd = keys(orc), keys(dev)
    order = np.argsort(ko)
    at = np.searchsorted(ko[order], kd)
    found = (at < len(ko)) & (ko[order][np.minimum(at, len(ko) - 1)] == kd)
    assert found.all(), "%s: %d device records the oracle does not have: %s" % (what, int((~found).sum()), _show(dev[~found]))
    twin = orc[order][at]
    same_q = dev["q"] == twin["q"]
    assert same_q.all(), "%s: %d records on another target: device %s, oracle %s" % (what, int((~same_q).sum()), _show(dev[~same_q]), _show(twin[~same_q]))
    same_r = bits_equal(dev["r"], twin["r"]).all(axis=1)
    assert same_r.all(), "%s: %d records with other values: device %s, oracle %s" % (what, int((~same_r).sum()), _show(dev[~same_r]), _show(twin[~same_r]))
    nz = nonzero(orc)
    have = np.isin(ko, kd)
    assert have[nz].all(), "%s: %d non-zero oracle records without a device record: %s" % (what, int((nz & ~have).sum()), _show(orc[nz & ~have]))
    extra = ~np.isin(kd, ko[nz])                   # device records outside the oracle's non-zero set: zeros, and the oracle's zero records of their keys
    assert (dev["r"][extra].view(np.uint32) << 1 == 0).all() and not nonzero(twin[extra]).any(), "%s: a device record beside the non-zero set with a value" % what
    return orc[nz]


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------------
def strategy_counts(rec):
    """non-zero records per admitted strategy"""
    nz = rec[nonzero(rec)]
    out = {s: 0 for s in STRATEGIES}
    for e, l in zip(nz["e"].tolist(), nz["l"].tolist()):
        out[(e, l)] += 1
    return out


def emitter_kind(scene, prim):
    """triangle / sphere / spot / laser: what kind of emitter a primitive of the light list is"""
    kind, index = int(scene.primitive_np[prim, 0]), int(scene.primitive_np[prim, 1])
    if kind == PRIMITIVE_TRI:
        return "triangle"
    return {SHAPE_SPHERE: "sphere", SHAPE_SPOT: "spot", SHAPE_LASER: "laser"}[int(scene.shape_np[index, 0])]


def end_kinds(rec, vex, scene, seed, spec):
    """per record the kinds of the two vertices the strategy connects and of the emitter the light sub-path began on, (eye kind, light kind, origin kind), from the oracle's vertex export `vex` (one BD_VERTICES row per
    (frame, pixel), any order).  Eye end eye[e - 1]: lens / disney / glass / emitter.  Light end: none (l == 0); light[l - 1] for l >= 2: disney / glass (the
    light sub-path stores surfaces only); l == 1 connects to a NEW point on an emitter, chosen by the first random number of the connection (Scene.sample_li at
    dimension 176 + 4 e, BDPT_SPEC: Scene.sample_light at 256 + 8 e): triangle / sphere / spot / laser of that choice.  Origin, for l >= 2 (None otherwise): the
    emitter light[0] lies on, chosen at dimension 80 (Scene.sample_light) -- the only way a spot or a laser, which no ray can hit, gets into a contribution."""
    mat_type = scene.material_np[:, 0].astype(np.int64)
    where = {(int(f), int(p)): k for k, (f, p) in enumerate(zip(vex["frame"].tolist(), vex["pixel"].tolist()))}
    rand = oa.load().orc_kat_rand
    out = []
    for r in rec:
        x = vex[where[(int(r["frame"]), int(r["p"]))]]
        e, l = int(r["e"]), int(r["l"])
        ev = x["v"][e - 1]
        ek = {VERTEX_LENS: "lens", VERTEX_LIGHT: "emitter"}.get(int(ev["type"])) or ("glass" if mat_type[int(ev["mat"])] == MAT_GLASS else "disney")
        ok = None
        if l == 0:
            lk = "none"
        elif l == 1:
            u = rand(int(seed), int(r["p"]), int(r["frame"]), (256 + 8 * e) if spec else (176 + 4 * e))
            lidx = min(int(np.float32(u) * np.float32(scene.light_count)), scene.light_count - 1)
            lk = emitter_kind(scene, int(scene.light_np[lidx]))
        else:
            lv = x["v"][BD_EYE_MAX + l - 1]
            assert int(lv["type"]) == VERTEX_SURFACE
            lk = "glass" if mat_type[int(lv["mat"])] == MAT_GLASS else "disney"
            u = rand(int(seed), int(r["p"]), int(r["frame"]), 80)
            ok = emitter_kind(scene, int(scene.light_np[min(int(np.float32(u) * np.float32(scene.light_count)), scene.light_count - 1)]))
        out.append((ek, lk, ok))
    return out


def kind_counts(kinds):
    eye = {k: 0 for k in EYE_KINDS}; light = {k: 0 for k in LIGHT_KINDS}; origin = {k: 0 for k in ORIGIN_KINDS}
    for ek, lk, ok in kinds:
        eye[ek] = eye.get(ek, 0) + 1; light[lk] = light.get(lk, 0) + 1
        if ok is not None:
            origin[ok] += 1
    return eye, light, origin


def add_counts(total, part):
    for k, v in part.items():
        total[k] = total.get(k, 0) + v
    return total


def strategy_table(counts, title):
    rows = ["%s: non-zero records per strategy (e down, l across 0..6)" % title]
    for e in range(1, BD_EYE_MAX + 1):
        rows.append("  e=%d " % e + " ".join("%7s" % (counts[(e, l)] if (e, l) in counts else "-") for l in range(0, BD_LIGHT_MAX + 1)))
    return "\n".join(rows)


def kind_table(eye, light, origin, title):
    return "%s: non-zero records per end-vertex kind -- eye end %s; light end %s; emitter the light sub-path of an l >= 2 record began on %s" % (title, dict(eye), dict(light), dict(origin))


# ---- vertices ---------------------------------------------------------------------------------------------------------------------------------------------
def active_slots(eye_depth, tail, light_depth):
    """[n, 13] bool: the slots below the sub-paths' depths, and the eye tail slot where the tail bit is set"""
    s = np.arange(BD_EYE_MAX + BD_LIGHT_MAX)[None, :]
    ed, ld, tl = (np.asarray(a, np.int64)[:, None] for a in (eye_depth, light_depth, tail))
    return ((s < BD_EYE_MAX) & ((s < ed) | ((s == ed) & (tl != 0)))) | ((s >= BD_EYE_MAX) & (s - BD_EYE_MAX < ld))


def compare_vertices(rows, verts, vex, what=""):
    """the device's items (ti_raytrace_amd._native: BD_ITEM_ROW rows, BD_VERTEX verts[n, 13]) against the oracle's export of the same frames (module docstring).
    Returns how many (slot, field) pairs were compared."""
    where = {(int(f), int(p)): k for k, (f, p) in enumerate(zip(vex["frame"].tolist(), vex["pixel"].tolist()))}
    assert len(where) == len(vex), what + ": the oracle exported a pixel sample twice"
    ids = list(zip(rows["frame"].tolist(), rows["pixel"].tolist()))
    assert len(set(ids)) == len(ids), what + ": the device handed out an item twice"
    missing = [i for i in ids if i not in where]
    assert not missing, "%s: items the oracle did not render: %s" % (what, missing[:6])
    x = vex[[where[i] for i in ids]]
    for name in ("eye_depth", "tail", "light_depth"):
        bad = np.nonzero(rows[name] != x[name])[0]
        assert len(bad) == 0, "%s: %s differs on %d items, first (frame, pixel) %s: device %d, oracle %d" % (what, name, len(bad), ids[bad[0]], rows[name][bad[0]], x[name][bad[0]])
    act = active_slots(x["eye_depth"], x["tail"], x["light_depth"])
    compared = 0
    for f in FIELDS:
        sel = act if f == "delta" else act & ((x["mask"] & oa.BVF[f]) != 0)
        d, o = verts[f], x["v"][f]
        if d.dtype == np.float32:
            eq = bits_equal(d, o)
            eq = eq.all(axis=2) if eq.ndim == 3 else eq
        else:
            eq = d.astype(np.int64) == o.astype(np.int64)
        bad = np.argwhere(sel & ~eq)
        assert len(bad) == 0, "%s: field %s differs on %d slots, first (frame, pixel) %s slot %d: device %r, oracle %r (mask %#x)" % (
            what, f, len(bad), ids[bad[0][0]], bad[0][1], d[bad[0][0], bad[0][1]], o[bad[0][0], bad[0][1]], int(x["mask"][bad[0][0], bad[0][1]]))
        compared += int(sel.sum())
    return compared


def as_device_vertices(vex):
    """the oracle's export in the device's formats, the way a correct device would hand it out under the 0xFF poison: what the comparison does not look at
    (inactive slots, fields the mask does not mark) is poison.  For the host tests, which plant their defects in it."""
    from ti_raytrace_amd._native import BD_ITEM_ROW, BD_VERTEX
    rows = np.zeros(len(vex), BD_ITEM_ROW)
    for name in ("frame", "pixel", "eye_depth", "tail", "light_depth"):
        rows[name] = vex[name]
    verts = np.zeros((len(vex), BD_EYE_MAX + BD_LIGHT_MAX), BD_VERTEX)
    verts.view(np.uint8)[...] = 0xFF
    act = active_slots(vex["eye_depth"], vex["tail"], vex["light_depth"])
    for f in FIELDS:
        sel = act if f == "delta" else act & ((vex["mask"] & oa.BVF[f]) != 0)
        verts[f][sel] = vex["v"][f][sel]
    return rows, verts


# the kinds a test asserts; the others -- a glass end vertex, a spot or a laser as the light end of an l == 1 connection -- the oracle makes non-zero on no
# input (tests/test_gpu_bdpt_records.py has the reasons), which assert_floors holds too: the day one of them appears, it wants a floor of its own
ASSERTED_LIGHT_KINDS = ("none", "triangle", "sphere", "disney")
IMPOSSIBLE = (("eye", "glass"), ("light", "glass"), ("light", "spot"), ("light", "laser"))


def assert_floors(strategies, eye, light, origin, title):
    """every strategy and every asserted kind has at least FLOOR non-zero records"""
    assert set(strategies) == set(STRATEGIES)
    low = {k: v for k, v in strategies.items() if v < FLOOR}
    assert not low, "%s: strategies with fewer than %d non-zero records: %s" % (title, FLOOR, low)
    for name, counts, kinds in (("eye end", eye, EYE_KINDS), ("light end", light, ASSERTED_LIGHT_KINDS), ("light sub-path origin", origin, ORIGIN_KINDS)):
        low = {k: counts.get(k, 0) for k in kinds if counts.get(k, 0) < FLOOR}
        assert not low, "%s: %s kinds with fewer than %d non-zero records: %s" % (title, name, FLOOR, low)
    tables = {"eye": eye, "light": light}
    seen = {(t, k): tables[t].get(k, 0) for t, k in IMPOSSIBLE if tables[t].get(k, 0)}
    assert not seen, "%s: a kind of end vertex held impossible has non-zero records: %s" % (title, seen)
