"""The checker of the 4-wide traversal nodes (wide_tree_expected.py) has to bite: downloads assembled by hand from expected_wide are
accepted, and every single defect of a list is rejected by check_wide_invariants or by the canonical comparison, with the reason in
the message.  No device.  (The experiments-only "wide_collapse" grouping is not covered: another collapse, another restatement.)"""
import copy
import re

import numpy as np
import pytest

import wide_tree_expected as wt

f32 = np.float32
SPHERE_ROW_PAD = f32(0.01)            # what the hand-made tree adds to a boxed sphere's radius in its leaf row


def chain_topology(n):
    t = 0
    for k in range(1, n):
        t = (t, k)                    # every right child a leaf
    return t


TOPOLOGIES = {
    "nine": (((((0, 1), (2, 3)), 4), ((5, 6), (7, 8))), 9, (4,)),
    "three": (((0, 1), 2), 3, ()),
    "chain40": (chain_topology(40), 40, (3, 11, 12, 30, 39)),        # five spheres: two chain nodes for far-origin rays
    "chain41": (chain_topology(41), 41, ()),                          # ends in a node of two leaves
    "wide24": (None, 24, ()),                                         # balanced: three levels of wide nodes
}


def balanced(lo, hi):
    return lo if hi - lo == 1 else (balanced(lo, (lo + hi) // 2), balanced((lo + hi) // 2, hi))


def fake(name):
    """(download, scene) as a device would hand them out, for a binary tree given as nested pairs of primitive ids"""
    topo, n, spheres = TOPOLOGIES[name]
    if topo is None:
        topo = balanced(0, n)
    r = np.random.RandomState(n)
    is_shape = np.isin(np.arange(n), spheres)
    boxed = 1 if n >= 2 and len(spheres) <= 8 else 0
    centre = r.uniform(-1, 1, (n, 3)).astype(f32)
    tris = (centre[:, None, :] + r.uniform(-0.15, 0.15, (n, 3, 3)).astype(f32)).astype(f32)
    radius = r.uniform(0.05, 0.2, n).astype(f32)
    vertex = np.zeros((3 * n, 9), f32); vertex[:, :3] = tris.reshape(-1, 3); vertex[:, 5] = 1.0
    primitive = np.zeros((n, 3), np.int32)
    primitive[:, 0] = np.where(is_shape, 2, 1); primitive[:, 1] = 3 * np.arange(n)
    shape = np.zeros((max(len(spheres), 1), 10), f32)
    for k, s in enumerate(spheres):
        primitive[s, 1] = k
        shape[k, 0] = 1.0; shape[k, 1:4] = centre[s]; shape[k, 4] = radius[s]
    box = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    for s in spheres:
        rr = radius[s] + SPHERE_ROW_PAD if boxed else radius[s]
        box[s, :3] = centre[s] - rr; box[s, 3:] = centre[s] + rr
    rows, order = [], []

    def emit(t):
        i = len(rows)
        rows.append(None)
        if isinstance(t, int):
            rows[i] = [1.0, float(t)] + box[t].tolist() + [0.0]
            order.append(t)
            return i
        l = emit(t[0]); rt = emit(t[1])
        lo = np.minimum(np.asarray(rows[l][2:5], f32), np.asarray(rows[rt][2:5], f32))
        hi = np.maximum(np.asarray(rows[l][5:8], f32), np.asarray(rows[rt][5:8], f32))
        rows[i] = [0.0, float(rt)] + lo.tolist() + hi.tolist() + [0.0]
        return i
    emit(topo)
    rows = np.asarray(rows, f32)
    prim_slot = np.zeros(n, np.int32); prim_slot[order] = np.arange(n)
    dl = {"prim_slot": prim_slot, "root_min": rows[0, 2:5].copy(), "root_max": rows[0, 5:8].copy(), "built_sah": 1, "shapes_boxed": boxed}
    ext = dl["root_max"] - dl["root_min"]
    pad = f32(1.0e-4) * np.sqrt((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2], dtype=f32)
    lo, hi = dl["root_min"] - pad, dl["root_max"] + pad
    e = (hi - lo).astype(f32)
    cell = (e / f32(60000.0)).astype(f32)
    dl.update(pad=f32(pad), grid_cell=cell, grid_min=(lo + f32(0.5) * e).astype(f32), grid_inv_extent=(f32(1.0) / e).astype(f32),
              grid_inv_cell=(f32(1.0) / cell).astype(f32))
    want = wt.expected_wide(rows, is_shape, prim_slot, dl, dl["pad"], boxed)
    number, level = {0: 0}, [0]                      # breadth-first numbering, a level's children in slot order
    while level:
        nxt = [s[1] for root in level for s in want[root] if s[0] == "node"]
        for c in nxt:
            number[c] = len(number)
        level = nxt
    wide = len(number)
    cn = np.zeros((wide, 16), np.uint32)
    for root, slots in want.items():
        for s, (kind, target, w0, w1, w2) in enumerate(slots):
            cn[number[root], 3 * s:3 * s + 3] = (w0, w1, w2)
            cn[number[root], 12 + s] = wt.TR_EMPTY if kind == "empty" else (target if kind == "leaf" else number[target])
    far = []
    if boxed and spheres:
        codes = [0] + [wt.leaf_code(prim_slot[s], True) for s in spheres]
        at = 0
        while at < len(codes):
            left = len(codes) - at
            take = left if left <= 4 else 3
            node = np.zeros(16, np.uint32)
            for s in range(4):
                used = s < take or (s == 3 and left > 4)
                node[3 * s:3 * s + 3] = wt.W_WHOLE if used else wt.W_INVERTED
                node[12 + s] = codes[at + s] if s < take else (wide + len(far) + 1 if used else wt.TR_EMPTY)
            far.append(node); at += take
    dl.update(cnode=np.concatenate([cn, np.asarray(far, np.uint32).reshape(-1, 16)]), wide_nodes=wide, n_far_nodes=len(far), root_code=0,
              far_qcode=wide if far else 0)
    leaf_row = np.zeros(n, np.int64); leaf_row[rows[rows[:, 0] == 1.0, 1].astype(np.int64)] = np.flatnonzero(rows[:, 0] == 1.0)
    rec = np.zeros((n, 12), np.uint32)
    for i in range(n):
        k = prim_slot[i]
        if is_shape[i]:
            rec[k, 0:3] = centre[i].view(np.uint32); rec[k, 4] = radius[i:i + 1].view(np.uint32)[0]; rec[k, 5] = f32(1.0).view(np.uint32)
        else:
            for v in range(3):
                rec[k, 4 * v:4 * v + 3] = tris[i, v].view(np.uint32)
        rec[k, 3] = leaf_row[i]; rec[k, 11] = i
    dl["tri"] = rec.view(f32)
    wn = np.zeros((rows.shape[0], 16), np.uint32)
    for o in np.flatnonzero(rows[:, 0] == 0.0):
        for k, c in enumerate((o + 1, int(rows[o, 1]))):
            lf = rows[c, 0] == 1.0
            p = dl["pad"] if lf else f32(0.0)
            wn[o, 6 * k:6 * k + 3] = (rows[c, 2:5] - p).astype(f32).view(np.uint32)
            wn[o, 6 * k + 3:6 * k + 6] = (rows[c, 5:8] + p).astype(f32).view(np.uint32)
            wn[o, 12 + k] = wt.leaf_code(prim_slot[int(rows[c, 1])], is_shape[int(rows[c, 1])]) if lf else c
    dl["wnode"] = wn.view(f32)
    sc = {"rows": rows, "primitive": primitive, "vertex": vertex, "shape": shape, "compact": rows.copy(), "is_shape": is_shape,
          "bvh_info": {"nodes": wide + len(far), "nodes_in_lds": min(wide + len(far), wt.TR_TOP_SLOTS)}}
    return dl, sc


def run_invariants(dl, sc):
    return wt.check_wide_invariants(dl, sc["rows"], sc["primitive"], sc["vertex"], sc["shape"], sc["compact"], sc["bvh_info"])


def run_canonical(dl, sc):
    want = wt.expected_wide(sc["rows"], sc["is_shape"], dl["prim_slot"], dl, dl["pad"], dl["shapes_boxed"])
    wt.assert_same_canonical(wt.canonical(dl["cnode"], dl["wide_nodes"], sc["rows"], dl["prim_slot"]), want)


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_hand_made_download_is_accepted(name):
    dl, sc = fake(name)
    st = run_invariants(dl, sc)
    run_canonical(dl, sc)
    assert 0.9 <= st["min_slack"] and st["max_outward"] < 1.05 + 32.0
    if name == "chain40":
        assert dl["n_far_nodes"] == 2 and dl["wide_nodes"] == 13          # three leaves and the rest of the chain per node: 13 levels
    if name == "chain41":
        assert dl["wide_nodes"] == 14 and (dl["cnode"][13, 14:16] == wt.TR_EMPTY).all() and dl["n_far_nodes"] == 0
    if name == "nine":
        assert dl["n_far_nodes"] == 1
    if name == "wide24":
        assert dl["wide_nodes"] >= 6


# ---- single defects -----------------------------------------------------------------------------------------------------------------
def _half_step(bits, up):
    h = np.uint16(bits).view(np.float16)
    return int(np.nextafter(h, np.float16(np.inf if up else -np.inf)).view(np.uint16))


def _find_slot(dl, want_leaf=None, want_inner=None, want_empty=None, node_min=0):
    cn = dl["cnode"]
    for i in range(node_min, dl["wide_nodes"]):
        for s in range(4):
            c = int(cn[i, 12 + s])
            kind = "empty" if c == wt.TR_EMPTY else ("leaf" if c & 0x80000000 else "inner")
            if (want_leaf and kind == "leaf") or (want_inner and kind == "inner") or (want_empty and kind == "empty"):
                return i, s
    raise AssertionError("no such slot in the hand-made tree")


def m_min_plane_inward(dl, sc):
    w = int(dl["cnode"][0, 0])
    dl["cnode"][0, 0] = (w & 0xffff0000) | _half_step(w & 0xffff, True)


def m_max_plane_inward(dl, sc):
    w = int(dl["cnode"][0, 4])
    dl["cnode"][0, 4] = (w & 0xffff) | (_half_step(w >> 16, False) << 16)


def m_plane_far_outward(dl, sc):
    w = int(dl["cnode"][0, 1])
    h = np.float16(np.uint16(w & 0xffff).view(np.float16).astype(f32) - f32(40.0))
    dl["cnode"][0, 1] = (w & 0xffff0000) | int(h.view(np.uint16))


def _two_leaf_slots(dl):
    cn = dl["cnode"]
    for i in range(dl["wide_nodes"]):
        s = [k for k in range(4) if int(cn[i, 12 + k]) & 0x80000000 and int(cn[i, 12 + k]) != wt.TR_EMPTY]
        if len(s) >= 2:
            return i, s[0], s[1]
    raise AssertionError("no node with two leaves")


def m_swap_leaf_codes(dl, sc):
    i, a, b = _two_leaf_slots(dl)
    dl["cnode"][i, [12 + a, 12 + b]] = dl["cnode"][i, [12 + b, 12 + a]]


def m_duplicate_leaf(dl, sc):
    i, a, b = _two_leaf_slots(dl)
    dl["cnode"][i, 12 + b] = dl["cnode"][i, 12 + a]


def m_drop_leaf(dl, sc):
    i, a, b = _two_leaf_slots(dl)
    dl["cnode"][i, 12 + b] = wt.TR_EMPTY


def m_empty_not_inverted(dl, sc):
    i, s = _find_slot(dl, want_empty=True)
    dl["cnode"][i, 3 * s + 1] = wt.W_WHOLE


def m_child_points_back(dl, sc):
    i, s = _find_slot(dl, want_inner=True, node_min=1)
    dl["cnode"][i, 12 + s] = 0


def m_exchange_levels(dl, sc):
    """the second node of level 1 and the first node of level 2 trade places; every child index follows, so the tree is still a tree"""
    cn = dl["cnode"]
    a = 2
    b = next(int(c) for c in cn[1, 12:16] if not int(c) & 0x80000000)
    codes = cn[:dl["wide_nodes"], 12:16]
    ia, ib = codes == a, codes == b
    codes[ia] = b; codes[ib] = a
    cn[[a, b]] = cn[[b, a]]


def m_record_id(dl, sc):
    dl["tri"].view(np.uint32)[2, 11] += 1


def m_record_v1_v2(dl, sc):
    k = int(dl["prim_slot"][0])
    dl["tri"][k, [4, 5, 6, 8, 9, 10]] = dl["tri"][k, [8, 9, 10, 4, 5, 6]]


def m_prim_slot_equal(dl, sc):
    dl["prim_slot"][1] = dl["prim_slot"][0]


def m_clear_shape_bit(dl, sc):
    cn = dl["cnode"][:dl["wide_nodes"]]
    i, s = np.argwhere(((cn[:, 12:16] & 0xc0000000) == 0x80000000) & (cn[:, 12:16] != wt.TR_EMPTY))[0]     # ~(slot | 1 << 30): bit 30 clear
    cn[i, 12 + s] |= 1 << 30


def m_chain_link(dl, sc):
    dl["cnode"][dl["wide_nodes"], 15] += 1


def m_chain_misses_sphere(dl, sc):
    last = dl["cnode"][-1]
    s = max(k for k in range(4) if int(last[12 + k]) != wt.TR_EMPTY)
    last[12 + s] = wt.TR_EMPTY; last[3 * s:3 * s + 3] = wt.W_INVERTED


def m_wnode_unpadded(dl, sc):
    rows = sc["compact"]
    o = next(int(o) for o in np.flatnonzero(rows[:, 0] == 0.0) if rows[o + 1, 0] == 1.0)
    dl["wnode"][o, 0:3] = rows[o + 1, 2:5]


MUTATIONS = [
    ("nine", m_min_plane_inward, r"plane words|containment"),
    ("nine", m_max_plane_inward, r"plane words|containment"),
    ("nine", m_plane_far_outward, r"tightness"),
    ("nine", m_swap_leaf_codes, r"slot order|containment"),
    ("nine", m_duplicate_leaf, r"reached more than once"),
    ("nine", m_drop_leaf, r"not reachable|inverted box"),
    ("three", m_empty_not_inverted, r"inverted box"),
    ("chain40", m_child_points_back, r"not a later node"),
    ("wide24", m_exchange_levels, r"breadth-first"),
    ("nine", m_record_id, r"id word"),
    ("nine", m_record_v1_v2, r"v1 is not the scene's vertex"),
    ("nine", m_prim_slot_equal, r"permutation"),
    ("nine", m_clear_shape_bit, r"codes of no primitive"),
    ("chain40", m_chain_link, r"its link is|not one of the chain nodes"),
    ("chain40", m_chain_misses_sphere, r"every sphere"),
    ("nine", m_wnode_unpadded, r"wnode .*child box"),
]


@pytest.mark.parametrize("name,mutate,reason", MUTATIONS, ids=[m[1].__name__[2:] for m in MUTATIONS])
def test_single_defect_is_rejected(name, mutate, reason):
    dl, sc = copy.deepcopy(fake(name))
    before = copy.deepcopy(dl)
    mutate(dl, sc)
    assert any(not np.array_equal(np.asarray(dl[k]).view(np.uint8), np.asarray(before[k]).view(np.uint8)) for k in ("cnode", "tri", "wnode", "prim_slot")), "the mutation changed nothing"
    said = []
    for check in (run_invariants, run_canonical):
        try:
            check(dl, sc)
        except AssertionError as exc:
            said.append(str(exc))
    assert said, "accepted by both checks"
    assert any(re.search(reason, s) for s in said), said


def test_every_defect_of_the_list_has_a_case():
    assert len(MUTATIONS) == 16 and len({m[1] for m in MUTATIONS}) == 16


# ---- the fp16 helper ----------------------------------------------------------------------------------------------------------------
def test_directed_rounding_against_enumeration():
    """every finite fp16 value h, and the float32 numbers just below, at and just above it: round-down gives the largest half <= v,
    round-up the smallest half >= v (by value; found by bisection in the sorted list of all finite halves)"""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    assert h.size == 2 * 31 * 1024
    table = np.unique(h.astype(np.float64))
    assert table.size == h.size - 1                     # +0 and -0
    hv = h.astype(f32)
    v = np.concatenate([np.nextafter(hv, f32(-np.inf)), hv, np.nextafter(hv, f32(np.inf))])
    v = v[np.abs(v) <= f32(65504.0)]
    down = wt.half_value(wt.half_down(v))
    up = wt.half_value(wt.half_up(v))
    v64 = v.astype(np.float64)
    assert np.array_equal(down, table[np.searchsorted(table, v64, side="right") - 1])
    assert np.array_equal(up, table[np.searchsorted(table, v64, side="left")])
    assert (down <= v64).all() and (up >= v64).all() and ((down == up) == np.isin(v64, table)).all()
    # the sign of a zero result is the input's, as the device's conversion gives it
    assert wt.half_down(f32([1e-10, -1e-10])).tolist() == [0x0000, 0x8001] and wt.half_up(f32([1e-10, -1e-10])).tolist() == [0x0001, 0x8000]
