"""What the traversal walks (tirt_wide_tree_download: cnode, tri, wnode, prim_slot, the grid), held to its definition in numpy.  No
device and no oracle here.  The experiments-only "wide_collapse" grouping (k_wide_dp) is a different collapse and is NOT restated.

Three independent pieces:

  expected_wide   the greedy collapse of k_wide_level restated: from a binary tree in `compact` layout (pre-order, left child = row + 1,
                  row = (leaf flag | prim or right child | box)) to {binary root: four slots}.  A wide node starts from its root's two
                  children and replaces one internal candidate by that node's two children (left in place, right appended) until it has
                  four or only leaves: first the candidate with the fewest leaves that fits completely into the free slots (leaves - 1 <=
                  free, strict <, first wins), else the one of largest dx*dy + dy*dz + dz*dx in float32 (strict >, first wins).
                  Planes: v = ((x - g0) -+ p) * inv_cell -+ 1 in float32 (the padding after the grid centre: it survives coarse coordinates), one rounding per operation, clamped to +-60000, then to fp16
                  toward -inf (min) / +inf (max); p = pad for leaf slots.  Shape leaves get the whole grid unless shapes_boxed.
  canonical       a downloaded cnode brought to the same form.  The numbering inside a level depends on the order in which the waves of
                  k_wide_level take their queue positions (one atomic per wave), so child indices are compared through the binary node
                  they stand for: the one whose leaves are exactly the leaves below the wide node.
  check_wide_invariants   what tirt_internal.h and DESIGN.md promise, checked without expected_wide: breadth-first numbering, every
                  primitive reachable once, the records, containment with a slack of >= 0.9 cell (float64), the derived tightness bound,
                  empty slots, the chain nodes of far-origin rays, wnode.

Boxes for containment and tightness: a triangle's min / max; under shapes_boxed a sphere's box in the tree's own leaf row (centre -+ (r +
sphere_pad), which must contain centre -+ r: the planes are made from that row, and no bound on tightness holds against the bare sphere);
without shapes_boxed centre -+ r for the ancestors, the leaf slot itself spanning the whole grid.  Spot and laser shapes are not handled."""
import numpy as np

f32 = np.float32
TR_EMPTY = 0x80000001
TR_H_POS, TR_H_NEG = 0x7b53, 0xfb53                 # fp16 +-60000
W_INVERTED = TR_H_POS | (TR_H_NEG << 16)            # min plane +60000, max plane -60000: no ray passes
W_WHOLE = TR_H_NEG | (TR_H_POS << 16)
TR_TOP_SLOTS = 224
SHAPE_BIT = 1 << 30
PRIMITIVE_TRI, SHAPE_SPHERE = 1, 1
MIN_SLACK_CELLS = 0.9            # the builder subtracts one whole cell; the three float32 roundings of the mapping cost ~0.01 cell at |h| <= 30001
TIGHT_EXTRA_CELLS = 0.05


# ---- fp16, rounded toward -inf / +inf ---------------------------------------------------------------------------------------------
def half_down(v):
    """bits (uint16) of the largest fp16 <= v, v a float32 array within the fp16 range"""
    v = np.asarray(v, f32)
    h = v.astype(np.float16)
    with np.errstate(over="ignore"):                  # (the neighbour of +-65504 that is never taken)
        return np.where(h.astype(f32) > v, np.nextafter(h, np.float16(-np.inf)), h).astype(np.float16).view(np.uint16)


def half_up(v):
    """bits (uint16) of the smallest fp16 >= v"""
    v = np.asarray(v, f32)
    h = v.astype(np.float16)
    with np.errstate(over="ignore"):
        return np.where(h.astype(f32) < v, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16).view(np.uint16)


def _clamp(v):
    return np.where(v < f32(-60000.0), f32(-60000.0), np.where(v > f32(60000.0), f32(60000.0), v)).astype(f32)


def half_value(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def half_spacing(bits):
    """the larger of the two distances from an fp16 value to its neighbours"""
    h = np.asarray(bits, np.uint16).view(np.float16)
    with np.errstate(over="ignore"):
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64)
        dn = h.astype(np.float64) - np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    return np.maximum(up, dn)


def leaf_code(slot, shape):
    return int(~(int(slot) | (SHAPE_BIT if shape else 0)) & 0xffffffff)


# ---- the binary tree ----------------------------------------------------------------------------------------------------------------
class Tree:
    """rows [N, 9] in compact layout -> leaf flags, right children, leaves per subtree, the rank of a node's first leaf in pre-order"""

    def __init__(self, rows):
        rows = np.ascontiguousarray(rows, f32)
        self.rows = rows
        self.N = N = rows.shape[0]
        self.leaf = (rows[:, 0].astype(np.int64) & 1) == 1
        self.right = np.where(self.leaf, -1, rows[:, 1].astype(np.int64))
        self.prim = np.where(self.leaf, rows[:, 1].astype(np.int64), -1)
        leaf, right = self.leaf.tolist(), self.right.tolist()
        leaves = [1] * N
        for i in range(N - 1, -1, -1):
            if not leaf[i]:
                assert i + 1 < right[i] < N, "row %d: right child %d out of place" % (i, right[i])
                leaves[i] = leaves[i + 1] + leaves[right[i]]
        self.leaves = np.asarray(leaves, np.int64)
        self.first = np.cumsum(self.leaf) - self.leaf          # leaves in rows before this one = rank of the subtree's first leaf
        n = int(self.leaf.sum())
        self.leaf_row = np.full(n, -1, np.int64)
        self.leaf_row[self.prim[self.leaf]] = np.flatnonzero(self.leaf)


def _area(rows):
    dx, dy, dz = rows[:, 5] - rows[:, 2], rows[:, 6] - rows[:, 3], rows[:, 7] - rows[:, 4]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((dx * dy + dy * dz) + dz * dx).astype(f32)


def slot_words(tree, shape_leaf, grid, pad, shapes_boxed):
    """[N, 3] uint32: the three plane words of every row standing in a slot"""
    rows = tree.rows
    g0, inv = np.asarray(grid["grid_min"], f32), np.asarray(grid["grid_inv_cell"], f32)
    p = np.where(tree.leaf, f32(pad), f32(0.0)).astype(f32)[:, None]
    lo = (((rows[:, 2:5] - g0).astype(f32) - p).astype(f32) * inv).astype(f32) - f32(1.0)
    hi = (((rows[:, 5:8] - g0).astype(f32) + p).astype(f32) * inv).astype(f32) + f32(1.0)
    w = half_down(_clamp(lo)).astype(np.uint32) | (half_up(_clamp(hi)).astype(np.uint32) << np.uint32(16))
    if not shapes_boxed:
        w[shape_leaf] = W_WHOLE
    return w


def expected_wide(rows, prim_is_shape, prim_slot, grid, pad, shapes_boxed):
    """{binary root: ((kind, target, w0, w1, w2) x 4)}, kind "leaf" (target = leaf code), "node" (target = the child's binary root) or
    "empty" (target None).  A one-row tree has no wide node."""
    t = Tree(rows)
    prim_is_shape = np.asarray(prim_is_shape, bool)
    shape_leaf = t.leaf & prim_is_shape[np.maximum(t.prim, 0)]
    words = slot_words(t, shape_leaf, grid, pad, shapes_boxed).tolist()
    leaf, right, leaves, area, prim = t.leaf.tolist(), t.right.tolist(), t.leaves.tolist(), _area(t.rows).tolist(), t.prim.tolist()
    out = {}
    if t.N == 1:
        return out
    level = [0]
    while level:
        nxt = []
        for root in level:
            cand = [root + 1, right[root]]
            while len(cand) < 4:
                free, best, best_leaves = 4 - len(cand), -1, 1 << 30
                for k, c in enumerate(cand):
                    if not leaf[c] and leaves[c] - 1 <= free and leaves[c] < best_leaves:
                        best_leaves, best = leaves[c], k
                if best < 0:
                    best_area = -1.0
                    for k, c in enumerate(cand):
                        if not leaf[c] and area[c] > best_area:
                            best_area, best = area[c], k
                if best < 0:
                    break
                b = cand[best]
                cand[best] = b + 1
                cand.append(right[b])
            slots = []
            for c in cand:
                if leaf[c]:
                    slots.append(("leaf", leaf_code(prim_slot[prim[c]], prim_is_shape[prim[c]])) + tuple(words[c]))
                else:
                    slots.append(("node", c) + tuple(words[c]))
                    nxt.append(c)
            while len(slots) < 4:
                slots.append(("empty", None, W_INVERTED, W_INVERTED, W_INVERTED))
            out[root] = tuple(slots)
        level = nxt
    return out


def _inverse_slots(prim_slot):
    prim_slot = np.asarray(prim_slot, np.int64)
    n = prim_slot.shape[0]
    assert np.array_equal(np.sort(prim_slot), np.arange(n)), "prim_slot is not a permutation of 0..n-1"
    inv = np.empty(n, np.int64)
    inv[prim_slot] = np.arange(n)
    return inv


def canonical(cnode, wide_nodes, rows, prim_slot):
    """the downloaded 4-wide tree, reachable from node 0, in the form of expected_wide"""
    t = Tree(rows)
    n = int(t.leaf.sum())
    slot_prim = _inverse_slots(prim_slot).tolist()
    rank_of_prim = t.first[t.leaf_row].tolist()
    node_of = {(int(f), int(c)): i for i, (f, c, lf) in enumerate(zip(t.first.tolist(), t.leaves.tolist(), t.leaf.tolist())) if not lf}
    cn = np.asarray(cnode, np.uint32)[:wide_nodes].tolist()
    lo, hi, cnt, root = [0] * wide_nodes, [0] * wide_nodes, [0] * wide_nodes, [-1] * wide_nodes
    for i in range(wide_nodes - 1, -1, -1):
        a, b, c = 1 << 40, -1, 0
        for s in range(4):
            code = cn[i][12 + s]
            if code == TR_EMPTY:
                continue
            if code & 0x80000000:
                rec = ~code & 0x3fffffff
                assert rec < n, "node %d slot %d: leaf code %#x names record %d of %d" % (i, s, code, rec, n)
                r = rank_of_prim[slot_prim[rec]]
                a, b, c = min(a, r), max(b, r), c + 1
            else:
                assert i < code < wide_nodes, "node %d slot %d: child index %d is not a later node of the %d" % (i, s, code, wide_nodes)
                a, b, c = min(a, lo[code]), max(b, hi[code]), c + cnt[code]
        assert c >= 2 and b - a + 1 == c and (a, c) in node_of, \
            "node %d: the %d leaves below it (ranks %d..%d) are not the leaves of one binary node" % (i, c, a, b)
        lo[i], hi[i], cnt[i], root[i] = a, b, c, node_of[(a, c)]
    out = {}
    level = [0] if wide_nodes else []
    while level:
        nxt = []
        for i in level:
            slots = []
            for s in range(4):
                code, w = cn[i][12 + s], tuple(cn[i][3 * s:3 * s + 3])
                if code == TR_EMPTY:
                    slots.append(("empty", None) + w)
                elif code & 0x80000000:
                    slots.append(("leaf", code) + w)
                else:
                    slots.append(("node", root[code]) + w)
                    nxt.append(code)
            assert root[i] not in out, "binary node %d is the root of two wide nodes" % root[i]
            out[root[i]] = tuple(slots)
        level = nxt
    return out


def assert_same_canonical(got, want):
    """bit for bit: the same binary roots, and per root the same slot order, codes, child roots and twelve plane words"""
    assert sorted(got) == sorted(want), "wide nodes stand for other binary nodes: %d only downloaded, %d only expected (first: %s / %s)" % (
        len(set(got) - set(want)), len(set(want) - set(got)), sorted(set(got) - set(want))[:3], sorted(set(want) - set(got))[:3])
    for r in sorted(want):
        for s, (g, w) in enumerate(zip(got[r], want[r])):
            assert g[:2] == w[:2], "wide node of binary root %d, slot %d: holds %s, expected %s (slot order = candidate order)" % (r, s, g[:2], w[:2])
            assert g[2:] == w[2:], "wide node of binary root %d, slot %d (%s): plane words %s, expected %s" % (
                r, s, w[0], ["%08x" % x for x in g[2:]], ["%08x" % x for x in w[2:]])


# ---- the invariants -----------------------------------------------------------------------------------------------------------------
def prim_tables(primitive, vertex, shape):
    """is_shape [n], is_sphere [n], exact boxes float64 [n, 6] (triangle min / max, sphere centre -+ radius)"""
    primitive = np.asarray(primitive, np.int64)
    n = primitive.shape[0]
    is_shape = primitive[:, 0] != PRIMITIVE_TRI
    pos = np.asarray(vertex, f32)[:, :3].astype(np.float64)
    shape = np.asarray(shape, f32).reshape(-1, 10)
    box = np.zeros((n, 6), np.float64)
    vi = primitive[~is_shape, 1]
    tv = np.stack([pos[vi], pos[vi + 1], pos[vi + 2]], axis=1) if vi.size else np.zeros((0, 3, 3))
    box[~is_shape, :3] = tv.min(axis=1); box[~is_shape, 3:] = tv.max(axis=1)
    sh = shape[primitive[is_shape, 1]].astype(np.float64)
    is_sphere = is_shape.copy()
    is_sphere[is_shape] = sh[:, 0].astype(np.int64) == SHAPE_SPHERE
    assert np.array_equal(is_shape, is_sphere), "spot / laser shapes are not handled by this checker"
    box[is_shape, :3] = sh[:, 1:4] - sh[:, 4:5]; box[is_shape, 3:] = sh[:, 1:4] + sh[:, 4:5]
    return is_shape, is_sphere, box


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check_records(dl, primitive, vertex, shape, compact):
    primitive = np.asarray(primitive, np.int64)
    n = primitive.shape[0]
    ps = np.asarray(dl["prim_slot"], np.int64)
    rec = _bits(dl["tri"]).reshape(n, 12)[ps]                       # record of primitive i
    ids = np.arange(n)
    assert np.array_equal(rec[:, 11], ids), "record of primitive %d: the id word holds %d" % (
        int(np.flatnonzero(rec[:, 11] != ids)[0]), int(rec[np.flatnonzero(rec[:, 11] != ids)[0], 11]))
    L = rec[:, 3].astype(np.int64)
    comp = np.asarray(compact, f32)
    assert ((L >= 0) & (L < comp.shape[0])).all(), "a record's compact index is out of range"
    assert (((comp[L, 0].astype(np.int64) & 1) == 1) & (comp[L, 1].astype(np.int64) == ids)).all(), \
        "a record's compact index is not the compact_node leaf of its primitive"
    tri = primitive[:, 0] == PRIMITIVE_TRI
    pos = _bits(np.asarray(vertex, f32)[:, :3])
    vi = primitive[tri, 1]
    for k in range(3):
        bad = (rec[tri, 4 * k:4 * k + 3] != pos[vi + k]).any(axis=1)
        assert not bad.any(), "record of primitive %d: v%d is not the scene's vertex" % (int(ids[tri][np.flatnonzero(bad)[0]]), k)
    assert (rec[tri, 7] == 0).all(), "word 7 of a triangle record is not zero"
    sh = _bits(np.asarray(shape, f32).reshape(-1, 10))[primitive[~tri, 1]]
    want = np.zeros((int((~tri).sum()), 12), np.uint32)
    want[:, 0:3] = sh[:, 1:4]; want[:, 4] = sh[:, 4]; want[:, 5] = sh[:, 0]
    got = rec[~tri].copy(); got[:, 3] = 0; got[:, 11] = 0
    assert np.array_equal(got, want), "a sphere's record is not (centre, L) (radius, type, 0, 0) (0, 0, 0, id)"


def check_wnode(dl, compact, prim_is_shape):
    comp = np.ascontiguousarray(compact, f32)
    pad = f32(dl["pad"])
    leaf = (comp[:, 0].astype(np.int64) & 1) == 1
    o = np.flatnonzero(~leaf)
    if o.size == 0:
        return
    ps = np.asarray(dl["prim_slot"], np.int64)
    want = np.zeros((o.size, 16), np.uint32)
    for k, c in enumerate((o + 1, comp[o, 1].astype(np.int64))):
        cl = leaf[c]
        p = np.where(cl, pad, f32(0.0)).astype(f32)[:, None]
        want[:, 6 * k:6 * k + 3] = _bits((comp[c, 2:5] - p).astype(f32))
        want[:, 6 * k + 3:6 * k + 6] = _bits((comp[c, 5:8] + p).astype(f32))
        prim = np.where(cl, comp[c, 1].astype(np.int64), 0)
        codes = ~(ps[prim] | np.where(np.asarray(prim_is_shape, bool)[prim], SHAPE_BIT, 0)) & 0xffffffff
        want[:, 12 + k] = np.where(cl, codes, c)
    got = _bits(dl["wnode"]).reshape(-1, 16)[o]
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        b = bad[0]
        col = int(np.flatnonzero(got[b] != want[b])[0])
        what = "a child code" if col in (12, 13) else ("words 14-15 are not zero" if col >= 14 else
                                                       "a child box (leaf children padded by pad, inner children as they are)")
        raise AssertionError("wnode %d, word %d: %s -- %08x, expected %08x" % (int(o[b]), col, what, int(got[b, col]), int(want[b, col])))


def check_chain(dl, n, is_sphere):
    cn = np.asarray(dl["cnode"], np.uint32)
    wide, nfar = dl["wide_nodes"], dl["n_far_nodes"]
    assert cn.shape[0] == wide + nfar
    spheres = np.flatnonzero(is_sphere)
    if not (dl["shapes_boxed"] and spheres.size):
        assert nfar == 0 and dl["far_qcode"] == dl["root_code"], "chain nodes without boxed spheres (n_far_nodes %d, far_qcode %d)" % (nfar, dl["far_qcode"])
        return
    ps = np.asarray(dl["prim_slot"], np.int64)
    want = [0] + [leaf_code(ps[s], True) for s in spheres]
    got, at, seen = [], dl["far_qcode"], 0
    while True:
        assert wide <= at < wide + nfar, "chain: link / far_qcode %d is not one of the chain nodes %d..%d" % (at, wide, wide + nfar - 1)
        seen += 1
        assert seen <= nfar, "chain: the links loop"
        codes, link = cn[at, 12:16].tolist(), None
        for s, code in enumerate(codes):
            used = code != TR_EMPTY
            w = W_WHOLE if used else W_INVERTED
            assert (cn[at, 3 * s:3 * s + 3] == w).all(), "chain node %d slot %d: a used slot spans the whole grid, an unused one is inverted" % (at, s)
            assert used or all(c == TR_EMPTY for c in codes[s:]), "chain node %d: an empty slot before a used one" % at
            if used and not code & 0x80000000 and not (at == dl["far_qcode"] and s == 0):
                assert s == 3, "chain node %d: the link is in slot %d, not 3" % (at, s)
                link = code
            elif used:
                got.append(code)
        if link is None:
            break
        assert link == at + 1, "chain node %d: its link is %d, the next chain node is %d" % (at, link, at + 1)
        at = link
    assert seen == nfar, "chain: %d of %d chain nodes are linked" % (seen, nfar)
    assert got == want, "chain: holds %s, expected the root and every sphere %s" % (["%x" % g for g in got], ["%x" % w for w in want])


def check_wide_invariants(dl, rows, primitive, vertex, shape, compact, bvh_info=None):
    """dl: Context.wide_tree_download();  rows: traversal_tree_download;  primitive / vertex / shape: the scene's rows as the device holds
    them;  compact: compact_node of lbvh_download;  bvh_info: Context.bvh_info().  Returns {"min_slack", "max_outward"} in cells."""
    primitive = np.asarray(primitive, np.int64)
    n = primitive.shape[0]
    is_shape, is_sphere, exact = prim_tables(primitive, vertex, shape)
    ps = np.asarray(dl["prim_slot"], np.int64)
    slot_prim = _inverse_slots(ps)
    wide, nfar, boxed = dl["wide_nodes"], dl["n_far_nodes"], dl["shapes_boxed"]
    codes_want = (~(ps | np.where(is_shape, SHAPE_BIT, 0)) & 0xffffffff).astype(np.uint32)
    check_records(dl, primitive, vertex, shape, compact)
    check_wnode(dl, compact, is_shape)
    check_chain(dl, n, is_sphere)
    if bvh_info is not None:
        assert wide == bvh_info["nodes"] - nfar, "bvh_info counts %d nodes, the download %d + %d" % (bvh_info["nodes"], wide, nfar)
        if n >= 2:
            assert bvh_info["nodes_in_lds"] == min(wide + nfar, TR_TOP_SLOTS)
    if n == 1:
        assert wide == 0 and nfar == 0, "one primitive: no wide node"
        assert (dl["root_code"] & 0xffffffff) == int(codes_want[0]), "one primitive: root_code %#x is not its leaf code %#x" % (dl["root_code"] & 0xffffffff, int(codes_want[0]))
        return {"min_slack": np.inf, "max_outward": -np.inf}
    assert dl["root_code"] == 0 and wide >= 1
    cn = np.asarray(dl["cnode"], np.uint32)[:wide]
    codes = cn[:, 12:16]
    empty = codes == TR_EMPTY
    inner = (codes & 0x80000000) == 0
    leafm = ~empty & ~inner
    idx = np.arange(wide)[:, None]

    # numbering
    bad = inner & ((codes.astype(np.int64) <= idx) | (codes.astype(np.int64) >= wide))
    assert not bad.any(), "node %d: child index %d is not a later node (a child index is greater than its parent's)" % (
        int(np.argwhere(bad)[0][0]), int(codes[tuple(np.argwhere(bad)[0])]))
    refs = np.bincount(codes[inner].astype(np.int64), minlength=wide)
    refs[0] += 1                                    # (the root: entered from outside)
    if (refs != 1).any():
        k = int(np.flatnonzero(refs != 1)[0])
        raise AssertionError("node %d is the child of %d slots, not of exactly one" % (k, int(refs[k]) - (k == 0)))
    depth = np.full(wide, -1, np.int64)
    level, d, levels = np.array([0]), 0, []
    while level.size:
        depth[level] = d
        levels.append(level)
        c = codes[level]
        level = c[inner[level]].astype(np.int64)
        d += 1
    assert (depth >= 0).all(), "the walk from node 0 visits %d of %d nodes" % (int((depth >= 0).sum()), wide)
    if (np.diff(depth) < 0).any():
        k = int(np.flatnonzero(np.diff(depth) < 0)[0])
        raise AssertionError("not breadth-first: node %d is of level %d, node %d of level %d" % (k, int(depth[k]), k + 1, int(depth[k + 1])))

    # empty slots
    assert (cn[:, :12].reshape(wide, 4, 3)[empty] == W_INVERTED).all(), "an empty slot does not hold the inverted box"
    gap = (empty[:, :-1] & ~empty[:, 1:]).any(axis=1)
    if gap.any():
        raise AssertionError("node %d: an empty slot before a used one" % int(np.flatnonzero(gap)[0]))

    # leaves
    got = np.sort(codes[leafm])
    want = np.sort(codes_want)
    if not np.array_equal(got, want):
        u, c = np.unique(got, return_counts=True)
        twice, missing, alien = u[c > 1], np.setdiff1d(want, got), np.setdiff1d(got, want)
        raise AssertionError("leaves: %d leaf codes reached more than once (%s), %d primitives not reachable (%s), %d codes of no primitive (%s)" % (
            twice.size, ["%x" % x for x in twice[:3]], missing.size, ["%x" % x for x in missing[:3]], alien.size, ["%x" % x for x in alien[:3]]))

    # boxes: per used slot [wide, 4, 6] in float64, bottom-up by level
    t = Tree(rows)
    leaf_prim = np.where(leafm, slot_prim[np.minimum((~codes & 0x3fffffff).astype(np.int64), n - 1)], 0)
    lbox = exact[leaf_prim]
    sph = leafm & is_shape[leaf_prim]
    if boxed and sph.any():
        rb = t.rows[t.leaf_row[leaf_prim[sph]], 2:8].astype(np.float64)
        assert (rb[:, :3] <= lbox[sph][:, :3]).all() and (rb[:, 3:] >= lbox[sph][:, 3:]).all(), "a sphere's box in the tree's leaf row does not contain the sphere"
        lbox[sph] = rb
    sbox = np.zeros((wide, 4, 6), np.float64)
    sbox[..., :3] = np.inf; sbox[..., 3:] = -np.inf
    sbox[leafm] = lbox[leafm]
    nbox = np.zeros((wide, 6), np.float64)
    for lv in reversed(levels):
        c = codes[lv].astype(np.int64)
        m = inner[lv]
        sb = sbox[lv]
        sb[m] = nbox[c[m]]
        sbox[lv] = sb
        nbox[lv, :3] = sb[..., :3].min(axis=1); nbox[lv, 3:] = sb[..., 3:].max(axis=1)
    words = cn[:, :12].reshape(wide, 4, 3)
    whole = sph & (not boxed)
    assert (words[whole] == W_WHOLE).all(), "a shape leaf does not span the whole grid although shapes_boxed is 0"
    test = ~empty & ~whole
    g0, cell = np.asarray(dl["grid_min"], f32).astype(np.float64), np.asarray(dl["grid_cell"], f32).astype(np.float64)
    hmin, hmax = (words & 0xffff).astype(np.uint16), (words >> 16).astype(np.uint16)
    p = np.where(leafm, float(f32(dl["pad"])), 0.0)[..., None]
    slack_min = ((sbox[..., :3] - p) - (g0 + half_value(hmin) * cell)) / cell
    slack_max = ((g0 + half_value(hmax) * cell) - (sbox[..., 3:] + p)) / cell
    slack = np.concatenate([slack_min, slack_max], axis=-1)[test]
    bound = (1.0 + TIGHT_EXTRA_CELLS + np.concatenate([half_spacing(hmin), half_spacing(hmax)], axis=-1))[test]
    where = np.argwhere(test)
    if slack.size:
        k = np.unravel_index(np.argmin(slack), slack.shape)
        assert slack[k] >= MIN_SLACK_CELLS, "containment: node %d slot %d, plane %d (0-2 min, 3-5 max) lies %.4f cells outside the box it stands for, less than %.1f" % (
            int(where[k[0]][0]), int(where[k[0]][1]), int(k[1]), float(slack[k]), MIN_SLACK_CELLS)
        over = slack - bound
        k = np.unravel_index(np.argmax(over), over.shape)
        assert over[k] <= 0.0, "tightness: node %d slot %d, plane %d lies %.3f cells outside the box it stands for, more than 1 + spacing + %.2f = %.3f" % (
            int(where[k[0]][0]), int(where[k[0]][1]), int(k[1]), float(slack[k]), TIGHT_EXTRA_CELLS, float(bound[k]))
    # the boxes the inner slots stand for are the binary tree's own (exact as float32 min / max of float32 numbers)
    return {"min_slack": float(slack.min()) if slack.size else np.inf, "max_outward": float(slack.max()) if slack.size else -np.inf}
