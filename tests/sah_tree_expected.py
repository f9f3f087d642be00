"""The traversal tree's definition (ti_raytrace_amd/csrc/tirt_sah.hip, header), restated in numpy, float32, operation by operation.

The library is compiled with -ffp-contract=off, so every decision below is the device's to the bit: no float64 takes part in one.

A node is a set of primitives ORDERED BY THEIR POSITION IN THE MORTON-SORTED ARRAY.  The device's first index array is the identity over
that array and every partition is stable, so this is the order of the node's range at the moment it is split -- which makes the decision of
a node a function of (its primitives' boxes in that order, its level) alone, and the check node-local.

  centroid      c = 0.5f * (mn + mx), per axis
  bins          ext = cmax - cmin; scale = ext > 0 ? 32.0f / ext : 0; bin = clamp((int)((c - cmin) * scale), 0, 31)      (the cast truncates)
  count > 16    binned: per axis and bin min / max / count; plane (axis, sp) has bins <= sp on the left; planes with an empty side are not
                admissible; cost = (dx*dy + dy*dz + dz*dx)_L * (float)n_L + (...)_R * (float)n_R; the smallest cost wins, a tie goes to the
                smallest axis * 32 + sp; no admissible plane: the first count / 2 BY POSITION go left
  count <= 16   exact sweep: candidate (axis, i) has j on the left iff c_j < c_i or (c_j == c_i and j <= i); candidates with an empty right
                side are not admissible; same cost; a tie goes to the smallest axis * 16 + i
  level >= 64   the first count / 2 by position go left, whatever the count
The size classes (which kernel splits the node: mini <= 16 < subtree <= 64 < small <= 512 < large <= 8192 < huge) decide nothing but
exact-against-binned at 16 | 17; they are tallied so that a test can say which code it has run.
"""
from collections import Counter, namedtuple

import numpy as np

f32 = np.float32
BINS = 32
MINI = 16
FORCE_HALVING_FROM = 64
CLASS_BOUNDS = (("mini", 16), ("subtree", 64), ("small", 512), ("large", 8192))
CLASSES = ("mini", "subtree", "small", "large", "huge")
KINDS = ("plane", "exact", "halved", "forced")        # binned plane, exact sweep, no admissible plane, level >= 64

# (left mask in node order, kind, another candidate with ANOTHER left set costs as little as the winner, axis, plane or candidate, n_left)
Split = namedtuple("Split", "left kind tied axis plane n_left")
_INF = f32(np.inf)


def size_class(count):
    for name, bound in CLASS_BOUNDS:
        if count <= bound:
            return name
    return "huge"


def half_area(d):
    """dx*dy + dy*dz + dz*dx in that order, d[..., 3] float32"""
    return (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]


def centroids(boxes):
    return f32(0.5) * (boxes[..., :3] + boxes[..., 3:])


def bins_of(boxes):
    """bin of every primitive on every axis, int [n, 3]"""
    c = centroids(boxes)
    cmin, cmax = c.min(axis=0), c.max(axis=0)
    ext = cmax - cmin
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        scale = np.where(ext > 0, f32(BINS) / np.where(ext > 0, ext, f32(1)), f32(0)).astype(f32)
        t = (c - cmin) * scale
    t = np.where(np.isnan(t), f32(0), np.clip(t, f32(-1), f32(BINS)))      # the device's cast saturates (NaN -> 0); in range it truncates
    return np.clip(t.astype(np.int32), 0, BINS - 1)


def halved(n):
    left = np.zeros(n, bool)
    left[:n // 2] = True
    return left


def plane_costs(boxes, bins):
    """cost float32 [3, 32] of the planes (inf: not admissible; plane 31 never is) and n_left [3, 32]"""
    n = boxes.shape[0]
    cost = np.full((3, BINS), _INF, f32)
    nleft = np.zeros((3, BINS), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ax in range(3):
            b = bins[:, ax]
            order = np.argsort(b, kind="stable")
            cnt = np.bincount(b, minlength=BINS)
            mn = np.full((BINS, 3), _INF, f32); mx = np.full((BINS, 3), -_INF, f32)
            used = np.flatnonzero(cnt)
            first = np.concatenate([[0], np.cumsum(cnt)[:-1]])[used]
            mn[used] = np.minimum.reduceat(boxes[order, :3], first, axis=0)
            mx[used] = np.maximum.reduceat(boxes[order, 3:], first, axis=0)
            lmn, lmx = np.minimum.accumulate(mn, axis=0)[:-1], np.maximum.accumulate(mx, axis=0)[:-1]              # bins <= sp, sp = 0 .. 30
            rmn, rmx = np.minimum.accumulate(mn[::-1], axis=0)[::-1][1:], np.maximum.accumulate(mx[::-1], axis=0)[::-1][1:]
            nl = np.cumsum(cnt)[:-1]; nr = n - nl
            ok = (nl > 0) & (nr > 0)
            c = half_area(np.where(ok[:, None], lmx - lmn, f32(0))) * nl.astype(f32) + half_area(np.where(ok[:, None], rmx - rmn, f32(0))) * nr.astype(f32)
            cost[ax, :-1] = np.where(ok & ~np.isnan(c), c, _INF)
            nleft[ax, :-1] = nl
    return cost, nleft


def binned(boxes):
    """the split of a node of more than 16 primitives"""
    n = boxes.shape[0]
    bins = bins_of(boxes)
    cost, nleft = plane_costs(boxes, bins)
    best = int(np.argmin(cost))                  # the first of equal costs: the smallest axis * 32 + plane
    lo = cost.reshape(-1)[best]
    if not lo < f32(3.0e38):
        return Split(halved(n), "halved", False, -1, 0, n // 2)
    ax, sp = divmod(best, BINS)
    left = bins[:, ax] <= sp
    tied = any(not np.array_equal(bins[:, a] <= p, left) for a, p in zip(*np.nonzero(cost == lo)) if (a, nleft[a, p]) != (ax, nleft[ax, sp]))
    return Split(left, "plane", tied, ax, sp, int(nleft[ax, sp]))


def exact_batch(boxes, count):
    """The exact sweep of M nodes at once: boxes float32 [M, 16, 6] (rows past count[m] are ignored), count int [M], 2 <= count <= 16.
    Returns left [M, 16] bool, winner id (axis * 16 + i, -1 without one) [M], tied [M].
    (c_j < c_i or (c_j == c_i and j <= i)) is (rank_j <= rank_i) in a stable sort by centroid: the sides of candidate i are a prefix and a
    suffix of that order, and their boxes running minima and maxima.)"""
    M = boxes.shape[0]
    j = np.arange(MINI)
    valid = j[None, :] < count[:, None]
    c = centroids(boxes)
    mn = np.where(valid[..., None], boxes[..., :3], _INF); mx = np.where(valid[..., None], boxes[..., 3:], -_INF)
    cost = np.full((M, 3, MINI), _INF, f32)
    lefts = np.zeros((M, 3, MINI, MINI), bool)              # [m, axis, candidate i, primitive j]
    nl = (j + 1)[None, :]; nr = count[:, None] - nl         # by rank
    ok = nr > 0
    with np.errstate(invalid="ignore", over="ignore"):
        for ax in range(3):
            perm = np.argsort(np.where(valid, c[..., ax], _INF), axis=1, kind="stable")
            rank = np.empty_like(perm); np.put_along_axis(rank, perm, np.broadcast_to(j, perm.shape), axis=1)
            smn, smx = np.take_along_axis(mn, perm[..., None], axis=1), np.take_along_axis(mx, perm[..., None], axis=1)
            lmn, lmx = np.minimum.accumulate(smn, axis=1), np.maximum.accumulate(smx, axis=1)
            rmn = np.concatenate([np.minimum.accumulate(smn[:, ::-1], axis=1)[:, ::-1][:, 1:], np.full((M, 1, 3), _INF, f32)], axis=1)
            rmx = np.concatenate([np.maximum.accumulate(smx[:, ::-1], axis=1)[:, ::-1][:, 1:], np.full((M, 1, 3), -_INF, f32)], axis=1)
            k = half_area(np.where(ok[..., None], lmx - lmn, f32(0))) * nl.astype(f32) + half_area(np.where(ok[..., None], rmx - rmn, f32(0))) * nr.astype(f32)
            cost[:, ax] = np.take_along_axis(np.where(ok & ~np.isnan(k), k, _INF), rank, axis=1)
            lefts[:, ax] = (rank[:, None, :] <= rank[:, :, None]) & valid[:, None, :]
    flat = cost.reshape(M, -1)
    win = np.argmin(flat, axis=1)                # the first of equal costs: the smallest axis * 16 + i
    lo = flat[np.arange(M), win]
    has = lo < f32(3.0e38)
    lefts = lefts.reshape(M, 3 * MINI, MINI)
    left = lefts[np.arange(M), win]
    tied = has & ((flat == lo[:, None]) & (lefts != left[:, None, :]).any(axis=2)).any(axis=1)      # ... by a candidate with another left set
    left[~has] = (j[None, :] < (count[:, None] // 2))[~has]
    return left, np.where(has, win, -1), tied


def exact(boxes):
    """the split of a node of at most 16 primitives"""
    n = boxes.shape[0]
    padded = np.zeros((1, MINI, 6), f32); padded[0, :n] = boxes
    left, win, tied = exact_batch(padded, np.array([n]))
    if win[0] < 0:
        return Split(left[0, :n], "halved", False, -1, 0, n // 2)
    return Split(left[0, :n], "exact", bool(tied[0]), int(win[0]) // MINI, int(win[0]) % MINI, int(left[0, :n].sum()))


def split(boxes_in_order, level):
    """The definition's decision for one node: boxes float32 [n, 6] (min xyz, max xyz) in the order of the Morton-sorted array, n >= 2.
    Returns Split(left mask, kind, tied, axis, plane or candidate, n_left)."""
    boxes = np.ascontiguousarray(boxes_in_order, f32)
    n = boxes.shape[0]
    assert n >= 2
    if level >= FORCE_HALVING_FROM:
        return Split(halved(n), "forced", False, -1, 0, n // 2)
    return exact(boxes) if n <= MINI else binned(boxes)


def build(boxes, sorted_prims, split_fn=None):
    """The whole tree, top down: rows float32 [2n-1, 9] as sah_write_leaf / sah_write_inner lay them out (leaf: 1, primitive, box, 0;
    inner: 0, right child, box, 0; pre-order, left = self + 1, right = self + 2 * n_left).  boxes [n, 6] by primitive id, sorted_prims the
    primitive ids in Morton order.  split_fn(boxes_in_order, level, pre) -> left mask replaces the definition's decision (to plant defects)."""
    boxes = np.ascontiguousarray(boxes, f32)
    sorted_prims = np.asarray(sorted_prims, np.int64)
    n = sorted_prims.shape[0]
    rows = np.zeros((2 * n - 1, 9), f32)
    stack = [(np.arange(n), 0, 0)]               # (positions in the sorted array, ascending; pre-order index; level)
    while stack:
        pos, pre, level = stack.pop()
        bx = boxes[sorted_prims[pos]]
        if pos.shape[0] == 1:
            rows[pre, 0] = 1.0; rows[pre, 1] = f32(sorted_prims[pos[0]]); rows[pre, 2:8] = bx[0]
            continue
        left = split(bx, level).left if split_fn is None else np.asarray(split_fn(bx, level, pre), bool)
        nl = int(left.sum())
        assert 0 < nl < pos.shape[0]
        rows[pre, 1] = f32(pre + 2 * nl); rows[pre, 2:5] = bx[:, :3].min(axis=0); rows[pre, 5:8] = bx[:, 3:].max(axis=0)
        stack.append((pos[~left], pre + 2 * nl, level + 1))
        stack.append((pos[left], pre + 1, level + 1))
    return rows


def tri_boxes(tris):
    t = np.asarray(tris, np.float64).astype(f32)
    return np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1)


def peeling_triangles(n_pile, n_out, ratio=1.04):
    """A pile of n_pile triangles with one centroid and n_out more in front of it at distances ratio ** i: [n_pile + n_out, 3, 3], float64.

    A set that keeps a node of n_pile primitives open for n_out levels.  Centroids spaced exponentially do NOT do that by themselves: with
    boxes that grow with the distance the cost s^2 n_L + n_R falls towards the low planes, a split takes 1/32 of the extent and the lot is
    through in log_32 of its range -- ten levels for 1e-3 .. 1e12.  Here every box spans the same [1, 2^39] in y and z and at most
    ratio ** n_out << 2^14 in x, so dy * dz = 2^78 swallows the other two products, every side of every plane has the half area 2^78, every
    cost is 2^78 * count exactly, and the tie goes to plane 0 of axis 0: bin 0, the far end.  ratio > 32 / 31 puts one primitive there.
    No plane on y or z: one centroid for all."""
    assert ratio > 32.0 / 31.0 and ratio ** n_out < 8192.0
    big = 2.0 ** 39
    x = np.concatenate([np.full(n_pile, 1000.0), 1000.0 - ratio ** np.arange(n_out)])
    t = np.zeros((x.shape[0], 3, 3))
    t[:, 0] = np.stack([x - 0.25, np.ones_like(x), np.ones_like(x)], axis=1)
    t[:, 1] = np.stack([x, np.full_like(x, big), np.ones_like(x)], axis=1)
    t[:, 2] = np.stack([x + 0.25, np.ones_like(x), np.full_like(x, big)], axis=1)
    return t


def tree_shape(rows):
    """(leaf flag, subtree size, level, rank of the first leaf under the node in depth-first order) of every row of a pre-order tree"""
    N = rows.shape[0]
    leaf = rows[:, 0] == 1.0
    isleaf, right = leaf.tolist(), rows[:, 1].astype(np.int64).tolist()
    size, level = [1] * N, [0] * N
    for i in range(N - 1, -1, -1):
        if not isleaf[i]:
            size[i] = 1 + size[i + 1] + size[right[i]]
    for i in range(N):
        if not isleaf[i]:
            level[i + 1] = level[right[i]] = level[i] + 1
    first_leaf = np.cumsum(leaf) - leaf
    return leaf, np.asarray(size, np.int64), np.asarray(level, np.int64), first_leaf.astype(np.int64)


def _recover(boxes, left):
    """(axis, plane, n_left) of the binned plane, or the (axis, candidate, n_left) of the exact sweep, that yields this left set; None if none does"""
    n = boxes.shape[0]
    if n > MINI:
        bins = bins_of(boxes)
        for ax in range(3):
            for sp in range(BINS - 1):
                if np.array_equal(bins[:, ax] <= sp, left):
                    return ax, sp, int(left.sum())
    else:
        c = centroids(boxes)
        j = np.arange(n)
        for ax in range(3):
            for i in range(n):
                if np.array_equal((c[:, ax] < c[i, ax]) | ((c[:, ax] == c[i, ax]) & (j <= i)), left):
                    return ax, i, int(left.sum())
    return None


def check_splits(rows, sorted_prims, nodes=None):
    """Every inner node of the downloaded tree (or those listed in `nodes`) split its primitives as the definition does: the leaves under
    it, ordered by position in the Morton-sorted array, with their boxes as the leaf rows hold them, go through split(), and the leaves
    under its left child must be the definition's left set.  Returns a Counter: nodes per size class, per kind, and "tied_<kind>" for winning
    costs that a candidate with another left set meets too (where the tie rule decides the tree)."""
    rows = np.ascontiguousarray(rows, f32)
    sorted_prims = np.asarray(sorted_prims, np.int64)
    n = sorted_prims.shape[0]
    assert rows.shape == (2 * n - 1, 9)
    leaf, size, level, first_leaf = tree_shape(rows)
    where = np.zeros(n, np.int64); where[sorted_prims] = np.arange(n)          # primitive -> position in the sorted array
    leaf_pos = where[rows[leaf, 1].astype(np.int64)]                            # by depth-first leaf rank
    leaf_box = rows[leaf, 2:8]
    nodes = np.flatnonzero(~leaf) if nodes is None else np.asarray(nodes, np.int64)
    assert not leaf[nodes].any()
    count = (size[nodes] + 1) // 2
    nleft = (size[nodes + 1] + 1) // 2
    tally = Counter()

    def ordered(k):
        a = first_leaf[nodes[k]]
        pos = leaf_pos[a:a + count[k]]
        order = np.argsort(pos, kind="stable")
        return leaf_box[a:a + count[k]][order], order < nleft[k]

    def fail(k, want, boxes, got):
        i = int(nodes[k])
        dev, ref = _recover(boxes, got), (want.axis, want.plane, want.n_left)
        raise AssertionError(
            f"node {i}: {int(count[k])} primitives, level {int(level[i])}, size class {size_class(int(count[k]))}, the definition takes a split of "
            f"kind '{want.kind}' with (axis, plane, n_left) = {ref}; the tree has n_left = {int(nleft[k])}, "
            f"{'which is (axis, plane, n_left) = ' + str(dev) if dev else 'a left set no plane or candidate yields'}; "
            f"{int((want.left != got).sum())} primitives on the other side")

    def book(k, kind, tied):
        tally[size_class(int(count[k]))] += 1; tally[kind] += 1
        if tied:
            tally["tied_" + kind] += 1

    mini = np.flatnonzero((count <= MINI) & (level[nodes] < FORCE_HALVING_FROM))
    for lo in range(0, mini.shape[0], 2048):                                    # the exact sweeps, 2048 nodes at a time
        ks = mini[lo:lo + 2048]
        bx = np.zeros((ks.shape[0], MINI, 6), f32); got = np.zeros((ks.shape[0], MINI), bool)
        for m, k in enumerate(ks):
            b, g = ordered(k)
            bx[m, :count[k]] = b; got[m, :count[k]] = g
        want, win, tied = exact_batch(bx, count[ks])
        for m in np.flatnonzero((want != got).any(axis=1)):
            k = ks[m]; b, g = ordered(k)
            fail(k, exact(b), b, g)
        for m, k in enumerate(ks):
            book(k, "exact" if win[m] >= 0 else "halved", tied[m])
    for k in np.flatnonzero((count > MINI) | (level[nodes] >= FORCE_HALVING_FROM)):
        b, g = ordered(k)
        want = split(b, int(level[nodes[k]]))
        if not np.array_equal(want.left, g):
            fail(k, want, b, g)
        book(k, want.kind, want.tied)
    return tally
