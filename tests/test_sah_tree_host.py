"""The restated definition of the traversal tree (sah_tree_expected.py) and its checker have to bite.  No device.

build() yields trees that check_tree (the old suite's whole demand on tirt_sah.hip) and check_splits accept; the vectorised costs pick what
a brute-force evaluation over sets picks; and eight single defects planted in a correct tree -- each leaves a perfectly valid tree, which
check_tree goes on accepting -- are rejected by check_splits with the node named in the message."""
import numpy as np
import pytest

import sah_tree_expected as se
from common import hostile_triangles
from test_gpu_tree import check_tree

f32 = np.float32


def soup(n, seed, spread=0.1):
    r = np.random.RandomState(seed)
    return r.uniform(-1, 1, (n, 1, 3)) + r.uniform(-spread, spread, (n, 3, 3))


def duplicates(seed=3):
    r = np.random.RandomState(seed)
    tris = []
    for c in r.uniform(-1, 1, (30, 3)):
        for _ in range(r.randint(1, 7)):
            a = r.uniform(-0.05, 0.05, (3,)); b = r.uniform(-0.05, 0.05, (3,))
            tris.append(c[None, :] + np.stack([a, -a, b * [1, 0, 0]]))            # (not all of one centroid in fp32: as in a scene)
    return np.asarray(tris)


def lattice():
    """64 equal boxes on a 4 x 4 x 4 grid: mirror-image planes cost the same"""
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(4.0), indexing="ij"), axis=-1).reshape(-1, 1, 3)
    return g + np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.25], [0.0, 0.25, 0.25]])[None]


INPUTS = {
    "soup2": lambda: soup(2, 1), "soup3": lambda: soup(3, 2), "soup5": lambda: soup(5, 3), "soup16": lambda: soup(16, 4),
    "soup17": lambda: soup(17, 5), "soup33": lambda: soup(33, 6), "soup65": lambda: soup(65, 7), "soup200": lambda: soup(200, 8),
    "soup600": lambda: soup(600, 9, 0.03),
    "soup12": lambda: soup(12, 181, 0.3),             # (two centroids share a bin where the exact sweep cuts between them)
    "duplicates": duplicates,
    "identical": lambda: hostile_triangles("identical", np.random.RandomState(7))[:300],
    "exponential": lambda: hostile_triangles("exponential", np.random.RandomState(7)),
    "lattice": lattice,
    "peeling": lambda: se.peeling_triangles(40, 80),
}
_cache = {}


def case(name):
    """(boxes by primitive, primitives in a stand-in for the Morton order, the definition's rows); built once"""
    if name not in _cache:
        boxes = se.tri_boxes(INPUTS[name]())
        order = np.random.RandomState(len(name)).permutation(boxes.shape[0])
        _cache[name] = (boxes, order, se.build(boxes, order))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_build_yields_a_tree_that_both_checkers_accept(name):
    boxes, order, rows = case(name)
    check_tree(rows, boxes)
    tally = se.check_splits(rows, order)
    n = boxes.shape[0]
    assert sum(tally[c] for c in se.CLASSES) == n - 1 == sum(tally[k] for k in se.KINDS)
    if name == "identical":
        assert tally["halved"] > 0 and tally["plane"] == 0
    if name == "peeling":
        assert tally["forced"] >= 20 and tally["tied_plane"] >= 40
        _, _, level, _ = se.tree_shape(rows)
        assert level.max() >= 64
    if name == "lattice":
        assert tally["tied_plane"] > 0 and tally["tied_exact"] > 0
    # a subset of the nodes, as the large scene's test asks for
    some = np.flatnonzero(rows[:, 0] == 0.0)[::3]
    assert sum(se.check_splits(rows, order, some)[c] for c in se.CLASSES) == some.shape[0]


def scalar_cost(boxes, left):
    def area(b):
        d = b[:, 3:].max(axis=0) - b[:, :3].min(axis=0)
        return f32(f32(f32(d[0] * d[1]) + f32(d[1] * d[2])) + f32(d[2] * d[0]))
    return f32(f32(area(boxes[left]) * f32(left.sum())) + f32(area(boxes[~left]) * f32((~left).sum())))


@pytest.mark.parametrize("n,seed", [(17, 1), (40, 2), (64, 3), (65, 4), (300, 5), (1000, 6)])
def test_binned_split_is_the_brute_force_one(n, seed):
    """every plane priced from the SETS on its two sides, one plane after the other"""
    boxes = se.tri_boxes(soup(n, seed, 0.3))
    c = se.centroids(boxes)
    best, best_id = f32(3.0e38), None
    for ax in range(3):
        ext = f32(c[:, ax].max() - c[:, ax].min())
        scale = f32(32.0) / ext
        b = np.clip(((c[:, ax] - c[:, ax].min()) * scale).astype(np.int32), 0, 31)
        for sp in range(31):
            left = b <= sp
            if left.all() or not left.any():
                continue
            k = scalar_cost(boxes, left)
            if k < best:
                best, best_id = k, (ax, sp, int(left.sum()))
    got = se.split(boxes, 0)
    assert got.kind == "plane" and (got.axis, got.plane, got.n_left) == best_id


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (7, 3), (12, 4), (16, 5)])
def test_exact_split_is_the_brute_force_one(n, seed):
    r = np.random.RandomState(seed)
    boxes = se.tri_boxes(soup(n, seed, 0.3))
    boxes[r.randint(0, n, 3)] = boxes[0]                       # equal centroids: the j <= i rule
    c = se.centroids(boxes)
    best, best_id = f32(3.0e38), None
    for ax in range(3):
        for i in range(n):
            left = np.array([c[j, ax] < c[i, ax] or (c[j, ax] == c[i, ax] and j <= i) for j in range(n)])
            if left.all():
                continue
            k = scalar_cost(boxes, left)
            if k < best:
                best, best_id = k, (ax, i, left)
    got = se.split(boxes, 0)
    assert got.kind == "exact" and (got.axis, got.plane) == best_id[:2] and np.array_equal(got.left, best_id[2])


def test_forced_halving_and_size_classes():
    boxes = se.tri_boxes(soup(40, 1))
    for n in (2, 3, 16, 17, 40):
        assert np.array_equal(se.split(boxes[:n], 64).left, np.arange(n) < n // 2) and se.split(boxes[:n], 64).kind == "forced"
        assert se.split(boxes[:n], 63).kind == ("exact" if n <= 16 else "plane")
    assert [se.size_class(k) for k in (2, 16, 17, 64, 65, 512, 513, 8192, 8193)] == ["mini", "mini", "subtree", "subtree", "small", "small", "large", "large", "huge"]


# ---- planted defects -------------------------------------------------------------------------------------------------------------
def valid(mask, want):
    return mask is not None and mask.any() and not mask.all() and not np.array_equal(mask, want.left)


def neighbouring_plane(bx, level, pre, want):
    if want.kind == "plane":
        return se.bins_of(bx)[:, want.axis] <= want.plane + 1


def other_axis_same_count(bx, level, pre, want):
    if want.kind == "plane":
        bins = se.bins_of(bx)
        for ax in range(3):
            for sp in range(31):
                m = bins[:, ax] <= sp
                if ax != want.axis and m.sum() == want.n_left and not np.array_equal(m, want.left):
                    return m


def tie_upwards(bx, level, pre, want):
    if want.kind == "plane" and want.tied:
        bins = se.bins_of(bx)
        cost, _ = se.plane_costs(bx, bins)
        ax, sp = divmod(int(np.flatnonzero(cost.reshape(-1) == cost.min())[-1]), 32)
        return bins[:, ax] <= sp


def one_primitive_across(bx, level, pre, want):
    if want.kind == "plane" and want.n_left >= 2:
        m = want.left.copy(); m[np.flatnonzero(m)[-1]] = False
        return m


def right_order_reversed(bx, level, pre, want):
    """under a halving root the right child's range is handed over back to front: ITS halves change places"""
    if want.kind == "halved" and level == 1 and pre > 1:
        return se.halved(bx.shape[0])[::-1]


def halving_from_63(bx, level, pre, want):
    if level == 63:
        return se.halved(bx.shape[0])


def halving_from_65(bx, level, pre, want):
    if level == 64:
        return se.split(bx, 0).left


def binned_in_a_12_node(bx, level, pre, want):
    if bx.shape[0] == 12 and want.kind == "exact":
        return se.binned(bx).left


DEFECTS = [
    ("soup600", neighbouring_plane, "kind 'plane'"),
    ("soup600", other_axis_same_count, "kind 'plane'"),
    ("lattice", tie_upwards, "kind 'plane'"),
    ("soup600", one_primitive_across, "a left set no plane or candidate yields"),
    ("identical", right_order_reversed, "kind 'halved'"),
    ("peeling", halving_from_63, "level 63"),
    ("peeling", halving_from_65, "level 64"),
    ("soup12", binned_in_a_12_node, "12 primitives"),
]


@pytest.mark.parametrize("name,defect,says", DEFECTS, ids=[d[1].__name__ for d in DEFECTS])
def test_a_planted_defect_is_rejected(name, defect, says):
    boxes, order, good = case(name)
    planted = []

    def split_fn(bx, level, pre):
        want = se.split(bx, level)
        if not planted:
            m = defect(bx, level, pre, want)
            if valid(m, want):
                planted.append(pre)
                return m
        return want.left
    rows = se.build(boxes, order, split_fn)
    assert len(planted) == 1, "the input has a node to plant this defect in"
    assert not np.array_equal(rows, good)
    check_tree(rows, boxes)                                      # still a tree: the old suite sees nothing
    with pytest.raises(AssertionError, match=rf"node {planted[0]}: .*{says}"):
        se.check_splits(rows, order)
    # ... and nothing else is wrong with it: every node but the planted one passes
    others = np.setdiff1d(np.flatnonzero(rows[:, 0] == 0.0), planted)
    se.check_splits(rows, order, others)
