"""The traversal tree held to its definition, node by node (ti_raytrace_amd/csrc/tirt_sah.hip against sah_tree_expected.py).

test_gpu_tree.py asks that the rows ARE a tree; every hit is re-verified against the reference's LBVH, so no film can tell a good tree
from a bad one.  Here every inner node must have split its primitives exactly as the header of tirt_sah.hip says -- bins, costs, tie
rule, stable order, halving -- on scenes that put the root, and both sides of every threshold, into each of the five code paths
(exact sweep <= 16 < k_sah_subtree's bins <= 64 < k_sah_level<1> <= 512 < k_sah_level<16> <= 8192 < the chunked k_sah_huge_*).
test_the_scenes_reach_every_path says what the scenes together have exercised: a pass of the others means nothing without it."""
from collections import Counter

import numpy as np
import pytest

import sah_tree_expected as se
from ti_raytrace_amd import scenes
from common import custom_scene, duplicate_code_scene, hostile_triangles, long_chain_scene, tiny_scene
from test_gpu_tree import check_tree, prim_boxes

pytestmark = pytest.mark.gpu


def soup(count):
    """a uniform soup of `count` primitives: count - 1 triangles and the sphere light"""
    return lambda: tiny_scene(count - 1, seed=count, W=16, H=16, spread=0.5 if count <= 5 else (0.1 if count <= 3000 else 0.03), device_id=0)


def hostile(kind):
    return lambda: custom_scene(hostile_triangles(kind, np.random.RandomState(7)), W=16, H=16)


def cube_tri(c, s):
    """a triangle whose box is c -+ s (all of it in binary fractions: mirror images have the same cost to the bit)"""
    c = np.asarray(c, float); s = np.asarray(s, float) * np.ones(3)
    return np.stack([c + s * [-1, -1, -1], c + s * [1, 1, -1], c + s * [0, 0, 1]])


def giant_at_the_top():
    """31 small triangles along x, one per bin, and a giant alone in bin 31: the LAST plane (bins <= 30 | bin 31) is the cheapest by far"""
    tris = [cube_tri((k, 0, 0), 0.125) for k in range(31)] + [cube_tri((31, 0, 0), (0.125, 64, 64))]
    return custom_scene(np.asarray(tris), W=16, H=16, spheres=((15.5, 0.0, 0.0, 1.0),))


def mirror_tie():
    """Three equal triangles in a row, the middle one a little off the line -- so that it is the last of them in Morton order -- and the light far
    away.  Cutting before or behind the middle one costs the same to the bit; which of the two wins hangs on the candidates' numbers alone."""
    tris = [cube_tri((0, 0, 0), 0.125), cube_tri((1, 0.125, 0), 0.125), cube_tri((2, 0, 0), 0.125)]
    return custom_scene(np.asarray(tris), W=16, H=16, spheres=((1.0, 0.0, 40.0, 0.125),))


# name -> (scene, primitives aimed for with the lights, check every node)
SCENES = {f"soup{c}": (soup(c), c, True) for c in (2, 3, 5, 16, 17, 33, 64, 65, 200, 512, 513, 3000, 8192, 8193, 20000)}
SCENES.update({
    "soup66000": (soup(66000), 66000, False),                  # a root of 65 chunks (k_sah_huge_eval's carry loop), huge children of huge nodes
    "duplicates": (lambda: duplicate_code_scene(W=16, H=16, device_id=0), None, True),
    "long_chain": (lambda: long_chain_scene(W=16, H=16, device_id=0), 631, True),
    "exponential": (hostile("exponential"), 301, True),
    "identical": (hostile("identical"), 3001, True),           # halving by position from the root: where a broken stable order shows
    "two_clusters": (hostile("two_clusters"), 5041, True),
    "one_point": (lambda: tiny_scene(5000, seed=6, W=16, H=16, spread=0.0001, device_id=0), 5001, True),
    "cornell": (lambda: scenes.cornell_box(16, 16, 4, device_id=0), None, True),      # zero-thickness boxes: zero areas, tied costs
    "teapot": (lambda: scenes.single_model(16, 16, 4, device_id=0), None, True),
    # a pile of 8900 behind 100 exponentially spaced triangles (sah_tree_expected.peeling_triangles): every split peels ONE primitive off a huge node
    # (leaf children of huge nodes), and the pile is still whole at level 64: the halving arm of the k_sah_huge_* kernels
    "peeling": (lambda: custom_scene(se.peeling_triangles(8900, 100), W=16, H=16), 9001, True),
    # two sets for the mutants of the kernels that every other scene let through (docs/HISTORY.md)
    "giant_at_the_top": (giant_at_the_top, 33, True),
    "mirror_tie": (mirror_tie, 4, True),
})
_done = {}


def checked(name):
    """(rows, Morton order, boxes by primitive, tally of check_splits) of a scene, built and checked once"""
    if name not in _done:
        make, aimed, every = SCENES[name]
        ex = make(); ex.build_scene()
        sc = ex.scene
        n = sc.primitive_count
        assert aimed is None or n == aimed
        rows = sc.ctx.traversal_tree_download(n)
        order = sc.ctx.lbvh_download(n, want_bvh=False, want_compact=False)[0][:, 1]
        sc.ctx.close()                                         # (27 contexts: freed here, not whenever the collector finds them)
        check_tree(rows, prim_boxes(sc), np.flatnonzero(sc.primitive_np[:, 0] != 1))
        nodes = None
        if not every:                                          # every node of more than 64 primitives and 2500 of the others
            leaf, size, _, _ = se.tree_shape(rows)
            big = ~leaf & (size > 2 * 64 - 1)
            rest = np.flatnonzero(~leaf & ~big)
            nodes = np.concatenate([np.flatnonzero(big), np.random.RandomState(1).choice(rest, 2500, replace=False)])
        tally = se.check_splits(rows, order, nodes)
        assert sum(tally[c] for c in se.CLASSES) == (n - 1 if every else nodes.shape[0])
        boxes = np.zeros((n, 6), np.float32)
        boxes[rows[rows[:, 0] == 1.0, 1].astype(np.int64)] = rows[rows[:, 0] == 1.0, 2:8]     # as the leaf rows hold them (spheres padded)
        _done[name] = (rows, order, boxes, tally)
    return _done[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_every_node_splits_as_defined(gpu_ctx_ok, name):
    rows, order, boxes, tally = checked(name)
    count = rows.shape[0] // 2 + 1
    assert tally[se.size_class(count)] >= 1                    # the root
    if name == "soup66000":
        leaf, size, _, _ = se.tree_shape(rows)
        assert count > 64 * 1024 and tally["huge"] >= 3        # more chunks than a wave has lanes; huge nodes below the huge root
        assert tally["huge"] + tally["large"] + tally["small"] == (~leaf & (size > 2 * 64 - 1)).sum()
    if name == "giant_at_the_top":
        assert rows[0, 1] == 2 * 32 and se.split(boxes[order], 0)[1:] == ("plane", False, 0, 30, 32)
    if name == "mirror_tie":
        three = boxes[order][np.isin(order, (0, 1, 2))]
        assert order[np.isin(order, (0, 1, 2))][-1] == 1 and se.split(three, 1)[1:] == ("exact", True, 0, 0, 1)
    if name == "identical":
        assert tally["plane"] == 1 and tally["halved"] >= 100      # (the one plane: the root's, between the light and the triangles)
    if name == "peeling":
        leaf, size, level, _ = se.tree_shape(rows)
        open64 = ~leaf & (level == 64) & (size > 2 * 8192 - 1)
        assert open64.sum() == 1, "a node of more than 8192 primitives is still open at level 64"
        huge = np.flatnonzero(~leaf & (size > 2 * 8192 - 1))
        assert (leaf[huge + 1] | leaf[rows[huge, 1].astype(np.int64)]).sum() >= 60, "leaf children of huge nodes"
        assert tally["forced"] >= 8000 and tally["tied_plane"] >= 60


@pytest.mark.parametrize("name", ["soup17", "soup513", "duplicates"])
def test_whole_tree_is_the_definitions_bit_for_bit(gpu_ctx_ok, name):
    """the same statement from the other end: built top down from the definition, the rows are the device's"""
    rows, order, boxes, _ = checked(name)
    want = se.build(boxes, order)
    assert np.array_equal(want.view(np.uint32), rows.view(np.uint32))


def test_the_scenes_reach_every_path(gpu_ctx_ok):
    total = Counter()
    for name in SCENES:
        total.update(checked(name)[3])
    for key in se.CLASSES + se.KINDS:
        assert total[key] >= 20, f"{key}: {total[key]} nodes over all scenes"
    assert total["tied_plane"] >= 1 and total["tied_exact"] >= 1
