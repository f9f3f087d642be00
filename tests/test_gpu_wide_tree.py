"""What k_trace<ordered>, the beam kernels and the ray queries walk -- cnode, tri, wnode, prim_slot, the grid, the chain nodes of
far-origin rays -- downloaded (tirt_wide_tree_download) and held to its definition: check_wide_invariants and, bit for bit, the canonical
form of cnode against the greedy collapse restated in numpy (wide_tree_expected.py).  Structure only: no test here launches a ray.  Every
case builds its own small scene, with the binned-SAH traversal tree (option "traversal_tree" 1) and on the reference's LBVH (0: the rows
are compact_node and no sphere slot is boxed).  The experiments-only "wide_collapse" grouping is not covered: it is a different collapse
and would need its own restatement.

The figures each case prints (pytest -s): the smallest containment slack and the largest outward distance of a plane, in cells."""
import ctypes

import numpy as np
import pytest

import wide_tree_expected as wt
from common import custom_scene, duplicate_code_scene, hostile_triangles, long_chain_scene, tiny_scene
from ti_raytrace_amd import scenes, _native

pytestmark = pytest.mark.gpu


def check_built(ex, tree=None, label=""):
    sc = ex.scene
    ctx, n = sc.ctx, sc.primitive_count
    dl = ctx.wide_tree_download(n)
    rows = ctx.traversal_tree_download(n)
    compact = ctx.lbvh_download(n, want_morton=False, want_bvh=False)[2]
    vertex = ctx.vertex_download(sc.vertex_count) if sc.vertex_count else np.zeros((0, 9), np.float32)
    assert dl["cnode"].shape == (dl["wide_nodes"] + dl["n_far_nodes"], 16) and dl["tri"].shape == (n, 12) and dl["wnode"].shape == (2 * n - 1, 16)
    if tree == 0:
        assert dl["built_sah"] == 0 and dl["shapes_boxed"] == 0 and np.array_equal(rows.view(np.uint32), compact.view(np.uint32))
    elif n >= 2:
        assert dl["built_sah"] == 1
    lo, hi = dl["root_min"].astype(np.float32), dl["root_max"].astype(np.float32)
    e = hi - lo
    assert dl["pad"] == np.float32(1.0e-4) * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], dtype=np.float32)
    assert np.array_equal(lo, compact[0, 2:5]) and np.array_equal(hi, compact[0, 5:8])
    st = wt.check_wide_invariants(dl, rows, sc.primitive_np, vertex, sc.shape_np, compact, ctx.bvh_info())
    is_shape = sc.primitive_np[:, 0] != wt.PRIMITIVE_TRI
    want = wt.expected_wide(rows, is_shape, dl["prim_slot"], dl, dl["pad"], dl["shapes_boxed"])
    got = wt.canonical(dl["cnode"], dl["wide_nodes"], rows, dl["prim_slot"])
    assert len(got) == dl["wide_nodes"]
    wt.assert_same_canonical(got, want)
    print("wide tree %s tree=%s: n %d, %d wide + %d chain nodes, min slack %.4f cells, max outward %.3f cells"
          % (label, tree, n, dl["wide_nodes"], dl["n_far_nodes"], st["min_slack"], st["max_outward"]))
    return dl, st


def build_and_check(make, tree, label=""):
    ex = make()
    if tree is not None:
        ex.scene.ctx.set_option("traversal_tree", tree)
    ex.build_scene()
    return check_built(ex, tree, label)


@pytest.mark.parametrize("tree", [1, 0])
@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 5, 6, 7, 9, 17, 64, 65, 129, 257, 3000])
def test_tiny_scenes(gpu_ctx_ok, ntri, tree):
    """root with a leaf child, partial nodes, the dissolve rule; levels of one wave, a ragged wave, two waves of a block, several blocks"""
    build_and_check(lambda: tiny_scene(ntri, seed=ntri, W=16, H=16, device_id=0), tree, "tiny %d" % ntri)


@pytest.mark.parametrize("kind", ["tri", "sphere"])
def test_one_primitive(gpu_ctx_ok, kind):
    """n == 1: no wide node, root_code is the leaf code (with the shape bit for a sphere)"""
    tris = [[[0, 0, 0], [1, 0, 0], [0, 1, 0]]] if kind == "tri" else np.zeros((0, 3, 3))
    dl, _ = build_and_check(lambda: custom_scene(tris, 16, 16, spheres=() if kind == "tri" else ((0.1, 0.2, -0.1, 0.75),)), None, "one " + kind)
    assert dl["wide_nodes"] == 0 and (dl["root_code"] & 0xffffffff) == (0xffffffff if kind == "tri" else 0xbfffffff)


@pytest.mark.parametrize("tree", [1, 0])
@pytest.mark.parametrize("name", ["cornell", "duplicates"])
def test_cornell_and_duplicate_codes(gpu_ctx_ok, name, tree):
    """a mesh light and zero-thickness axis-aligned boxes; runs of equal Morton codes"""
    make = (lambda: scenes.cornell_box(16, 16, 4, device_id=0)) if name == "cornell" else (lambda: duplicate_code_scene(16, 16, device_id=0))
    build_and_check(make, tree, name)


def test_very_long_chain_on_the_lbvh(gpu_ctx_ok):
    """600 triangles with one Morton code on the reference's tree: ~200 wide levels, build_wide's batches of 16 levels many times over"""
    dl, _ = build_and_check(lambda: long_chain_scene(16, 16), 0, "600-chain")
    codes = dl["cnode"][:dl["wide_nodes"], 12:16]
    depth = np.zeros(dl["wide_nodes"], np.int64)
    for i in range(dl["wide_nodes"]):
        for c in codes[i]:
            if not int(c) & 0x80000000:
                depth[int(c)] = depth[i] + 1
    assert depth.max() >= 150


@pytest.mark.parametrize("tree", [1, 0])
@pytest.mark.parametrize("kind", ["one_point", "exponential", "two_clusters"])
def test_hostile_distributions(gpu_ctx_ok, kind, tree):
    """SAH range halving, and planes near +-30000 cells where the spacing of fp16 is 16 cells"""
    if kind == "one_point":
        make = lambda: tiny_scene(5000, seed=6, W=16, H=16, spread=1e-4, device_id=0)
    else:
        make = lambda: custom_scene(hostile_triangles(kind, np.random.RandomState(7)), 16, 16)
    build_and_check(make, tree, kind)


@pytest.mark.parametrize("tree", [1, 0])
@pytest.mark.parametrize("kind", ["flat", "offset"])
def test_flat_and_offset_scenes(gpu_ctx_ok, kind, tree):
    """flat: every triangle in the plane z = 0, one grid axis spans 2 * pad only;  offset: 300 small triangles far from the origin, float32
    positions coarse against the cell"""
    r = np.random.RandomState(21)
    if kind == "flat":
        tris = r.uniform(-1, 1, (300, 1, 3)) + r.uniform(-0.1, 0.1, (300, 3, 3))
        tris[:, :, 2] = 0.0
    else:
        tris = r.uniform(-1, 1, (300, 1, 3)) + r.uniform(-0.05, 0.05, (300, 3, 3)) + np.array([1e5, -3e4, 7e5])
    build_and_check(lambda: custom_scene(tris, 16, 16, spheres=()), tree, kind)


@pytest.mark.parametrize("tree", [1, 0])
@pytest.mark.parametrize("count", [1, 3, 4, 8, 9])
def test_sphere_lights_and_chain_nodes(gpu_ctx_ok, count, tree):
    """one chain node without a link, a full one without, a full one with a link, three chain nodes; nine spheres: whole-grid slots, no chain"""
    tris = scenes.synthetic_triangles(200, 77, 0.2)
    spheres = [(1.6 * np.cos(k), 0.4 * k - 1.5, 1.6 * np.sin(k), 0.25) for k in range(count)]
    dl, _ = build_and_check(lambda: custom_scene(tris, 16, 16, spheres=spheres), tree, "%d spheres" % count)
    if tree == 1:
        assert (dl["shapes_boxed"], dl["n_far_nodes"]) == {1: (1, 1), 3: (1, 1), 4: (1, 2), 8: (1, 3), 9: (0, 0)}[count]
        if count == 4:
            assert dl["cnode"][dl["wide_nodes"], 15] == dl["wide_nodes"] + 1


@pytest.mark.parametrize("name", ["teapot", "synthetic"])
def test_large_scenes(gpu_ctx_ok, name):
    make = (lambda: scenes.single_model(16, 16, 4, device_id=0)) if name == "teapot" else (lambda: scenes.synthetic(16, 16, 4, device_id=0))
    dl, _ = build_and_check(make, None, name)
    assert dl["prim_slot"].shape[0] == (25201 if name == "teapot" else 100001)


def test_after_update_vertices(gpu_ctx_ok):
    ex = tiny_scene(3000, seed=5, W=16, H=16, device_id=0)
    ex.build_scene()
    check_built(ex, None, "before the move")
    r = np.random.RandomState(4)
    pos = ex.scene.vertex_np[:, :3].reshape(-1, 3, 3)
    moved = (pos.mean(axis=1, keepdims=True) * np.float32(1.5) + (pos - pos.mean(axis=1, keepdims=True)) * r.uniform(0.5, 2.0, (pos.shape[0], 1, 1))).astype(np.float32)
    ex.scene.update_vertices(moved)
    assert np.array_equal(ex.scene.ctx.vertex_download(ex.scene.vertex_count)[:, :3].view(np.uint32), moved.reshape(-1, 3).view(np.uint32))
    check_built(ex, None, "after the move")


def test_refusals(gpu_ctx_ok):
    """an unbuilt context and a null pointer: the argument error, and nothing is written"""
    L = _native.lib()
    grid = np.full(19, 7.0, np.float32); info = np.full(6, 7, np.int32); cnode = np.full((8, 16), 7, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ctx = _native.Context(0)
    assert L.tirt_wide_tree_download(ctx.handle, p(cnode), None, None, None, p(grid), p(info)) == -2          # TIRT_ERR_ARG
    with pytest.raises(_native.TirtError):
        ctx.wide_tree_download(4)
    ex = tiny_scene(3, seed=3, W=16, H=16, device_id=0); ex.build_scene()
    h = ex.scene.ctx.handle
    assert L.tirt_wide_tree_download(h, p(cnode), None, None, None, None, p(info)) == -2
    assert L.tirt_wide_tree_download(h, p(cnode), None, None, None, p(grid), None) == -2
    assert L.tirt_wide_tree_download(None, p(cnode), None, None, None, p(grid), p(info)) == -2
    assert (grid == 7.0).all() and (info == 7).all() and (cnode == 7).all()
    assert L.tirt_wide_tree_download(h, None, None, None, None, p(grid), p(info)) == 0 and info[0] >= 1 and (cnode == 7).all()
