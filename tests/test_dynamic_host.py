"""Scene.update_vertices without a GPU: its argument checks run before any native call (a stub context records the calls), what it
hands to the context, the host mirrors it refreshes, and the header / binding agreement of the new entry points."""
import os
import re
import sys

import numpy as np
import pytest

from ti_raytrace_amd import _native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tirt_vertex_update", "tirt_vertex_update_device", "tirt_scene_box")


class StubContext:
    """stands where Scene._ctx is: records the calls, moves nothing"""
    device_id = 0

    def __init__(self, nv):
        self.calls = []
        self.rows = np.zeros((nv, 9), np.float32)

    def vertex_update(self, first, count, pos, pos_stride=3, nrm=0, nrm_stride=3, device=False, stream=0):
        self.calls.append(("vertex_update", first, count, pos_stride, bool(nrm), nrm_stride, device, stream))
        src = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_float * (count * pos_stride)).from_address(pos)).reshape(count, pos_stride)
        self.rows[first:first + count, 0:3] = src[:, 0:3]

    def lbvh_build(self):
        self.calls.append(("lbvh_build",))

    def scene_box(self):
        self.calls.append(("scene_box",))
        return np.asarray([-1, -2, -3], np.float32), np.asarray([4, 5, 6], np.float32)

    def vertex_download(self, nv):
        self.calls.append(("vertex_download",))
        return self.rows.copy()

    def process_normal(self, vertex_index):
        self.calls.append(("process_normal",))

    def total_area(self):
        self.calls.append(("total_area",))
        return 2.5


@pytest.fixture
def scene():
    ex = scenes.synthetic(8, 8, 4, ntri=10, device_id=0)
    ex.scene.setup_data_cpu()
    ex.scene._ctx = StubContext(ex.scene.vertex_count)
    return ex.scene


def test_header_and_binding_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "tirt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name), name
    assert len(_native.SIGNATURES["tirt_vertex_update"][1]) == 7 and len(_native.SIGNATURES["tirt_vertex_update_device"][1]) == 8
    decl = re.search(r"int tirt_vertex_update_device\s*\(([^)]*)\)", text).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "first", "count", "pos", "pos_stride", "nrm", "nrm_stride", "stream"]
    src = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "Makefile")).read()
    assert "tirt_dynamic.hip" in src and "-ffp-contract=off" in src and "-fno-fast-math" in src


def test_numpy_update_calls_and_mirrors(scene):
    nv = scene.vertex_count
    new = np.arange(nv * 3, dtype=np.float32).reshape(nv, 3)
    old_min, old_bvh_min = scene.minboundarynp, scene.bvh.minboundarynp
    scene.update_vertices(new)
    ctx = scene._ctx
    assert [c[0] for c in ctx.calls] == ["vertex_update", "lbvh_build", "scene_box"]
    assert ctx.calls[0][1:] == (0, nv, 3, False, 3, False, 0)
    assert scene.minboundarynp is old_min and scene.bvh.minboundarynp is old_bvh_min and old_min is old_bvh_min
    assert scene.minboundarynp.tolist() == [[-1, -2, -3]] and scene.bvh.maxboundarynp.tolist() == [[4, 5, 6]]
    assert np.array_equal(scene.vertex_np[:, 0:3], new)     # lazily, from the context
    assert [c[0] for c in ctx.calls][3:] == ["vertex_download"]
    scene.vertex_np
    assert len(ctx.calls) == 4                              # once
    # [k/3, 3, 3], a range, a view that is not contiguous, normals
    del ctx.calls[:]
    wide = np.zeros((6, 3, 5), np.float32); wide[:, :, 1:4] = 7.0
    scene.update_vertices(wide[:, :, 1:4], normals=np.ones((18, 3), np.float32), first_vertex=6)
    assert ctx.calls[0][1:] == (6, 18, 3, True, 3, False, 0)
    assert (scene.vertex_np[6:24, 0:3] == 7.0).all() and (scene.vertex_np[0:6, 0:3] == new[0:6]).all()
    del ctx.calls[:]
    scene.update_vertices(new[:0])
    assert ctx.calls == []


def test_no_torch_import_for_numpy_positions():
    import subprocess
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_dynamic_host as t\n"
            "from ti_raytrace_amd import scenes\n"
            "ex = scenes.synthetic(8, 8, 4, ntri=4, device_id=0); ex.scene.setup_data_cpu(); ex.scene._ctx = t.StubContext(12)\n"
            "ex.scene.update_vertices(np.zeros((12, 3), np.float32))\n"
            "assert 'torch' not in sys.modules, 'update_vertices imported torch'\n" % (ROOT, os.path.join(ROOT, "tests")))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_process_normal_and_light_area_follow(scene):
    scene.total_area()
    scene.total_area()                                      # accumulates, like the reference's +=
    assert scene.light_area.to_numpy()[0] == 5.0
    scene.process_normal()
    del scene._ctx.calls[:]
    scene.update_vertices(np.zeros((scene.vertex_count, 3), np.float32))
    assert [c[0] for c in scene._ctx.calls] == ["vertex_update", "lbvh_build", "scene_box", "vertex_download", "process_normal", "total_area"]
    assert scene.light_area.to_numpy()[0] == 2.5            # what a fresh scene holds after one total_area()


@pytest.mark.parametrize("make,exc,match", [
    (lambda nv: [[0.0, 0.0, 0.0]] * 3, TypeError, "numpy array or a torch.Tensor"),
    (lambda nv: np.zeros((3, 3), np.float64), TypeError, "must be float32"),
    (lambda nv: np.zeros((3, 3), np.int32), TypeError, "must be float32"),
    (lambda nv: np.zeros((3, 4), np.float32), ValueError, r"\[k, 3\] or \[k/3, 3, 3\]"),
    (lambda nv: np.zeros(9, np.float32), ValueError, r"\[k, 3\] or \[k/3, 3, 3\]"),
    (lambda nv: np.zeros((2, 2, 3), np.float32), ValueError, r"\[k, 3\] or \[k/3, 3, 3\]"),
    (lambda nv: np.zeros((4, 3), np.float32), ValueError, "whole triangles"),
    (lambda nv: np.zeros((nv + 3, 3), np.float32), ValueError, "past the scene"),
])
def test_bad_positions_are_refused_before_any_native_call(scene, make, exc, match):
    with pytest.raises(exc, match=match):
        scene.update_vertices(make(scene.vertex_count))
    assert scene._ctx.calls == []


def test_bad_ranges_and_normals_are_refused_before_any_native_call(scene):
    ok = np.zeros((6, 3), np.float32)
    for first in (1, -3, 2.5):
        with pytest.raises(ValueError, match="first_vertex"):
            scene.update_vertices(ok, first_vertex=first)
    with pytest.raises(ValueError, match="past the scene"):
        scene.update_vertices(ok, first_vertex=scene.vertex_count - 3)
    with pytest.raises(ValueError, match="normals hold 3 vertices, positions 6"):
        scene.update_vertices(ok, normals=np.zeros((3, 3), np.float32))
    with pytest.raises(TypeError, match="normals must be float32"):
        scene.update_vertices(ok, normals=np.zeros((6, 3), np.float64))
    assert scene._ctx.calls == []


def test_a_scene_that_is_not_on_the_device_is_refused():
    ex = scenes.synthetic(8, 8, 4, ntri=4, device_id=0)
    with pytest.raises(RuntimeError, match="not on the device"):
        ex.scene.update_vertices(np.zeros((12, 3), np.float32))
    assert ex.scene._ctx is None                            # and no context was made for the refusal


def test_host_tensors_and_mixed_kinds_are_refused(scene):
    import torch
    with pytest.raises(TypeError, match="tensor on the GPU, got a cpu tensor"):
        scene.update_vertices(torch.zeros((6, 3)))
    with pytest.raises(TypeError, match="must be float32"):
        scene.update_vertices(torch.zeros((6, 3), dtype=torch.float64))
    assert scene._ctx.calls == []


def test_partial_update_of_a_smoothed_scene_restores_the_other_rows_first(scene):
    """process_normal smooths what it finds: the rows a partial update leaves alone get their un-smoothed normals back before it runs again"""
    scene.process_normal()
    raw = scene.vertex_np.copy()
    ctx = scene._ctx
    seen = []
    plain = ctx.vertex_update

    def recording(first, count, pos, pos_stride=3, nrm=0, nrm_stride=3, device=False, stream=0):
        if nrm:
            rows = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_float * (count * pos_stride)).from_address(pos)).reshape(count, pos_stride)
            seen.append((first, rows.copy(), nrm - pos))
        plain(first, count, pos, pos_stride, nrm, nrm_stride, device, stream)
    ctx.vertex_update = recording
    del ctx.calls[:]
    scene.update_vertices(np.zeros((6, 3), np.float32), first_vertex=6)
    assert [c[:3] for c in ctx.calls[:3]] == [("vertex_update", 6, 6), ("vertex_update", 0, 6), ("vertex_update", 12, scene.vertex_count - 12)]
    assert [c[0] for c in ctx.calls[3:]] == ["lbvh_build", "scene_box", "vertex_download", "process_normal"]
    assert [c[3:6] for c in ctx.calls[1:3]] == [(6, True, 6)] * 2           # rows of six floats: position, normal
    assert seen[0][0] == 0 and np.array_equal(seen[0][1], raw[0:6, 0:6]) and seen[0][2] == 12
    assert seen[1][0] == 12 and np.array_equal(seen[1][1], raw[12:, 0:6]) and seen[1][2] == 12
