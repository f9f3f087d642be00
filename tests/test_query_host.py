"""RayQuery's argument checks on a machine without a GPU: wrong inputs raise TypeError / ValueError before the library is touched
(the scene's context is never created), and without torch RayQuery says it needs it."""
import sys

import numpy as np
import pytest
import torch

from ti_raytrace_amd import RayQuery, _native, scenes


def unbuilt_scene():
    ex = scenes.cornell_box(16, 16, 1, device_id=0)
    assert ex.scene._ctx is None
    return ex.scene


def test_cpu_inputs_are_refused_without_a_context():
    sc = unbuilt_scene()
    q = RayQuery(sc)
    rays = torch.zeros((10, 6), dtype=torch.float32)
    with pytest.raises(TypeError, match="GPU"):
        q.closest(rays)
    with pytest.raises(TypeError, match="GPU"):
        q.occluded(rays, 1.0)
    with pytest.raises(TypeError, match="float32"):
        q.closest(rays.double())
    with pytest.raises(TypeError, match="torch.Tensor"):
        q.closest(np.zeros((10, 6), np.float32))
    with pytest.raises(TypeError):
        q.closest(torch.zeros((10, 6), dtype=torch.float16))
    assert sc._ctx is None


def test_constructor_arguments():
    sc = unbuilt_scene()
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="stack_size"):
            RayQuery(sc, stack_size=bad)
    with pytest.raises(ValueError, match="flags"):
        RayQuery(sc, flags=4)
    q = RayQuery(sc, 128, _native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES)
    assert q.stack_size == 128
    assert sc._ctx is None


def test_without_torch(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError, match="needs PyTorch"):
        RayQuery(unbuilt_scene())
