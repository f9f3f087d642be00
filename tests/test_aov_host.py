"""The feature buffers (tirt_aov_*) without a device: the header, the binding and the Python surface agree, and the expected-value helper the
GPU tests hold the device to (tests/aov_expected.py) computes the recurrence a hand computation gives."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np

import aov_expected as ae
from ti_raytrace_amd import Example, PT_RGB, PT_Spec, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tirt.h")).read()
f = np.float32


def test_entry_points_are_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, nargs in (("tirt_aov_enable", 2), ("tirt_aov_download", 2), ("tirt_aov_export_device", 2)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_native.lib(), name), name
    for method in ("aov_enable", "aov_download", "aov_export_device"):
        assert callable(getattr(_native.Context, method))


def test_word_offsets_equal_the_header():
    defs = dict(re.findall(r"#define\s+TIRT_AOV_([A-Z]+)\s+(\d+)", HEADER))
    assert sorted(defs) == ["ALBEDO", "ALPHA", "DEPTH", "NORMAL", "WORDS"]
    for name, value in defs.items():
        assert getattr(_native, "AOV_" + name) == int(value), name
    assert (_native.AOV_ALBEDO, _native.AOV_NORMAL, _native.AOV_DEPTH, _native.AOV_ALPHA, _native.AOV_WORDS) == (0, 3, 6, 7, 8)


def test_the_keyword_goes_last_and_defaults_to_off():
    for cls in (PT_RGB.PathTrace, PT_Spec.PathTrace):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "aov" and params[-1].default is False, cls
        for method in ("aov_to_numpy", "aov_to_torch"):
            assert callable(getattr(cls, method))
    assert inspect.signature(Example.example.__init__).parameters["aov"].default is None
    pt = PT_RGB.PathTrace(4, 4, None, SimpleNamespace(), 64)
    assert pt.aov is False and all(hasattr(pt, name) for name in ("albedo", "normal", "depth", "alpha"))


def hand_made():
    """two primitives of two materials; three rays: a hit on each and a miss"""
    scene = SimpleNamespace(primitive_np=np.array([[0, 0, 1], [0, 3, 0]], np.int32),
                            material_np=np.array([[0, 0, 0.25, 0.5, 0.75, 0, 0, 0, 0, 0], [0, 0, 0.1, 0.2, 0.3, 0, 0, 0, 0, 0]], f))
    hit = np.zeros((3, 13), f)
    hit[0, 0] = 2.5; hit[0, 7:10] = (0.0, 0.6, -0.8)
    hit[1, 0] = 7.0; hit[1, 7:10] = (1.0, 0.0, 0.0)
    hit[2, 0] = 1000000.0; hit[2, 7:10] = (9.0, 9.0, 9.0)          # a miss: whatever the record holds does not count
    prim = np.array([0, 1, -1], np.int32)
    rays = np.zeros((3, 6), f)
    return scene, rays, hit, prim


def test_samples_of_hand_made_hits():
    x = ae.samples(*hand_made())
    want = np.array([[0.1, 0.2, 0.3, 0.0, 0.6, -0.8, 2.5, 1.0],
                     [0.25, 0.5, 0.75, 1.0, 0.0, 0.0, 7.0, 1.0],
                     [0, 0, 0, 0, 0, 0, 0, 0]], f)
    assert x.dtype == f and np.array_equal(x.view(np.uint32), want.view(np.uint32))


def test_fold_is_the_films_recurrence_one_rounding_per_operation():
    x0, x1, x2 = f(0.1), f(0.7), f(0.3)
    a = f(0.0)
    a = ae.fold(np.array([a]), np.array([x0]), 0)[0]
    assert a == x0                                       # coff = 1: x * 1 + 0 * 0
    a1 = ae.fold(np.array([a]), np.array([x1]), 1)[0]
    half = f(0.5)
    assert a1 == f(f(x1 * half) + f(x0 * half))
    a2 = ae.fold(np.array([a1]), np.array([x2]), 2)[0]
    third = f(1.0) / f(3.0)
    assert a2 == f(f(x2 * third) + f(a1 * f(f(1.0) - third)))
    # not the same number as a mean formed in double precision and rounded once
    xs = np.array([0.1, 0.7, 0.3, 0.9, 0.2, 0.6, 0.4], f)
    acc = np.zeros(1, f)
    for frame, x in enumerate(xs):
        acc = ae.fold(acc, np.array([x], f), frame)
    assert acc.dtype == f and abs(float(acc[0]) - float(xs.astype(np.float64).mean())) < 1e-6
    # a later start continues the mean; a NaN stays
    b = ae.fold(np.array([f(4.0)]), np.array([f(8.0)]), 3)[0]
    assert b == f(f(f(8.0) * f(0.25)) + f(f(4.0) * f(0.75)))
    assert np.isnan(ae.fold(np.array([f(1.0)]), np.array([f(np.nan)]), 5)[0])
    assert np.isnan(ae.fold(np.array([f(np.nan)]), np.array([f(1.0)]), 6)[0])
