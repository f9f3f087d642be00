"""The Debug integrator (integrator/Debug.py:44-67) on the CPU: the views the oracle composes (tests/debug_views.py) against the views
the reference's own source text produced (tests/golden/refkat_debug.npz, tools/refkat/make_refkat_debug.py: 16 x 16, the Cornell box,
the Cornell box with a glass wall, single_model.py's sphere; all four views at frames 0 and 3), bit for bit -- no transcendental
function is on this path.  Plus the Python class's argument check and the binding's constants."""
import os
import re

import numpy as np
import pytest

import oracle_api as oa
import debug_views as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GD = np.load(os.path.join(os.path.dirname(__file__), "golden", "refkat_debug.npz"))


def debug_scene(name, W, H):
    from common import host_only, cornell_glass_wall
    from ti_raytrace_amd import scenes
    if name == "cornell":
        ex = scenes.cornell_box(W, H, 4, device_id=None)
    elif name == "cornell_glass":
        ex = cornell_glass_wall(W, H)
    else:
        ex = scenes.single_model(W, H, 4, model="sphere.obj", device_id=None)
    host_only(ex, 0.8)
    orc = oa.OracleScene(ex.scene, ex.cam)
    orc.lbvh_build()
    if name == "sphere":                                           # smooth normals (Scene.process_normal)
        orc.process_normal(ex.scene.vertex_index_np)
    return ex, orc


@pytest.mark.parametrize("name", ["cornell", "cornell_glass", "sphere"])
def test_oracle_views_equal_the_reference_text_views(name):
    W, H, seed = [int(x) for x in GD["cfg"]]
    ex, orc = debug_scene(name, W, H)
    for frame in [int(x) for x in GD["frames"]]:
        got = dv.views(ex, orc, W, H, frame, seed)
        for mode in dv.MODES:
            want = GD["%s_%s_f%d" % (name, mode, frame)]
            assert (want != 0).any(axis=2).sum() > 50, (name, mode, frame)            # the view has hits
            assert dv.same_bits(got[mode], want), (name, mode, frame, int((got[mode] != want).any(axis=2).sum()))
    # the jitter moves the rays: frames 0 and 3 are different views
    assert not np.array_equal(GD["%s_normal_f0" % name], GD["%s_normal_f3" % name])


def test_views_differ_from_each_other():
    for name in ("cornell", "cornell_glass", "sphere"):
        for m in ("fnormal", "normal", "gnormal"):
            assert not np.array_equal(GD["%s_albedo_f0" % name], GD["%s_%s_f0" % (name, m)]), (name, m)
    assert not np.array_equal(GD["sphere_normal_f0"], GD["sphere_gnormal_f0"])          # smooth against face normals


def test_unknown_mode_is_a_value_error():
    from ti_raytrace_amd import Debug, scenes
    ex = scenes.cornell_box(8, 8, 1, device_id=None)
    with pytest.raises(ValueError):
        Debug.Debug(8, 8, ex.cam, ex.scene, 64, mode="bogus")
    d = Debug.Debug(8, 8, ex.cam, ex.scene, 64, mode="gnormal")
    assert d.mode == "gnormal" and d.stack_size == 64


def test_native_constants_match_the_header():
    from ti_raytrace_amd import _native
    text = open(os.path.join(ROOT, "include", "tirt.h")).read()
    want = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define TIRT_DEBUG_([A-Z]+) (\d+)", text)}
    assert want == {"ALBEDO": 0, "FNORMAL": 1, "NORMAL": 2, "GNORMAL": 3}
    for k, v in want.items():
        assert getattr(_native, "DEBUG_" + k) == v
    assert "tirt_debug_render" in _native.SIGNATURES


def test_package_exports_debug():
    import ti_raytrace_amd
    assert "Debug" in ti_raytrace_amd.__all__
    from ti_raytrace_amd.Debug import Debug, MODES
    assert sorted(MODES) == sorted(dv.MODES) and callable(Debug)
