"""The temporal accumulation's interface without a device: header, binding and exports agree, the structures have the header's layout, the defaults are
the header's, every entry point refuses a null context, and the Python layer says what it needs before it reaches the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import temporal_expected as te
from test_film_shapes import make
from ti_raytrace_amd import PT_RGB, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tirt_temporal_device", "tirt_temporal_enable", "tirt_temporal_accumulate", "tirt_temporal_reset", "tirt_temporal_download",
         "tirt_temporal_export_device", "tirt_temporal_denoise_var")


def header():
    return open(os.path.join(ROOT, "include", "tirt.h")).read()


def test_header_binding_and_exports_agree():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = _native.lib()
    for name in NAMES:
        assert name in _native.SIGNATURES and re.search(r"\bint %s\s*\(" % name, text) and hasattr(lib, name), name
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name          # as many parameters as the binding passes
    assert sorted(n for n in _native.SIGNATURES if n.startswith("tirt_temporal")) == sorted(NAMES)
    assert re.search(r"typedef struct \{ float max_history, sigma_n, sigma_z; \} tirt_temporal_t;", text)
    assert re.search(r"typedef struct \{ float view\[16\], view_inv\[16\], eye\[3\], fx, fy, cx, cy; \} tirt_temporal_camera_t;", text)
    assert ctypes.sizeof(_native.TemporalParams) == 12 and ctypes.sizeof(_native.TemporalCamera) == 4 * (16 + 16 + 3 + 4)
    assert [n for n, _ in _native.TemporalParams._fields_] == ["max_history", "sigma_n", "sigma_z"]
    assert [n for n, _ in _native.TemporalCamera._fields_] == ["view", "view_inv", "eye", "fx", "fy", "cx", "cy"]
    assert float(re.search(r"#define TIRT_TEMPORAL_MAX_HISTORY ([0-9.]+)f", text).group(1)) == _native.TEMPORAL_DEFAULTS["max_history"]
    assert _native.TEMPORAL_DEFAULTS == te.DEFAULTS
    # the header says why a caller must change the seed per view
    assert "counter-based on (seed, pixel, frame" in header() and "change the seed per view" in header()


def test_every_entry_point_refuses_a_null_context():
    lib = _native.lib()
    cam = _native.TemporalCamera()
    prm = _native.TemporalParams(32.0, 0.3, 0.1)
    dn = _native.DenoiseParams(5, 3.0, 0.3, 0.1)
    for rc in (lib.tirt_temporal_device(None, None, None, None, None, None, None, ctypes.byref(cam), ctypes.byref(cam), None, None, 4, 4, ctypes.byref(prm), None),
               lib.tirt_temporal_enable(None, 1), lib.tirt_temporal_accumulate(None, ctypes.byref(prm)), lib.tirt_temporal_reset(None),
               lib.tirt_temporal_download(None, None, None), lib.tirt_temporal_export_device(None, None, None),
               lib.tirt_temporal_denoise_var(None, ctypes.byref(dn))):
        assert rc == -2 and b"null context" in lib.tirt_last_error()


def test_python_layer_says_what_it_needs():
    ex = make("cornell", 8, 8, 0.8)
    for kw in (dict(), dict(aov=True), dict(moments=True)):
        with pytest.raises(ValueError, match="aov=True, moments=True, temporal=True"):
            PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, temporal=True, **kw)
        it = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, **kw)
        assert it.temporal is False and hasattr(it, "accumulated") and hasattr(it, "accumulated_samples")
        for call in (it.temporal_accumulate, it.temporal_reset, it.denoise_temporal, it.temporal_to_numpy, it.temporal_to_torch):
            with pytest.raises(ValueError, match="temporal=True"):
                call()
    it = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, aov=True, moments=True, temporal=True)
    assert it.temporal and it.aov and it.moments


def test_cameras_go_to_the_library_as_the_camera_pushes_them():
    ex = make("cornell", 8, 8, 0.8)
    ex.cam.set_view_point(0.3, 0.1, 0.0, ex.cam.scale)
    snap = te.Cam(ex.cam)
    tup = (ex.cam.view_np[0], ex.cam.view_inv_np[0], ex.cam.eye_np[0], ex.cam.fx, ex.cam.fy, ex.cam.cx, ex.cam.cy)
    a, b, c = _native.temporal_camera(ex.cam), _native.temporal_camera(tup), _native.temporal_camera(snap)
    for s in (a, b, c):
        assert np.array_equal(np.float32(list(s.view)).reshape(4, 4), ex.cam.view_np[0]) and np.array_equal(np.float32(list(s.view_inv)).reshape(4, 4), ex.cam.view_inv_np[0])
        assert np.array_equal(np.float32(list(s.eye)), ex.cam.eye_np[0]) and (s.fx, s.fy, s.cx, s.cy) == tuple(np.float32([ex.cam.fx, ex.cam.fy, ex.cam.cx, ex.cam.cy]))
    assert _native.temporal_camera(a) is a
    ex.cam.set_view_point(0.4, 0.1, 0.0, ex.cam.scale)          # the snapshot does not follow the camera
    assert not np.array_equal(snap.view_np[0], ex.cam.view_np[0])
    with pytest.raises(ValueError):
        _native.temporal_camera((np.zeros(9), np.zeros(16), np.zeros(3), 1, 1, 1, 1))
