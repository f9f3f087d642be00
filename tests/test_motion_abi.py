"""The motion records' interface without a device: header, binding and exports agree, the record's layout constants are the header's, every entry point
refuses a null context, the header states the arithmetic and the snapshot rule, and the Python layer says what it needs before it reaches the library."""
import ctypes
import os
import re

import pytest

import motion_expected as mx
from test_film_shapes import make
from ti_raytrace_amd import PT_RGB, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tirt_motion_enable", "tirt_motion_download", "tirt_motion_export_device", "tirt_motion_temporal_device")


def header():
    return open(os.path.join(ROOT, "include", "tirt.h")).read()


def test_header_binding_and_exports_agree():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = _native.lib()
    for name in NAMES:
        assert name in _native.SIGNATURES and re.search(r"\bint %s\s*\(" % name, text) and hasattr(lib, name), name
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name          # as many parameters as the binding passes
    assert sorted(n for n in _native.SIGNATURES if n.startswith("tirt_motion")) == sorted(NAMES)
    assert int(re.search(r"#define TIRT_MOTION_WORDS (\d+)", text).group(1)) == _native.MOTION_WORDS == mx.WORDS == 8
    # tirt_motion_temporal_device is tirt_temporal_device with `motion` before `stream`
    plain = [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint tirt_temporal_device\s*\((.*?)\);", text, re.S).group(1).split(",")]
    mv = [a.strip().split()[-1].lstrip("*") for a in re.search(r"\bint tirt_motion_temporal_device\s*\((.*?)\);", text, re.S).group(1).split(",")]
    assert mv == plain[:-1] + ["motion", "stream"]
    assert _native.SIGNATURES["tirt_motion_temporal_device"][1] == _native.SIGNATURES["tirt_temporal_device"][1][:-1] + [ctypes.c_void_p, ctypes.c_void_p]


def test_the_header_states_the_record_the_rule_and_the_limits():
    h = header()
    for phrase in ("P(R) = (v1*a + v2*u) + v3*v", "P(snapshot) - P(current)", "N(snapshot) - N(current)", "X = X + D_motion", "n_c = n_c + dN",
                   "tirt_lbvh_build must follow the vertex update", "tirt_process_normal are not tracked", "the vertex rows of the last accumulated view"):
        assert phrase in h, phrase


def test_every_entry_point_refuses_a_null_context():
    lib = _native.lib()
    cam = _native.TemporalCamera()
    prm = _native.TemporalParams(32.0, 0.3, 0.1)
    for rc in (lib.tirt_motion_enable(None, 1), lib.tirt_motion_download(None, None), lib.tirt_motion_export_device(None, None),
               lib.tirt_motion_temporal_device(None, None, None, None, None, None, None, ctypes.byref(cam), ctypes.byref(cam), None, None, 4, 4,
                                               ctypes.byref(prm), None, None)):
        assert rc == -2 and b"null context" in lib.tirt_last_error()


def test_python_layer_says_what_it_needs():
    ex = make("cornell", 8, 8, 0.8)
    for kw in (dict(), dict(aov=True, moments=True)):
        with pytest.raises(ValueError, match="temporal=True, motion=True"):
            PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, motion=True, **kw)
    it = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, aov=True, moments=True, temporal=True)
    assert it.motion_records is False and hasattr(it, "motion")
    for call in (it.motion_to_numpy, it.motion_to_torch, it.motion.to_numpy):
        with pytest.raises(ValueError, match="motion=True"):
            call()
    it = PT_RGB.PathTrace(8, 8, ex.cam, ex.scene, 64, aov=True, moments=True, temporal=True, motion=True)
    assert it.motion_records and it.temporal
