"""The entry points of the roughness, metallic and normal-map textures in the header, the binding and the library alike, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_kat_material_maps", "tirt_obj_material_map")
FIX = os.path.join(ROOT, "tests", "golden", "material_maps_obj")


def test_symbols_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _native.SF_TEXTURE_PARAM == 256 and _native.SHADE_INSTANTIATION_MAPS == 511
    assert (_native.KAT_MAPS_IN, _native.KAT_MAPS_OUT) == (3, 8)
    # tirt_obj_material_texture keeps its signature
    assert re.search(r"int\s+tirt_obj_material_texture\s*\(\s*const tirt_obj \*obj, int index, char \*path, int cap\)", text)


def test_kat_material_maps_refusals_without_a_context():
    L = _native.lib()
    rows, out = np.zeros((2, 3), np.float32), np.zeros((2, 8), np.float32)
    assert L.tirt_kat_material_maps(None, rows.reshape(-1), 2, out.reshape(-1), 8, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_material_maps(None, rows.reshape(-1), 3, out.reshape(-1), 7, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_material_maps(None, rows.reshape(-1), 3, out.reshape(-1), 8, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_material_maps(None, rows.reshape(-1), 3, out.reshape(-1), 8, 2) == -2 and b"null context" in L.tirt_last_error()


def test_kat_shade_step_knows_the_new_instantiation():
    rows = np.zeros((1, 23), np.uint32)
    with pytest.raises(_native.TirtError, match="null context"):          # 511 passes the instantiation check
        _native.kat_shade_step(None, 511, rows)
    for feat in (256, 127 | 256, 128 | 256):                               # no other word with bit 256 is one
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)


def test_obj_material_map_answers_and_refusals():
    L = _native.lib()
    buf = C.create_string_buffer(8)
    assert L.tirt_obj_material_map(None, 0, 0, buf, 8) == -2
    h = C.c_void_p()
    _native.check(L.tirt_obj_load(os.fsencode(os.path.join(FIX, "quad.obj")), C.byref(h)))
    try:
        assert L.tirt_obj_material_map(h, 0, 0, buf, 8) == -2 and b"bytes" in L.tirt_last_error()          # the path does not fit
        assert L.tirt_obj_material_map(h, 9, 0, buf, 8) == -2
        for kind in (-1, 3):
            assert L.tirt_obj_material_map(h, 0, kind, buf, 8) == -2 and b"kind" in L.tirt_last_error()
        big = C.create_string_buffer(4096)
        want = {(0, 0): b"/rough.png", (0, 1): b"/orm map.png", (0, 2): b"/normal.png", (1, 0): b"/orm map.png", (1, 1): b"/orm map.png", (1, 2): b"/normal.png",
                (2, 0): b"/rough.png", (2, 1): b"", (2, 2): b"/normal.png", (3, 0): b"", (3, 1): b"", (3, 2): b""}
        for (i, kind), tail in want.items():
            assert L.tirt_obj_material_map(h, i, kind, big, 4096) == 0
            assert big.value.endswith(tail) and bool(big.value) == bool(tail), (i, kind, big.value)
        assert L.tirt_obj_material_texture(h, 0, big, 4096) == 0 and big.value == b""                       # no map_Kd in this file: the old entry says so
    finally:
        L.tirt_obj_free(h)
