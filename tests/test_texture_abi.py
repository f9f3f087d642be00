"""The entry points of the albedo textures in the header, the binding and the library alike, and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_texture_upload", "tirt_kat_texture", "tirt_obj_material_texture")


def test_symbols_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _native.SF_TEXTURE == 128 and _native.SF_ALL == 127
    assert _native.SHADE_INSTANTIATIONS[-1] == 255 and _native.SHADE_INSTANTIATIONS[:3] == (32, 4, 127)


def tex(w, h):
    return np.zeros((w, h), np.int32)


def raw_upload(count, texels, total, offset, w, h, wrap):
    arr = lambda a, t: np.ascontiguousarray(a, t)
    texels, offset, w, h, wrap = arr(texels, np.int32), arr(offset, np.int64), arr(w, np.int32), arr(h, np.int32), arr(wrap, np.int32)
    return _native.lib().tirt_texture_upload(None, count, texels.ctypes.data, total, offset.ctypes.data, w.ctypes.data, h.ctypes.data, wrap.ctypes.data)


def test_upload_refusals_without_a_context():
    """each TIRT_ERR_ARG (-2) for its own reason, before the context is looked at"""
    L = _native.lib()
    cases = {
        "w and h": (1, np.zeros(4), 4, [0], [0], [4], [1]),
        "w and h ": (1, np.zeros(4), 4, [0], [2], [-2], [0]),
        "wrap": (1, np.zeros(4), 4, [0], [2], [2], [2]),
        "past": (1, np.zeros(4), 4, [1], [2], [2], [0]),
        "past ": (1, np.zeros(4), 3, [0], [2], [2], [0]),
        "past  ": (1, np.zeros(4), 4, [-1], [1], [1], [0]),
        "overlap": (2, np.zeros(8), 8, [0, 3], [2, 2], [2, 2], [0, 1]),
        "overlap ": (2, np.zeros(8), 8, [4, 1], [2, 2], [2, 2], [0, 1]),
        "count": (-1, np.zeros(4), 4, [0], [2], [2], [0]),
        "total": (1, np.zeros(4), -4, [0], [2], [2], [0]),
    }
    for what, args in cases.items():
        assert raw_upload(*args) == -2, what
        assert what.strip().split()[0] in L.tirt_last_error().decode(), (what, L.tirt_last_error())
    assert L.tirt_texture_upload(None, 1, None, 4, None, None, None, None) == -2 and b"null pointer" in L.tirt_last_error()
    # what is in order reaches the context check: a null context
    assert raw_upload(2, np.zeros(8), 8, [4, 0], [2, 2], [2, 2], [0, 1]) == -2 and b"null context" in L.tirt_last_error()
    assert raw_upload(0, np.zeros(1), 0, [0], [0], [0], [0]) == -2 and b"null context" in L.tirt_last_error()
    with pytest.raises(_native.TirtError, match="null context"):
        _native.texture_upload(None, [(tex(2, 3), 1), (tex(1, 1), 0)])
    with pytest.raises(ValueError, match="packed"):
        _native.texture_upload(None, [(np.zeros((2, 3, 3), np.int32), 1)])


def test_kat_texture_refusals_without_a_context():
    L = _native.lib()
    rows, out = np.zeros((2, 3), np.float32), np.zeros((2, 6), np.float32)
    assert L.tirt_kat_texture(None, rows.reshape(-1), 2, out.reshape(-1), 6, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_texture(None, rows.reshape(-1), 3, out.reshape(-1), 5, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_texture(None, rows.reshape(-1), 3, out.reshape(-1), 6, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_texture(None, rows.reshape(-1), 3, out.reshape(-1), 6, 2) == -2 and b"null context" in L.tirt_last_error()


def test_kat_shade_step_knows_the_textured_instantiation():
    rows = np.zeros((1, 23), np.uint32)
    with pytest.raises(_native.TirtError, match="null context"):          # 255 passes the instantiation check
        _native.kat_shade_step(None, 255, rows)
    with pytest.raises(_native.TirtError, match="instantiation"):         # 128 alone is none
        _native.kat_shade_step(None, 128, rows)


def test_obj_material_texture_refusals():
    L = _native.lib()
    import ctypes as C
    buf = C.create_string_buffer(8)
    assert L.tirt_obj_material_texture(None, 0, buf, 8) == -2
    here = os.path.join(ROOT, "tests", "golden", "texture_obj", "quad.obj")
    h = C.c_void_p()
    _native.check(L.tirt_obj_load(os.fsencode(here), C.byref(h)))
    try:
        assert L.tirt_obj_material_texture(h, 0, buf, 8) == -2 and b"bytes" in L.tirt_last_error()          # the path does not fit
        assert L.tirt_obj_material_texture(h, 9, buf, 8) == -2
        assert L.tirt_obj_material_texture(h, 2, buf, 8) == 0 and buf.value == b""                           # a material without map_Kd
        big = C.create_string_buffer(4096)
        assert L.tirt_obj_material_texture(h, 1, big, 4096) == 0 and big.value.endswith(b"/sub dir.png")
    finally:
        L.tirt_obj_free(h)
