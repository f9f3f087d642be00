"""The entry points of the alpha cut-outs in the header, the binding and the library alike, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_texture_cutout", "tirt_kat_texture_alpha", "tirt_obj_material_opacity")
FIX = os.path.join(ROOT, "tests", "golden", "cutout_obj")


def test_symbols_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _native.SF_CUTOUT == 512
    assert (_native.KAT_ALPHA_IN, _native.KAT_ALPHA_OUT) == (3, 2)
    # k_shade does not change with the bit: the instantiations are what they were
    assert _native.SHADE_INSTANTIATIONS == (32, 4, 127, 255) and _native.SHADE_INSTANTIATION_MAPS == 511
    # tirt_texture_upload and tirt_obj_material_map keep their signatures
    assert re.search(r"int\s+tirt_texture_upload\s*\(\s*tirt_ctx \*ctx, int count, const int32_t \*texels, int64_t total, const int64_t \*offset, const int32_t \*w, "
                     r"const int32_t \*h,\s*const int32_t \*wrap\)", text)
    assert re.search(r"int\s+tirt_obj_material_map\s*\(\s*const tirt_obj \*obj, int index, int kind, char \*path, int cap\)", text)


def test_no_word_with_bit_512_is_an_instantiation():
    rows = np.zeros((1, 23), np.uint32)
    for feat in (512, 127 | 512, 255 | 512, 511 | 512):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)


def test_texture_cutout_refusals_without_a_context():
    L = _native.lib()
    flags = np.array([0, 1, 2], np.int32)
    assert L.tirt_texture_cutout(None, flags.ctypes.data_as(C.c_void_p), 3) == -2 and b"neither 0 nor 1" in L.tirt_last_error()
    flags[2] = -1
    assert L.tirt_texture_cutout(None, flags.ctypes.data_as(C.c_void_p), 3) == -2 and b"neither 0 nor 1" in L.tirt_last_error()
    assert L.tirt_texture_cutout(None, None, 3) == -2 and b"null pointer" in L.tirt_last_error()
    assert L.tirt_texture_cutout(None, None, -1) == -2 and b"negative" in L.tirt_last_error()
    flags[2] = 1
    assert L.tirt_texture_cutout(None, flags.ctypes.data_as(C.c_void_p), 3) == -2 and b"null context" in L.tirt_last_error()
    with pytest.raises(_native.TirtError, match="neither 0 nor 1"):
        _native.texture_cutout(None, [0, 7])


def test_kat_texture_alpha_refusals_without_a_context():
    L = _native.lib()
    rows, out = np.zeros((2, 3), np.float32), np.zeros((2, 2), np.float32)
    assert L.tirt_kat_texture_alpha(None, rows.reshape(-1), 2, out.reshape(-1), 2, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_texture_alpha(None, rows.reshape(-1), 3, out.reshape(-1), 1, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_texture_alpha(None, rows.reshape(-1), 3, out.reshape(-1), 2, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_texture_alpha(None, rows.reshape(-1), 3, out.reshape(-1), 2, 2) == -2 and b"null context" in L.tirt_last_error()


def test_shade_features_host_never_sets_the_bit():
    material = np.zeros((1, 10), np.float32); material[0, 1] = 1.0
    primitive = np.array([[1, 0, 0]], np.int32); shape = np.zeros((1, 10), np.float32); light = np.zeros(1, np.int32)
    assert _native.shade_features_host(material, primitive, shape, light, 0) & (_native.SF_CUTOUT | _native.SF_TEXTURE) == 0


def test_obj_material_opacity_answers_and_refusals():
    L = _native.lib()
    buf = C.create_string_buffer(8)
    assert L.tirt_obj_material_opacity(None, 0, buf, 8) == -2
    h = C.c_void_p()
    _native.check(L.tirt_obj_load(os.fsencode(os.path.join(FIX, "cutouts.obj")), C.byref(h)))
    try:
        assert L.tirt_obj_material_opacity(h, 0, buf, 8) == -2 and b"bytes" in L.tirt_last_error()          # the path does not fit
        assert L.tirt_obj_material_opacity(h, 9, buf, 8) == -2 and L.tirt_obj_material_opacity(h, -1, buf, 8) == -2
        big = C.create_string_buffer(4096)
        assert L.tirt_obj_material_opacity(h, 0, None, 4096) == -2
        for i, tail in enumerate((b"/leaf rgba.png", b"/mask_grey.png", b"/mask_grey.png", b"", b"/mask_grey.png")):
            assert L.tirt_obj_material_opacity(h, i, big, 4096) == 0
            assert big.value.endswith(tail) and bool(big.value) == bool(tail), (i, big.value)
        assert L.tirt_obj_material_texture(h, 0, big, 4096) == 0 and big.value.endswith(b"/leaf rgba.png")
        assert L.tirt_obj_material_texture(h, 2, big, 4096) == 0 and big.value == b""
        for kind in range(3):                                                                                # map_d is no kind of tirt_obj_material_map
            assert L.tirt_obj_material_map(h, 0, kind, big, 4096) == 0 and big.value == b""
    finally:
        L.tirt_obj_free(h)
