"""The entry points of the emitter choice by power in the header, the binding and the library alike; the refusals that need no context; and the host-side
feature word against hand-built light lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32
BIT = 4096
NEW = {
    "tirt_light_sampling": r"tirt_ctx \*ctx, int mode, float uniform_share",
    "tirt_light_table_download": r"tirt_ctx \*ctx, uint32_t \*q, uint64_t \*prefix, float \*P, int32_t info\[4\]",
    "tirt_kat_light_pick": r"tirt_ctx \*ctx, const float \*in, int in_stride, float \*out, int out_stride, int n",
    "tirt_shade_features_host_lights": r"const float \*material, int nm, const int32_t \*primitive, int n, const float \*shape, int ns,\s*const int32_t \*light, int light_count, "
                                       r"const int32_t \*env, int env_w, int env_h, float env_power,\s*int env_sampling, int env_format, const float \*vertex, int nv, "
                                       r"int light_sampling, uint32_t \*out",
}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def test_new_symbols_in_header_binding_and_library():
    text, lib = header(), _native.lib()
    for name, args in NEW.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\)" % (name, args), text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _native.SIGNATURES["tirt_light_sampling"] == _native.SIGNATURES["tirt_env_sampling"]
    assert _native.SIGNATURES["tirt_kat_light_pick"] == _native.SIGNATURES["tirt_kat_env_sample"]
    assert len(_native.SIGNATURES["tirt_shade_features_host_lights"][1]) == len(_native.SIGNATURES["tirt_shade_features_host_env_hdr"][1]) + 3
    assert _native.SF_LIGHT_POWER == BIT and not _native.SF_ALL & BIT
    assert _native.SHADE_INSTANTIATIONS_POWER == tuple(a | b | c | BIT for c in (0, 2048) for b in (0, 1024) for a in (127, 511))
    assert (_native.KAT_LIGHT_PICK_IN, _native.KAT_LIGHT_PICK_OUT) == (1, 2)
    assert lib.tirt_version() >= 102


def test_older_instantiation_tables_are_unchanged():
    assert _native.SHADE_INSTANTIATIONS == (32, 4, 127, 255) and _native.SHADE_INSTANTIATION_MAPS == 511
    assert _native.SHADE_INSTANTIATIONS_ENV == (127 | 1024, 511 | 1024)
    assert _native.SHADE_INSTANTIATIONS_HDR == (127 | 2048, 511 | 2048, 127 | 1024 | 2048, 511 | 1024 | 2048)


def test_feature_words_of_the_step_entry():
    """the eight twins are instantiations (they get as far as the null context); no other word with the bit is"""
    rows = np.zeros((1, 23), np.uint32)
    for feat in _native.SHADE_INSTANTIATIONS_POWER:
        with pytest.raises(_native.TirtError, match="null context"):
            _native.kat_shade_step(None, feat, rows)
    for feat in (BIT, 32 | BIT, 4 | BIT, 255 | BIT, 127 | BIT | 512, 127 | BIT | 8192):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)


def test_refusals_without_a_context():
    L = _native.lib()
    for mode, share, word in ((2, 0.0, b"mode"), (-1, 0.0, b"mode"), (1, 1.0, b"uniform_share"), (1, -0.001, b"uniform_share"), (0, float("nan"), b"uniform_share"),
                              (1, float("inf"), b"uniform_share")):
        assert L.tirt_light_sampling(None, mode, share) == -2 and word in L.tirt_last_error(), (mode, share)
    assert L.tirt_light_sampling(None, 1, 0.0) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_light_sampling(None, 0, 0.999) == -2 and b"null context" in L.tirt_last_error()
    rows, out = np.zeros((2, 2), f), np.zeros((2, 2), f)
    assert L.tirt_kat_light_pick(None, rows.reshape(-1), 0, out.reshape(-1), 2, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_light_pick(None, rows.reshape(-1), 1, out.reshape(-1), 1, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_light_pick(None, rows.reshape(-1), 1, out.reshape(-1), 2, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_light_pick(None, rows.reshape(-1), 1, out.reshape(-1), 2, 2) == -2 and b"null context" in L.tirt_last_error()
    info = (C.c_int32 * 4)()
    assert L.tirt_light_table_download(None, None, None, None, info) == -2 and b"null context" in L.tirt_last_error()
    with pytest.raises(_native.TirtError, match="uniform_share"):
        _native.light_sampling(None, 1, 1.5)


# ---- the host-side feature word ---------------------------------------------------------------------------------------------------------
def tables(emissions=(5.0, 2.0), degenerate=False, shapes=()):
    """two emissive triangles (one material each) and one grey triangle; `shapes`: (type, material emission) shape emitters appended to the list"""
    vertex = np.zeros((9, 9), f)
    vertex[0:3, 0:3] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    vertex[3:6, 0:3] = [(0, 0, 1), (2, 0, 1), (0, 2, 1)] if not degenerate else [(0, 0, 1), (1, 0, 1), (2, 0, 1)]
    vertex[6:9, 0:3] = [(0, 0, 2), (1, 0, 2), (0, 1, 2)]
    material = np.zeros((3 + len(shapes), 10), f)
    material[0, 0], material[0, 2:5] = 2, emissions[0]
    material[1, 0], material[1, 2:5] = 2, emissions[1]
    material[2, 0], material[2, 2:5] = 0, 0.7
    primitive = [(1, 0, 0), (1, 3, 1), (1, 6, 2)]
    shape = np.zeros((max(1, len(shapes)), 10), f)
    light = [0, 1]
    for k, (kind, e) in enumerate(shapes):
        shape[k, 0], shape[k, 4], shape[k, 5] = kind, 0.5, 0.6
        material[3 + k, 0], material[3 + k, 2:5] = 2, e
        primitive.append((2, k, 3 + k))
        light.append(3 + k)
    return material, np.array(primitive, np.int32), shape, np.array(light, np.int32), vertex


def word(material, primitive, shape, light, vertex, on=True, count=None, **kw):
    return _native.shade_features_host_lights(material, primitive, shape, light, light.shape[0] if count is None else count, vertex=vertex, light_sampling=on, **kw)


def test_host_feature_word_predicts_the_bit():
    t = tables()
    base = _native.shade_features_host(*t[:4], t[3].shape[0])
    assert base == _native.SF_LIGHT_TRI
    assert word(*t, on=False) == base
    assert word(*t) == base | BIT
    assert word(*t, count=0) == _native.SF_NO_LIGHT                       # an empty list: nothing to choose
    # a sphere beside the triangles keeps the bit; a spot, a laser or an unknown kind clears it
    assert word(*tables(shapes=((1, 9.0),))) == _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPHERE | BIT
    for kind in (3, 4):
        assert word(*tables(shapes=((kind, 9.0),))) == _native.SF_LIGHT_TRI | _native.SF_LIGHT_SPOT_LASER
    assert word(*tables(shapes=((7, 9.0),))) == _native.SF_LIGHT_TRI | _native.SF_LIGHT_OTHER
    # total == 0: every emitter black, negative or NaN, or its area degenerate
    assert word(*tables(emissions=(0.0, 0.0))) == base
    assert word(*tables(emissions=(-1.0, float("nan")))) == base
    assert word(*tables(emissions=(0.0, 3.0), degenerate=True)) == base
    assert word(*tables(emissions=(0.0, 3.0))) == base | BIT
    assert word(*tables(emissions=(float("inf"), 0.0))) == base
    # beside the environment's bits
    sky = np.full((4, 2), 0x00808080, np.int32)
    assert word(*t, env=sky, env_power=1.0, env_sampling=True) == base | _native.SF_ENV | _native.SF_ENV_SAMPLE | BIT


def test_host_feature_word_refusals():
    t = tables()
    with pytest.raises(_native.TirtError, match="light_sampling"):
        _native.check(_native.lib().tirt_shade_features_host_lights(t[0].reshape(-1), 3, t[1].reshape(-1), 3, t[2].reshape(-1), 1, t[3], 2, None, 0, 0, 0.0, 0, 0,
                                                                    t[4].ctypes.data_as(C.c_void_p), 9, 2, C.byref(C.c_uint32(0))))
    with pytest.raises(_native.TirtError, match="vertex"):
        _native.shade_features_host_lights(t[0], t[1], t[2], t[3], 2, vertex=t[4][:4], light_sampling=True)
