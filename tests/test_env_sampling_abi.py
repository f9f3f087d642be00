"""The entry points of the environment's importance sampling in the header, the binding and the library alike; the older ones keep their signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "tirt_env_sampling": r"tirt_ctx \*ctx, int on, float share",
    "tirt_env_table_download": r"tirt_ctx \*ctx, uint32_t \*q, uint64_t \*row_sums, uint64_t \*marginal, int32_t info\[4\]",
    "tirt_kat_env_sample": r"tirt_ctx \*ctx, const float \*in, int in_stride, float \*out, int out_stride, int n",
    "tirt_kat_env_pdf": r"tirt_ctx \*ctx, const float \*in, int in_stride, float \*out, int out_stride, int n",
    "tirt_shade_features_host_env": r"const float \*material, int nm, const int32_t \*primitive, int n, const float \*shape, int ns,\s*const int32_t \*light, int light_count, "
                                    r"const int32_t \*env, int env_w, int env_h, float env_power,\s*int env_sampling, uint32_t \*out",
}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def test_new_symbols_in_header_binding_and_library():
    text, lib = header(), _native.lib()
    for name, args in NEW.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\)" % (name, args), text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    vp, i32, f32p = C.c_void_p, C.c_int, _native.SIGNATURES["tirt_kat_shade_step"][1][2]
    assert _native.SIGNATURES["tirt_env_sampling"] == (C.c_int, [vp, i32, C.c_float])
    assert _native.SIGNATURES["tirt_kat_env_sample"] == (C.c_int, [vp, f32p, i32, f32p, i32, i32])
    assert _native.SIGNATURES["tirt_kat_env_pdf"] == _native.SIGNATURES["tirt_kat_env_sample"]
    assert len(_native.SIGNATURES["tirt_shade_features_host_env"][1]) == len(_native.SIGNATURES["tirt_shade_features_host"][1]) + 1
    assert _native.SF_ENV_SAMPLE == 1024 and not _native.SF_ALL & 1024
    assert _native.SHADE_INSTANTIATIONS_ENV == (127 | 1024, 511 | 1024)
    assert (_native.KAT_ENV_SAMPLE_IN, _native.KAT_ENV_SAMPLE_OUT, _native.KAT_ENV_PDF_IN, _native.KAT_ENV_PDF_OUT) == (2, 10, 3, 5)


def test_old_symbols_are_unchanged():
    text = header()
    assert re.search(r"int\s+tirt_env_upload\s*\(\s*tirt_ctx \*ctx, const int32_t \*rgb_packed, int w, int h, float power\)", text)
    assert re.search(r"int\s+tirt_shade_features\s*\(\s*tirt_ctx \*ctx, uint32_t \*out\)", text)
    assert re.search(r"int\s+tirt_shade_features_host\s*\(\s*const float \*material, int nm, const int32_t \*primitive, int n, const float \*shape, int ns,\s*"
                     r"const int32_t \*light, int light_count, const int32_t \*env, int env_w, int env_h, float env_power,\s*uint32_t \*out\)", text)
    assert re.search(r"int\s+tirt_kat_shade_step\s*\(\s*tirt_ctx \*ctx, uint32_t feat, const float \*in, int in_stride, float \*out, int out_stride, int n\)", text)
    assert _native.SHADE_INSTANTIATIONS == (32, 4, 127, 255) and _native.SHADE_INSTANTIATION_MAPS == 511
    assert (_native.KAT_STEP_IN, _native.KAT_STEP_OUT) == (23, 28)


def test_feature_words_of_the_step_entry():
    """127 | 1024 and 511 | 1024 are instantiations (they get as far as the null context); no other word with the bit is"""
    rows = np.zeros((1, 23), np.uint32)
    for feat in _native.SHADE_INSTANTIATIONS_ENV:
        with pytest.raises(_native.TirtError, match="null context"):
            _native.kat_shade_step(None, feat, rows)
    for feat in (1024, 32 | 1024, 4 | 1024, 255 | 1024, 127 | 1024 | 512):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)


def test_kat_refusals_without_a_context():
    L = _native.lib()
    rows, out = np.zeros((2, 3), np.float32), np.zeros((2, 10), np.float32)
    assert L.tirt_kat_env_sample(None, rows.reshape(-1), 1, out.reshape(-1), 10, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_env_sample(None, rows.reshape(-1), 2, out.reshape(-1), 9, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_env_pdf(None, rows.reshape(-1), 2, out.reshape(-1), 5, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_env_pdf(None, rows.reshape(-1), 3, out.reshape(-1), 5, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_env_pdf(None, rows.reshape(-1), 3, out.reshape(-1), 5, 2) == -2 and b"null context" in L.tirt_last_error()
