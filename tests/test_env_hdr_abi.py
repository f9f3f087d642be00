"""The entry points of the HDR environment (include/tirt.h, "HDR environment") in the header, the binding and the library alike; what they refuse without a
context; the host feature word with the texel format as an input.  No device is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import env_hdr_expected as eh
import shade_step_cases as cases
from ti_raytrace_amd import _native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = r"tirt_ctx \*ctx, const float \*in, int in_stride, float \*out, int out_stride, int n"
NEW = {
    "tirt_env_upload_hdr": r"tirt_ctx \*ctx, const int32_t \*rgbe_packed, int w, int h, float power",
    "tirt_env_format": r"tirt_ctx \*ctx, int32_t out\[2\]",
    "tirt_kat_env_lookup": KAT,
    "tirt_shade_features_host_env_hdr": r"const float \*material, int nm, const int32_t \*primitive, int n, const float \*shape, int ns,\s*const int32_t \*light, int light_count, "
                                        r"const int32_t \*env, int env_w, int env_h, float env_power,\s*int env_sampling, int env_format, uint32_t \*out",
}
HDR, SAMPLE = _native.SF_ENV_HDR, _native.SF_ENV_SAMPLE


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "tirt.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_symbols_in_header_binding_and_library():
    text, lib = header(), _native.lib()
    for name, args in NEW.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\)" % (name, args), text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_native.SIGNATURES["tirt_shade_features_host_env_hdr"][1]) == len(_native.SIGNATURES["tirt_shade_features_host_env"][1]) + 1
    assert _native.SIGNATURES["tirt_kat_env_lookup"] == _native.SIGNATURES["tirt_kat_env_pdf"]
    assert HDR == 2048 and not _native.SF_ALL & 2048
    assert _native.SHADE_INSTANTIATIONS_HDR == (127 | 2048, 511 | 2048, 127 | 1024 | 2048, 511 | 1024 | 2048)
    assert (_native.KAT_ENV_LOOKUP_IN, _native.KAT_ENV_LOOKUP_OUT) == (2, 3)


def test_old_symbols_and_the_limit_sentence():
    text = header()
    assert re.search(r"int\s+tirt_env_upload\s*\(\s*tirt_ctx \*ctx, const int32_t \*rgb_packed, int w, int h, float power\)", text)
    assert re.search(r"int\s+tirt_env_table_download\s*\(\s*tirt_ctx \*ctx, uint32_t \*q, uint64_t \*row_sums, uint64_t \*marginal, int32_t info\[4\]\)", text)
    assert re.search(r"int\s+tirt_shade_features_host_env\s*\(\s*const float \*material, int nm, const int32_t \*primitive, int n, const float \*shape, int ns,\s*"
                     r"const int32_t \*light, int light_count, const int32_t \*env, int env_w, int env_h, float env_power,\s*int env_sampling, uint32_t \*out\)", text)
    full = header(comments=True)
    assert "RGBE environment is out of scope" not in full and "HDR environment" in full
    assert "RGBE environment is a follow-up" not in open(os.path.join(ROOT, "README.md")).read()
    assert _native.SHADE_INSTANTIATIONS_ENV == (127 | 1024, 511 | 1024)


def test_feature_words_of_the_step_entry():
    """the four new words are instantiations (they get as far as the null context); no other word with bit 2048 is"""
    rows = np.zeros((1, 23), np.uint32)
    for feat in _native.SHADE_INSTANTIATIONS_HDR:
        with pytest.raises(_native.TirtError, match="null context"):
            _native.kat_shade_step(None, feat, rows)
    for feat in (2048, 32 | 2048, 4 | 2048, 255 | 2048, 255 | 1024 | 2048, 127 | 512 | 2048):
        with pytest.raises(_native.TirtError, match="instantiation"):
            _native.kat_shade_step(None, feat, rows)


def test_upload_refusals_without_a_context():
    good = eh.encode(scenes.hdr_sun_sky())
    with pytest.raises(_native.TirtError, match="bad image"):
        _native.env_upload_hdr(None, None, 1.0, dims=(4, 4))
    for dims in ((0, 8), (16, 0), (-1, 8), (16, -3)):
        with pytest.raises(_native.TirtError, match="bad image"):
            _native.env_upload_hdr(None, good, 1.0, dims=dims)
    bad = good.copy()
    bad[3, 5] = 0x00000100                                                                  # E == 0 with a green mantissa, at index 3 * 8 + 5
    bad[9, 0] = 0x00FF0000
    with pytest.raises(_native.TirtError, match=r"tirt_env_upload_hdr: texel 29 "):
        _native.env_upload_hdr(None, bad, 1.0)
    with pytest.raises(_native.TirtError, match="null context"):
        _native.env_upload_hdr(None, good, 1.0)                                            # a valid image gets as far as the context
    L = _native.lib()
    rows, out = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)
    assert L.tirt_kat_env_lookup(None, rows.reshape(-1), 1, out.reshape(-1), 3, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_env_lookup(None, rows.reshape(-1), 2, out.reshape(-1), 2, 2) == -2 and b"stride" in L.tirt_last_error()
    assert L.tirt_kat_env_lookup(None, rows.reshape(-1), 2, out.reshape(-1), 3, -1) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_env_lookup(None, rows.reshape(-1), 2, out.reshape(-1), 3, 2) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_env_format(None, (C.c_int32 * 2)()) == -2 and b"null context" in L.tirt_last_error()


def tables(name="env_only"):
    ex, _, _ = cases.build(name)
    sc = ex.scene
    return sc.material_np, sc.primitive_np, sc.shape_np, sc.light_np, sc.light_count


def test_host_feature_word_refusals():
    t = tables()
    good = eh.encode(scenes.hdr_sun_sky())
    with pytest.raises(_native.TirtError, match="bad image"):
        _native.shade_features_host_env_hdr(*t, env=None, env_power=1.0, env_format=1, dims=(4, 4))
    for dims in ((0, 8), (16, 0)):
        with pytest.raises(_native.TirtError, match="bad image"):
            _native.shade_features_host_env_hdr(*t, env=good, env_power=1.0, env_format=1, dims=dims)
    bad = good.copy(); bad[0, 1] = 0x00000001
    with pytest.raises(_native.TirtError, match=r"tirt_shade_features_host_env_hdr: texel 1 "):
        _native.shade_features_host_env_hdr(*t, env=bad, env_power=1.0, env_format=1)
    with pytest.raises(_native.TirtError, match="env_format"):
        _native.shade_features_host_env_hdr(*t, env=good, env_power=1.0, env_format=2)
    # format 0 is the old function: an image is optional there
    assert _native.shade_features_host_env_hdr(*t, env=None, env_power=1.0, env_format=0) == _native.shade_features_host_env(*t, env=None, env_power=1.0)


@pytest.mark.parametrize("name", ["env_only", "generic"])
def test_host_feature_word_bits(name):
    """bit 2048 exactly when the format is RGBE8 and the environment lit; bit 1024 under the conditions of the 8-bit image: switch on, power != 0, a table that is not empty"""
    t = tables(name)
    base = cases.SCENES[name][1] & ~_native.SF_ENV
    sky = eh.encode(scenes.hdr_sun_sky())
    black = np.zeros((16, 8), np.int32)
    dim = eh.pack([[1]], [[0]], [[0]], [[1]])                                               # one denormal texel: lit, and its table is not empty (the scale follows E_max)
    word = lambda img, power, on, fmt=1: _native.shade_features_host_env_hdr(*t, env=img, env_power=power, env_sampling=on, env_format=fmt)
    assert word(sky, 2.0, False) == base | 2 | HDR
    assert word(sky, 2.0, True) == base | 2 | HDR | SAMPLE
    assert word(sky, 0.0, True) == base | 2 | HDR                                           # lit by its texels, but no table without power
    assert word(black, 0.0, True) == base                                                   # not lit: neither bit
    assert word(black, 3.0, True) == base | 2 | HDR                                         # lit by the power alone: no table from a black image
    assert word(dim, 1.0, True) == base | 2 | HDR | SAMPLE
    assert eh.table(dim)["total"] > 0
    # the same texels read as an 8-bit image never get bit 2048
    for on in (False, True):
        w8 = word(sky, 2.0, on, fmt=0)
        assert not w8 & HDR and w8 == _native.shade_features_host_env(*t, env=sky, env_power=2.0, env_sampling=on)
    # 8-bit and RGBE8 agree on bit 1024 for images that say the same thing
    from ti_raytrace_amd import Texture
    t8 = Texture.Texture(); t8.load_array(scenes.sun_sky_image())
    for power in (0.0, 2.0):
        for on in (False, True):
            assert (word(sky, power, on) & ~HDR) == _native.shade_features_host_env(*t, env=t8.np_img, env_power=power, env_sampling=on)
