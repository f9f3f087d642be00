"""Which instantiation of k_shade / k_shade_spec a render launches (include/tirt.h, tirt_shade_instantiation), on the host: no context, no device.
The rule over the one table of tirt_render.hip is held, case by case over every word a context can hold, to the selection it replaced -- five tables, chosen
from by index arithmetic and one covering scan -- restated here literally; the words tirt_kat_shade_step accepts are held to the same table."""
import ctypes as C

import numpy as np
import pytest

from ti_raytrace_amd import _native

ERR_ARG = -2      # TIRT_ERR_ARG, include/tirt.h
E, H, P, CUT = _native.SF_ENV_SAMPLE, _native.SF_ENV_HDR, _native.SF_LIGHT_POWER, _native.SF_CUTOUT
WORDS = (_native.SHADE_INSTANTIATIONS + (_native.SHADE_INSTANTIATION_MAPS,) + _native.SHADE_INSTANTIATIONS_ENV + _native.SHADE_INSTANTIATIONS_HDR
         + _native.SHADE_INSTANTIATIONS_POWER)

# ---- the selection before the one table: the five tables of words, pick_shade_inst and pick_shade_rgb ----
OLD_INST = (32, 4, 127, 127 | 128, 127 | 128 | 256)
OLD_ENV_INST = (127 | 1024, 511 | 1024)
OLD_HDR_INST = (127 | 2048, 511 | 2048)
OLD_ENV_HDR_INST = (127 | 1024 | 2048, 511 | 1024 | 2048)
OLD_POWER_INST = (127 | 4096, 511 | 4096, 127 | 1024 | 4096, 511 | 1024 | 4096, 127 | 2048 | 4096, 511 | 2048 | 4096, 127 | 1024 | 2048 | 4096, 511 | 1024 | 2048 | 4096)
OLD_SPEC_INST = (32, 4, 127)


def old_pick_shade_inst(tab, features, specialize):
    n, k = len(tab), 0
    if not specialize:
        while k + 1 < n and tab[k] != 127:
            k += 1
    while k + 1 < n:
        if features & ~tab[k] == 0:
            return tab[k]
        k += 1
    return tab[n - 1]


def old_pick_shade_rgb(features, env_sample, env_hdr, light_power, specialize):
    maps = 1 if features & ~127 else 0
    if light_power:
        return OLD_POWER_INST[(4 if env_hdr else 0) + (2 if env_sample else 0) + maps]
    if env_hdr:
        return (OLD_ENV_HDR_INST if env_sample else OLD_HDR_INST)[maps]
    if env_sample:
        return OLD_ENV_INST[maps]
    return old_pick_shade_inst(OLD_INST, features, specialize)


def code_of(word, specialize, spectral, feat=True):
    out = C.c_uint32(0)
    return _native.lib().tirt_shade_instantiation(word, specialize, spectral, C.byref(out) if feat else None)


def test_selection_equals_the_five_tables_it_replaced():
    assert (E, H, P, CUT) == (1024, 2048, 4096, 512)
    n = 0
    for stored in range(512):
        for derived in range(8):
            env_sample, env_hdr, light_power = derived & 1, derived & 2, derived & 4
            word = stored | (E if env_sample else 0) | (H if env_hdr else 0) | (P if light_power else 0)
            for specialize in (0, 1):
                want = old_pick_shade_rgb(stored, env_sample, env_hdr, light_power, specialize)
                for cut in (0, CUT):
                    assert _native.shade_instantiation(word | cut, specialize, 0) == want, (word | cut, specialize, want)
                    n += 1
    assert n == 16384


def test_spectral_selection_equals_the_scan_it_replaced():
    for stored in range(128):
        for specialize in (0, 1):
            assert _native.shade_instantiation(stored, specialize, 1) == old_pick_shade_inst(OLD_SPEC_INST, stored, specialize), (stored, specialize)


def test_the_known_answer_set_is_the_table():
    assert len(WORDS) == len(set(WORDS)) == 19
    lib = _native.lib()
    rows = np.zeros(_native.KAT_STEP_IN, np.float32); out = np.zeros(_native.KAT_STEP_OUT, np.float32)
    for feat in range(8192):
        assert lib.tirt_kat_shade_step(None, feat, rows, _native.KAT_STEP_IN, out, _native.KAT_STEP_OUT, 1) == ERR_ARG, feat
        msg = lib.tirt_last_error().decode()
        if feat in WORDS:
            assert "null context" in msg and "instantiation" not in msg, (feat, msg)
        else:
            assert "instantiation" in msg, (feat, msg)
    for feat in WORDS:
        assert _native.shade_instantiation(feat, 1, 0) == feat, feat


def test_refusals():
    assert code_of(127, 1, 0) == 0 and code_of(127, 1, 1) == 0
    assert code_of(127, 1, 0, feat=False) == ERR_ARG
    assert "null" in _native.lib().tirt_last_error().decode()
    for specialize, spectral in ((2, 0), (-1, 0), (1, 2), (1, -1)):
        assert code_of(127, specialize, spectral) == ERR_ARG, (specialize, spectral)
    for word in (8192, 127 | 8192, 1 << 16, 1 << 31, 0xffffffff):
        assert code_of(word, 1, 0) == ERR_ARG and code_of(word, 0, 0) == ERR_ARG, word
    assert code_of(8191, 1, 0) == 0
    for word in (128, 256, 255, 511, CUT, 127 | CUT, 127 | E, 127 | H, 127 | P, 8191):
        assert code_of(word, 1, 1) == ERR_ARG and code_of(word, 0, 1) == ERR_ARG, word
    with pytest.raises(_native.TirtError, match="tirt_shade_instantiation"):
        _native.shade_instantiation(8192)
