"""The entry points of the signed distance in the header, the binding and the library alike, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ti_raytrace_amd import _native, PointQuery, SignedHits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_query_signed_distance", "tirt_signed_distance", "tirt_signed_distance_prepare", "tirt_signed_distance_table_download",
       "tirt_kat_signed_distance")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def test_symbols_in_header_binding_and_library():
    text = header()
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int


def test_argument_lists_are_the_closest_point_ones_plus_out_sd():
    text = header()

    def params(name):
        m = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params("tirt_query_signed_distance") == params("tirt_query_closest_point") + ["float *out_sd"]
    assert params("tirt_signed_distance") == params("tirt_closest_point") + ["float *out_sd"]
    assert params("tirt_signed_distance_prepare") == ["tirt_ctx *ctx", "int64_t report[5]"]
    assert params("tirt_signed_distance_table_download") == ["tirt_ctx *ctx", "float *out"]
    assert params("tirt_kat_signed_distance") == ["tirt_ctx *ctx", "const float *in", "int n", "float *out"]
    S = _native.SIGNATURES
    assert S["tirt_query_signed_distance"][1] == S["tirt_query_closest_point"][1] + [C.c_void_p]
    assert S["tirt_signed_distance"][1] == S["tirt_closest_point"][1] + [C.c_void_p]
    # the unsigned entries keep their signatures
    assert len(S["tirt_query_closest_point"][1]) == 17 and len(S["tirt_closest_point"][1]) == 11


def test_refusals_without_a_context():
    L = _native.lib()
    rows, out = np.zeros((2, 33), np.float32), np.zeros((2, 2), np.float32)
    report = (C.c_int64 * 5)()
    assert L.tirt_signed_distance_prepare(None, report) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_signed_distance_table_download(None, out.reshape(-1)) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_kat_signed_distance(None, rows.reshape(-1), -1, out.reshape(-1)) == -2 and b"negative" in L.tirt_last_error()
    assert L.tirt_kat_signed_distance(None, rows.reshape(-1), 2, out.reshape(-1)) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_query_signed_distance(None, None, 0, 3, None, 1, 0.0, 64, 0, None, None, None, 3, None, 2, None, None, None) == -2
    assert L.tirt_signed_distance(None, np.zeros(3, np.float32), 1, None, 64, 0, None, None, None, None, None, None) == -2


def test_point_query_has_the_signed_methods_and_checks_first():
    assert SignedHits._fields == ("dist", "prim", "point", "uv")
    for name in ("signed_distance", "inside", "mesh_report"):
        assert callable(getattr(PointQuery, name))
    for name in ("query_signed_distance", "signed_distance", "signed_distance_prepare", "signed_distance_table", "kat_signed_distance"):
        assert callable(getattr(_native.Context, name))
    assert _native.SD_REPORT == ("boundary_edges", "nonmanifold_edges", "flipped_edges", "invalid_triangles", "primitives")
    import torch

    class NoScene:
        _ctx = None
        _device_id = 0
    q = PointQuery(NoScene())
    with pytest.raises(TypeError, match="signed_distance: points must be a torch.Tensor"):
        q.signed_distance(np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match="signed_distance: points must be float32"):
        q.signed_distance(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"signed_distance: points must be \[N, C >= 3\]"):
        q.signed_distance(torch.zeros((4, 2)))
    with pytest.raises(TypeError, match="signed_distance: points must be on the GPU"):
        q.inside(torch.zeros((4, 3)))
