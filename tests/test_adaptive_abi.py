"""The pixel-set and adaptive-sampling entry points of the C-ABI (include/tirt.h): declared, bound with the declared argument lists, exported, and
refusing a null context or null parameters without a device."""
import ctypes as C
import os
import re

from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_pixel_set_upload", "tirt_pixel_set_from_moments", "tirt_pixel_set_clear", "tirt_pixel_set_download", "tirt_pt_rgb_render_adaptive")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def test_declared_bound_and_exported():
    text = header()
    lib = _native.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(params), (name, params)
        assert params[0] == "tirt_ctx *ctx" and argtypes[0] is C.c_void_p
        for text_arg, ctype in zip(params, argtypes):
            if "*" in text_arg:
                assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, text_arg)
            elif text_arg.startswith("int64_t"):
                assert ctype is C.c_int64, (name, text_arg)
            elif text_arg.startswith("uint32_t"):
                assert ctype is C.c_uint32, (name, text_arg)
            elif text_arg.startswith("float"):
                assert ctype is C.c_float, (name, text_arg)
            else:
                assert text_arg.startswith("int ") and ctype is C.c_int, (name, text_arg)
        assert hasattr(lib, name), name


def test_structs_match_the_header():
    text = header()
    a = re.search(r"typedef struct \{([^}]*)\} tirt_adaptive_t;", text).group(1)
    r = re.search(r"typedef struct \{([^}]*)\} tirt_adaptive_result_t;", text).group(1)
    assert [n for n, _ in _native.AdaptiveParams._fields_] == re.findall(r"(\w+)\s*[,;]", a) == ["threshold", "min_samples", "max_samples", "pass_frames"]
    assert [n for n, _ in _native.AdaptiveResult._fields_] == re.findall(r"(\w+)\s*[,;]", r) == ["passes", "pixel_samples", "pixels_at_max", "frames"]
    assert C.sizeof(_native.AdaptiveParams) == 16 and C.sizeof(_native.AdaptiveResult) == 32
    assert _native.AdaptiveParams._fields_[0][1] is C.c_float and all(t is C.c_int32 for _, t in _native.AdaptiveParams._fields_[1:])
    assert all(t is C.c_int64 for _, t in _native.AdaptiveResult._fields_)


def test_a_null_context_is_refused():
    lib = _native.lib()
    n = C.c_int64(7)
    prm = _native.AdaptiveParams(0.3, 4, 32, 4)
    res = _native.AdaptiveResult()
    calls = (lambda: lib.tirt_pixel_set_upload(None, None, 0), lambda: lib.tirt_pixel_set_from_moments(None, 0.3, 4, 32, C.byref(n)),
             lambda: lib.tirt_pixel_set_clear(None), lambda: lib.tirt_pixel_set_download(None, None, 0, C.byref(n)),
             lambda: lib.tirt_pt_rgb_render_adaptive(None, 0, 1, 15, 64, 0, C.byref(prm), C.byref(res)))
    for call in calls:
        assert call() == -2 and b"null context" in lib.tirt_last_error()
    assert n.value == 7 and res.passes == 0
