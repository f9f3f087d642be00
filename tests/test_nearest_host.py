"""K nearest primitives without a device (include/tirt.h, "K nearest primitives"): the three entry points in the header, the binding and the library with
their argument types, the refusals that need no device, the list code of csrc/tirt_nearest.h on the host (tirt_kat_nearest_list) against a stable numpy
sort -- on random arrival orders, with exact ties, NaN and +inf candidates and every kind of lim2 --, the order-free claim (every permutation of one
candidate set gives one list), and the restatement of the GPU tests against the closest point's."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_expected as E
import nearest_expected as NE
from ti_raytrace_amd import PointNearest, PointQuery, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("tirt_query_nearest", "tirt_nearest", "tirt_kat_nearest_list")
KS = (0, 1, 2, 7, 64)
LIM2 = (-1.0, 0.0, 2.5, float("inf"))


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def c_types_of(decl):
    """the ctypes a C parameter list of include/tirt.h maps to, the way _native.SIGNATURES writes them (every pointer is a void pointer there, but the
    int32 out_info of the known-answer entry)"""
    out = []
    for prm in decl.split(","):
        prm = " ".join(prm.split())
        if "*" in prm:
            out.append("ptr")
        else:
            out.append({"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}[prm.rsplit(" ", 1)[0].replace("const ", "")])
    return out


def test_symbols_in_header_binding_and_library():
    text = header()
    lib = _native.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
        res, args = _native.SIGNATURES[name]
        assert res is C.c_int and getattr(lib, name).restype is C.c_int
        want = c_types_of(m.group(1))
        assert len(args) == len(want), (name, len(args), len(want))
        for a, w in zip(args, want):
            if w == "ptr":
                assert a is C.c_void_p or hasattr(a, "from_param") and a not in (C.c_int, C.c_int64, C.c_float), (name, a)
            else:
                assert a is w, (name, a, w)
    assert sorted(_native.SIGNATURES) == sorted(set(re.findall(r"\b(tirt_[a-z_0-9]+)\s*\(", text)))
    assert re.search(r"#define\s+TIRT_NEAREST_MAX\s+64\b", text) and _native.NEAREST_MAX == 64
    S = _native.SIGNATURES
    assert len(S["tirt_query_nearest"][1]) == 19 and len(S["tirt_nearest"][1]) == 13 and len(S["tirt_kat_nearest_list"][1]) == 8
    # the entries beside them keep their signatures
    assert len(S["tirt_query_closest_point"][1]) == 17 and len(S["tirt_closest_point"][1]) == 11 and len(S["tirt_query_hits"][1]) == 17


def test_refusals_without_a_device():
    L = _native.lib()
    out = np.zeros(4, F)
    cnt = np.zeros(4, np.int32)
    q = lambda k, out_d2, out_count: L.tirt_query_nearest(None, None, 0, 3, None, 1, float("inf"), k, 64, 0, out_d2, None, None, 3, None, 2, out_count, None, None)
    h = lambda k, out_d2, out_count: L.tirt_nearest(None, out, 0, None, k, 64, 0, out_d2, None, None, None, out_count, None)
    for f, what in ((q, b"tirt_query_nearest"), (h, b"tirt_nearest")):
        assert f(1, out.ctypes.data, None) == -2 and b"null context" in L.tirt_last_error()      # k and outputs in order: the context is looked at next
        assert f(65, out.ctypes.data, None) == -2 and b"TIRT_NEAREST_MAX" in L.tirt_last_error() and what in L.tirt_last_error()
        assert f(-1, out.ctypes.data, None) == -2 and b"TIRT_NEAREST_MAX" in L.tirt_last_error()
        assert f(0, out.ctypes.data, None) == -2 and b"k == 0 without out_count" in L.tirt_last_error()
        assert f(3, None, None) == -2 and b"no output at all" in L.tirt_last_error()
        assert f(0, None, cnt.ctypes.data) == -2 and b"null context" in L.tirt_last_error()
        assert f(64, None, cnt.ctypes.data) == -2 and b"null context" in L.tirt_last_error()
    with pytest.raises(_native.TirtError, match="TIRT_NEAREST_MAX"):
        _native.kat_nearest_list([1.0], [0], 65)
    with pytest.raises(_native.TirtError, match="negative"):
        _native.kat_nearest_list([1.0, 2.0], [0, -1], 2)


class NoDeviceScene:
    """a scene whose context is never made: every check below has to come before anything needs a device"""
    _ctx = None
    _device_id = 0

    @property
    def ctx(self):
        raise AssertionError("the check needed a device")


def test_python_argument_checks_need_no_device():
    torch = pytest.importorskip("torch")
    assert PointNearest._fields == ("dist2", "prim", "point", "uv", "count")
    q = PointQuery(NoDeviceScene())
    pts = torch.zeros((5, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="float32"):
        q.nearest(pts.double(), 3)
    with pytest.raises(TypeError, match="torch.Tensor"):
        q.nearest(np.zeros((5, 3), F), 3)
    for bad in (torch.zeros((5, 2)), torch.zeros(5), torch.zeros((5, 3, 1))):
        with pytest.raises(ValueError, match="points must be"):
            q.nearest(bad, 3)
    with pytest.raises(ValueError, match="stride 1"):
        q.nearest(torch.zeros((5, 8))[:, ::2], 3)
    with pytest.raises(ValueError, match="overlap"):
        q.nearest(torch.zeros((3, 5)).t(), 3)
    for k in (-1, 65, 1000):
        with pytest.raises(ValueError, match="k must be 0..64"):
            q.nearest(pts, k)
    with pytest.raises(TypeError, match="k must be an int"):
        q.nearest(pts, 2.5)
    with pytest.raises(ValueError, match="k == 0 without count"):
        q.nearest(pts, 0)
    with pytest.raises(TypeError, match="max_distance is required"):
        q.count_within(pts, None)
    with pytest.raises(TypeError):
        q.count_within(pts)
    with pytest.raises(TypeError, match="on the GPU"):           # the layout is right: only now does the device matter
        q.nearest(pts, 3)
    for name in ("query_nearest", "nearest"):
        assert callable(getattr(_native.Context, name))


def check_list(d2, prim, k, lim2):
    got_d2, got_prim, held, members, thr = _native.kat_nearest_list(d2, prim, k, lim2)
    want_d2, want_prim, want_held, want_members = NE.list_of(d2, prim, k, lim2)
    what = (k, lim2, len(d2))
    assert held == want_held and members == want_members, what + (held, want_held, members, want_members)
    assert np.array_equal(got_prim, want_prim), what
    assert np.array_equal(bits(got_d2), bits(want_d2)), what
    if k and held == k:
        assert thr[1] == want_prim[k - 1] and bits([thr[0]])[0] == bits(want_d2[k - 1:k])[0], what
    else:
        assert thr == (float("inf"), -1), what
    return got_d2, got_prim


def candidates(r, n, kind):
    """n candidates with distinct ids in a random arrival order: D2 from a few values (many exact ties), or spread, with NaN and +inf among them"""
    prim = r.permutation(4 * n + 8)[:n].astype(np.int32)
    if kind == "ties":
        d2 = r.choice(np.array([0.0, 0.5, 2.5, 2.5000002, 7.0], F), n).astype(F)
    else:
        d2 = r.uniform(0.0, 5.0, n).astype(F)
    if kind == "hostile" and n:
        pick = r.randint(0, 4, n)
        d2 = np.where(pick == 0, F(np.nan), np.where(pick == 1, F(np.inf), d2)).astype(F)
    return d2, prim


@pytest.mark.parametrize("k", KS)
def test_list_against_a_stable_sort(k):
    r = np.random.RandomState(100 + k)
    sizes = list(range(0, 20)) + [31, 63, 64, 65, 100, 127, 128, 200]
    for n in sizes:
        for kind in ("ties", "spread", "hostile"):
            d2, prim = candidates(r, n, kind)
            for lim2 in LIM2:
                check_list(d2, prim, k, lim2)
    # arrival orders that move the most and the least: ascending (every insertion at the back), descending (every insertion at the front)
    asc = (np.arange(200, dtype=F) * F(0.25)).astype(F)
    ids = np.arange(200, dtype=np.int32)
    for d2, prim in ((asc, ids), (asc[::-1], ids), (np.full(200, 2.5, F), ids[::-1]), (np.full(200, 2.5, F), r.permutation(200))):
        for lim2 in LIM2:
            check_list(d2, prim, k, lim2)


def test_list_details():
    inf, nan = float("inf"), float("nan")
    # ties at the cut-off: the smaller ids stay, whatever the arrival order
    d2, prim = check_list([1.0] * 8 + [0.5], [7, 3, 5, 1, 6, 0, 2, 4, 9], 3, inf)
    assert list(prim) == [9, 0, 1] and list(d2) == [0.5, 1.0, 1.0]
    # a candidate that equals a full list's threshold in D2 joins only with a smaller id
    assert list(check_list([1.0, 1.0, 1.0], [5, 6, 4], 2, inf)[1]) == [4, 5]
    # NaN and +inf never join and never count; -1 finds nothing; lim2 = 0 keeps D2 == 0; D2 == lim2 is in
    assert _native.kat_nearest_list([nan, inf, 1.0], [0, 1, 2], 4)[2:4] == (1, 1)
    assert _native.kat_nearest_list([0.0, 1.0], [0, 1], 4, -1.0)[2:4] == (0, 0)
    assert _native.kat_nearest_list([0.0, 1.0], [0, 1], 4, 0.0)[2:4] == (1, 1)
    assert _native.kat_nearest_list([2.5, np.nextafter(F(2.5), F(3))], [0, 1], 4, 2.5)[2:4] == (1, 1)
    assert _native.kat_nearest_list([1.0, 2.0], [0, 1], 4, nan)[2:4] == (0, 0)      # (a NaN lim2 cannot come from cp_limit2; nothing is <= NaN)
    # k == 0: the count alone; the count may exceed k
    assert _native.kat_nearest_list([1.0, 2.0, 3.0], [0, 1, 2], 0, 2.0)[2:4] == (0, 2)
    assert _native.kat_nearest_list([1.0, 2.0, 3.0], [0, 1, 2], 1, 2.0)[2:4] == (1, 2)
    # no candidates at all
    d2, prim, held, members, thr = _native.kat_nearest_list([], [], 3)
    assert np.isposinf(d2).all() and (prim == -1).all() and (held, members) == (0, 0) and thr == (inf, -1)


def test_every_permutation_gives_the_same_list():
    """the order-free claim: all 5040 arrival orders of 7 candidates with ties, a NaN and a +inf, for every k up to 7 and two bounds"""
    d2 = np.array([1.0, 1.0, 0.5, np.nan, 1.0, np.inf, 2.0], F)
    prim = np.array([4, 2, 9, 0, 7, 1, 3], np.int32)
    for k in (1, 2, 3, 4, 7):
        for lim2 in (1.0, float("inf")):
            want = NE.list_of(d2, prim, k, lim2)
            for perm in itertools.permutations(range(7)):
                p = list(perm)
                got = _native.kat_nearest_list(d2[p], prim[p], k, lim2)
                assert np.array_equal(got[1], want[1]) and np.array_equal(bits(got[0]), bits(want[0])) and got[2:4] == want[2:4], (k, lim2, perm)
    r = np.random.RandomState(5)
    d2, prim = candidates(r, 150, "ties")
    base = _native.kat_nearest_list(d2, prim, 64, 2.5)
    for _ in range(50):
        p = r.permutation(150)
        got = _native.kat_nearest_list(d2[p], prim[p], 64, 2.5)
        assert np.array_equal(got[1], base[1]) and np.array_equal(bits(got[0]), bits(base[0])) and got[2:] == base[2:]


def test_restatement_element_0_is_the_closest_point():
    """tests/nearest_expected.py against tests/closest_point_expected.py: element 0 of any k is the brute-force closest point, bit for bit; the count
    is the number of D2 within the bound; the lists are sorted and hold no primitive twice"""
    r = np.random.RandomState(2)
    tris = r.uniform(-1, 1, (60, 1, 3)) + r.uniform(-0.3, 0.3, (60, 3, 3))
    tris[10:18] = tris[10]                                    # eight copies of one triangle: ties in every list that reaches them
    geom = E.Geometry(tris, np.arange(60), np.array([[0.2, 0.1, 1.4, 0.5], [-1.0, 0.5, 0.0, 0.25]], F), np.array([60, 61]))
    pts = r.uniform(-1.5, 1.5, (200, 3)).astype(F)
    pts[:8] = tris[10].mean(axis=0) + r.normal(size=(8, 3)) * 0.05
    pts[8] = np.nan; pts[9, 1] = np.inf
    tab = NE.Table(pts, geom)
    for dmax in (None, 0.4, np.where(np.arange(200) % 2, 0.3, -1.0).astype(F)):
        cp = E.brute_force(pts, geom, dmax)
        for k in (1, 5, 64):
            d2, prim, q, uv, count = tab.nearest(k, dmax)
            assert np.array_equal(bits(d2[:, 0]), bits(cp[0])) and np.array_equal(prim[:, 0], cp[1])
            assert np.array_equal(bits(q[:, 0]), bits(cp[2])) and np.array_equal(bits(uv[:, 0]), bits(cp[3]))
            held = (prim >= 0).sum(axis=1)
            assert np.array_equal(held, np.minimum(count, k))
            with np.errstate(invalid="ignore"):
                assert not (np.diff(d2, axis=1) < 0).any()
            for i in range(200):
                ids = prim[i, :held[i]]
                assert len(set(ids.tolist())) == held[i]
                assert np.isposinf(d2[i, held[i]:]).all() and (prim[i, held[i]:] == -1).all() and (q[i, held[i]:] == 0).all() and (uv[i, held[i]:] == 0).all()
        if dmax is None:
            assert (count[np.isfinite(pts).all(axis=1)] == 62).all() and (count[8:10] == 0).all()
    ties = tab.nearest(3, None)[1][:8]
    assert np.isin(ties, np.arange(10, 18)).any()


def test_list_header_stand_alone_under_sanitizers(tmp_path):
    """csrc/tirt_nearest.h in a program of its own (tests/nearest_list_main.hip: exactly-sized heap arrays, every k and n of the list test, against
    std::stable_sort) with the host code under AddressSanitizer and UndefinedBehaviorSanitizer; the program is run directly"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "nearest_list_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "ti_raytrace_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "nearest_list_main.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "4020 cases equal std::stable_sort" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
