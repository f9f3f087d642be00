"""Pair lists without a device (include/tirt.h, "Point pairs" / "Triangle pairs"): the five entry points in the header, the binding and the library with
their argument types, the refusals that need no device, the scan, the capacity rule and the sorting network of csrc/tirt_pairs.h on the host
(tirt_kat_pairs_host) against numpy's stable sort -- every row length at which the kernels take another path, exact ties, +0 and denormal D2, every
permutation of one row --, and the restatement tests/pairs_expected.py against the closest point's, the k nearest's and the triangle distance's."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_expected as CE
import nearest_expected as NE
import pairs_expected as PE
import triangle_query_expected as TE
from ti_raytrace_amd import PointPairs, PointQuery, TrianglePairs, TriangleQuery, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("tirt_query_point_pairs", "tirt_point_pairs", "tirt_query_mesh_pairs", "tirt_mesh_pairs", "tirt_kat_pairs_host")
LENGTHS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 3000)      # around a wave, around the longest row the kernel orders in LDS, and well beyond


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_symbols_in_header_binding_and_library():
    text = header()
    lib = _native.lib()
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        res, args = _native.SIGNATURES[name]
        assert res is C.c_int
        prms = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(args) == len(prms), (name, len(args), len(prms))
        for a, p in zip(args, prms):
            if "*" in p:
                assert a is C.c_void_p, (name, p, a)
            else:
                assert a is ctype[p.rsplit(" ", 1)[0]], (name, p, a)
    for macro, value in (("TIRT_PAIRS_COUNT", _native.PAIRS_COUNT), ("TIRT_PAIRS_FILL", _native.PAIRS_FILL), ("TIRT_PAIRS_BOTH", _native.PAIRS_BOTH),
                         ("TIRT_PAIRS_UNORDERED", _native.PAIRS_UNORDERED)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    assert _native.PAIRS_UNORDERED & (_native.TRAVERSE_EXHAUSTIVE | _native.COUNT_NODES) == 0
    for section in ("Point pairs", "Triangle pairs"):
        assert ("/* %s (" % section) in open(os.path.join(ROOT, "include", "tirt.h")).read()
    # the kernels live in a file of their own, which is built and whose resource usage is printed
    mk = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC = .*\btirt_pairs\.hip\b", mk, re.M) and re.search(r"^HDR = .*\btirt_pairs\.h\b", mk, re.M)
    assert re.search(r"^\tfor f in .*\btirt_pairs\.hip\b.*kernel-resource-usage", mk, re.M)


def test_refusals_without_a_device():
    L = _native.lib()
    buf = np.zeros(64, np.int64)
    a = buf.ctypes.data
    err = lambda: L.tirt_last_error()

    def point(mode=2, capacity=8, row_start=a, out_d2=a, out_prim=a, flags=0, out_point=None):
        return L.tirt_query_point_pairs(None, None, 0, 3, None, 1, float("inf"), mode, capacity, 64, flags, row_start, out_d2, out_prim, out_point, 3, None, 2,
                                        None, None)

    def mesh(mode=2, capacity=8, row_start=a, out_d2=a, out_prim=a, flags=0, out_point=None):
        return L.tirt_query_mesh_pairs(None, None, 0, 9, None, 1, float("inf"), mode, capacity, 64, flags, row_start, out_d2, out_prim, None, out_point, 6,
                                       None, None)

    def point_host(mode=2, capacity=8, row_start=a, out_d2=a, out_prim=a, flags=0, out_point=None):
        return L.tirt_point_pairs(None, None, 0, None, mode, capacity, 64, flags, row_start, out_d2, out_prim, out_point, None, None)

    def mesh_host(mode=2, capacity=8, row_start=a, out_d2=a, out_prim=a, flags=0, out_point=None):
        return L.tirt_mesh_pairs(None, None, 0, None, mode, capacity, 64, flags, row_start, out_d2, out_prim, None, out_point, None)

    for f, what in ((point, b"tirt_query_point_pairs"), (mesh, b"tirt_query_mesh_pairs"), (point_host, b"tirt_point_pairs"), (mesh_host, b"tirt_mesh_pairs")):
        assert f() == -2 and b"null context" in err()                       # the arguments are in order: the context is looked at next
        for mode in (0, 1, 2):
            assert f(mode=mode) == -2 and b"null context" in err()
        for mode in (-1, 3, 4, 100):
            assert f(mode=mode) == -2 and b"unknown mode" in err() and what in err()
        for mode in (1, 2):
            assert f(mode=mode, out_d2=None, out_prim=None) == -2 and b"without out_prim and without out_d2" in err()
            assert f(mode=mode, capacity=-1) == -2 and b"capacity < 0" in err()
            assert f(mode=mode, out_d2=None) == -2 and b"TIRT_PAIRS_UNORDERED" in err()
            assert f(mode=mode, out_prim=None) == -2 and b"TIRT_PAIRS_UNORDERED" in err()
            assert f(mode=mode, out_d2=None, flags=4) == -2 and b"null context" in err()      # either suffices when the rows are not ordered
            assert f(mode=mode, out_prim=None, flags=4, out_point=a) == -2 and b"need out_prim" in err()
        assert f(mode=0, capacity=-1, out_d2=None, out_prim=None) == -2 and b"null context" in err()      # the sizing call looks at neither
        assert f(row_start=a + 4) == -2 and b"8-byte aligned" in err()
        assert f(row_start=None) == -2 and b"null row_start" in err()
    with pytest.raises(_native.TirtError, match="no member"):
        _native.kat_pairs_host([1.0, np.nan], [0, 1], [2])
    with pytest.raises(_native.TirtError, match="no member"):
        _native.kat_pairs_host([1.0, np.inf], [0, 1], [2])
    with pytest.raises(_native.TirtError, match="no member"):
        _native.kat_pairs_host([1.0, 2.0], [0, -1], [2])
    with pytest.raises(_native.TirtError, match="capacity < 0"):
        _native.kat_pairs_host([1.0], [0], [1], capacity=-1)


class NoDeviceScene:
    """a scene whose context is never made: every check below has to come before anything needs a device"""
    _ctx = None
    _device_id = 0

    @property
    def ctx(self):
        raise AssertionError("the check needed a device")


def test_python_argument_checks_need_no_device():
    torch = pytest.importorskip("torch")
    assert PointPairs._fields == ("row_start", "prim", "dist2", "point", "uv")
    assert TrianglePairs._fields == ("row_start", "prim", "d2", "code", "point_query", "point_scene")
    q, t = PointQuery(NoDeviceScene()), TriangleQuery(NoDeviceScene())
    pts, tris = torch.zeros((5, 3), dtype=torch.float32), torch.zeros((5, 3, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match="float32"):
        q.within(pts.double(), 1.0)
    with pytest.raises(ValueError, match="points must be"):
        q.within(torch.zeros((5, 2)), 1.0)
    with pytest.raises(TypeError, match="on the GPU"):
        q.within(pts, 1.0)
    with pytest.raises(ValueError, match="triangles must be"):
        t.pairs(torch.zeros((5, 3)))
    with pytest.raises(TypeError, match="on the GPU"):
        t.pairs(tris)
    with pytest.raises(TypeError, match="max_distance is required"):
        t.count_within(tris, None)
    # query(): row_start expanded to the query of every pair; the pairs of rows cut by a capacity are not among them
    rs = torch.tensor([0, 2, 2, 5, 9], dtype=torch.int64)
    full = PointPairs(rs, torch.zeros(9, dtype=torch.int32), torch.zeros(9), None, None)
    assert full.query().tolist() == [0, 0, 2, 2, 2, 3, 3, 3, 3]
    cut = TrianglePairs(rs, torch.zeros(6, dtype=torch.int32), torch.zeros(6), torch.zeros(6, dtype=torch.int32), None, None)
    assert cut.query().tolist() == [0, 0, 2, 2, 2]
    for name in ("query_point_pairs", "query_mesh_pairs", "point_pairs", "mesh_pairs"):
        assert callable(getattr(_native.Context, name))


def members(r, n, kind):
    """n members with distinct ids in a random arrival order"""
    prim = r.permutation(4 * n + 8)[:n].astype(np.int32)
    if kind == "ties":            # equal D2 bits with distinct ids, +0 among them
        d2 = r.choice(np.array([0.0, 0.5, 2.5, 2.5000002, 7.0], F), n).astype(F)
    elif kind == "tiny":          # +0, denormals and the smallest normals: the order of the bits is the order of the floats there too
        d2 = r.choice(np.array([0.0, 1e-45, 3e-45, 1e-40, 1.1754942e-38, 1.1754944e-38, 2e-38], F), n).astype(F)
    else:
        d2 = r.uniform(0.0, 5.0, n).astype(F)
    return d2, prim


def check_rows(d2, prim, row_len, capacity=None):
    got = _native.kat_pairs_host(d2, prim, row_len, capacity)
    want = PE.ordered_rows(d2, prim, row_len, capacity)
    what = (list(np.asarray(row_len)[:12]), capacity)
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[2], want[2]), what + (np.nonzero(got[2] != want[2])[0][:8],)
    assert np.array_equal(bits(got[1]), bits(want[1])), what
    return got


@pytest.mark.parametrize("kind", ["ties", "tiny", "spread"])
def test_rows_against_a_stable_sort(kind):
    r = np.random.RandomState(7)
    rows = [members(r, n, kind) for n in LENGTHS + tuple(range(3, 40))]
    d2 = np.concatenate([x[0] for x in rows]); prim = np.concatenate([x[1] for x in rows])
    row_len = [x[0].size for x in rows]
    check_rows(d2, prim, row_len)
    for n in LENGTHS:                                        # each length as the only row, in ascending and in descending arrival order
        a, p = members(r, n, kind)
        order = np.lexsort((p, a))
        check_rows(a[order], p[order], [n])
        check_rows(a[order[::-1]], p[order[::-1]], [n])


def test_every_permutation_of_one_row():
    d2 = np.array([1.0, 1.0, 0.0, 1e-45, 1.0, 2.0], F)
    prim = np.array([4, 2, 9, 0, 7, 3], np.int32)
    perms = np.array(list(itertools.permutations(range(6))))
    got = check_rows(d2[perms].reshape(-1), prim[perms].reshape(-1), [6] * perms.shape[0])      # 720 rows, one call
    assert (got[2].reshape(-1, 6) == [9, 0, 2, 4, 7, 3]).all()
    assert np.array_equal(got[0], 6 * np.arange(perms.shape[0] + 1))


def test_scan_and_capacity_rule():
    r = np.random.RandomState(9)
    row_len = r.randint(0, 6, 5000)                          # more rows than one block of the scan: the block sums are themselves scanned
    row_len[1023:1026] = (0, 7, 0)
    d2, prim = [], []
    for n in row_len:
        a, p = members(r, n, "ties")
        d2.append(a); prim.append(p)
    d2, prim = np.concatenate(d2), np.concatenate(prim)
    full = check_rows(d2, prim, row_len)
    rs = full[0]
    assert np.array_equal(rs, np.concatenate([[0], np.cumsum(row_len)])) and rs.dtype == np.int64
    end = int(rs[2500]) if rs[2500] > rs[2499] else int(rs[rs > rs[2499]][0])      # the end of a row that is not empty
    for capacity in (end, end - 1, 0, int(rs[-1]), int(rs[-1]) + 5):
        got = check_rows(d2, prim, row_len, capacity)
        rows, written = PE.rows_that_fit(rs, capacity)
        assert np.array_equal(got[0], rs)                    # row_start is complete whatever the capacity
        assert np.array_equal(bits(got[1][:written]), bits(full[1][:written])) and np.array_equal(got[2][:written], full[2][:written])
        assert np.isnan(got[1][written:]).all() and (got[2][written:] == -1).all()      # nothing behind the last row that fits: no partial row
    assert PE.rows_that_fit(rs, end - 1)[1] < end == PE.rows_that_fit(rs, end)[1]
    assert _native.kat_pairs_host([], [], [])[0].tolist() == [0]
    assert _native.kat_pairs_host([], [], [0, 0, 0])[0].tolist() == [0, 0, 0, 0]


def small_geometry():
    r = np.random.RandomState(2)
    tris = r.uniform(-1, 1, (40, 1, 3)) + r.uniform(-0.3, 0.3, (40, 3, 3))
    tris[10:18] = tris[10]                                   # eight copies of one triangle: ties in every row that reaches them
    return r, CE.Geometry(tris, np.arange(40), np.array([[0.2, 0.1, 1.4, 0.5], [-1.0, 0.5, 0.0, 0.25]], F), np.array([40, 41]))


def test_restatement_of_point_pairs_links_to_nearest_and_closest():
    r, geom = small_geometry()
    pts = r.uniform(-1.5, 1.5, (120, 3)).astype(F)
    pts[:8] = geom.tris[10].mean(axis=0) + r.normal(size=(8, 3)) * 0.05
    pts[8] = np.nan; pts[9, 1] = np.inf
    tab, near = PE.PointTable(pts, geom), NE.Table(pts, geom)
    for dmax in (None, 0.4, 0.0, -1.0, np.nan, np.where(np.arange(120) % 3, 0.3, -1.0).astype(F)):
        rs, prim, d2, q, uv = tab.within(dmax)
        nd2, nprim, nq, nuv, count = near.nearest(5, dmax)
        cp = CE.brute_force(pts, geom, dmax)
        assert np.array_equal(np.diff(rs), count)
        for i in range(120):
            a, m = rs[i], min(5, count[i])
            assert np.array_equal(prim[a:a + m], nprim[i, :m]) and np.array_equal(bits(d2[a:a + m]), bits(nd2[i, :m]))
            assert np.array_equal(bits(q[a:a + m]), bits(nq[i, :m])) and np.array_equal(bits(uv[a:a + m]), bits(nuv[i, :m]))
            if count[i]:
                assert prim[a] == cp[1][i] and bits(d2[a:a + 1])[0] == bits(cp[0][i:i + 1])[0]
            else:
                assert cp[1][i] == -1
        if dmax is None:
            assert (np.diff(rs)[np.isfinite(pts).all(axis=1)] == 42).all() and (np.diff(rs)[8:10] == 0).all()
        if isinstance(dmax, float) and not dmax >= 0:
            assert rs[-1] == 0
    assert np.array_equal(PE.query_of(np.array([0, 2, 2, 5])), [0, 0, 2, 2, 2])


def test_restatement_of_triangle_pairs_links_to_the_triangle_distance():
    r, geom = small_geometry()
    tris = (r.uniform(-1.2, 1.2, (60, 1, 3)) + r.uniform(-0.4, 0.4, (60, 3, 3))).astype(F)
    tris[0] = geom.tris[10]; tris[1, 0, 0] = np.nan; tris[2, 2, 1] = -np.inf
    tab = PE.TriangleTable(tris, geom)
    for dmax in (0.0, 0.25, None, -1.0, np.where(np.arange(60) % 2, 0.2, np.nan).astype(F)):
        rs, prim, d2, code, P, Q = tab.pairs(dmax)
        cp = TE.brute_force(tris, geom, dmax)
        n = np.diff(rs)
        assert np.array_equal(n > 0, cp[1] >= 0) and (n[1:3] == 0).all()
        first = rs[:-1][n > 0]
        assert np.array_equal(prim[first], cp[1][n > 0]) and np.array_equal(bits(d2[first]), bits(cp[0][n > 0])) and np.array_equal(code[first], cp[2][n > 0])
        assert np.array_equal(bits(P[first]), bits(cp[3][n > 0])) and np.array_equal(bits(Q[first]), bits(cp[4][n > 0]))
        assert np.isin(prim, geom.tri_prim).all()            # an analytic sphere is in nobody's row
        for i in range(60):
            row = slice(rs[i], rs[i + 1])
            assert np.array_equal(np.lexsort((prim[row], d2[row])), np.arange(n[i])) and len(set(prim[row].tolist())) == n[i]
        if isinstance(dmax, float) and dmax == 0.0:
            assert n[0] >= 8 and (d2 == 0).all()            # the copy of the tied triangle touches all eight copies
        if dmax is None:
            assert (n[np.isfinite(tris).all(axis=(1, 2))] == 40).all()


def test_header_stand_alone_under_sanitizers(tmp_path):
    """csrc/tirt_pairs.h in a program of its own (tests/pairs_order_main.hip: exactly-sized heap arrays, the row lengths of the tests above, against
    std::stable_sort and a running sum) with the host code under AddressSanitizer and UndefinedBehaviorSanitizer; the program is run directly"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "pairs_order_main")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-I" + os.path.join(ROOT, "ti_raytrace_amd", "csrc"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "pairs_order_main.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "66 cases equal std::stable_sort" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
