"""The yardstick of tests/test_gpu_beam_lists.py without a device: the two entry points in the header, the binding and the library; the float32 restatement of the
camera ray; check_lists and expected_walk of tests/beam_lists_expected.py on lists made from the hit set H itself (reference_lists, over the oracle's LBVH) --
accepted as they are, rejected with the promised message for every single defect --; and, per named case of tests/beam_lists_cases.py and from the reference
alone, the conditions without which the GPU test would show nothing:

  * at least 90 % of the sample rays that have a hit have it within `start`, the start of the pixel's bound (else most rows would be left to k_trace).  The two
    overflow cases (`sparse`) are exempt by name and must have a pixel where more than 24 leaves carry a hit instead;
  * the aimed rows do their job -- each count is printed and must be > 0:
      rows whose hit leaf is not the first entry of the pixel's list     (not asked of one_triangle, one_sphere: one leaf; identical: 200 leaves at one distance,
                                                                          the overflow rule leaves the lists empty)
      vertex / edge rows whose hit primitive no lattice row of the       (not asked of those three either: a corner clip needs a second primitive behind it or
      pixel hits: the corner clips                                        a silhouette finer than the lattice, one triangle's straight edges are not)
      pixels with a probe that misses and a sample row that hits         (not asked of cornell_inside and teapot_window: the scene fills the tested pixels,
                                                                          every probe hits)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import beam_lists_expected as bl
import oracle_api as oa
from beam_lists_cases import CASES, make_cases
from ti_raytrace_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tirt_primary_beam_lists_download", "tirt_kat_primary_list_walk")
f = np.float32
ONE_LEAF = ("one_triangle", "one_sphere", "identical")
FILLED = ("cornell_inside", "teapot_window")


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tirt.h")).read(), flags=re.S)
    lib = _native.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    assert len(_native.SIGNATURES["tirt_primary_beam_lists_download"][1]) == 5 and len(_native.SIGNATURES["tirt_kat_primary_list_walk"][1]) == 7
    assert _native.KAT_LIST_WALK_OUT == 9
    for name in ("primary_beam_lists_info", "primary_beam_lists_download", "kat_primary_list_walk"):
        assert callable(getattr(_native.Context, name))
    # PVB_CMAX of the restatement is the kernels'
    src = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_pvb.h")).read()
    assert int(re.search(r"constexpr int PVB_CMAX = (\d+);", src).group(1)) == bl.PVB_CMAX
    src = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_pvb.hip")).read()
    assert float(re.search(r"constexpr float PVB_REACH = ([0-9.]+)f;", src).group(1)) == float(bl.PVB_REACH)
    src = open(os.path.join(ROOT, "ti_raytrace_amd", "csrc", "tirt_internal.h")).read()
    m = re.search(r"TR_MARGIN_CELLS = ([0-9.]+)f, TR_MARGIN_PER_RHO = ([0-9.]+)f, TR_MARGIN_BEAM_EXTRA = ([0-9.]+)f", src)
    assert tuple(float(x) for x in m.groups()) == (bl.TR_MARGIN_CELLS, bl.TR_MARGIN_PER_RHO, bl.TR_MARGIN_BEAM_EXTRA)
    assert float(re.search(r"TR_FAR_RHO = ([0-9.]+)f", src).group(1)) == bl.TR_FAR_RHO


def test_refusals_without_a_device():
    L = _native.lib()
    info = np.full(4, 7, np.int32)
    z = np.zeros(4, f); k = np.zeros(4, np.int32); out = np.full(36, 7.0, f)
    assert L.tirt_primary_beam_lists_download(None, None, None, None, info.ctypes.data) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_primary_beam_lists_download(None, None, None, None, None) == -2 and b"null info" in L.tirt_last_error()
    assert L.tirt_primary_beam_lists_download(None, info.ctypes.data, None, None, info.ctypes.data) == -2 and b"together" in L.tirt_last_error()
    assert L.tirt_kat_primary_list_walk(None, 4, k, z, z, out, 9) == -2 and b"null context" in L.tirt_last_error()
    assert L.tirt_kat_primary_list_walk(None, 4, k, z, z, out, 8) == -2 and b"stride too small" in L.tirt_last_error()
    assert L.tirt_kat_primary_list_walk(None, -1, k, z, z, out, 9) == -2 and b"negative n" in L.tirt_last_error()
    assert (info == 7).all() and (out == 7.0).all()


# ---- the camera ray ---------------------------------------------------------------------------------------------------------------------
def test_direction_restatement_is_camera_rays_plus_the_jitter():
    spec = CASES["cornell_13x7"]
    ex = spec.make(spec.W, spec.H); ex.scene.setup_data_cpu(); spec.aim(ex)
    px = np.arange(spec.W * spec.H)
    zero = np.zeros(px.shape[0], f)
    assert np.array_equal(bl.jittered_rays(ex.cam, spec.H, px, zero, zero).view(np.uint32), oa.camera_rays(ex.cam, spec.W, spec.H).view(np.uint32))
    assert np.array_equal(bl.jittered_rays(ex.cam, spec.H, px[5:9], zero[:4], zero[:4]).view(np.uint32), oa.camera_rays(ex.cam, spec.W, spec.H, px[5:9]).view(np.uint32))
    moved = bl.jittered_rays(ex.cam, spec.H, px, zero + f(0.25), zero - f(0.5))
    assert (moved[:, 3:] != oa.camera_rays(ex.cam, spec.W, spec.H)[:, 3:]).any(axis=1).all()
    assert bl.clip_jitter([0.5, 0.49999999, -0.7, 0.1]).tolist() == [float(bl.J_HI), float(bl.J_HI), -0.5, float(f(0.1))]


# ---- the cases, from the reference alone ---------------------------------------------------------------------------------------------------
_built = {}


def reference_case(name):
    """(spec, geo, [Case], [reference lists per Case], P) of a named case over the oracle's LBVH; made once and shared (nothing changes it: the defect tests copy)"""
    if name not in _built:
        spec = CASES[name]
        ex = spec.make(spec.W, spec.H)
        ex.scene.setup_data_cpu()
        spec.aim(ex)
        orc = oa.OracleScene(ex.scene, ex.cam)
        assert orc.lbvh_build() == ex.scene.primitive_count - 1
        compact = orc.lbvh_get()[2]
        geo = bl.from_reference(compact, ex.scene.primitive_np, ex.cam)
        cases = make_cases(spec, ex.scene, ex.cam, compact, geo)
        P = spec.order().shape[0]
        _built[name] = (spec, geo, cases, [bl.reference_lists(c, P) for c in cases], P)
    return _built[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_conditions_and_reference_lists(name):
    spec, geo, cases, ref, P = reference_case(name)
    assert geo.far == (not spec.lists)
    n = {"rows": 0, "hit": 0, "within": 0, "not_first": 0, "clips": 0, "probe_miss_with_hit": 0, "over_24": 0, "dropped": 0}
    for case, lists in zip(cases, ref):
        st = bl.check_lists(case, lists)
        assert st["pixels"] == case.ks.shape[0]
        w = bl.expected_walk(case, lists)
        res = w["resolved"]
        # lists made from H: a resolved row's walk finds H's first element
        for got, want in zip(w["walk"], w["first"]):
            assert np.array_equal(np.asarray(got)[res].view(np.uint32), np.asarray(want)[res].view(np.uint32))
        assert (w["steps"][w["dead"]] == 0).all() and (w["steps"] <= bl.PVB_CMAX).all()
        ft, _, _, fp = case.hits["first"]
        hit = fp >= 0
        n["rows"] += hit.shape[0]; n["hit"] += int(hit.sum()); n["within"] += int((hit & (ft <= case.start[case.rows["at"]])).sum()); n["dropped"] += case.dropped
        assert np.bincount(case.rows["at"], minlength=case.ks.shape[0]).max() <= bl.ROW_CAP
        assert (case.rows["jx"] >= bl.J_LO).all() and (case.rows["jx"] <= bl.J_HI).all() and (case.rows["jy"] >= bl.J_LO).all() and (case.rows["jy"] <= bl.J_HI).all()
        for a, k in enumerate(case.ks.tolist()):
            r = slice(int(case.span[a]), int(case.span[a + 1]))
            kinds, prim = case.rows["kind"][r], fp[r]
            if lists["count"][k] > 0:
                first_code = np.uint32(np.int32(lists["code"][0, k]).view(np.uint32))
                n["not_first"] += int(((prim >= 0) & (geo.code[np.maximum(prim, 0)] != first_code)).sum())
            lattice = set(prim[(kinds == bl.LATTICE) & (prim >= 0)].tolist())
            aimed = ((kinds == bl.VERTEX) | (kinds == bl.EDGE)) & (prim >= 0)
            n["clips"] += sum(1 for p in prim[aimed].tolist() if p not in lattice)
            n["probe_miss_with_hit"] += int(case.start[a] >= bl.INF_VALUE and (prim >= 0).any())
            n["over_24"] += int(np.isfinite(case.hits["T"][r]).any(axis=0).sum() > bl.PVB_CMAX)
    print("beam lists, reference %-16s %s" % (name, n))
    if spec.sparse:
        assert n["over_24"] >= 1, "no pixel of an overflow case has more than %d leaves with a hit" % bl.PVB_CMAX
    elif spec.lists:
        assert n["hit"] > 0 and n["within"] >= 0.9 * n["hit"], "%d of %d sample rays that hit do so within the start of their pixel's bound" % (n["within"], n["hit"])
    if name not in ONE_LEAF:
        assert n["not_first"] > 0 and n["clips"] > 0
    if name not in FILLED:
        assert n["probe_miss_with_hit"] > 0


# ---- every single defect is rejected, with the message the check promises -----------------------------------------------------------------------
def copy_lists(lists):
    return {k: v.copy() for k, v in lists.items()}


def first_case(name):
    spec, geo, cases, ref, P = reference_case(name)
    return cases[0], ref[0]


def corner_clip(case, lists):
    """(tested pixel a, entry e): a pixel with a vertex or edge row whose hit primitive no lattice row of the pixel hits, and that primitive's entry on its list"""
    fp = case.hits["first"][3]
    for a, k in enumerate(case.ks.tolist()):
        r = slice(int(case.span[a]), int(case.span[a + 1]))
        kinds, prim = case.rows["kind"][r], fp[r]
        lattice = set(prim[(kinds == bl.LATTICE) & (prim >= 0)].tolist())
        for p in prim[((kinds == bl.VERTEX) | (kinds == bl.EDGE)) & (prim >= 0)].tolist():
            if p not in lattice:
                codes = lists["code"][:lists["count"][k], k].view(np.uint32)
                e = np.flatnonzero(codes == case.geo.code[p])
                if e.size:
                    return a, int(e[0])
    raise AssertionError("no corner clip in this case")


def drop_entry(lists, k, e):
    n = int(lists["count"][k])
    for name in ("code", "nr"):
        lists[name][e:n - 1, k] = lists[name][e + 1:n, k]
    lists["count"][k] = n - 1


def test_accepts_the_reference_lists_of_the_defect_cases():
    for name in ("cornell_16x12", "slivers"):
        case, lists = first_case(name)
        bl.check_lists(case, lists)


def test_rejects_a_dropped_corner_leaf():
    case, ref = first_case("cornell_16x12")
    a, e = corner_clip(case, ref)
    k = int(case.ks[a])
    lists = copy_lists(ref)
    code = int(np.int32(lists["code"][e, k]).view(np.uint32))
    drop_entry(lists, k, e)
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): its (vertex|edge) ray .* but leaf %#x is not on the list" % (k, code)):
        bl.check_lists(case, lists)


def long_list(case, lists, at_least=3):
    for a, k in enumerate(case.ks.tolist()):
        if lists["count"][k] >= at_least and len(set(lists["nr"][:lists["count"][k], k].tolist())) >= at_least:
            return a, k
    raise AssertionError("no list of %d entries at different distances" % at_least)


def test_rejects_a_swap_that_makes_nr_fall():
    case, ref = first_case("cornell_16x12")
    a, k = long_list(case, ref)
    lists = copy_lists(ref)
    nr = lists["nr"][:, k]
    e = next(e for e in range(1, lists["count"][k]) if nr[e] > nr[e - 1])
    for name in ("code", "nr"):
        lists[name][[e - 1, e], k] = lists[name][[e, e - 1], k]
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): nr falls from .* at leaf %#x \(entry %d\)" % (k, int(np.int32(lists["code"][e, k]).view(np.uint32)), e)):
        bl.check_lists(case, lists)


def test_rejects_an_nr_above_a_sampled_t():
    case, ref = first_case("cornell_16x12")
    a, k = long_list(case, ref)
    lists = copy_lists(ref)
    e = int(lists["count"][k]) - 1                      # the last entry: raising it keeps the order
    col = case.hits["col"][case.geo.prim_of[int(np.int32(lists["code"][e, k]).view(np.uint32))]]
    t = case.hits["T"][int(case.span[a]):int(case.span[a + 1]), col]
    tmin = t[np.isfinite(t)].min()
    assert tmin <= lists["bound"][k]
    lists["nr"][e, k] = np.nextafter(tmin, f(np.inf))
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): its .* but leaf %#x is listed at nr .* beyond that hit" % (k, int(np.int32(lists["code"][e, k]).view(np.uint32)))):
        bl.check_lists(case, lists)


def test_rejects_a_bound_above_start():
    case, ref = first_case("cornell_16x12")
    a = int(np.flatnonzero(case.start < bl.INF_VALUE)[0])
    k = int(case.ks[a])
    lists = copy_lists(ref)
    lists["bound"][k] = np.nextafter(case.start[a], f(np.inf))
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): bound .* lies above its start" % k):
        bl.check_lists(case, lists)


def test_rejects_a_code_twice_and_a_code_that_is_no_leaf():
    case, ref = first_case("cornell_16x12")
    a, k = long_list(case, ref, 2)
    lists = copy_lists(ref)
    lists["code"][1, k] = lists["code"][0, k]
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): leaf %#x appears 2 times" % (k, int(np.int32(lists["code"][0, k]).view(np.uint32)))):
        bl.check_lists(case, lists)
    lists = copy_lists(ref)
    alien = int(case.geo.code.min()) - 1                # (codes are ~slot: the smallest code minus one names a slot past the last)
    assert alien not in set(case.geo.code.tolist())
    lists["code"][0, k] = np.uint32(alien).view(np.int32)
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): leaf %#x on its list is no leaf of the tree" % (k, alien)):
        bl.check_lists(case, lists)


def test_rejects_a_count_of_25():
    case, ref = first_case("cornell_16x12")
    lists = copy_lists(ref)
    k = int(case.ks[0])
    lists["count"][k] = bl.PVB_CMAX + 1
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): count 25 is outside \[-1, 24\]" % k):
        bl.check_lists(case, lists)


def test_rejects_an_overflow_whose_bound_did_not_come_in():
    """more leaves than a list holds: the farthest goes -- and the bound stays at its start, so the leaf that went still holds a hit within it"""
    case, ref = first_case("slivers")
    cut = [(a, k) for a, k in enumerate(case.ks.tolist()) if ref["count"][k] == bl.PVB_CMAX and ref["bound"][k] < case.start[a]]
    assert cut, "no full list whose bound came in among the slivers"
    a, k = cut[0]
    lists = copy_lists(ref)
    lists["bound"][k] = case.start[a]
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): its .* ray .* but leaf 0x[0-9a-f]+ is not on the list" % k):
        bl.check_lists(case, lists)
    # and the other way round: a bound that comes in although the list is not full
    case, ref = first_case("cornell_16x12")
    a = int(np.flatnonzero(case.start < bl.INF_VALUE)[0]); k = int(case.ks[a])
    lists = copy_lists(ref)
    lists["bound"][k] = max(lists["nr"][:lists["count"][k], k].max(), f(0.5) * case.start[a])
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): bound .* came in below its start .* although only \d+ leaves meet" % k):
        bl.check_lists(case, lists)


def test_rejects_a_list_of_every_leaf():
    """what film equality cannot see at all: a list that holds leaves the pixel's rays cannot reach"""
    case, ref = first_case("soup_0.8")
    lists = copy_lists(ref)
    a = next(a for a, k in enumerate(case.ks.tolist()) if 0 <= lists["count"][k] < bl.PVB_CMAX - 1 and not bl._meets(case, a, 1.5).all())
    k = int(case.ks[a])
    outside = int(np.flatnonzero(~bl._meets(case, a, 1.5))[0])
    n = int(lists["count"][k])
    lists["code"][n, k] = case.geo.code[outside:outside + 1].view(np.int32)[0]
    lists["nr"][n, k] = lists["nr"][n - 1, k] if n else f(0.0)
    lists["count"][k] = n + 1
    with pytest.raises(AssertionError, match=r"pixel k=%d \(.*\): leaf %#x is on its list although its box" % (k, int(case.geo.code[outside]))):
        bl.check_lists(case, lists)
