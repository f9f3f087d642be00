"""Moving geometry in place (csrc/tirt_dynamic.hip through tirt_vertex_update / tirt_vertex_update_device and Scene.update_vertices).

The definition of correct is bit-identity with a FRESH scene: a second Scene on the same device built the existing way (add_mesh / add_shape,
setup_data_cpu, setup_data_gpu) from the moved positions.  Compared: vertex rows, scene box, unsorted and sorted Morton pairs, the LBVH's
node arrays, the traversal tree, both shading tables, bvh_info, the host mirrors, films of every integrator, ray queries.  Plus the refusals,
which must leave the old geometry and the old build answering as before."""
import numpy as np
import pytest

import oracle_api as oa
from common import rel_l2, same_bits, tiny_scene
from ti_raytrace_amd import Example, PT_RGB, BDPT_RGB, Debug, scenes, _native

pytestmark = pytest.mark.gpu

# tests/test_gpu_bdpt.py: two device runs of one BDPT job differ by the float-atomic order of the splats (1e-6 there), device against oracle 1e-3
BDPT_DEVICE_TOL = 1e-6
BDPT_ORACLE_TOL = 1e-3


def same(a, b):
    return same_bits(a, b, nan_payload=True)


def positions_of(ex):
    return ex.scene.vertex_np[:, 0:3].copy()


def wobble(pos, seed=1, amount=0.05):
    """every vertex moved by up to `amount` of the mesh's extent (float32 in, float32 out)"""
    r = np.random.RandomState(seed)
    ext = (pos.max(axis=0) - pos.min(axis=0)).astype(np.float64)
    return (pos.astype(np.float64) + r.uniform(-amount, amount, size=pos.shape) * ext).astype(np.float32)


def fresh_example(src, positions, W, H, integrator=None, build=True):
    """a second example on the same device, built the existing way from `positions` ([nv, 3] float32 in src's vertex order): the
    materials, shapes and environment of `src` in the order src added them"""
    s0 = src.scene
    ex = Example.example(W, H, src.sample_count, 0)
    blocks = {mat: (vfirst, ntri) for _, ntri, mat, vfirst in s0._prim_mat}
    shapes = {mat: sha for _, sha, mat in s0._shape_prims}
    for m in range(s0.material_count):
        if m in shapes:
            ex.scene.add_shape(s0.shape_cpu[shapes[m]], s0.material_cpu[m])
        else:
            vfirst, ntri = blocks.get(m, (0, 0))
            ex.scene.add_mesh(positions[vfirst:vfirst + 3 * ntri].reshape(-1, 3, 3), s0.material_cpu[m])
    ex.scene.env, ex.scene.env_power = s0.env, s0.env_power
    ex.integrator = (integrator or type(src.integrator))(W, H, ex.cam, ex.scene, 64)
    if build:
        ex.build_scene()
        if getattr(s0, "normals_processed", False):
            ex.scene.process_normal()
        if s0._area_called:
            ex.scene.total_area()
        ex.cam.target[:] = src.cam.target                  # the camera of `src` as it stands
        ex.cam.set_view_point(src.cam.yaw, src.cam.pitch, src.cam.roll, src.cam.scale)
    return ex


def state(ex):
    sc, ctx = ex.scene, ex.scene.ctx
    n = sc.primitive_count
    morton_s, bvh_node, compact = ctx.lbvh_download(n)
    lo, hi = ctx.scene_box()
    return {"vertex": ctx.vertex_download(sc.vertex_count), "box": np.concatenate([lo, hi]), "morton": ctx.morton_download(n),
            "morton_sorted": morton_s, "bvh_node": bvh_node, "compact_node": compact, "traversal_tree": ctx.traversal_tree_download(n),
            "shade_table": ctx.shade_table_download(0, n), "light_table": ctx.shade_table_download(1, sc.light_count),
            "bvh_info": np.asarray(sorted(ctx.bvh_info().items()), dtype=object),
            "mirror_vertex_np": sc.vertex_np,
            "mirror_box": np.concatenate([sc.minboundarynp[0], sc.maxboundarynp[0], sc.bvh.minboundarynp[0], sc.bvh.maxboundarynp[0]]),
            "mirror_light_area": sc.light_area.to_numpy(), "mirror_vertex_field": sc.vertex.to_numpy()}


def assert_same_state(a, b, what=""):
    sa, sb = state(a), state(b)
    for k in sa:
        if sa[k].dtype == np.float32:
            assert same(sa[k], sb[k]), (what, k, int((sa[k].view(np.uint32) != sb[k].view(np.uint32)).sum()))
        else:
            assert sa[k].shape == sb[k].shape and (sa[k] == sb[k]).all(), (what, k)


def spectral_style_cornell(W, H):
    """the Cornell box with process_normal and total_area applied (what scenes.spectral_box does to it), through PT_RGB"""
    ex = scenes.cornell_box(W, H, 4, device_id=0)
    ex.build_scene()
    ex.scene.process_normal()
    return ex


MAKERS = {
    "tiny": lambda: (tiny_scene(300, seed=5, W=32, H=32, device_id=0), 32),
    "cornell": lambda: (scenes.cornell_box(32, 32, 4, device_id=0), 32),
    "headline_100k": lambda: (scenes.synthetic(64, 64, 4, device_id=0), 64),
}


def built(name):
    ex, W = MAKERS[name]()
    ex.build_scene()
    return ex, W


# ---- (a) build state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MAKERS))
def test_state_after_update_equals_fresh(gpu_ctx_ok, name):
    ex, W = built(name)
    new = wobble(positions_of(ex))
    ex.scene.update_vertices(new)
    assert_same_state(ex, fresh_example(ex, new, W, W), name)
    # the [k/3, 3, 3] form and a numpy array that is not contiguous say the same
    again = wobble(positions_of(ex), seed=2)
    wide = np.zeros((again.shape[0], 5), np.float32); wide[:, 1:4] = again
    ex.scene.update_vertices(wide[:, 1:4].reshape(-1, 3, 3) if name == "tiny" else wide[:, 1:4])
    assert_same_state(ex, fresh_example(ex, again, W, W), name + " strided")


# ---- (b) the box follows -----------------------------------------------------------------------------------------------------------
def test_box_follows_the_mesh(gpu_ctx_ok):
    ex, W = built("tiny")
    pos = positions_of(ex)
    old_lo, old_hi = ex.scene.minboundarynp.copy(), ex.scene.maxboundarynp.copy()
    ext = pos.max(axis=0) - pos.min(axis=0)
    far = pos.copy()
    far[: (far.shape[0] // 6) * 3] += (np.float32(10.0) * ext * np.asarray([1.0, -2.0, 0.5], np.float32)).astype(np.float32)      # half the triangles, well outside the old box
    ex.scene.update_vertices(far)
    assert (ex.scene.maxboundarynp[0, 0] > old_hi[0, 0] + 5 * ext[0]) and (ex.scene.minboundarynp[0, 1] < old_lo[0, 1] - 5 * ext[1])
    assert_same_state(ex, fresh_example(ex, far, W, W), "far")
    small = (pos * np.float32(0.1)).astype(np.float32)
    ex.scene.update_vertices(small)
    assert np.all(ex.scene.maxboundarynp - ex.scene.minboundarynp < 0.11 * (old_hi - old_lo))
    assert_same_state(ex, fresh_example(ex, small, W, W), "shrunk")


# ---- (c) films -----------------------------------------------------------------------------------------------------------------------
def render_pt(ex, frames, seed=5):
    ctx = ex.scene.ctx
    ctx.film_clear()
    ctx.pt_rgb_render(0, frames, seed, 15, 64, 0)
    return ctx.film_download(ex.imgSizeX, ex.imgSizeY)[0]


def test_pt_rgb_film_after_update(gpu_ctx_ok):
    W = H = 48
    frames = 4
    ex = scenes.cornell_box(W, H, frames, device_id=0)
    ex.build_scene()
    render_pt(ex, frames)                                   # a film of the old geometry first: tables and lists of it exist
    new = wobble(positions_of(ex), amount=0.02)
    ex.scene.update_vertices(new)
    ex.frame_camera(0.8)                                    # from the refreshed box mirrors
    got = render_pt(ex, frames)
    fr = fresh_example(ex, new, W, H)
    fr.frame_camera(0.8)
    assert same(ex.cam.view_inv_np, fr.cam.view_inv_np)
    assert same(got, render_pt(fr, frames))
    o = oa.OracleScene(ex.scene, ex.cam); o.lbvh_build()    # the oracle reads the UPDATED scene's host mirrors
    want, _ = o.render(W, H, 0, frames, seed=5)
    assert same_bits(got, want), "rel-L2 %.3e" % rel_l2(got, want)


def test_debug_views_after_update(gpu_ctx_ok):
    W = H = 64
    ex = scenes.cornell_box(W, H, 4, device_id=0)
    ex.integrator = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode="albedo", seed=3)
    ex.build_scene(); ex.frame_camera(0.8)
    ex.integrator.render()
    new = wobble(positions_of(ex), amount=0.02)
    ex.scene.update_vertices(new)
    fr = fresh_example(ex, new, W, H, integrator=lambda *a: Debug.Debug(*a, mode="albedo", seed=3))
    ex.frame_camera(0.8); fr.frame_camera(0.8)
    for mode in sorted(Debug.MODES):
        for e in (ex, fr):
            e.integrator.mode = mode
            e.integrator.render()
        assert same(ex.integrator.hdr.to_numpy(), fr.integrator.hdr.to_numpy()), mode


def test_bdpt_film_after_update(gpu_ctx_ok):
    W = H = 40
    frames = 3
    ex = scenes.cornell_box(W, H, 4, device_id=0)
    ex.integrator = BDPT_RGB.BDPT(W, H, ex.cam, ex.scene, 64)
    ex.build_scene()
    ex.integrator.render_frames(2)                          # BDPT state of the old geometry
    new = wobble(positions_of(ex), amount=0.02)
    ex.scene.update_vertices(new)
    ex.frame_camera(0.8)
    fr = fresh_example(ex, new, W, H)
    fr.frame_camera(0.8)
    films = []
    for e in (ex, fr):
        e.scene.ctx.film_clear()                            # (the film, BDPT's per-pixel memory included, is the caller's to clear)
        e.scene.ctx.bdpt_rgb_render(0, frames, 1)
        films.append(e.scene.ctx.film_download(W, H)[0])
    o = oa.OracleScene(ex.scene, ex.cam); o.lbvh_build()
    want, _, _ = o.bdpt_render(ex.cam, W, H, 0, frames, seed=1)
    r_dev, r_orc = rel_l2(films[0], films[1]), rel_l2(films[0], want)
    print("BDPT after update: rel-L2 to fresh %.3e, to the oracle %.3e" % (r_dev, r_orc))
    assert np.isfinite(films[0]).all()
    assert r_dev <= BDPT_DEVICE_TOL
    assert r_orc <= BDPT_ORACLE_TOL


# ---- (d) candidate lists -----------------------------------------------------------------------------------------------------------------
def test_candidate_lists_are_made_again(gpu_ctx_ok):
    W = H = 64
    films, stats = {}, {}
    new = None
    for beams in (1, 0):
        ex = scenes.cornell_box(W, H, 64, device_id=0)
        ex.build_scene()
        ctx = ex.scene.ctx
        frames = 16
        ctx.set_option("primary_beams", beams)
        ctx.set_option("primary_beams_min_frames", frames)
        render_pt(ex, frames)
        ctx.sync()
        if beams:
            assert ctx.primary_beam_stats()["list_builds"] >= 1, "the first render made no lists: the test would show nothing"
        new = wobble(positions_of(ex), amount=0.02)
        ex.scene.update_vertices(new)
        ctx.stats_reset()
        films[beams] = render_pt(ex, frames)
        stats[beams] = ctx.primary_beam_stats()
        last = ex
    print(stats[1])
    assert stats[1]["list_builds"] >= 1 and stats[1]["rays"] == 16 * W * H, "no new candidate lists after the update"
    assert same(films[1], films[0])
    fr = fresh_example(last, new, W, H)
    fr.scene.ctx.set_option("primary_beams_min_frames", 16)
    assert same(films[1], render_pt(fr, 16))


# ---- (e) torch route ---------------------------------------------------------------------------------------------------------------------
def test_torch_route_on_a_side_stream(gpu_ctx_ok):
    import torch
    from ti_raytrace_amd import RayQuery
    dev = torch.device("cuda", 0)
    exs = [built("headline_100k")[0] for _ in range(2)]
    W = 64
    new = wobble(positions_of(exs[0]))
    exs[0].scene.update_vertices(new)                       # the numpy route
    k = new.shape[0]
    perm = np.random.RandomState(3).permutation(k)
    shuffled = torch.from_numpy(new[perm]).to(dev)
    back = torch.from_numpy(np.argsort(perm)).to(dev)
    rays_np = oa.camera_rays(exs[0].cam, W, W)
    rays = torch.from_numpy(rays_np).to(dev)
    big = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for _ in range(20):
            big = big @ big * 1.0e-3                        # work in front of the kernel that makes the positions
        buf = torch.zeros((k, 8), dtype=torch.float32, device=dev)
        buf[:, :3] = shuffled[back]                         # the positions: a gather kernel on the side stream, not synchronised
        view = buf[:, :3]
        assert view.stride(0) == 8
        exs[1].scene.update_vertices(view)
        hits = RayQuery(exs[1].scene).closest(rays, attributes=True)
    side.synchronize()
    assert_same_state(exs[1], exs[0], "torch against numpy")
    fr = fresh_example(exs[0], new, W, W)
    want, wprim, _ = fr.scene.ctx.trace_closest(rays_np, 64, 0)
    assert np.array_equal(hits.prim.cpu().numpy(), wprim)
    assert same(hits.record.cpu().numpy(), want)
    assert 0.05 < (wprim >= 0).mean()
    # [k/3, 3, 3] tensors and explicit normals
    nrm = torch.nn.functional.normalize(torch.randn(k, 3, device=dev), dim=1)
    exs[1].scene.update_vertices(shuffled[back].reshape(-1, 3, 3), normals=nrm.reshape(-1, 3, 3))
    exs[0].scene.update_vertices(new, normals=nrm.cpu().numpy())
    assert_same_state(exs[1], exs[0], "normals given")
    assert same(exs[0].scene.ctx.vertex_download(k)[:, 3:6], nrm.cpu().numpy())


# ---- (f) partial range -------------------------------------------------------------------------------------------------------------------
def test_partial_range_and_two_updates(gpu_ctx_ok):
    """(the scene that is updated is itself built from float32 positions: scenes.synthetic makes its face normals from float64 positions, which
    a fresh scene from vertex_np's float32 ones cannot reproduce for the triangles that are NOT moved)"""
    ex0, W = built("tiny")
    pos = positions_of(ex0)
    ex = fresh_example(ex0, pos, W, W)
    new = wobble(pos, seed=4)
    a, b = 3 * 40, 3 * 170                                  # triangles 40 .. 169
    part = pos.copy(); part[a:b] = new[a:b]
    junk = wobble(pos, seed=9, amount=0.5)
    ex.scene.update_vertices(junk[a:b], first_vertex=a)     # two updates in a row: the second one decides
    ex.scene.update_vertices(new[a:b], first_vertex=a)
    assert_same_state(ex, fresh_example(ex, part, W, W), "partial")
    ex.scene.update_vertices(new[:0])                       # nothing
    ex.scene.update_vertices(new[b:], first_vertex=b)
    ex.scene.update_vertices(new[:a])
    assert_same_state(ex, fresh_example(ex, new, W, W), "in three parts")


# ---- (g) refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_old_build_answering(gpu_ctx_ok):
    import torch
    dev = torch.device("cuda", 0)
    ex, W = built("tiny")
    ctx, sc = ex.scene.ctx, ex.scene
    nv = sc.vertex_count
    rays = oa.camera_rays(ex.cam, W, W)
    before, bprim, _ = ctx.trace_closest(rays, 64, 0)
    vbefore = ctx.vertex_download(nv)
    box_before = np.concatenate(ctx.scene_box())
    good = wobble(positions_of(ex), seed=8)
    good_t = torch.from_numpy(good).to(dev)
    nrm_t = torch.zeros((nv, 3), dtype=torch.float32, device=dev)

    def unchanged(what):
        after, aprim, _ = ctx.trace_closest(rays, 64, 0)     # needs the old build: "LBVH not built" if it was dropped
        assert np.array_equal(aprim, bprim) and same(after, before), what
        assert same(ctx.vertex_download(nv), vbefore) and same(np.concatenate(ctx.scene_box()), box_before), what

    for name, value in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        bad = good.copy(); bad[nv - 2, 1] = value
        for route in ("host", "device"):
            with pytest.raises(_native.TirtError, match="NaN or infinite"):
                if route == "host":
                    ctx.vertex_update(0, nv, bad.ctypes.data, 3)
                else:
                    bad_t = torch.from_numpy(bad).to(dev)
                    ctx.vertex_update(0, nv, bad_t.data_ptr(), 3, device=True, stream=torch.cuda.current_stream(dev).cuda_stream)
            unchanged((name, route))
    cases = {
        "past the end": lambda: ctx.vertex_update(3, nv, good.ctypes.data, 3),
        "first past the end": lambda: ctx.vertex_update(nv + 3, 3, good.ctypes.data, 3),
        "negative first": lambda: ctx.vertex_update(-3, 3, good.ctypes.data, 3),
        "count not whole triangles": lambda: ctx.vertex_update(0, 4, good.ctypes.data, 3),
        "first not whole triangles": lambda: ctx.vertex_update(1, 3, good.ctypes.data, 3),
        "stride < 3": lambda: ctx.vertex_update(0, nv, good.ctypes.data, 2),
        "device stride < 3": lambda: ctx.vertex_update(0, nv, good_t.data_ptr(), 2, device=True),
        "normal stride < 3": lambda: ctx.vertex_update(0, nv, good.ctypes.data, 3, good.ctypes.data, 1),
        "null pos": lambda: ctx.vertex_update(0, nv, 0, 3),
        "host pos, device nrm": lambda: ctx.vertex_update(0, nv, good.ctypes.data, 3, nrm_t.data_ptr(), 3),
        "device pos, host nrm": lambda: ctx.vertex_update(0, nv, good_t.data_ptr(), 3, good.ctypes.data, 3, device=True),
        "device pos to the host entry": lambda: ctx.vertex_update(0, nv, good_t.data_ptr(), 3),
        "host pos to the device entry": lambda: ctx.vertex_update(0, nv, good.ctypes.data, 3, device=True),
    }
    for what, call in cases.items():
        with pytest.raises(_native.TirtError):
            call()
        unchanged(what)
    # a capturing stream
    side = torch.cuda.Stream(dev)
    x = torch.zeros(16, device=dev)
    with torch.cuda.stream(side):
        x.add_(1.0)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(_native.TirtError, match="capturing"):
        with torch.cuda.graph(g, stream=side):
            x.add_(1.0)
            sc.update_vertices(good_t)
    torch.cuda.synchronize(dev)
    unchanged("capturing stream")
    # no scene
    empty = _native.Context(0)
    with pytest.raises(_native.TirtError, match="no scene"):
        empty.vertex_update(0, 3, good.ctypes.data, 3)
    empty.close()
    unchanged("no scene in another context")
    # and the context takes a good update afterwards
    sc.update_vertices(good)
    assert_same_state(ex, fresh_example(ex, good, W, W), "after the refusals")


# ---- (h) face normals ----------------------------------------------------------------------------------------------------------------------
def test_face_normals_equal_cal_normal(gpu_ctx_ok):
    """double-precision cross product, sqrt and 1.0 / x on the device against numpy's, rounded to float32 once: bit for bit, NaN bits included"""
    from ti_raytrace_amd import Scene, SceneData as SCD
    ntri = 6000
    ex = tiny_scene(ntri, seed=3, W=16, H=16, device_id=0)
    ex.build_scene()
    r = np.random.RandomState(11)
    tri = (r.normal(size=(ntri, 3, 3)) * 10.0 ** r.uniform(-6, 6, size=(ntri, 1, 1))).astype(np.float32)      # every size of triangle
    tri[0] = np.asarray([[1.0, 2.0, 3.0]] * 3, np.float32)                                                   # zero area: one point
    tri[1] = np.asarray([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [3.0, 3.0, 3.0]], np.float32)                      # zero area: collinear
    tri[2] = np.asarray([[0.0, 0.0, 0.0], [3.0e18, 1.0e-30, 0.0], [1.0e-38, 2.0e18, 7.0e-41]], np.float32)    # huge and tiny edges, a denormal
    tri[3] = np.asarray([[1.0e-40, 0.0, 0.0], [0.0, 1.0e-40, 0.0], [0.0, 0.0, 1.0e-40]], np.float32)          # denormal edges
    tri[4] = np.asarray([[-0.0, 0.0, -0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, 0.0]], np.float32)                   # signed zeros
    pos = tri.reshape(-1, 3)
    rows = np.zeros((3 * ntri, SCD.VER_VEC_SIZE), np.float64)
    rows[:, 0:3] = pos
    with np.errstate(all="ignore"):
        Scene.Scene.cal_normal(None, rows)
    want = rows.astype(np.float32)[:, 3:6]
    assert np.isnan(want[0:6]).all() and not np.isnan(want[6:9]).any()
    ex.scene.update_vertices(pos)
    got = ex.scene.ctx.vertex_download(3 * ntri)
    assert same(got[:, 0:3], pos)
    bad = (got[:, 3:6].view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5], got[bad][:3, 3:6], want[bad][:3])
    assert same_bits(got[:, 3:6], want, nan_payload=True)
    assert same(ex.scene.vertex_np, got)                    # the lazy host mirror


# ---- (i) process_normal, analytic spheres, a sphere light --------------------------------------------------------------------------------------
def test_smooth_normals_and_spheres(gpu_ctx_ok):
    W = H = 32
    ex = spectral_style_cornell(W, H)
    new = wobble(positions_of(ex), amount=0.02)
    before = ex.scene.ctx.vertex_download(ex.scene.vertex_count)
    ex.scene.update_vertices(new)
    fr = fresh_example(ex, new, W, H)
    assert fr.scene.normals_processed and not same(fr.scene.vertex.to_numpy()[:, 3:6], fr.scene.vertex_np[:, 3:6])     # smoothing did something
    assert not same(before, ex.scene.vertex.to_numpy())
    assert_same_state(ex, fr, "cornell, process_normal")

    ex = tiny_scene(500, seed=2, W=W, H=H, device_id=0)    # triangles + the sphere light of scenes.synthetic
    sph = ex.scene.shape_cpu[0]
    ex.add_sphere_light(pos=(0.4, -2.5, 0.3), radius=0.5, emission=5.0)
    ex.build_scene()
    ex.scene.process_normal()
    assert ex.scene.shape_count == 2 and ex.scene.light_count == 2 and ex.scene._area_called
    new = (wobble(positions_of(ex)) * np.float32(0.5)).astype(np.float32)      # the mesh shrinks away from the spheres
    ex.scene.update_vertices(new)
    assert_same_state(ex, fresh_example(ex, new, W, H), "spheres")
    lo, hi = ex.scene.ctx.scene_box()
    assert same(lo, new.min(axis=0)) and same(hi, new.max(axis=0))            # the triangles' box alone
    assert hi[1] < sph.pos[1] - 1.0                                           # the sphere light is far outside it
    got = render_pt(ex, 2)
    assert same(got, render_pt(fresh_example(ex, new, W, H), 2))


def test_partial_updates_of_a_smoothed_scene_do_not_smooth_twice(gpu_ctx_ok):
    """process_normal applied, then a range moved, frame after frame: the rows that are not moved must not be smoothed a second time.  State and
    the vertex_np mirror (the rows BEFORE smoothing) equal a fresh scene's after every step.  (The updated scene is itself built from float32
    positions, as in test_partial_range_and_two_updates.)"""
    W = H = 32
    ex0 = spectral_style_cornell(W, H)
    pos = positions_of(ex0)
    ex = fresh_example(ex0, pos, W, H)
    assert ex.scene.normals_processed and ex.scene._area_called
    nv = ex.scene.vertex_count
    a, b = 3 * 4, 3 * 20
    cur = pos.copy()
    for step in range(3):
        new = wobble(cur, seed=20 + step, amount=0.01)
        cur[a:b] = new[a:b]
        ex.scene.update_vertices(new[a:b], first_vertex=a)
        fr = fresh_example(ex, cur, W, H)
        assert not same(fr.scene.vertex.to_numpy()[:, 3:6], fr.scene.vertex_np[:, 3:6])       # smoothing does something here
        assert same(ex.scene.vertex_np, fr.scene.vertex_np), step
        assert_same_state(ex, fr, "smoothed, partial, step %d" % step)
    # the torch route and given normals, at the end of the array
    import torch
    dev = torch.device("cuda", 0)
    new = wobble(cur, seed=30, amount=0.01)
    nrm = np.random.RandomState(31).normal(size=(nv - b, 3)).astype(np.float32)
    cur[b:] = new[b:]
    ex.scene.update_vertices(torch.from_numpy(new[b:]).to(dev), normals=torch.from_numpy(nrm).to(dev), first_vertex=b)
    assert same(ex.scene.vertex_np[b:, 3:6], nrm) and same(ex.scene.vertex_np[:b], fr.scene.vertex_np[:b])
    want = fr.scene.vertex_np.copy(); want[b:, 0:3] = new[b:]; want[b:, 3:6] = nrm
    assert same(ex.scene.vertex_np, want)
    # a fresh scene holding those rows before its process_normal: the existing upload route
    fr2 = fresh_example(ex, cur, W, H, build=False)
    fr2.scene.setup_data_cpu(); fr2.scene.vertex_np[b:, 3:6] = nrm
    fr2.integrator.setup_data_cpu(); fr2.integrator.setup_data_gpu(); fr2.scene.setup_data_gpu()
    fr2.scene.process_normal(); fr2.scene.total_area()
    assert_same_state(ex, fr2, "smoothed, partial, normals given")
