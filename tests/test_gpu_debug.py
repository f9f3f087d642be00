"""The Debug integrator on the device (csrc/tirt_debug.hip through tirt_debug_render and ti_raytrace_amd.Debug): bit for bit against the
reference's own source text (tests/golden/refkat_debug.npz) and against the view the oracle composes (tests/debug_views.py) at user
sizes; both traversal orders; the multi-GPU tiling; no interference with PT_RGB on the same context; ray counts; the Example harness."""
import os

import numpy as np
import pytest

import oracle_api as oa
import debug_views as dv

pytestmark = pytest.mark.gpu
GD = np.load(os.path.join(os.path.dirname(__file__), "golden", "refkat_debug.npz"))


def make(kind, W, H, mode="albedo", seed=1, **kw):
    """an example with a Debug integrator, built on device 0, and its oracle scene"""
    from common import cornell_glass_wall
    from ti_raytrace_amd import Debug, scenes
    if kind == "cornell":
        ex = scenes.cornell_box(W, H, 4, device_id=0)
    elif kind == "cornell_glass":
        ex = cornell_glass_wall(W, H, device_id=0)
    elif kind == "sphere":
        ex = scenes.single_model(W, H, 4, model="sphere.obj", device_id=0)
    elif kind == "teapot":
        ex = scenes.single_model(W, H, 4, device_id=0)
    else:
        ex = scenes.synthetic(W, H, 4, device_id=0)
    ex.integrator = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode=mode, seed=seed, **kw)
    ex.build_scene()
    orc = oa.OracleScene(ex.scene, ex.cam)
    orc.lbvh_build()
    if kind in ("sphere", "teapot"):
        orc.process_normal(ex.scene.vertex_index_np)
    return ex, orc


def render(ex, mode, frame, flags=None):
    d = ex.integrator
    d.mode = mode
    if flags is not None:
        d.flags = flags
    ex.cam.frame = frame; ex.cam.frame_cpu[0] = frame
    d.render()
    return d.hdr.to_numpy()


def check(got, want, what):
    assert dv.same_bits(got, want), (what, int(((got != want) & ~(np.isnan(got) & np.isnan(want))).any(axis=2).sum()))


@pytest.mark.parametrize("name", ["cornell", "cornell_glass", "sphere"])
def test_device_equals_reference_text(gpu_ctx_ok, name):
    W, H, seed = [int(x) for x in GD["cfg"]]
    ex, _ = make(name, W, H, seed=seed)
    for frame in [int(x) for x in GD["frames"]]:
        for mode in dv.MODES:
            check(render(ex, mode, frame), GD["%s_%s_f%d" % (name, mode, frame)], (name, mode, frame))


@pytest.mark.parametrize("kind,W,modes,frames", [
    ("cornell", 512, dv.MODES, (0, 5)),
    ("teapot", 1024, ("albedo", "normal"), (0,)),
    ("synthetic", 1024, ("albedo", "fnormal"), (0,)),
])
def test_device_equals_oracle_at_user_sizes(gpu_ctx_ok, kind, W, modes, frames):
    ex, orc = make(kind, W, W, seed=3)
    for frame in frames:
        want = dv.views(ex, orc, W, W, frame, 3, modes)
        for mode in modes:
            got = render(ex, mode, frame)
            check(got, want[mode], (kind, mode, frame))
            assert (got != 0).any(axis=2).sum() > W * W // 10
    if kind == "teapot":
        assert np.isnan(want["normal"]).any()             # the Teapot's NaN smooth normals stay NaN, at the same pixels


@pytest.mark.parametrize("kind,W", [("cornell", 512), ("synthetic", 1024)])
def test_exhaustive_equals_ordered(gpu_ctx_ok, kind, W):
    from ti_raytrace_amd import _native
    ex, _ = make(kind, W, W)
    for mode in ("albedo", "fnormal"):
        a = render(ex, mode, 2, flags=_native.TRAVERSE_ORDERED)
        b = render(ex, mode, 2, flags=_native.TRAVERSE_EXHAUSTIVE)
        check(b, a, (kind, mode))


def test_tiles_sum_to_the_whole_view(gpu_ctx_ok):
    W = H = 256
    ts = 8 * H                                            # 8 whole columns: the device walks the tiles in 8 x 8 blocks
    whole, _ = make("cornell", W, H, tile_size=ts)
    want = render(whole, "normal", 1)
    parts = []
    for rank in (0, 1):
        ex, _ = make("cornell", W, H, tile_rank=rank, tile_count=2, tile_size=ts)
        parts.append(render(ex, "normal", 1))
    p = np.arange(W * H).reshape(W, H)
    for rank, film in enumerate(parts):
        mine = (p // ts) % 2 == rank
        assert (film[~mine] == 0).all(), rank
        check(film[mine], want[mine], rank)
    check(parts[0] + parts[1], want, "sum")


def test_does_not_disturb_pt_rgb(gpu_ctx_ok):
    from ti_raytrace_amd import Debug, scenes
    W = H = 64
    only, _ = make("cornell", W, H)
    want_debug = render(only, "fnormal", 3)

    ex = scenes.cornell_box(W, H, 8, device_id=0)
    ex.build_scene()
    ex.integrator.render_frames(8)                        # deferred: submitted by the Debug call below
    d = Debug.Debug(W, H, ex.cam, ex.scene, 64, mode="fnormal")
    ex.cam.frame = 3; ex.cam.frame_cpu[0] = 3
    d.render()
    check(d.hdr.to_numpy(), want_debug, "after PT_RGB")

    ex.scene.ctx.film_clear()
    ex.cam.frame = 0; ex.cam.frame_cpu[0] = 0
    ex.integrator.render_frames(4)
    got = ex.integrator.hdr.to_numpy()
    fresh = scenes.cornell_box(W, H, 8, device_id=0)
    fresh.build_scene()
    fresh.integrator.render_frames(4)
    assert np.array_equal(got.view(np.uint32), fresh.integrator.hdr.to_numpy().view(np.uint32))


def test_ray_count_and_queued_frames(gpu_ctx_ok):
    W, H, N = 64, 48, 5
    ex, orc = make("cornell", W, H, mode="gnormal", seed=11)
    ctx = ex.scene.ctx
    before = ctx.stats()["rays_closest"]
    for f in range(N):                                    # no sync in between
        ex.cam.frame = f; ex.cam.frame_cpu[0] = f
        ex.integrator.render()
    got = ex.integrator.hdr.to_numpy()
    assert ctx.stats()["rays_closest"] - before == N * W * H
    check(got, dv.views(ex, orc, W, H, N - 1, 11, ("gnormal",))["gnormal"], "frame N-1")


def test_example_harness_writes_the_tone_mapped_view(gpu_ctx_ok, tmp_path):
    from ti_raytrace_amd import Debug, scenes
    W = H = 32
    ex = scenes.cornell_box(W, H, 3, device_id=0)
    ex.integrator = Debug.Debug(W, H, ex.cam, ex.scene, 64)
    ex.out_path = str(tmp_path / "out.png")
    ex.build_scene()
    while ex.render():
        pass
    assert os.path.getsize(ex.out_path) > 0
    orc = oa.OracleScene(ex.scene, ex.cam)
    orc.lbvh_build()
    view = dv.views(ex, orc, W, H, 2, ex.integrator.seed, ("albedo",))["albedo"]
    check(ex.integrator.hdr.to_numpy(), view, "hdr")
    check(ex.integrator.rgb_film.to_numpy(), orc.tone_map(0.5, view), "rgb_film")
