"""Golden views of the Debug integrator computed by the REFERENCE'S OWN SOURCE TEXT -- build container only (needs the reference tree).

    python tools/refkat/make_refkat_debug.py      # writes tests/golden/refkat_debug.npz

integrator/Debug.py's `render` (:44-67) -- Camera.get_ray_origin / get_ray_direction, Scene.closet_hit, UF.faceforward,
UF.get_prim_mindex, UF.get_material_color -- run through the taichi stand-in of make_refkat.py over a 16 x 16 film, on the scenes of
refkat_render.npz: the Cornell box, the Cornell box with a glass wall, and example/single_model.py's sphere (smooth normals, sphere
light, env map).  Frame 0 (no jitter) and frame 3 (jittered: ti.random() answers with tm_rand(seed, pixel, frame, dim) at the
dimension of its call site, TM_DIM_JX / TM_DIM_JY).

The reference's function writes one of four values on a hit; three of the lines are commented out.  Each view is the SAME function
text, read from the reference file at run time, with one of those lines live:
    albedo    line 65  radiance = UF.get_material_color(scene.material, mat_id)     (live in the reference)
    fnormal   line 62  radiance = (fnormal + 1) * 0.5
    normal    line 63  radiance = (normal  + 1) * 0.5
    gnormal   line 64  radiance = (gnormal + 1) * 0.5
For fnormal / normal / gnormal the script un-comments that line and comments out line 65 in memory; nothing of the reference's text
is written anywhere.  It prints the comparison with the view the oracle composes (tests/debug_views.py), which tests/test_debug_refkat.py
asserts bit for bit."""
import io
import contextlib
import linecache
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_refkat as mk               # noqa: E402  (sets up the stand-in and the reference's import paths)

ti = mk.ti
ROOT, REF = mk.ROOT, mk.REF
LIVE = 65
VIEW_LINE = {"albedo": 65, "fnormal": 62, "normal": 63, "gnormal": 64}
SCENES = ("cornell", "cornell_glass", "sphere")
FRAMES = (0, 3)
W = H = 16
SEED = 7


def debug_module(view):
    """integrator/Debug.py compiled with the line of `view` live (and line 65 commented out for the other views)."""
    path = os.path.join(REF, "integrator", "Debug.py")
    lines = open(path).read().split("\n")
    for ln in VIEW_LINE.values():
        assert "radiance" in lines[ln - 1] and "=" in lines[ln - 1], (ln, lines[ln - 1])
    if view != "albedo":
        k = VIEW_LINE[view] - 1
        assert lines[k].lstrip().startswith("#")
        lines[k] = lines[k].replace("#", "", 1)
        lines[LIVE - 1] = lines[LIVE - 1].replace("radiance", "#radiance", 1)
    # under a name of its own in linecache: the stand-in's decorators recompile each function from inspect.getsource, which must
    # see this text and not the file's
    name = "%s <view %s>" % (path, view)
    text = "\n".join(lines)
    linecache.cache[name] = (len(text), None, [ln + "\n" for ln in lines], name)
    mod = types.ModuleType("Debug_" + view)
    mod.__file__ = name
    exec(compile(text, name, "exec"), mod.__dict__)
    return mod


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import oracle_api as oa
    import debug_views as dv
    L = oa.load()
    mods = {v: debug_module(v) for v in VIEW_LINE}
    out = {"cfg": np.array([W, H, SEED], np.int64), "frames": np.array(FRAMES, np.int64)}
    for name in SCENES:
        ex, sc, orc, rcam, rs = mk.reference_scene(W, H, name)
        # Taichi compiles the camera's Python-scope intrinsics into its f32 kernels as f32 constants; as Python floats the stand-in
        # would evaluate frame 0's unjittered `(u + 0.0 - cx) / fx` (Camera.py:138-139) in float64
        rcam.fx, rcam.fy, rcam.cx, rcam.cy = (np.float32(v) for v in (rcam.fx, rcam.fy, rcam.cx, rcam.cy))
        draws = {}

        def rnd():
            f = sys._getframe(2)                                   # rnd <- ti.random <- Camera.get_ray_direction
            assert f.f_code.co_name == "get_ray_direction", f.f_code.co_name
            if f.f_code not in draws:
                import inspect
                src, first = inspect.getsourcelines(f.f_code)
                draws[f.f_code] = [first + n for n, line in enumerate(src) if "ti.random()" in line and not line.lstrip().startswith("#")]
            dim = draws[f.f_code].index(f.f_lineno)                 # TM_DIM_JX, TM_DIM_JY
            g = f.f_back
            i, j = g.f_locals["i"], g.f_locals["j"]
            return L.orc_kat_rand(SEED, int(i) * H + int(j), int(rcam.frame_gpu[0]), dim)
        ti.set_random(rnd)
        for fr in FRAMES:
            want = dv.views(ex, orc, W, H, fr, SEED)
            for view, mod in mods.items():
                dbg = mod.Debug(W, H, rcam, rs, 64)
                dbg.setup_data_cpu()
                rcam.frame_gpu[0] = fr
                with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                    dbg.render()
                got = dbg.hdr.to_numpy().astype(np.float32)
                key = "%s_%s_f%d" % (name, view, fr)
                out[key] = got
                same = dv.same_bits(got, want[view])
                ident = int(((got.view(np.uint32) == want[view].view(np.uint32)) | (np.isnan(got) & np.isnan(want[view]))).all(axis=2).sum())
                print("%-28s reference text vs oracle composition: bit-identical %s (%d / %d pixels), NaN components %d, hit pixels %d"
                      % (key, same, ident, W * H, int(np.isnan(got).sum()), int((got != 0).any(axis=2).sum())))
    path = os.path.join(ROOT, "tests", "golden", "refkat_debug.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "(%d arrays, %.1f KB)" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
