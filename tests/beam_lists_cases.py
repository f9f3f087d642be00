"""The named cases of the candidate-list tests (tests/test_beam_lists_host.py on the CPU, tests/test_gpu_beam_lists.py on the device): scene, film, camera
distance (Example.frame_camera), tiles and -- Teapot only -- the window of pixels that is tested.  Each is the smallest that still reaches its rule:

  cornell_16x12 / _13x7 / _1x1   few large leaves; P = 91: a ragged last wave of k_pvb_beam; one pixel that sees the whole box
  cornell_inside                 the eye inside the scene: entries with nr == 0
  soup_0.8 / soup_4              400 triangles: k_trace's margin grows with the eye's distance (frame_camera 4.0: 6.9 extents along the view axis)
  soup_7 / soup_far              frame_camera 7.0 and 40.0: 12 and 69 extents along the view axis, beyond TR_FAR_RHO = 8 -- there are no lists
  slivers                        800 long triangles on a 12 x 8 film: lists overflow, bounds come in
  identical                      200 copies of one triangle: entries evicted among equal nr
  one_triangle / one_sphere      the root is the leaf
  gallery_sphere / spheres_9     analytic spheres in padded boxes / in slots that span the grid
  teapot_window                  8 x 8 pixels of a 64 x 48 film: triangles about a pixel wide, the regime of the benchmark
  ranks_tile100 / _tile64 / _tile128   a 16 x 16 film as rank 1 of 3: linear order with a ragged last tile, linear order in whole tiles, 8 x 8 blocks

`sparse`: the two overflow cases are exempt from the condition that 90 % of the sample rays that hit do so within the start of the bound; they must have a pixel
where more than 24 leaves carry a hit instead."""
import numpy as np

import common
from adaptive_expected import local_order
from ti_raytrace_amd import scenes


class CaseSpec:
    def __init__(self, make, W, H, scale=0.8, tiles=(0, 1, 4096), window=None, sparse=False, prefilter=False, lists=True, look_at=None):
        self.make, self.W, self.H, self.scale, self.tiles, self.window, self.sparse, self.prefilter, self.lists = make, W, H, scale, tiles, window, sparse, prefilter, lists
        self.look_at = look_at

    def aim(self, ex):
        """the case's camera: Example.frame_camera(scale), or -- look_at = (target, distance): a scene of analytic shapes alone has no box to frame -- set directly"""
        if self.look_at is None:
            ex.frame_camera(self.scale)
        else:
            ex.cam.scale = float(self.look_at[1])
            ex.cam.set_target(*self.look_at[0])

    def order(self):
        return local_order(self.W, self.H, *self.tiles)

    def tested(self):
        """local pixel indices that are tested: all of the rank's, or those inside the window (i0, j0, w, h)"""
        order = self.order()
        if self.window is None:
            return np.arange(order.shape[0])
        i0, j0, w, h = self.window
        i, j = order // self.H, order % self.H
        return np.flatnonzero((i >= i0) & (i < i0 + w) & (j >= j0) & (j < j0 + h))


def make_cases(spec, sc, cam, compact, geo):
    """the beam_lists_expected.Case objects of a spec: one over all tested pixels, or -- prefilter: scenes of thousands of primitives -- one per 4 x 4 block of
    tested pixels, each over the primitives that are not wholly outside that block's pyramid widened by two pixels (beam_lists_expected.prims_near)"""
    import beam_lists_expected as bl
    order, ks = spec.order(), spec.tested()
    if not spec.prefilter:
        return [bl.Case(sc, cam, spec.H, order, ks, compact, geo)]
    i, j = order[ks] // spec.H, order[ks] % spec.H
    block = (i // 4) * 4096 + j // 4
    c64 = bl.Cam64(cam)
    out = []
    for b in np.unique(block):
        sub = ks[block == b]
        prims = bl.prims_near(c64, spec.H, order[sub], sc.primitive_np, sc.vertex_np, sc.shape_np)
        out.append(bl.Case(sc, cam, spec.H, order, sub, compact, geo, prims=prims))
    return out


def _one_primitive(kind):
    def make(W, H):
        from test_gpu_beams import one_primitive
        return one_primitive(W, H, 4, kind)
    return make


def _identical(W, H):
    tris = common.hostile_triangles("identical", np.random.RandomState(7))[:200]
    return common.custom_scene(tris, W, H, device_id=0)


def _spheres_9(W, H):
    tris = scenes.synthetic_triangles(60, 77, 0.3)
    spheres = [(1.2 * np.cos(0.7 * k), 0.25 * k - 1.0, 1.2 * np.sin(0.7 * k), 0.3) for k in range(9)]
    return common.custom_scene(tris, W, H, device_id=0, spheres=spheres)


_cornell = lambda W, H: scenes.cornell_box(W, H, 4, device_id=0)
_soup = lambda W, H: common.tiny_scene(400, seed=21, W=W, H=H, spread=0.25, device_id=0)

CASES = {
    "cornell_16x12": CaseSpec(_cornell, 16, 12),
    "cornell_13x7": CaseSpec(_cornell, 13, 7),
    "cornell_1x1": CaseSpec(_cornell, 1, 1),
    "cornell_inside": CaseSpec(_cornell, 16, 12, scale=0.05),
    "soup_0.8": CaseSpec(_soup, 16, 12, scale=0.8),
    "soup_4": CaseSpec(_soup, 16, 12, scale=4.0),
    "soup_7": CaseSpec(_soup, 16, 12, scale=7.0, lists=False),
    "soup_far": CaseSpec(_soup, 16, 12, scale=40.0, lists=False),
    "slivers": CaseSpec(lambda W, H: common.tiny_scene(800, seed=11, W=W, H=H, spread=0.9, device_id=0), 12, 8, sparse=True),
    "identical": CaseSpec(_identical, 8, 8, sparse=True),
    "one_triangle": CaseSpec(_one_primitive("tri"), 8, 8),
    "one_sphere": CaseSpec(_one_primitive("sphere"), 8, 8, look_at=((0.1, 0.2, -0.1), 3.0)),
    "gallery_sphere": CaseSpec(lambda W, H: scenes.gallery_sphere(W, H, 4, device_id=0), 12, 8, scale=1.0),
    "spheres_9": CaseSpec(_spheres_9, 12, 8),
    "teapot_window": CaseSpec(lambda W, H: scenes.single_model(W, H, 4, device_id=0), 64, 48, window=(28, 20, 8, 8), prefilter=True),
    "ranks_tile100": CaseSpec(_cornell, 16, 16, tiles=(1, 3, 100)),
    "ranks_tile64": CaseSpec(_cornell, 16, 16, tiles=(1, 3, 64)),
    "ranks_tile128": CaseSpec(_cornell, 16, 16, tiles=(1, 3, 128)),
}
