"""BDPT_RGB / BDPT_SPEC films of the device held to the oracle PER PIXEL-CHANNEL, within what the order of fp32 additions can explain and no more
(tests/bdpt_bound_expected.py; the cases and the bound itself are held to the oracle in tests/test_bdpt_bound_host.py).

The device and the oracle compute every single contribution from the same tirt_math.h with contraction off; the device adds them to a pixel with float
atomics, some pre-summed pairwise (k_bd_resolve), the oracle one after the other.  So after frame 0 a pixel-channel that got at most two contributions is
the oracle's bit for bit (the zeros included), every other one lies within the rounding bound of the contributions' exact sum -- about 5e-7 of its value --
and so does every later frame's running mean.  A contribution dropped, added twice or sent to a neighbouring pixel, or one MIS weight off by 1e-4, is far
outside that and far inside the rel-L2 <= 1e-3 of tests/test_gpu_bdpt.py (docs/HISTORY.md has the table of mutants)."""
import numpy as np
import pytest

import bdpt_bound_expected as bb
from test_bdpt_bound_host import BY_NAME, CASE_IDS, build, oracle_render

pytestmark = pytest.mark.gpu
ONE_BATCH = 1 << 29


class Device:
    """one case on the device and in the oracle: the contribution record once, any number of renders against it"""

    def __init__(self, name, options=()):
        self.case = c = BY_NAME[name]
        self.ex, self.o = build(c, device_id=0)
        self.ctx = self.ex.scene.ctx
        self.ctx.set_option("bdpt_state_fill", 2)                # vertex arrays poisoned with 0xFF before every batch: nothing may read an unwritten slot
        for k, v in options:
            self.ctx.set_option(k, v)
        self.film, self.ost, _, self.rec = oracle_render(self.o, self.ex, c)
        self.worst = 0.0

    def render(self, frame_begin, frames):
        (self.ctx.bdpt_spec_render if self.case.spec else self.ctx.bdpt_rgb_render)(frame_begin, frames, self.case.seed)

    def check(self, frames, rec=None, what=""):
        c = self.case
        got = self.ctx.film_download(c.W, c.H)[0]
        rec = self.rec if rec is None else rec
        info = bb.assert_film_within(got, rec[rec["frame"] < frames], c.W, c.H, frames, what="%s %s" % (c.name, what))
        self.worst = max(self.worst, info["ratio"])
        return info

    def run(self, mode, rank=0, ranks=1, tile=None, counts=True):
        """a fresh film (and per-pixel BDPT memory), frame 0 alone held to the bits, then all the frames the way `mode` says: "frames" one call per frame, checked
        after each; "call" all in one call, one batch; "batches" all in one call, in batches of two frames"""
        c, ctx = self.case, self.ctx
        rec = self.rec if ranks == 1 else bb.owned_records(self.rec, rank, ranks, tile)
        if ranks > 1:
            ctx.film_create(c.W, c.H, rank, ranks, tile)
        what = "%s rank %d of %d" % (mode, rank, ranks)
        ctx.set_option("bdpt_batch_items", c.W * c.H * 2 if mode == "batches" else ONE_BATCH)
        ctx.set_option("overlap_lanes", 4 if mode == "batches" else 1)
        ctx.film_clear(); ctx.stats_reset()
        self.render(0, 1)
        first = self.check(1, rec, what + ", frame 0")
        if mode == "frames":
            for f in range(1, c.frames):
                self.render(f, 1)
                self.check(f + 1, rec, what + ", frame %d" % f)
        else:
            ctx.film_clear(); ctx.stats_reset()
            self.render(0, c.frames)
            self.check(c.frames, rec, what)
        st = ctx.stats()
        if counts and ranks == 1:
            assert (st["rays_closest"], st["rays_shadow"]) == (self.ost["rays_closest"], self.ost["rays_shadow"]), (c.name, what)
        assert st["stack_overflow"] == 0
        return first, st


@pytest.mark.parametrize("name", CASE_IDS)
def test_device_film_within_the_rounding_bound_of_the_oracles_contributions(gpu_ctx_ok, name):
    d = Device(name, options=(("trace_lds_depth", 12),) if name.startswith("duplicates") else ())
    first, _ = d.run("frames")
    d.run("call")
    print("%s: frame 0 %d pixel-channels exact, %d bounded, %d excluded; largest error / bound on the device %.3f" % (name, first["exact"], first["bounded"], first["excluded"], d.worst))


@pytest.mark.parametrize("name", ["cornell_24x20", "veach_24x20"])
def test_batches_bounded_rays_and_tiles_stay_within_the_bound(gpu_ctx_ok, name):
    c = BY_NAME[name]
    d = Device(name)
    d.run("batches")
    d.ctx.set_option("bdpt_bounded", 0)            # connection rays as full closest-hit queries
    d.run("call")
    d.ctx.set_option("bdpt_bounded", 1)
    counts = [0, 0]
    for mode in ("frames", "batches"):
        for rank in range(2):                      # each rank's full-size film against the contributions its own pixels make
            _, st = d.run(mode, rank=rank, ranks=2, tile=64)
            if mode == "batches":
                counts[0] += st["rays_closest"]; counts[1] += st["rays_shadow"]
    assert tuple(counts) == (d.ost["rays_closest"], d.ost["rays_shadow"]), "the two ranks' rays do not add up to the oracle's"
    print("%s: largest error / bound on the device %.3f" % (name, d.worst))
