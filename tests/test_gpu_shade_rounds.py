"""The persistent loop of the shading kernels (csrc/tirt_render.hip: k_shade, k_pvb_cand_shade, k_shade_spec) over MORE than one round.  Their grid is
min(ceil(S / 256), option "shade_grid"), 1024 blocks by default, so a film of the suite's size is one round of every block: the two halves of the double-buffered
per-wave counts and block bases (`it & 1`), a last round with dead waves, a block that appends nothing in a round are reached by the benchmark alone.  Here the option
is 1, 2 and 3: the same paths go through 94, 47 and 32 rounds, and the film, the counters and the list statistics must be what the default grid gives -- byte for
byte, NaN payloads included, device against device -- and what the CPU oracle gives (a NaN equals any NaN there: the oracle's payloads need not be the device's)."""
import numpy as np
import pytest

import oracle_api as oa
from common import same_bits
from test_gpu_primary_fused import DEPTH, FRAMES, SEED, STACK, build, differing, on_and_off, oracle_of, run, synthetic
from ti_raytrace_amd import scenes

pytestmark = pytest.mark.gpu
BLOCK = 256                                          # SH_BLOCK


def rounds(S, g):
    """(rounds of the persistent loop, live lanes of the last one) for S paths on min(ceil(S / BLOCK), g) blocks"""
    grid = min(-(-S // BLOCK), g)
    n = -(-S // (grid * BLOCK))
    return n, S - (n - 1) * grid * BLOCK


def same_as(ctx, W, H, g, ref, render=None):
    """the job at shade_grid = g with primary_fused 1 and 0 (on_and_off compares those two) against the default grid's: film, counters, list statistics, launches"""
    ctx.set_option("shade_grid", g)
    on = on_and_off(ctx, W, H, render)
    assert same_bits(on[0], ref[0], nan_payload=True), (g, differing(on[0], ref[0]))
    assert on[1:] == ref[1:], (g, on[1:], ref[1:])


def against_the_oracle(film, counts, orc, W, H):
    want, ost = orc.render(W, H, 0, FRAMES, seed=SEED)
    assert same_bits(film, want), differing(film, want)
    assert counts[:3] == (ost["rays_closest"], ost["rays_shadow"], ost["paths"])


# 50 x 30: S = 24 000 = 93.75 blocks, P is no multiple of 64 (frame-major paths); 48 x 32: S = 96 blocks, pixel-block-major numbering
@pytest.mark.parametrize("size", [(50, 30), (48, 32)])
def test_cornell_box_in_94_47_and_32_rounds(gpu_ctx_ok, size):
    W, H = size
    S = FRAMES * W * H
    if size == (50, 30):
        assert rounds(S, 1) == (94, 192)             # an even number of rounds, the last with one dead wave
        assert rounds(S, 2) == (47, 448)             # an odd number; the last round's second block has a dead wave
        assert rounds(S, 3) == (32, 192)             # in the last round two of the three blocks have no live lane at all
    else:
        assert [rounds(S, g) for g in (1, 2, 3)] == [(96, 256), (48, 512), (32, 768)]
    ex = build("cornell", W, H, FRAMES, aov=False)
    ctx = ex.scene.ctx
    ref = on_and_off(ctx, W, H)                      # the default grid: one round
    assert ref[2] == S, "the camera rays did not go through the lists"
    against_the_oracle(ref[0], ref[1], oracle_of(ex, "cornell"), W, H)
    for g in (1, 2, 3):
        same_as(ctx, W, H, g, ref)


def test_sphere_light_kernel_on_one_block(gpu_ctx_ok):
    W, H = 50, 30
    ex = synthetic(W, H)
    ex.build_scene()
    ctx = ex.scene.ctx
    ref = on_and_off(ctx, W, H)
    assert ref[2] == FRAMES * W * H
    orc = oa.OracleScene(ex.scene, ex.cam); orc.lbvh_build()
    against_the_oracle(ref[0], ref[1], orc, W, H)
    same_as(ctx, W, H, 1, ref)


def test_generic_kernel_on_one_block(gpu_ctx_ok):
    """Teapot: glass, a lit environment whose misses read-add-write the accumulator at later bounces, NaN pixels; 48 x 40 x 16 = 120 rounds of one block"""
    W, H = 48, 40
    ex = build("teapot", W, H, FRAMES, aov=False)
    assert ex.scene.env_power > 0
    ctx = ex.scene.ctx
    ref = on_and_off(ctx, W, H)
    assert ref[2] == FRAMES * W * H
    against_the_oracle(ref[0], ref[1], oracle_of(ex, "teapot"), W, H)
    same_as(ctx, W, H, 1, ref)


def test_pt_spec_in_four_rounds_and_two(gpu_ctx_ok):
    """the smallest film test_gpu_spectral.py renders: 16 x 16 x 4 frames of the spectral box, S = 4 blocks"""
    W = H = 16
    frames = 4
    assert [rounds(frames * W * H, g) for g in (1, 2)] == [(4, 256), (2, 512)]
    ex = scenes.spectral_box(W, H, frames, device_id=0)
    ex.build_scene()
    ctx = ex.scene.ctx
    render = lambda c: c.pt_spec_render(0, frames, 3, 10, STACK, 0)
    ref = run(ctx, W, H, 0, render)
    assert ref[1][2] == frames * W * H and ref[1][3] > 0 and np.nan_to_num(ref[0], nan=1.0).any()
    for g in (1, 2):
        ctx.set_option("shade_grid", g)
        got = run(ctx, W, H, 0, render)
        assert same_bits(got[0], ref[0], nan_payload=True), (g, differing(got[0], ref[0]))
        assert got[1:] == ref[1:], (g, got[1:], ref[1:])
