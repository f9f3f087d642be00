"""The device round trip every known-answer entry makes (kat_round_trip, csrc/tirt_internal.h): what the helper itself can get wrong, not the
arithmetic of an entry (tests/test_gpu_kat.py and the tests of each feature hold that to the oracle).  The words of an output row beyond those an
entry writes are zero whatever the caller's array held; the words it writes do not depend on either stride; n == 0 touches nothing; an entry that
waits for the renders in flight still does so before its launch.  The HIP-failure paths are not provoked here: they are checked by reading."""
import numpy as np
import pytest

from ti_raytrace_amd import _native, scenes

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEF
BRDF_WIDTHS = {4: (2, 3), 17: (24, 3)}           # which -> (words in, words out) of tirt_kat_brdf: cosine_sample_hemisphere, camera_ray_direction
ROWS = (1, 64, 65, 257)                          # one lane, a full wave, one past it, one past a 256-thread block


@pytest.fixture(scope="module")
def ctx(gpu_ctx_ok):
    c = _native.Context(0)
    yield c
    c.close()


def brdf_rows(which, n):
    r = np.random.RandomState(100 * which + n)
    rows = r.uniform(0.05, 0.95, size=(n, BRDF_WIDTHS[which][0])).astype(np.float32)
    if which == 17:
        rows[:, 20:22] = r.randint(0, 32, size=(n, 2))          # the pixel, whole numbers
    return rows


def raw_brdf(ctx, which, rows, out_stride, n=None):
    """tirt_kat_brdf into an array the caller has poisoned, as 32-bit words"""
    rows = np.ascontiguousarray(rows, np.float32)
    out = np.full((rows.shape[0], out_stride), POISON, np.uint32)
    _native.check(_native.lib().tirt_kat_brdf(ctx.handle, which, rows.reshape(-1), rows.shape[1], out.view(np.float32).reshape(-1), out_stride,
                                              rows.shape[0] if n is None else n))
    return out


def raw_math(ctx, fn, x, n=None):
    x = np.ascontiguousarray(x, np.float32)
    out = np.full(x.shape, POISON, np.uint32)
    _native.check(_native.lib().tirt_kat_math(ctx.handle, fn, x, np.ones_like(x), out.view(np.float32), x.size if n is None else n))
    return out


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("which", sorted(BRDF_WIDTHS))
def test_brdf_padding_is_zero_and_the_row_does_not_depend_on_out_stride(ctx, which, n):
    need = BRDF_WIDTHS[which][1]
    rows = brdf_rows(which, n)
    tight, wide = raw_brdf(ctx, which, rows, need), raw_brdf(ctx, which, rows, need + 3)
    assert tight.shape == (n, need) and wide.shape == (n, need + 3)
    assert np.array_equal(wide[:, :need], tight)
    assert not (tight == POISON).any()
    assert (wide[:, need:] == 0).all(), "padding words that are not 0x00000000 in rows %s" % np.nonzero((wide[:, need:] != 0).any(axis=1))[0][:8]
    assert np.array_equal(ctx.kat_brdf(which, rows, need + 3).view(np.uint32), wide)


@pytest.mark.parametrize("n", ROWS)
def test_brdf_row_does_not_depend_on_in_stride(ctx, n):
    which = 4
    need_in, need_out = BRDF_WIDTHS[which]
    rows = brdf_rows(which, n)
    loose = np.full((n, need_in + 2), POISON, np.uint32).view(np.float32)          # garbage in the words no row reads
    loose[:, :need_in] = rows
    assert np.array_equal(raw_brdf(ctx, which, loose, need_out), raw_brdf(ctx, which, rows, need_out))


@pytest.mark.parametrize("n", (1, 257))
def test_math_twice(ctx, n):
    x = np.random.RandomState(n).uniform(-3.0, 3.0, size=n).astype(np.float32)
    a, b = raw_math(ctx, 0, x), raw_math(ctx, 0, x)
    assert np.array_equal(a, b)
    assert not (a == POISON).any()                 # (every word was written: no sine has these bits)
    assert np.array_equal(ctx.kat_math(0, x).view(np.uint32), a)


def test_no_rows_touch_nothing(ctx):
    assert (raw_brdf(ctx, 4, brdf_rows(4, 3), 3 + 3, n=0) == POISON).all()
    assert (raw_math(ctx, 0, np.float32([0.5, 1.5, 2.5]), n=0) == POISON).all()


def test_shade_tables_wait_for_a_pending_render(gpu_ctx_ok):
    """which 0 on the Cornell box (the smallest scene of tests/test_gpu_shade_tables.py): the same (n, 4) words with a render call still pending as without"""
    ex = scenes.cornell_box(32, 32, 4, device_id=0)
    ex.build_scene()
    sc = ex.scene
    n = sc.primitive_count
    idle = sc.ctx.kat_shade_tables(0, n)
    assert idle.shape == (n, 4) and idle.any()
    ex.integrator.render_frames(2)                 # deferred: submitted by the next entry point
    busy = sc.ctx.kat_shade_tables(0, n)
    assert np.array_equal(busy.view(np.uint32), idle.view(np.uint32))
    sc.ctx.sync()
    assert np.array_equal(sc.ctx.kat_shade_tables(0, n).view(np.uint32), idle.view(np.uint32))
