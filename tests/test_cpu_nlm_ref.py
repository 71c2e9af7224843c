"""The NLM reference helper (tests/nlm_ref.py) and what the float32 kernel tests rest on, without a GPU: the helper equals the
oracle bit for bit; every float32 case of tests/test_gpu_nlm_forms.py meets the two conditions on its input (few pixels
with a running distance near the cut, no live distance in the range where the reference's fast_exp wraps); the constructed
overflow case does leave fast_exp's integer range; and both NLM entry points refuse an image smaller than one reflection
allows, before anything is launched."""
import numpy as np
import pytest

import nlm_ref as R
from oracle import denoise as od


@pytest.mark.parametrize('H,W,s,d,h', [(17, 33, 7, 8, 0.1), (5, 40, 4, 5, 0.05)])
def test_helper_equals_the_oracle_bit_for_bit(H, W, s, d, h):
    z = R.images(H, W)[0]
    np.testing.assert_array_equal(R.nlm_ref(z, h, h, s, d)[0], od.nl_means_2d(z, h, h, patch_size=s, patch_distance=d))
    np.testing.assert_array_equal(R.nlm_ref(z, h, 0.0, s, d)[0], od.nl_means_2d(z, h, 0.0, patch_size=s, patch_distance=d))
    assert R.reference(H, W, R.side_of(s), d, h)[0] is R.reference(H, W, R.side_of(s), d, h)[0]      # computed once


def test_images_are_exact_in_float32_and_the_first_is_the_documented_one():
    z = R.images(17, 33)
    assert z.shape == (6, 17, 33) and z.min() >= 0.0 and z.max() <= 1.0
    np.testing.assert_array_equal(z * 65536.0, np.round(z * 65536.0))
    np.testing.assert_array_equal(z.astype(np.float32).astype(np.float64), z)
    rng = np.random.default_rng(100 * 17 + 33)
    u = rng.random((17, 33))
    box = sum(np.roll(np.roll(u, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) / 9.0
    first = np.clip(np.round((box + 0.05 * rng.standard_normal((17, 33))) * 65536.0) / 65536.0, 0.0, 1.0)
    np.testing.assert_array_equal(z[0], first)


def test_near_cut_marks_a_distance_at_the_cut_and_nothing_else():
    """Two-valued image, patch side 3, radius 1, var = 0: the distance of a candidate across the edge is a known multiple of
    1 / h^2, so h can put it exactly on the cut after the first patch row."""
    z = np.zeros((8, 8))
    z[:, 4:] = 1.0
    s, off = 3, 1
    A = (s - 1.0) / 4.0
    g = np.arange(-off, off + 1)
    w0 = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2 * A * A))
    # pixel (r, 3) against (r, 4): patch columns 2,3,4 against 3,4,5 differ by 1 in the middle column only
    first_row = w0[0, 1] / w0.sum()
    h_on = float(np.sqrt(first_row / R.CUT))                   # first-row distance = 5 (to rounding)
    _, near, live = R.nlm_ref(z, h_on, 0.0, s, 1)
    assert near[:, 3].all() and near[:, 4].all() and not near[:, :2].any() and not near[:, 6:].any()
    _, near, live = R.nlm_ref(z, 2.0 * h_on, 0.0, s, 1)        # first-row distance 1.25, final 5 / 4 / first_row share: far from 5
    assert not near.any()
    # the candidate across the edge is cut there (its middle row brings it to 10.5); the largest distance left is that of a
    # patch pair that differs in its last column
    assert live == pytest.approx(1.0 / (2.0 * h_on) ** 2 * w0[:, 2].sum() / w0.sum(), rel=1e-12)


_F32 = R.f32_reference_cases()


@pytest.mark.parametrize('kw', [c[1] for c in _F32], ids=[c[0] for c in _F32])
def test_f32_case_meets_its_conditions(kw):
    """Conditions on the inputs of the float32 tests, not measurements of a kernel: a case that misses one gets another
    seed; the caps stay."""
    _, near, live = R.reference(**kw)
    assert near.mean() <= R.NEAR_CUT_CAP, near.mean()
    assert live < R.LIVE_DIST_CAP, live


def test_overflow_case_leaves_the_integer_range_of_fast_exp():
    z = R.overflow_image()
    o = R.OVERFLOW
    out, _, live = R.nlm_ref(z, o['h'], o['h'], o['patch_size'], o['patch_distance'])
    assert live > R.FAST_EXP_RANGE
    assert abs(np.trunc(1512775.3951951856938 * -live)) >= 2.0 ** 31
    # the oracle's out-of-range branch: the conversion gives INT_MIN, the high word INT_MIN + 1072632447, a negative weight
    wgt = od.fast_exp(np.array([-live]))
    assert wgt.view(np.int64)[0] == (-2 ** 31 + 1072632447) << 32 and wgt[0] < 0
    with np.errstate(invalid='ignore'):                        # (0 / 0 at the two ends of row 8)
        np.testing.assert_array_equal(out, od.nl_means_2d(z, o['h'], o['h'], o['patch_size'], o['patch_distance']))
    # row 8 is where it happens: the horizontal neighbours weigh -fast_exp(0) each
    assert np.all(out[8, 1:15] == z[8, 1:15]) and not np.isfinite(out[8, 0])


# --------------------------------------------------------------------------
# argument errors of the native entry points (they return before anything is launched)
# --------------------------------------------------------------------------
def _lib():
    from pnp_svrg_amd import _native
    return _native.lib()


def _call(lib, pp, H, W, patch_size):
    a = [16, 32, H, W, 1, 1, patch_size, 5, None, 1.0]
    if pp:
        a.append(16)
    return (lib.pnp_nlm2d_pp if pp else lib.pnp_nlm2d)(*a, 0.1, 16, 1.0, None, None, None, None)


@pytest.mark.parametrize('pp', [False, True])
@pytest.mark.parametrize('H,W,patch_size,least', [(0, 16, 3, 2), (16, 0, 3, 2), (-1, 16, 5, 3), (16, -4, 7, 4),
                                                  (1, 16, 3, 2), (16, 1, 3, 2), (2, 16, 4, 3), (16, 2, 5, 3),
                                                  (3, 16, 7, 4), (16, 3, 7, 4), (3, 16, 6, 4), (2, 2, 7, 4)])
def test_too_small_an_image_is_refused_by_both_entries(pp, H, W, patch_size, least):
    lib = _lib()
    assert _call(lib, pp, H, W, patch_size) != 0
    err = lib.pnp_last_error()
    assert b'nlm2d' in err and f'at least {least} '.encode() in err, err


def test_ops_refuses_it_before_it_allocates():
    import torch
    from pnp_svrg_amd import _native, ops
    for shape, patch_size, least in [((1, 3, 16), 7, 4), ((2, 16, 2), 4, 3), ((1, 1, 1), 3, 2), ((1, 0, 8), 3, 2)]:
        with pytest.raises(_native.NativeError, match=f'pnp_nlm2d: H and W must be at least {least} '):
            ops.nlm2d(torch.zeros(shape, dtype=torch.float64), fixed_h=0.1, patch_size=patch_size)
