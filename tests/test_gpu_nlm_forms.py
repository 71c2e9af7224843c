"""Every NLM kernel form (csrc/nlm.hip: k_nlm_strip and k_nlm, patch sides 3 / 5 / 7, float64 and float32, their per-problem
`PP` twins, the fixed_h branch, the sse partial sums) against the float64 NumPy reference of tests/nlm_ref.py, on small and
awkward images: ragged tiles, exactly one tile, an image lower than the search radius, the smallest image a patch side takes
(where the LDS tile has its largest side), batches of 1 and 6.

float64 is bit-exact.  float32 is compared with the same float64 reference, evaluated with the float32-rounded h on the same
image (the images lie on the 2^-16 grid: exact in float32): pixels the reference marks `near_cut` -- a running distance within
1e-3 of the cut at one of the row tests, where `dist > 5` may fall on the other side in float32 -- are left out (at most 2 % of
a case, asserted), every other pixel is within 2e-4, the project's float32 NLM bound (tests/test_gpu_nlm.py).  The left-out
pixels are measured too: one flipped candidate moves them by at most exp(-5) of the image's value range."""
import numpy as np
import pytest
import torch

import nlm_ref as R

pytestmark = pytest.mark.gpu

F32_TOL = 2e-4
DT = {'f64': torch.float64, 'f32': torch.float32}


def dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda', dtype)


def xrec_of(z):
    """Something to take the squared error against: the images shifted by one column, fixed."""
    return np.ascontiguousarray(np.roll(z, 1, axis=-1))


def check_image(out, ref, f32_case, what, z):
    """out: one image from the kernel (NumPy); ref: `R.reference(...)` of the same image z."""
    img, near, _ = ref
    if not f32_case:
        np.testing.assert_array_equal(out, img, err_msg=what)
        return
    share = near.mean()
    err = np.abs(out.astype(np.float64) - img)
    kept = float(err[~near].max())
    left_out = float(err[near].max()) if near.any() else 0.0
    print(f'NLM f32 {what}: max |out - ref| = {kept:.3e} outside near_cut, {left_out:.3e} inside; share left out {share:.4f}')
    assert share <= R.NEAR_CUT_CAP, what
    assert kept <= F32_TOL, what
    assert left_out <= np.exp(-5.0) * (z.max() - z.min()), what          # one flipped candidate: exp(-5) of a pixel difference


def check_sse(sse, xrec, out):
    """sse[b] = sum (xrec - out)^2 taken in double from the kernel's own (rounded) output; xrec is exact in float32."""
    assert np.array_equal(xrec.astype(np.float32).astype(np.float64), xrec)
    want = ((xrec - out.astype(np.float64)) ** 2).reshape(out.shape[0], -1).sum(1)
    np.testing.assert_allclose(sse.cpu().numpy(), want, rtol=1e-12)


def _ids(c):
    return f'{c[0]}x{c[1]}-s{c[2]}-d{c[3]}'


@pytest.mark.parametrize('hi', [0, 1])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('case', R.CASES, ids=_ids)
def test_every_form_alone_and_in_a_batch(case, dt, hi):
    """h = sigma: one image (patch 5, radius 5: the strip form) and a batch of 6 (there the LDS form in float64, the strip form
    in float32), both with the squared error; image 0 against the reference, every image of the batch against its own run
    alone (made without xrec: the launch without partial sums)."""
    from pnp_svrg_amd import ops
    H, W, s, d = case
    f32_case = dt == 'f32'
    dtype = DT[dt]
    h = (R.H_F32 if f32_case else R.H_F64)[hi]
    ref = R.reference(H, W, s, d, R.h_of(h, f32_case))
    z = R.images(H, W)
    xr = xrec_of(z)
    zd, xd = dev(z, dtype), dev(xr, dtype)
    sig = torch.full((6,), h, dtype=dtype, device='cuda')
    one, sse1 = ops.nlm2d(zd[:1], sigma_in=sig[:1], patch_size=s, patch_distance=d, xrec=xd[:1])
    six, sse6 = ops.nlm2d(zd, sigma_in=sig, patch_size=s, patch_distance=d, xrec=xd)
    check_image(one[0].cpu().numpy(), ref, f32_case, f'{_ids(case)} h={h} B=1', z[0])
    check_image(six[0].cpu().numpy(), ref, f32_case, f'{_ids(case)} h={h} B=6', z[0])
    check_sse(sse1, xr[:1], one.cpu().numpy())
    check_sse(sse6, xr, six.cpu().numpy())
    for b in range(1, 6):
        alone, none = ops.nlm2d(zd[b:b + 1], sigma_in=sig[b:b + 1], patch_size=s, patch_distance=d)
        assert none is None
        assert torch.equal(six[b], alone[0]), b


@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('case', R.FIXED_H_CASES, ids=_ids)
def test_fixed_h(case, dt):
    """No sigma_in: h = fixed_h, var = 0, on the strip form (patch 5, radius 5) and the LDS form (patch 3, radius 8)."""
    from pnp_svrg_amd import ops
    H, W, s, d = case
    f32_case = dt == 'f32'
    ref = R.reference(H, W, s, d, R.h_of(R.FIXED_H, f32_case), fixed=True)
    z = R.images(H, W)
    xr = xrec_of(z)
    zd, xd = dev(z, DT[dt]), dev(xr, DT[dt])
    one, sse1 = ops.nlm2d(zd[:1], fixed_h=R.FIXED_H, patch_size=s, patch_distance=d, xrec=xd[:1])
    six, _ = ops.nlm2d(zd, fixed_h=R.FIXED_H, patch_size=s, patch_distance=d)
    check_image(one[0].cpu().numpy(), ref, f32_case, f'fixed_h {_ids(case)} B=1', z[0])
    check_image(six[0].cpu().numpy(), ref, f32_case, f'fixed_h {_ids(case)} B=6', z[0])
    check_sse(sse1, xr[:1], one.cpu().numpy())


@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('s,d', R.PP_PAIRS)
def test_per_problem_twins(s, d, dt):
    """pnp_nlm2d_pp, three images with three modifiers: image b against the reference at h = (T)(sigma_b * m_b), and equal to
    the plain call made with its modifier.  Radius 5 with patch 5 is the strip form's twin, everything else k_nlm's."""
    from pnp_svrg_amd import ops
    H, W = R.PP_SHAPE
    f32_case = dt == 'f32'
    dtype = DT[dt]
    z = R.images(H, W)[:3]
    xr = xrec_of(z)
    zd, xd = dev(z, dtype), dev(xr, dtype)
    sig = dev(np.array(R.PP_SIGMA), dtype)
    mod = dev(np.array(R.PP_MODIFIER), torch.float64)
    out, sse = ops.nlm2d(zd, sigma_in=sig, sigma_modifier=mod, patch_size=s, patch_distance=d, xrec=xd)
    o = out.cpu().numpy()
    check_sse(sse, xr, o)
    for b in range(3):
        ref = R.reference(H, W, s, d, R.pp_h(b, f32_case), b=b)
        check_image(o[b], ref, f32_case, f'pp s{s} d{d} b{b}', z[b])
        plain, _ = ops.nlm2d(zd[b:b + 1], sigma_in=sig[b:b + 1], sigma_modifier=R.PP_MODIFIER[b], patch_size=s, patch_distance=d)
        assert torch.equal(out[b], plain[0]), b


def test_sse_partial_sums_are_indexed_by_image_tile_row_and_tile_column():
    """33 x 16 (three tile rows, one tile column) and 17 x 33 (two by three), batch 6, with a squared error that differs from
    image to image and from tile to tile by orders of magnitude: a partial sum stored under another (b, tile row, tile
    column) lands in another image's total or outside the workspace's used part."""
    from pnp_svrg_amd import ops
    for (H, W) in [(33, 16), (17, 33)]:
        for dt in ('f64', 'f32'):
            z = R.images(H, W)
            scale = 2.0 ** (np.arange(6)[:, None, None] + 3 * (np.arange(H)[None, :, None] // 16) + (np.arange(W)[None, None, :] // 16))
            xr = z + scale / 64.0
            for s, d in [(5, 5), (7, 8)]:
                out, sse = ops.nlm2d(dev(z, DT[dt]), fixed_h=0.2, patch_size=s, patch_distance=d, xrec=dev(xr, DT[dt]))
                check_sse(sse, xr, out.cpu().numpy())


def test_fast_exp_out_of_range_matches_the_reference():
    """A live candidate whose distance is beyond 2^31 / (2^20 / ln 2) ~ 1420: the (int) conversion inside fast_exp is out of
    range; the compiled reference (and the oracle) get INT_MIN, a negative weight.  float64, bit for bit."""
    from pnp_svrg_amd import ops
    o = R.OVERFLOW
    z = R.overflow_image()
    ref, _, live = R.nlm_ref(z, o['h'], o['h'], o['patch_size'], o['patch_distance'])
    assert live > R.FAST_EXP_RANGE
    sig = torch.full((1,), o['h'], dtype=torch.float64, device='cuda')
    out, _ = ops.nlm2d(dev(z[None], torch.float64), sigma_in=sig, patch_size=o['patch_size'], patch_distance=o['patch_distance'])
    np.testing.assert_array_equal(out[0].cpu().numpy(), ref)


def test_smallest_images_are_taken_and_smaller_ones_refused():
    from pnp_svrg_amd import _native, ops
    for s in (3, 5, 7):
        n = s // 2 + 1
        z = R.images(4, 4)[:1, :n, :n]
        out, _ = ops.nlm2d(dev(z, torch.float64), fixed_h=0.2, patch_size=s, patch_distance=8)
        np.testing.assert_array_equal(out[0].cpu().numpy(), R.nlm_ref(z[0], 0.2, 0.0, s, 8)[0])
        with pytest.raises(_native.NativeError, match=f'at least {n} '):
            ops.nlm2d(dev(z[:, :n - 1], torch.float64), fixed_h=0.2, patch_size=s, patch_distance=8)
