"""The float64 Deblur reference of tests/deblur_ref.py pinned on the CPU: its pieces against oracle.problems.Deblur / Bilinear,
the taps and CSR of problems._deblur_taps against its down-sampler as dense matrices, its own adjoint identity, the condition on
its float32 error that the GPU tests' bound rests on, and the table checks of pnp_deblur_plan_create (made before any device
work: this machine needs no GPU for them).

Non-square images with a down-sampler.  The reference's grid binds the outputs of its `meshgrid` in swapped order: rows are
sampled at the points laid over W and columns at those over H.  On 32 x 128 at scale_percent 50 the rows then run to 126 of an
image with 32 of them: oracle.problems.Bilinear refuses it (IndexError from the ravelled index), deblur_ref.down refuses it too
(its 2-D index), and so does problems._deblur_taps (while it builds the CSR), so no plan is ever made of it.  On 128 x 32 the
ravelled index stays inside the image and wraps from one row into the next, which is no bilinear interpolation; deblur_ref.down
refuses that as well.  The grid is
the reference's and is left as it is; non-square images are held to scale_percent == 100 here and in
tests/test_gpu_deblur_forms.py."""
import ctypes
import os

import numpy as np
import pytest

import deblur_ref as dr
from oracle import problems as op

REL = 1e-12
SIZES = [(64, 64), (32, 128)]
SCALES = [100, 50, 75, 2]
GRAD_CASES = [(64, 64, s) for s in SCALES] + [(32, 128, 100)]        # (32 x 128 below 100: test_non_square_grid_is_refused)


def _close(got, ref, rel=REL):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() <= rel * np.abs(ref).max()


def _oracle(H, W, scale, kname):
    """(oracle problem, deblur_ref kernel): 'minimal' is the oracle's own Minimal kernel read off as taps, 'edge' deblur_ref's
    edge kernel put in place of the oracle's B."""
    np.random.seed(0)
    img = np.random.default_rng(5).random((H, W))
    po = op.Deblur(None, H=H, W=W, kernel='Minimal', scale_percent=scale, snr=20., img=img)
    if kname == 'edge':
        kern = dr.kernel('edge', H * W)
        po.B = kern.Bk.copy()
    else:
        nz = np.nonzero(po.B)[0]
        kern = dr.Kernel('minimal', H * W, taps=(nz, po.B[nz]))
        assert len(nz) == 4
    return po, kern


@pytest.mark.parametrize('kname', ['minimal', 'edge'])
@pytest.mark.parametrize('H,W', SIZES)
def test_blur_and_adjoint_blur_equal_fft_blur(H, W, kname):
    N = H * W
    po, kern = _oracle(H, W, 100, kname)
    a = np.random.default_rng(1).normal(size=(2, N))
    for b in range(2):
        ref = po.fft_blur(a[b], po.B)
        assert _close(dr.blur(a[b], kern.taps, N), ref) and _close(dr.blur_dense(a[b], kern.Bk), ref)
        ref = po.fft_blur(a[b], np.roll(np.flip(po.B), 1))
        assert _close(dr.blur_adj(a[b], kern.taps, N), ref) and _close(dr.blur_dense(a[b], dr.adjoint_kernel(kern.Bk)), ref)
    assert _close(dr.blur(a, kern.taps, N)[1], dr.blur(a[1], kern.taps, N), 0)                     # the leading axis is a batch
    dense = dr.kernel('dense', N)
    assert _close(dense.fwd(a[0]), po.fft_blur(a[0], dense.Bk)) and _close(dense.adj(a[0]), po.fft_blur(a[0], np.roll(np.flip(dense.Bk), 1)))


@pytest.mark.parametrize('scale', [50, 75, 2])
def test_down_and_up_equal_oracle_bilinear(scale):
    H = W = 64
    po, _ = _oracle(H, W, scale, 'minimal')
    pts = dr.bilinear_points(H, W, scale)
    assert po.M == dr.n_meas(H, W, scale) == pts[0].shape[0]
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=H * W), rng.normal(size=po.M)
    assert _close(dr.down(x, pts, H, W), po._down(x)) and _close(dr.up(y, pts, H, W), po._up(y))
    assert _close(dr.up(np.stack([y, 2 * y]), pts, H, W)[1], 2 * po._up(y))


@pytest.mark.parametrize('kname', ['minimal', 'edge'])
@pytest.mark.parametrize('H,W,scale', GRAD_CASES)
def test_grad_full_and_grad_stoch_equal_oracle(H, W, scale, kname):
    po, kern = _oracle(H, W, scale, kname)
    pts = dr.bilinear_points(H, W, scale)
    rng = np.random.default_rng(3)
    z = rng.normal(size=H * W)
    po.Y = po.forward_model(rng.normal(size=H * W)) + 0.1 * rng.normal(size=po.M)
    assert _close(dr.forward(z, kern, pts, H, W), po.forward_model(z))
    assert _close(dr.grad(z[None], po.Y[None], None, 1.0 / po.M, kern, pts, H, W)[0], po.grad_full(z))
    mb = dr.selection(po.M, 1)[0]
    assert _close(dr.grad(z[None], po.Y[None], mb[None], 1.0, kern, pts, H, W)[0], po.grad_stoch(z, mb))
    assert abs(dr.objective(z, po.Y, 0.5 / po.M, kern, pts, H, W) - po.f(z)) <= REL * po.f(z)


def test_non_square_grid_is_refused():
    """32 x 128, scale 50 (module docstring): the oracle, the reference and the package's taps all refuse it."""
    from pnp_svrg_amd.problems import _deblur_taps
    H, W = 32, 128
    with pytest.raises(IndexError):
        op.Deblur(None, H=H, W=W, kernel='Minimal', scale_percent=50, img=np.random.default_rng(5).random((H, W)))
    pts = dr.bilinear_points(H, W, 50)
    assert pts[0].shape == (16 * 64,) and pts[0].max() > H
    with pytest.raises(IndexError):
        dr.down(np.zeros(H * W), pts, H, W)
    with pytest.raises(IndexError):
        _deblur_taps(H, W, 50)
    with pytest.raises(IndexError):                              # 128 x 32: the columns leave the image
        dr.down(np.zeros(H * W), dr.bilinear_points(W, H, 50), W, H)


@pytest.mark.parametrize('scale', [50, 75, 2])
def test_deblur_taps_equal_the_reference_matrix(scale):
    """problems._deblur_taps (what the plans upload) as dense M x N matrices, from the taps and from the CSR of the adjoint."""
    from pnp_svrg_amd.problems import _deblur_taps
    H = W = 64
    N, M = H * W, dr.n_meas(H, W, scale)
    ref = dr.down_matrix(dr.bilinear_points(H, W, scale), H, W)
    assert ref.shape == (M, N)
    g_idx, g_w, rp, col, val = _deblur_taps(H, W, scale)
    A = np.zeros((M, N))
    np.add.at(A, (np.repeat(np.arange(M), 4), g_idx.ravel()), g_w.ravel())
    assert np.abs(A - ref).max() <= 1e-15
    assert rp[0] == 0 and rp[N] == 4 * M == len(col) == len(val) and (np.diff(rp) >= 0).all()
    At = np.zeros((M, N))
    np.add.at(At, (col, np.repeat(np.arange(N), np.diff(rp))), val)
    assert np.abs(At - ref).max() <= 1e-15


@pytest.mark.parametrize('kname', ['edge', 'dense'])
@pytest.mark.parametrize('scale', SCALES)
def test_reference_adjoint_identity(scale, kname):
    H = W = 64
    kern, pts = dr.kernel(kname, H * W), dr.bilinear_points(H, W, scale)
    rng = np.random.default_rng(4)
    x, y = rng.normal(size=H * W), rng.normal(size=dr.n_meas(H, W, scale))
    lhs = np.dot(dr.forward(x, kern, pts, H, W), y)
    rhs = np.dot(x, kern.adj(dr.up(y, pts, H, W)))
    assert lhs == pytest.approx(rhs, rel=1e-12)


def test_inputs_are_what_the_gpu_cases_say():
    for N, n in ((4096, 64), (16384, 128), (65536, 256)):
        pos, val = dr.edge_taps(N)
        assert pos.tolist() == [0, 1, n - 1, n, N // 2 + n // 3, N - 1]
        assert len(set(np.abs(val))) == 6 and (val > 0).any() and (val < 0).any()
        B = dr.kernel('edge', N).Bk
        assert not np.array_equal(B, dr.adjoint_kernel(B)) and np.count_nonzero(B) == 6
        assert np.count_nonzero(dr.kernel('dense', N).Bk) == N
        ident = dr.kernel('identity', N)
        assert np.array_equal(ident.fwd(np.arange(N)), np.arange(N))
        im = dr.images(N)
        assert im.shape == (42, N) and [int(np.argmax(r)) for r in im[2:6]] == [0, n - 1, n, N - 1]
        RA = dr.LINE_SPLIT[n][0]
        assert dr.plane_wave_orders(N)[:6] == [0, 1, RA - 1, RA, n // 2, n - 1] and dr.plane_wave_orders(N)[-1] == N - 1
        k = dr.plane_wave_orders(N)[8]
        spec = np.fft.fft(im[6 + 8])
        assert np.abs(spec[k] - N / 2) <= 1e-6 and np.abs(spec[N - k] - N / 2) <= 1e-6


def test_e32_leaves_the_margin():
    """The float32 error of the reference operation itself, for every size, scale and kernel the GPU cases run: below
    F32_CAP / F32_MARGIN, so that the device bound F32_MARGIN * e32 never reaches the cap of the natural-image tests."""
    rows = []
    for H, W, scale, kname in dr.E32_CASES:
        e = dr.e32(H, W, scale, kname)
        rows.append(f'{H:4d} x {W:3d}  scale {scale:3d}  {kname:8s}  e32 = {e:.3e}')
        assert 0 < e < dr.F32_CAP / dr.F32_MARGIN, rows[-1]
        assert dr.f32_bound(H, W, scale, kname) == dr.F32_MARGIN * e
    print('\n'.join(rows))


# ------------------------------------------------------------------------------------------------------------ host table checks
def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def _plan_create(taps, H=64, W=64, M=None):
    g_idx, g_w, rp, col, val = taps
    keep = [np.zeros(H * W), np.ascontiguousarray(g_idx, np.int32), np.ascontiguousarray(g_w, np.float64),
            np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float64)]
    vp = [a.ctypes.data_as(ctypes.c_void_p) for a in keep]
    out = ctypes.c_void_p()
    rc = _lib().pnp_deblur_plan_create(ctypes.byref(out), H, W, 1, 1, vp[0], g_idx.shape[0] if M is None else M, *vp[1:])
    assert out.value is None
    return rc


def test_plan_create_checks_its_tables_without_gpu():
    """PNP_ERR_ARG (1) for one corrupted entry of each table, before any allocation (no GPU here: a device call would fail with
    another code)."""
    from pnp_svrg_amd.problems import _deblur_taps
    h = _lib()
    for what, taps, msg in dr.corrupted_tables(_deblur_taps(64, 64, 50), 4096):
        assert _plan_create(taps) == 1 and msg.encode() in h.pnp_last_error(), what
