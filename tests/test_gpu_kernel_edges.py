"""The small kernels at their dispatch edges, each against a float64 NumPy restatement or the oracle: the TV prox / noise
estimate at every supported H, non-square images and both dispatch forms (split up to 32 images, one workgroup per image
above); the bit-sliced median of the 256-row f32 noise estimate on constructed columns; non-finite inputs; the
phase-retrieval GEMV pair in both load branches and at its selection edges; the CSMRI gradient at the one-kernel batch
boundary and the one-kernel iteration with its start-up stagger on; the elementwise / reduction kernels at lengths around
their block and grid caps.

Tolerances: f64 <= 1e-12 relative to the reference's max, f32 <= 2e-5 absolute on O(1) images (as tests/test_gpu_kernels.py);
a looser bound says why.  Where NaN can appear, NaN positions are compared first, then the finite values."""
import numpy as np
import pytest
import torch
from conftest import golden

from oracle import denoise as od

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x, order='C'))              # (a copy: broadcast views are read-only)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.double().cpu().numpy()


@pytest.fixture(scope='module')
def ops():
    from pnp_svrg_amd import ops as o
    o.require_gpu()
    return o


def assert_close_nan(got, ref, atol):
    """NaN positions equal, infinities equal, finite values within atol."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and not np.isinf(got[~inf]).any()
    fin = np.isfinite(ref)
    if fin.any():
        assert np.abs(got[fin] - ref[fin]).max() <= atol


def images(B, H, W, seed, bits=16):
    """Smoothed noise + noise, on the 2^-bits grid (exact in f32: both dtypes see the same input)."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, H, W))
    p = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode='wrap')
    y = sum(p[:, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    y = y + 0.05 * rng.standard_normal((B, H, W))
    return np.round(y * 2.0 ** bits) / 2.0 ** bits


def tol_img(dtype, ref):
    return 1e-12 * max(1.0, np.nanmax(np.abs(ref))) if dtype == F64 else 2e-5


def tol_sigma(dtype):
    return 1e-12 if dtype == F64 else 3e-5          # relative (test_sigma_est_and_tv)


# ----------------------------------------------------------------------------------------------------------------- A. TV prox
SHAPES = [(16, 16), (16, 48), (32, 256), (64, 64), (128, 32), (128, 128), (256, 112), (256, 256)]


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('H,W', SHAPES)
def test_prox_tv_shapes_and_batch_forms(ops, H, W, dtype):
    """Every mode of pnp_prox_tv / pnp_sigma_est at B = 1, 32 (split form) and 33 (one workgroup per image) against
    oracle.estimate_sigma / haar_bayes_cols; image b of B = 33 == image b run alone, bit for bit."""
    Bmax = 33
    z = images(Bmax, H, W, seed=H * 1000 + W)
    xr = np.clip(z, 0, 1)
    s_ref = np.array([od.estimate_sigma(x) for x in z])
    mod = 1.3
    tv_ref = np.stack([od.haar_bayes_cols(x, s * mod) for x, s in zip(z, s_ref)])
    sig_in = 0.02 + 0.001 * np.arange(Bmax)
    sig_in[::4] = 0.0                                       # the sigma_est <= 0 fallback
    sig_in = sig_in.astype(np.float32).astype(np.float64)
    fb = 0.0625
    given_ref = np.stack([od.haar_bayes_cols(x, s if s > 0 else fb) for x, s in zip(z, sig_in)])
    sse_ref = ((xr - tv_ref) ** 2).reshape(Bmax, -1).sum(1)
    zt_all, xr_all, sig_all = dev(z, dtype), dev(xr, dtype), dev(sig_in, dtype)
    rs, ssr = tol_sigma(dtype), 1e-10 if dtype == F64 else 1e-4
    alone = {}
    for B in (1, 32, 33):
        zt, xrt = zt_all[:B].contiguous(), xr_all[:B].contiguous()
        s = host(ops.sigma_est(zt))
        np.testing.assert_allclose(s, s_ref[:B], rtol=rs)
        out, sse, sig = ops.prox_tv(zt, sigma_modifier=mod, xrec=xrt)
        np.testing.assert_allclose(host(sig), s_ref[:B], rtol=rs)
        assert np.abs(host(out) - tv_ref[:B]).max() <= tol_img(dtype, tv_ref)
        np.testing.assert_allclose(sse.cpu().numpy(), sse_ref[:B], rtol=ssr)
        g, _, gsig = ops.prox_tv(zt, sigma_in=sig_all[:B].contiguous(), fallback_sigma=fb)
        assert np.abs(host(g) - given_ref[:B]).max() <= tol_img(dtype, given_ref)
        assert torch.equal(gsig, sig_all[:B])
        zz = zt.clone()
        ops.prox_tv(zz, sigma_modifier=mod, xrec=xrt, out=zz)                 # in place
        assert torch.equal(zz, out)
        if B == 1:
            alone[0] = (out, sig, sse, g)
            o32 = ops.prox_tv(zt_all[32:].contiguous(), sigma_modifier=mod, xrec=xr_all[32:].contiguous())
            g32 = ops.prox_tv(zt_all[32:].contiguous(), sigma_in=sig_all[32:].contiguous(), fallback_sigma=fb)[0]
            alone[32] = (o32[0], o32[2], o32[1], g32)
        if B == 33:
            for b, (o1, s1, e1, g1) in alone.items():
                assert torch.equal(out[b], o1[0]) and torch.equal(sig[b], s1[0]) and torch.equal(g[b], g1[0])
                assert torch.equal(sse[b], e1[0])


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('tag', ['h16w48', 'h128w32', 'h32w256'])
def test_prox_tv_vs_reference_fixture(ops, tag, dtype):
    """The kernels against the real library's outputs at the shapes of tests/golden/tv_shapes.npz, in both forms."""
    g = golden('tv_shapes.npz')
    z0 = g[f'{tag}_z0']
    s0 = float(g[f'{tag}_sigma_est'])
    for B in (1, 33):
        zt = dev(np.broadcast_to(z0, (B,) + z0.shape), dtype)
        np.testing.assert_allclose(host(ops.sigma_est(zt)), s0, rtol=tol_sigma(dtype))
        for key, kw in (('tv', {}), ('tv_mod', dict(sigma_modifier=1.7)),
                        ('tv_strength', dict(sigma_in=torch.zeros(B, dtype=dtype, device='cuda'), fallback_sigma=0.07 * 0.9))):
            out = host(ops.prox_tv(zt, **kw)[0])
            assert np.abs(out - g[f'{tag}_{key}']).max() <= tol_img(dtype, g[f'{tag}_{key}']), (B, key)


def test_small_batch_prox_on_two_streams(ops):
    """Two streams running a split-form prox (with the error sum: last-workgroup counter) at the same time: each result
    equals the serial result bit for bit (per-stream scratch)."""
    z = images(8, 256, 256, seed=5)
    za, zb = dev(z[:4], F32), dev(z[4:], F32)
    xa, xb = dev(np.clip(z[:4], 0, 1), F32), dev(np.clip(z[4:], 0, 1), F32)
    want_a, want_b = ops.prox_tv(za, xrec=xa), ops.prox_tv(zb, xrec=xb)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    got_a, got_b = [], []
    for _ in range(12):
        with torch.cuda.stream(s1):
            got_a.append(ops.prox_tv(za, xrec=xa))
        with torch.cuda.stream(s2):
            got_b.append(ops.prox_tv(zb, xrec=xb))
    torch.cuda.synchronize()
    for ga, gb in zip(got_a, got_b):
        for u, v in zip(ga, want_a):
            assert torch.equal(u, v)
        for u, v in zip(gb, want_b):
            assert torch.equal(u, v)


# --------------------------------------------------------------------------------------- B. bit-sliced median, 256 x 256 f32
def _extra_median_column(rng, even):
    """A column that is zero except for its last rows, whose masked median involves the bottom chunk's extra (129th)
    db2 coefficient: the median itself (odd count) or one of the two middle values (even count)."""
    for _ in range(20000):
        x = np.zeros(256)
        k = int(rng.integers(6, 14))
        x[256 - k:] = rng.integers(1, 65536, k) / 65536.0
        d = np.abs(od.db2_detail_cols(x[:, None])[:, 0])
        nz = np.flatnonzero(d)
        if len(nz) % 2 != (0 if even else 1) or len(np.unique(d[nz])) != len(nz):
            continue
        order = nz[np.argsort(d[nz])]
        mid = order[(len(nz) - 1) // 2: len(nz) // 2 + 1]
        if 128 in mid:
            return x
    raise AssertionError('no column found')


def db2_detail_cols_f32(img):
    """oracle.db2_detail_cols evaluated in float32 with float32 taps, as the f32 kernel does (no contraction)."""
    x = np.asarray(img, np.float32)
    n = (x.shape[0] + 3) // 2
    xe = np.pad(x, ((3, 3), (0, 0)), mode='symmetric')
    i2 = 2 * np.arange(n) + 3
    h0, h1, h2, h3 = (np.float32(h) for h in od.DB2_DEC_HI)
    return ((h0 * xe[i2 + 1] + h1 * xe[i2]) + h2 * xe[i2 - 1]) + h3 * xe[i2 - 2]


def median_edge_images():
    """[6, 256, 256] on the 2^-16 grid (exact in f32).  Flat parts are 0: a nonzero constant (or a linear ramp, db2 has
    two vanishing moments) gives rounding-noise coefficients whose zero / nonzero class differs between dtypes."""
    rng = np.random.default_rng(2024)
    z = rng.integers(0, 65536, (6, 256, 256)) / 65536.0
    # 0: zero bands of per-column length -> exact-zero coefficients, even and odd nonzero counts
    for c in range(256):
        r0 = int(rng.integers(0, 200))
        z[0, r0:r0 + 1 + (c * 7) % 57, c] = 0.0
    # 1: ties at the median: period-2 / period-4 columns repeat one or two coefficient magnitudes
    for c in range(0, 256, 3):
        p, q = rng.integers(1, 65536, 2) / 65536.0
        z[1, :, c] = np.where(np.arange(256) % 2 == 0, p, q)
        if c % 2:
            z[1, 128:, c] = np.where(np.arange(128) % 4 < 2, p, q)
        z[1, 255, c] = rng.integers(1, 65536) / 65536.0     # rows 254 / 255 equal: a rounding-noise last coefficient
    # 2: medians on the extra coefficient (odd counts) / next to it (even counts)
    for c in range(256):
        z[2, :, c] = _extra_median_column(rng, even=bool(c % 2))
    # 3: more of them, the other parity on odd / even columns
    for c in range(256):
        z[3, :, c] = _extra_median_column(rng, even=not c % 2)
    # 4: a constant (zero) column -> no nonzero coefficient -> NaN, like np.median([])
    z[4, :, 77] = 0.0
    # 5: a NaN pixel in one column
    z[5, 131, 200] = np.nan
    return z


def test_bit_sliced_median_edges(ops):
    """The 256-row f32 noise estimate (bit-plane radix select, 33rd key as a flag) on constructed columns against
    oracle.sigma_cols / estimate_sigma, in both prox forms, in f64, and in the one-kernel CSMRI iteration."""
    z = median_edge_images()
    d = np.abs(od.db2_detail_cols(z[0]))
    cnt = (d != 0).sum(0)
    assert (cnt % 2 == 0).any() and (cnt % 2 == 1).any() and (cnt < 129).sum() > 128
    cols = [od.sigma_cols(x) for x in z]
    assert np.isfinite(cols[0]).all() and np.isfinite(cols[1]).all() and np.isfinite(cols[2]).all()
    assert np.isfinite(cols[3]).all() and np.isnan(cols[4]).sum() == 1 and np.isnan(cols[5]).sum() == 1
    with np.errstate(invalid='ignore'):                       # the zero / nonzero class is the same in f32
        assert all(np.array_equal(od.db2_detail_cols(x) != 0, db2_detail_cols_f32(x) != 0) for x in z[:5])
    ref = np.array([np.mean(c) for c in cols])                # estimate_sigma: NaN if any column is NaN
    fin = np.isfinite(ref)
    for dtype in (F32, F64):
        zt = dev(z, dtype)
        for B in (6, 33):
            zb = zt if B == 6 else torch.cat([zt] * 6)[:33].contiguous()
            s = host(ops.sigma_est(zb))[:6]
            assert np.array_equal(np.isnan(s), ~fin), (dtype, B, s)
            np.testing.assert_allclose(s[fin], ref[fin], rtol=tol_sigma(dtype))
            out, _, sig = ops.prox_tv(zb)
            np.testing.assert_array_equal(host(sig), host(ops.sigma_est(zb)))       # (NaN == NaN here)
            tv_ref = np.stack([od.haar_bayes_cols(x, r if r > 0 else 0.0) for x, r in zip(z, ref)])
            for b in np.flatnonzero(fin):
                assert np.abs(host(out[b]) - tv_ref[b]).max() <= tol_img(dtype, tv_ref[b]), (dtype, B, b)
    # the one-kernel CSMRI iteration with a zero step: its noise estimate is the same median on the same data
    plan = ops.CsmriPlan(256, 256, 6, F32)
    zt = dev(z, F32)
    bits = torch.zeros((6, 256, 8), dtype=torch.int32, device='cuda')
    stepped, _, sig = plan.svrg_step(zt, None, bits, alpha=0.0, beta=1.0, c1=zt, denoise=False)
    s = host(sig)
    assert np.array_equal(np.isnan(s), ~fin)
    np.testing.assert_allclose(s[fin], ref[fin], rtol=tol_sigma(F32))
    assert torch.equal(stepped[:5], zt[:5])                  # (0 * finite gradient + z)


# ------------------------------------------------------------------------------------------------------- C. non-finite input
@pytest.mark.parametrize('dtype', [F64, F32])
def test_minmax_nonfinite(ops, dtype):
    """pnp_minmax == np.min / np.max per image: NaN anywhere gives NaN (first, middle, last element), +-inf kept."""
    n = 4099
    x = np.random.default_rng(7).standard_normal((9, n))
    x[0, 0] = np.nan
    x[1, 2050] = np.nan
    x[2, n - 1] = np.nan
    x[3, 17] = np.inf
    x[4, 300] = -np.inf
    x[5, 1], x[5, n - 2] = np.inf, -np.inf
    x[6, 5], x[6, 6] = np.inf, np.nan
    x[7] = 0.25                                              # constant: max == min
    x = x.astype(np.float32 if dtype == F32 else np.float64)
    mm = host(ops.minmax(dev(x)))
    np.testing.assert_array_equal(mm[:, 0], x.min(1).astype(np.float64))
    np.testing.assert_array_equal(mm[:, 1], x.max(1).astype(np.float64))


@pytest.mark.parametrize('dtype', [F64, F32])
def test_sse_and_psnr_nonfinite(ops, dtype):
    """pnp_sse and the PSNR the engines log (CsmriBatch.psnr_init) with NaN / inf iterates against oracle.psnr."""
    from pnp_svrg_amd.engine import CsmriBatch
    H = 64
    rng = np.random.default_rng(8)
    xrec = rng.random((5, H, H))
    xin = np.clip(xrec + 0.05 * rng.standard_normal((5, H, H)), 0, 1)
    xin[0, 3, 4] = np.nan
    xin[1, 60, 1] = np.inf
    xin[2, 0, 0] = -np.inf
    xin[3] = xrec[3]                                         # zero error: +inf PSNR
    npdt = np.float32 if dtype == F32 else np.float64
    xr32, xi32 = xrec.astype(npdt).astype(np.float64), xin.astype(npdt).astype(np.float64)
    with np.errstate(invalid='ignore'):
        sse_ref = ((xr32 - xi32) ** 2).reshape(5, -1).sum(1)
    got = ops.sse(dev(xi32, dtype), dev(xr32, dtype)).cpu().numpy()
    assert_close_nan(got, sse_ref, 1e-12 * np.nanmax(sse_ref[np.isfinite(sse_ref)]))
    mask = (rng.random((5, H, H)) < 0.3).astype(np.uint8)
    Y = np.fft.fft2(xrec) * mask
    batch = CsmriBatch(xr32, mask, Y, xi32.reshape(5, -1), dtype=dtype)
    with np.errstate(all='ignore'):
        want = np.array([od.psnr(a, b) for a, b in zip(xr32, xi32)])
    assert_close_nan(batch.psnr_init(), want, 0.0)
    assert np.isnan(want[0]) and want[1] == -np.inf and want[2] == -np.inf and want[3] == np.inf


def test_prox_nonfinite_pixels(ops):
    """Noise estimate and TV prox with NaN / +-inf pixels against the oracle (f64: the same products, so the same
    NaN / inf pattern): a NaN column makes the estimate NaN and the prox falls back to the given strength."""
    z = images(6, 64, 64, seed=9)
    z[0, 30, 7] = np.nan
    z[1, 0, 9] = np.inf                                      # row 0: two taps on the same pixel (symmetric edge): inf - inf
    z[2, 33, 40] = -np.inf
    z[3, 63, 63] = np.inf
    z[4, 10, :] = np.nan
    zt = dev(z, F64)
    with np.errstate(all='ignore'):
        s_ref = np.array([od.estimate_sigma(x) for x in z])
    s = host(ops.sigma_est(zt))
    assert_close_nan(s, s_ref, 1e-12)
    fb = 0.05
    with np.errstate(all='ignore'):
        ref = np.stack([od.TVDenoiser(denoise_strength=fb).denoise(x, sigma_est=r) for x, r in zip(z, s_ref)])
    for B in (6, 33):
        zb = zt if B == 6 else torch.cat([zt] * 6)[:33].contiguous()
        out, _, sig = ops.prox_tv(zb, fallback_sigma=fb)
        assert_close_nan(host(sig)[:6], s_ref, 1e-12)
        assert_close_nan(host(out)[:6], ref, 1e-12 * np.nanmax(np.abs(ref[np.isfinite(ref)])))
    # the real library's outputs (tests/golden/tv_shapes.npz)
    g = golden('tv_shapes.npz')
    zt = dev(g['nonfinite_z0'], F64)
    out, _, sig = ops.prox_tv(zt, fallback_sigma=0.05)
    assert_close_nan(host(sig), g['nonfinite_sigma_est'], 1e-12)
    assert_close_nan(host(out), g['nonfinite_tv'], 1e-12)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_dncnn_wrapper_nan_and_constant(ops, dtype):
    """The RealSN_DnCNN wrapper (normalise by min / max, net, undo) on an image with one NaN pixel and on a constant
    image: the reference's np.min / np.max make both all-NaN (NaN min; 0 / 0 normalisation); so must the kernel."""
    wts = dict(golden('dncnn_noise15.npz'))
    z = images(3, 64, 64, seed=10)
    z[0, 20, 33] = np.nan
    z[1] = 0.375
    den = od.DnCNNDenoiser(wts, 15)
    with np.errstate(all='ignore'):
        ref = np.stack([den.denoise(x) for x in z])
    assert np.isnan(ref[0]).all() and np.isnan(ref[1]).all() and np.isfinite(ref[2]).all()
    plan = ops.DncnnPlan(wts, 64, 64, 3)
    out, _ = plan.denoise(dev(z, dtype), 15)
    o = host(out)
    assert np.isnan(o[0]).all() and np.isnan(o[1]).all()
    assert np.abs(o[2] - ref[2]).max() <= 3e-5             # (the finite image: test_denoise_wrapper's bound)


# ---------------------------------------------------------------------------------------------- D. phase-retrieval GEMV pair
def pr_ref(A, w, y, rows, scale):
    """float64 restatement of PR.py:75-87 on the selected rows (NaN where |a.w| = 0, like NumPy)."""
    As = A[rows]
    t = As @ w
    with np.errstate(all='ignore'):
        u = ((np.abs(t) - y[rows]) / np.abs(t)) * t
        return scale * (As.T @ u)


def pr_tol(dtype, ref):
    return (1e-12 if dtype == F64 else 2e-5) * np.abs(ref).max()


def pr_data(M, N, dtype, seed, B=None):
    rng = np.random.default_rng(seed)
    shp = (M, N) if B is None else (B, M, N)
    A = rng.standard_normal(shp)
    w = rng.standard_normal(shp[:-2] + (N,))
    y = np.abs(rng.standard_normal(shp[:-1]))
    if dtype == F32:
        A, w, y = (a.astype(np.float32).astype(np.float64) for a in (A, w, y))
    return A, w, y


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('N', [1024, 1026, 1023])
def test_pr_grad_and_spectral_branches(ops, N, dtype):
    """Vector and scalar load branches of k_pr_rows (N = 1024: both vector; 1026: f32 scalar, f64 vector; 1023: both
    scalar), the gradient and the spectral step, selections of 1, 63, 64, 65 and all rows, and rows = NULL."""
    M = 300
    A, w, y = pr_data(M, N, dtype, seed=N)
    Ad, wd, yd = dev(A, dtype), dev(w, dtype), dev(y, dtype)
    rng = np.random.default_rng(N + 1)
    for nsel in (1, 63, 64, 65, M):
        rows = np.sort(rng.choice(M, nsel, replace=False)).astype(np.int32)
        got = host(ops.pr_grad(Ad, wd, yd, rows=dev(rows), scale=1.0 / nsel))
        ref = pr_ref(A, w, y, rows, 1.0 / nsel)
        assert np.abs(got - ref).max() <= pr_tol(dtype, ref), nsel
    ref = pr_ref(A, w, y, np.arange(M), 1.0 / M)
    got = host(ops.pr_grad(Ad, wd, yd, scale=1.0 / M))
    assert np.abs(got - ref).max() <= pr_tol(dtype, ref)
    ref = A.T @ (y * (A @ w)) / M
    got = host(ops.pr_spectral_apply(Ad, wd, yd, scale=1.0 / M))
    assert np.abs(got - ref).max() <= pr_tol(dtype, ref)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_pr_grad_batch_edges(ops, dtype):
    """pnp_pr_grad_batch with different rows per problem (an unsorted selection included), a row with a.w = 0 exactly
    (NaN propagates to the whole gradient, as in NumPy), and nsel = 0 (out = 0)."""
    from pnp_svrg_amd import _native as Nt
    B, M, N = 3, 200, 1030
    A, w, y = pr_data(M, N, dtype, seed=11, B=B)
    A[2, 5] = 0.0                                           # a.w = 0 exactly for problem 2, row 5
    rng = np.random.default_rng(12)
    for nsel in (1, 63, 64, 65, 150):
        rows = np.stack([rng.choice(M, nsel, replace=False) for _ in range(B)]).astype(np.int32)
        if nsel >= 64:
            rows[2, 0] = 5
        else:
            rows[2] = np.where(rows[2] == 5, (5 + 1) % M, rows[2])
        got = host(ops.pr_grad_batch(dev(A, dtype), dev(w, dtype), dev(y, dtype), rows=dev(rows), scale=0.5))
        for b in range(B):
            ref = pr_ref(A[b], w[b], y[b], rows[b], 0.5)
            if b == 2 and nsel >= 64:
                assert np.isnan(ref).all() and np.isnan(got[b]).all()
            else:
                assert np.abs(got[b] - ref).max() <= pr_tol(dtype, ref), (nsel, b)
    # nsel = 0: an empty selection (rows non-NULL) gives a zero gradient
    Ad, wd, yd = dev(A, dtype), dev(w, dtype), dev(y, dtype)
    rows1 = torch.zeros((B, 1), dtype=torch.int32, device='cuda')
    ws = torch.empty(B * Nt.lib().pnp_pr_workspace_elems(M, N), dtype=dtype, device='cuda')
    out = torch.full((B, N), 7.0, dtype=dtype, device='cuda')
    Nt.call('pnp_pr_grad_batch', ops._p(Ad), ops._p(wd), ops._p(yd), ops._p(rows1), 0, M, N, B, ops._DT[dtype], 1.0,
            ops._p(ws), ops._p(out), ops._stream())
    assert torch.equal(out, torch.zeros_like(out))
    out1 = torch.full((N,), 7.0, dtype=dtype, device='cuda')
    Nt.call('pnp_pr_grad', ops._p(Ad[0]), ops._p(wd[0]), ops._p(yd[0]), ops._p(rows1[0]), 0, M, N, ops._DT[dtype], 1.0,
            ops._p(ws), ops._p(out1), ops._stream())
    assert torch.equal(out1, torch.zeros_like(out1))


def test_pr_grad_reference_size(ops):
    """The reference's 128 x 128, alpha = 0.5 shape: A is 8192 x 16384 (f32 <= 5e-4 relative: 16384-term f32 dot
    products; f64 <= 1e-9 relative)."""
    M, N = 8192, 16384
    rng = np.random.default_rng(13)
    A = rng.standard_normal((M, N), dtype=np.float32)
    w = rng.standard_normal(N)
    y = np.abs(rng.standard_normal(M))
    w32, y32 = w.astype(np.float32), y.astype(np.float32)
    for dtype, wv, yv, tol in ((F32, w32, y32, 5e-4), (F64, w, y, 1e-9)):
        Ad = torch.from_numpy(A).cuda().to(dtype)
        t = np.empty(M)
        for r in range(0, M, 1024):
            t[r:r + 1024] = A[r:r + 1024].astype(np.float64) @ wv.astype(np.float64)
        u = ((np.abs(t) - yv) / np.abs(t)) * t
        ref = np.zeros(N)
        for r in range(0, M, 1024):
            ref += A[r:r + 1024].astype(np.float64).T @ u[r:r + 1024]
        ref /= M
        got = host(ops.pr_grad(Ad, dev(wv, dtype), dev(yv, dtype), scale=1.0 / M))
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), dtype
        del Ad
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- E. CSMRI batch edges
def test_csmri_grad_across_fused_min_batch(ops):
    """The same three problems through plan.grad(bits=...) at B = 191 (streaming kernels) and B = 192 (one-kernel
    gradient) against the masked-FFT gradient in float64 NumPy."""
    from pnp_svrg_amd.engine import CsmriBatch
    b3 = CsmriBatch.synthetic(3, 256, 256, 0.2, 20.0, seed=41)
    xrec = host(b3.xrec)
    mask = b3.mask_np.astype(bool)
    Y = np.swapaxes(b3.YT.cpu().numpy(), 1, 2).astype(np.complex128)
    z = host(b3.xinit)
    inv_m0 = 1.0 / b3.M0
    ref = np.stack([inv_m0[b] * np.real(np.fft.ifft2(mask[b] * np.fft.fft2(z[b]) - mask[b] * Y[b])) for b in range(3)])
    tol = 2e-5 * np.abs(ref).max() * 10                     # f32 FFT pair (test_csmri_grad's bound)
    del xrec
    for B in (191, 192):
        idx = np.arange(B) % 3
        plan = ops.CsmriPlan(256, 256, B, F32)
        bits = b3.bits[idx].contiguous()
        YT = b3.YT[idx].contiguous()
        zt = b3.xinit[idx].contiguous()
        av = b3.inv_m0[idx].contiguous()
        yh = plan.pack_y(YT, plan.sel_from_dense(torch.from_numpy(b3.mask_np[idx]).cuda()))
        g = host(plan.grad(zt, bits=bits, yh=yh, alpha_vec=av))
        assert np.abs(g[:3] - ref).max() <= tol, B
        assert np.abs(g[189:192 if B == 192 else 191] - ref[idx[189:B]]).max() <= tol, B
        del plan


def test_fused_iteration_with_stagger(ops):
    """k_svrg_iter with its start-up stagger on (B = number of CUs + 1): SvrgEngine.step() with the TV prox and a direct
    plan.svrg_step(denoise=False); the first items == the same items at B = 3, bit for bit."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = num_cu + 1
    big = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=43)
    small = CsmriBatch.synthetic(3, 256, 256, 0.2, 20.0, seed=43)
    assert torch.equal(small.bits, big.bits[:3])
    res = []
    for batch in (big, small):
        eng = SvrgEngine(batch, TVProx(), 2e3, 3, 1000, seed=1, fused=True)
        for _ in range(4):                                   # outer refresh folded in, two inner steps, a second refresh
            eng.step()
        res.append((eng.z[:3].clone(), eng.psnr_trace()[:, :3].copy()))
        del eng
    assert torch.equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])
    out = []
    for batch in (big, small):
        p = batch.plan
        selbits = torch.empty((1, batch.B, 256, 8), dtype=torch.int32, device='cuda')
        p.draw_thresholds(batch.bits, 1000, seed=3, step0=2, nsteps=1, selbits=selbits)
        w = (batch.xinit * 0.5).contiguous()
        st, _, sig = p.svrg_step(batch.xinit, w, selbits[0], alpha=-2.0, beta=1.0, c1=batch.xinit, denoise=False)
        out.append((st[:3].clone(), sig[:3].clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    del big, small
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- F. lengths
LENGTHS = [1, 63, 255, 257, 2048 * 256 + 1, 4096 * 256 + 3]


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('n', LENGTHS)
def test_elementwise_and_reductions_lengths(ops, n, dtype):
    """pnp_sse, pnp_minmax (per image, batch 1 and 7), pnp_axpbypcz (with and without y / w; grid capped at 2048 blocks)
    and pnp_saga_table_update (capped at 4096) around the block size and past the caps, against NumPy."""
    npdt = np.float32 if dtype == F32 else np.float64
    rng = np.random.default_rng(n)
    atol = 2e-5 if dtype == F32 else 1e-14
    for B in (1, 7):
        x = rng.standard_normal((B, n)).astype(npdt)
        r = rng.standard_normal((B, n)).astype(npdt)
        xd, rd = dev(x), dev(r)
        sse_ref = ((r.astype(np.float64) - x.astype(np.float64)) ** 2).sum(1)
        np.testing.assert_allclose(ops.sse(xd, rd).cpu().numpy(), sse_ref, rtol=1e-12)
        mm = host(ops.minmax(xd))
        np.testing.assert_array_equal(mm[:, 0], x.min(1).astype(np.float64))
        np.testing.assert_array_equal(mm[:, 1], x.max(1).astype(np.float64))
    x, y, w = (rng.standard_normal(n).astype(npdt) for _ in range(3))
    xd, yd, wd = dev(x), dev(y), dev(w)
    x6, y6, w6 = (a.astype(np.float64) for a in (x, y, w))
    for kw, ref in ((dict(), 1.5 * x6),
                    (dict(b=-0.5, y=yd), 1.5 * x6 - 0.5 * y6),
                    (dict(c=0.25, w=wd), 1.5 * x6 + 0.25 * w6),
                    (dict(b=-0.5, y=yd, c=0.25, w=wd), 1.5 * x6 - 0.5 * y6 + 0.25 * w6)):
        got = host(ops.axpbypcz(1.5, xd, **kw))
        assert np.abs(got - ref).max() <= atol, kw.keys()
    z, g, slot, prev, ts = (rng.standard_normal(n).astype(npdt) for _ in range(5))
    zd, gd, sd, pd, td = (dev(v) for v in (z, g, slot, prev, ts))
    ops.saga_table_update(zd, gd, sd, pd, td, 0.7, 0.25)
    z6, g6, sl6, p6, t6 = (a.astype(np.float64) for a in (z, g, slot, prev, ts))
    s2 = t6 + g6 - sl6
    stol = 2e-5 if dtype == F32 else 1e-13                  # (a few more flops on O(1) values: test_saga_table_update's f64 bound)
    assert np.abs(host(zd) - (z6 - 0.7 * ((g6 - p6) + s2 * 0.25))).max() <= stol
    assert np.abs(host(td) - s2).max() <= stol
    assert torch.equal(sd, gd)
