"""float64 NumPy restatement of the device-side Deblur and phase-retrieval problem generators (pnp_deblur_generate,
pnp_pr_generate, pnp_pr_spectral_init_batch), from the stream published in include/pnp_hip.h -- not from the kernels
(mix64 / state / keys are those of tests/csmri_generate_ref.py):

    noise    : n(m) = sqrt(-2 ln u1) cos(2 pi u2), u1 = (key_1(m) + 1) 2^-32, u2 = key_2(m) 2^-32      m = measurement index
    PR matrix: pair j = (m N + n) >> 1: r = sqrt(-2 ln u1(key_3(j))); element m N + n = r cos(2 pi u2(key_4(j))) (even),
               r sin(2 pi u2(key_4(j))) (odd)
    Xinit    : Deblur: key_5(i) 2^-32
    sigma    : sqrt(||Y0||_2 * snr_fac / H / W), snr_fac = 10^(-snr/10)
    Deblur   : Y0 = bilinear(fft_blur(x, B))            (problems/DeblurSR.py:38-57, 95-120)
    PR       : Y0 = |A x|, Xinit = minmax(spec_init)    (problems/PR.py:26-63)

tests/test_cpu_setup_generate.py holds the keys to literals computed with plain Python integers, and fixes the PR test items
(PR_ITEMS_32, PR_ITEM_128) whose stopping rule is far from its tolerance."""
import numpy as np

import csmri_generate_ref as gr

TOL = 1e-5                     # PR.py:56
EPS = 1e-10                    # DeblurSR.py:14

# ------------------------------------------------------------------------------------------------ the fixed PR test items
# (32 x 32, M = 5120: alpha = 5; 128 x 128, M = 8192: alpha = 0.5).  Chosen on the CPU so that the two stop quantities of the
# restatement, at the last iteration and at the one before, are not within a factor 2 of TOL and the iteration count is the
# same with A, x, Y rounded to float32 (tests/test_cpu_setup_generate.py::test_stop_margin_of_the_pr_test_items asserts it).
PR_SHAPE_32 = (32, 5120)
PR_SHAPE_128 = (128, 8192)


def images(n_img, n, seed=0):
    """Smoothed-noise test images (not normalised)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_img):
        x = rng.random((n, n))
        p = np.pad(x, 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def snr_fac(snr):
    return 10.0 ** (-np.float64(snr) / 10)


def sigma_of(Y0, snr, H, W):
    """problems/problem.py:58-61: the norm, not its square."""
    return float(np.sqrt(np.linalg.norm(np.ravel(Y0)) * snr_fac(snr) / H / W))


def noise(seed, item_id, M):
    """[M] standard normal draws n(m) of the item."""
    pos = np.arange(M)
    u1 = (gr.keys(seed, item_id, 1, pos).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = gr.keys(seed, item_id, 2, pos).astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def uniform(seed, item_id, N):
    """[N] draws in [0, 1): Deblur's Xinit."""
    return gr.keys(seed, item_id, 5, np.arange(N)).astype(np.float64) * 2.0 ** -32


def pr_matrix(seed, item_id, M, N, rows_per_block=256):
    """[M, N] float64 Gaussian matrix of the item."""
    assert M * N <= 2 ** 32
    A = np.empty(M * N)
    step = max(2, (rows_per_block * N) // 2 * 2)
    for e0 in range(0, M * N, step):
        e1 = min(e0 + step, M * N)
        j = np.arange(e0 >> 1, (e1 + 1) >> 1)
        r = np.sqrt(-2.0 * np.log((gr.keys(seed, item_id, 3, j).astype(np.float64) + 1.0) * 2.0 ** -32))
        ang = 2.0 * np.pi * (gr.keys(seed, item_id, 4, j).astype(np.float64) * 2.0 ** -32)
        both = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1).ravel()          # elements 2j, 2j + 1
        A[e0:e1] = both[:e1 - e0]                                                      # (e0 is even)
    return A.reshape(M, N)


# ------------------------------------------------------------------------------------------------ Deblur
def blur_kernel(H, W, kernel='Minimal'):
    """DeblurSR.py:76-93, already divided by N."""
    Bk = np.zeros((H, W))
    Bk[0, 0] = 1
    if kernel == 'Minimal':
        Bk[H // 2, H // 2] = Bk[H // 2, H // 3] = Bk[H // 2, H // 4] = 1
        Bk /= 4
    else:
        assert kernel == 'Identity'
    return Bk.ravel() / (H * W)


def fft_blur(a, b):
    """DeblurSR.py:119-120."""
    a, b = np.ravel(a), np.ravel(b)
    return np.real(np.fft.ifft(np.fft.fft(a) * np.fft.fft(b))) * np.sqrt(a.size)


def bilinear(v, H, W, scale_percent):
    """The down-sampler of DeblurSR.py:39-40, 95-108 applied to the raveled H x W image v: identity at 100, else 4-tap bilinear
    interpolation (floor index + fractional weights) on the reference's sampling grid."""
    if scale_percent == 100:
        return np.ravel(v).copy()
    lrH, lrW = int(H * scale_percent / 100), int(W * scale_percent / 100)
    ptsH = np.linspace(EPS, H - (1 + EPS), lrH)
    ptsW = np.linspace(EPS, W - (1 + EPS), lrW)
    meshW, meshH = np.meshgrid(ptsH, ptsW)
    rr, cc = meshH.ravel(), meshW.ravel()
    r0, c0 = np.floor(rr).astype(np.int64), np.floor(cc).astype(np.int64)
    wr, wc = rr - r0, cc - c0
    im = np.reshape(v, (H, W))
    return ((1 - wr) * (1 - wc) * im[r0, c0] + wr * (1 - wc) * im[r0 + 1, c0] + (1 - wr) * wc * im[r0, c0 + 1]
            + wr * wc * im[r0 + 1, c0 + 1])


def deblur_generate(x, item, kernel='Minimal', scale_percent=100):
    """One item on the normalised H x W image x -> dict(Y0, sigma, noise, Y, xinit)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    Y0 = bilinear(fft_blur(x, blur_kernel(H, W, kernel)), H, W, scale_percent)
    sg = sigma_of(Y0, item['snr'], H, W)
    n = noise(item['seed'], item['id'], Y0.size)
    return dict(Y0=Y0, sigma=sg, noise=n, Y=Y0 + sg * n, xinit=uniform(item['seed'], item['id'], H * W))


# ------------------------------------------------------------------------------------------------ phase retrieval
def pr_data(x, item, M, A=None):
    """A, Y0, sigma, noise, Y of one item on the normalised image x (PR.py:26-34)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    if A is None:
        A = pr_matrix(item['seed'], item['id'], M, H * W)
    Y0 = np.absolute(A @ x.ravel())
    sg = sigma_of(Y0, item['snr'], H, W)
    n = noise(item['seed'], item['id'], M)
    return dict(A=A, Y0=Y0, sigma=sg, noise=n, Y=Y0 + sg * n)


def _apply(A, Y, v, order):
    """A^T (Y o (A v)) / M; order 'plain' = two BLAS products, 'chunked' = both products summed over 7 blocks, last block first."""
    M = A.shape[0]
    if order == 'plain':
        return A.T @ (Y * (A @ v)) / M
    cb = np.array_split(np.arange(A.shape[1]), 7)
    t = np.zeros(M)
    for c in cb[::-1]:
        t = t + A[:, c] @ v[c]
    u = Y * t
    out = np.zeros(A.shape[1])
    for r in np.array_split(np.arange(M), 7)[::-1]:
        out = out + A[r].T @ u[r]
    return out / M


def spec_init(A, Y, x, order='plain', max_iters=100000):
    """PR.py:50-63 then :38 -> dict(xinit, iters, hist): hist[k] = (|m - mold|, ||y - y_old||) after step k + 1, the two
    quantities the rule of :57 tests before step k + 2."""
    N = A.shape[1]
    nrm = np.linalg.norm(np.ravel(x))
    m, mold = 1, 2
    y, y_old = 2 * np.ones(N), np.ones(N)
    hist = []
    while abs(m - mold) > TOL and np.linalg.norm(y - y_old) > TOL:
        assert len(hist) < max_iters
        mold = m
        y_old = y
        y = _apply(A, Y, y, order)
        m = np.max(y)
        y = y / m
        hist.append((abs(m - mold), float(np.linalg.norm(y - y_old))))
    x0 = np.sqrt(m) * y / np.linalg.norm(y) * nrm
    return dict(xinit=(x0 - x0.min()) / (x0.max() - x0.min()), iters=len(hist), hist=hist, lead=float(m))


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def stop_margin_ok(hist):
    """None of the stop quantities of the last two iterations within a factor 2 of TOL."""
    return all(not (TOL / 2 <= q <= 2 * TOL) for h in hist[-2:] for q in h)
