"""NumPy float64 restatement of the data-fidelity objective f(w) = ||Y - forward_model(w)||^2 / 2 / M of the three problems
(reference problems/CSMRI.py:61-64, DeblurSR.py:114-117, PR.py:70-73), written from the formulas alone: what the device
objectives (pnp_csmri_objective, pnp_deblur_objective, pnp_pr_objective) are held against.  tests/test_cpu_objective.py pins
it to the oracle's `f` (the dense-DFT form of CSMRI included)."""
import numpy as np


def csmri_f(w, mask, Y):
    """sum over the FULL spectrum of |Y - mask o fft2(w)|^2 / 2 / N, N = H W (the mask need not be Hermitian)."""
    H, W = mask.shape
    r = np.asarray(Y, np.complex128) - mask * np.fft.fft2(np.asarray(w, np.float64).reshape(H, W))
    return float(np.sum(r.real ** 2 + r.imag ** 2) / 2 / (H * W))


def fft_blur(a, b):
    """DeblurSR.py:119-120: 1-D circular convolution of the ravelled image, times sqrt(N)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.real(np.fft.ifft(np.fft.fft(a) * np.fft.fft(b))) * np.sqrt(a.size)


def minimal_kernel(H, W):
    """DeblurSR.py:80-93, kernel 'Minimal': four taps of 1/4, divided by N."""
    B = np.zeros((H, W))
    B[0, 0] = B[H // 2, H // 2] = B[H // 2, H // 3] = B[H // 2, H // 4] = 0.25
    return B.ravel() / (H * W)


def deblur_taps(H, W, scale_percent, eps=1e-10):
    """The down-sampler of DeblurSR.py:95-108 as (idx [M, 4], weights [M, 4]) -- bilinear interpolation at the reference's grid of
    lrH x lrW points (floor index + fractional weights) -- or None for scale_percent == 100."""
    if scale_percent == 100:
        return None
    lrH, lrW = int(H * scale_percent / 100), int(W * scale_percent / 100)
    ptsH = np.linspace(eps, H - (1 + eps), lrH)
    ptsW = np.linspace(eps, W - (1 + eps), lrW)
    meshW, meshH = np.meshgrid(ptsH, ptsW)                              # (sic) DeblurSR.py:102
    rows, cols = meshH.ravel(), meshW.ravel()
    r0, c0 = np.floor(rows).astype(np.int64), np.floor(cols).astype(np.int64)
    wr, wc = rows - r0, cols - c0
    idx = np.stack([r0 * W + c0, (r0 + 1) * W + c0, r0 * W + c0 + 1, (r0 + 1) * W + c0 + 1], axis=1)
    wts = np.stack([(1 - wr) * (1 - wc), wr * (1 - wc), (1 - wr) * wc, wr * wc], axis=1)
    return idx, wts


def deblur_forward(w, Bk, taps=None):
    y = fft_blur(w, Bk)
    return y if taps is None else np.sum(taps[1] * y[taps[0]], axis=1)


def deblur_f(w, Bk, Y, taps=None):
    """||Y - S B w||^2 / 2 / M, M = number of measurements (lrH lrW)."""
    r = np.asarray(Y, np.float64).ravel() - deblur_forward(w, Bk, taps)
    return float(np.sum(r ** 2) / 2 / r.size)


def pr_f(w, A, Y):
    """|| Y - |A w| ||^2 / 2 / M."""
    r = np.asarray(Y, np.float64).ravel() - np.abs(np.asarray(A, np.float64) @ np.asarray(w, np.float64).ravel())
    return float(np.sum(r ** 2) / 2 / r.size)
