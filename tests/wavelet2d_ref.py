"""float64 NumPy restatement of TVDenoiser(multi=False): skimage denoise_wavelet(method='BayesShrink', wavelet='db1',
mode='soft', multichannel=False) on a float image whose sides are divisible by 2^L (every shape pnp_prox_wavelet2d takes).
It lets GPU tests use inputs the fixture does not hold; it is trusted only because tests/test_cpu_wavelet2d.py holds it
to the real library's outputs in tests/golden/wavelet2d*.npz, bit for bit."""
import numpy as np
from conftest import golden

HA = 0.7071067811865476


def load_fixture():
    """tests/golden/wavelet2d.npz + wavelet2d_h256w256.npz (one fixture, two files below 1 MiB each) as one dict."""
    out = dict(golden('wavelet2d.npz'))
    out.update(golden('wavelet2d_h256w256.npz'))
    return out


def levels(H, W):
    return max(min(int(np.floor(np.log2(H))), int(np.floor(np.log2(W)))) - 3, 1)


def _ana(a, axis):
    a = np.moveaxis(a, axis, 0)
    ev, od = a[0::2], a[1::2]
    return np.moveaxis(HA * od + HA * ev, 0, axis), np.moveaxis(-HA * od + HA * ev, 0, axis)


def _syn(lo, hi, axis):
    lo, hi = np.moveaxis(lo, axis, 0), np.moveaxis(hi, axis, 0)
    up = np.empty((2 * lo.shape[0],) + lo.shape[1:], dtype=lo.dtype)
    up[0::2] = HA * lo + HA * hi
    up[1::2] = HA * lo - HA * hi
    return np.moveaxis(up, 0, axis)


def wavelet2d_bayes(img, sigma):
    """pywt.wavedecn (axis 0 first), one BayesShrink threshold per detail sub-band, pywt.waverecn (last axis first)."""
    a = np.asarray(img, np.float64)
    L = levels(*a.shape)
    assert a.shape[0] % (1 << L) == 0 and a.shape[1] % (1 << L) == 0
    var = float(sigma) ** 2
    eps = np.finfo(np.float64).eps
    det = []
    for _ in range(L):
        lo, hi = _ana(a, 0)
        aa, ad = _ana(lo, 1)
        da, dd = _ana(hi, 1)
        det.append((ad, da, dd))
        a = aa
    with np.errstate(all='ignore'):
        for bands in reversed(det):
            shr = []
            for d in bands:
                thr = var / np.sqrt(max(np.mean(d * d) - var, eps))     # max(NaN, eps) is NaN
                shr.append(d * np.clip(1.0 - thr / np.abs(d), 0, None))  # 0/0 -> NaN kept
            a = _syn(_syn(a, shr[0], 1), _syn(shr[1], shr[2], 1), 0)
    return a


def prox(img, sigma_est, sigma_modifier=1.0, fallback_sigma=0.0):
    """denoisers/TV.py:21-26: sigma = sigma_est * sigma_modifier when sigma_est > 0, else the fixed strength."""
    return wavelet2d_bayes(img, sigma_est * sigma_modifier if sigma_est > 0 else fallback_sigma)


class Wavelet2dDenoiser:
    """The restatement behind the reference's denoiser protocol (t, denoise(noisy=, sigma_est=)), for oracle loops."""

    def __init__(self, decay=1, denoise_strength=0, sigma_modifier=1):
        self.t, self.decay, self.denoise_strength, self.sigma_modifier = 0, decay, denoise_strength, sigma_modifier

    def denoise(self, noisy, sigma_est=0):
        self.t += 1
        return prox(noisy, sigma_est, self.sigma_modifier, self.denoise_strength * self.decay ** self.t)
