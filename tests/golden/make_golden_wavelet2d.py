#!/usr/bin/env python3.9
"""Golden vectors of the 2-D wavelet BayesShrink prox, TVDenoiser(multi=False), produced by RUNNING THE REAL REFERENCE
(harness conventions of make_golden.py / make_golden_tv_shapes.py: modules imported by path, arrays only, a counting
clock bound to the algorithm module; the reference's Python environment: NumPy 1.26.4, scikit-image 0.18.3,
PyWavelets 1.1.1).

    python3.9 tests/golden/make_golden_wavelet2d.py REFERENCE_ROOT

Writes tests/golden/wavelet2d.npz and, for the (256, 256) prox vectors alone, tests/golden/wavelet2d_h256w256.npz (each
file stays below 1 MiB).  Per shape `h{H}w{W}` in SHAPES (one to five Haar levels, non-square images, widths
that are not a power of two):
  *_z0          : the input (make_golden_tv_shapes.py's test_image, on the 2^-16 grid: exact in float32 too)
  *_sigma_est   : estimate_sigma(z0, multichannel=True, average_sigmas=True)
  *_w2d         : TVDenoiser(multi=False).denoise(noisy=z0, sigma_est=sigma_est)
  *_w2d_mod     : TVDenoiser(multi=False, sigma_modifier=1.7).denoise(noisy=z0, sigma_est=sigma_est)
  *_w2d_strength: TVDenoiser(multi=False, denoise_strength=0.07, decay=0.9).denoise(noisy=z0, sigma_est=0)
nonfinite_{z0, sigma_est, w2d}: three 64 x 64 images with a NaN, +inf or -inf pixel, their estimates and
TVDenoiser(multi=False, denoise_strength=0.05).denoise(noisy=z0, sigma_est=estimate).
Loop traces with TVDenoiser(multi=False) (seeds and arguments of make_golden.py's traces64.npz / traces256.npz; the
minibatches come back from the legacy RNG seeds): svrg64_{z, psnr}, saga64_{z, psnr}, svrg256_{z, psnr}.

The GPU box never runs this script; tests read the .npz files only.
"""
import os
import sys
import types
import warnings
import numpy as np

warnings.filterwarnings('ignore')
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REF, REF + '/problems', REF + '/denoisers']

# pylops is absent and the reference's DeblurSR.py (pulled in by the problems package) imports it at module scope
_pl = types.ModuleType('pylops')
_pl.Identity = object
_pl.signalprocessing = types.SimpleNamespace()
sys.modules.setdefault('pylops', _pl)

import algorithms                                            # noqa: E402,F401
from CSMRI import CSMRI                                      # noqa: E402
from TV import TVDenoiser                                    # noqa: E402
from skimage.restoration import estimate_sigma               # noqa: E402

SHAPES = ((16, 16), (16, 48), (128, 32), (32, 256), (64, 80), (256, 112), (256, 256))


class FakeClock:
    def __init__(self):
        self.n = -1.0

    def time(self):
        self.n += 1.0
        return self.n


def run_algo(name, *args, **kw):
    mod = sys.modules['algorithms.' + name]
    mod.time = FakeClock()
    return getattr(mod, name)(*args, verbose=False, **kw)


def test_image(H, W, seed):
    """Smoothed uniform noise (3x3 box, wrapped) + Gaussian noise of sigma 0.05, on the 2^-16 grid."""
    rng = np.random.default_rng(seed)
    x = rng.random((H, W))
    p = np.pad(x, 1, mode='wrap')
    y = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    y = y + 0.05 * rng.standard_normal((H, W))
    return np.round(y * 65536.0) / 65536.0


def main():
    out = {}
    for k, (H, W) in enumerate(SHAPES):
        tag = f'h{H}w{W}'
        z0 = test_image(H, W, 800 + k)
        s = estimate_sigma(z0, multichannel=True, average_sigmas=True)
        out[f'{tag}_z0'] = z0
        out[f'{tag}_sigma_est'] = np.array(s)
        out[f'{tag}_w2d'] = TVDenoiser(multi=False).denoise(noisy=z0, sigma_est=s)
        out[f'{tag}_w2d_mod'] = TVDenoiser(multi=False, sigma_modifier=1.7).denoise(noisy=z0, sigma_est=s)
        out[f'{tag}_w2d_strength'] = TVDenoiser(multi=False, denoise_strength=0.07, decay=0.9).denoise(noisy=z0, sigma_est=0)
    z = test_image(64, 64, 810)[None].repeat(3, 0)
    z[0, 30, 7] = np.nan
    z[1, 0, 9] = np.inf
    z[2, 33, 40] = -np.inf
    out['nonfinite_z0'] = z
    out['nonfinite_sigma_est'] = np.array([estimate_sigma(x, multichannel=True, average_sigmas=True) for x in z])
    out['nonfinite_w2d'] = np.stack([TVDenoiser(multi=False, denoise_strength=0.05).denoise(noisy=x, sigma_est=s)
                                     for x, s in zip(z, out['nonfinite_sigma_est'])])

    img64, img256 = os.path.join(HERE, 'synth64.png'), os.path.join(HERE, 'synth256.png')
    runs = {
        'svrg64': (img64, 64, lambda p, d: run_algo('pnp_svrg', p, d, 5e2, 60, 4, 200, converge_check=False)),
        'saga64': (img64, 64, lambda p, d: run_algo('pnp_saga', p, d, 5e2, 53, 200, hist_size=5, converge_check=False)),
        'svrg256': (img256, 256, lambda p, d: run_algo('pnp_svrg', p, d, 2e3, 2 + 4 * (3 + 5 * 10), 10, 1000,
                                                       converge_check=False)),
    }
    for name, (img, n, fn) in runs.items():
        np.random.seed(0)
        p = CSMRI(img, H=n, W=n, sample_prob=0.2, snr=20.)
        np.random.seed(1)
        r = fn(p, TVDenoiser(multi=False))
        out[f'{name}_z'] = r['z']
        out[f'{name}_psnr'] = np.array(r['psnr_per_iter'])
        print(name, len(r['psnr_per_iter']), r['psnr_per_iter'][:3], r['psnr_per_iter'][-1])
    # two files, each below the repository's 1 MiB limit for a committed file: the 256 x 256 prox vectors on their own
    big = {k: out.pop(k) for k in list(out) if k.startswith('h256w256_')}
    np.savez_compressed(os.path.join(HERE, 'wavelet2d.npz'), **out)
    np.savez_compressed(os.path.join(HERE, 'wavelet2d_h256w256.npz'), **big)
    print('wrote wavelet2d.npz', {k: v.shape for k, v in out.items()})
    print('wrote wavelet2d_h256w256.npz', {k: v.shape for k, v in big.items()})


if __name__ == '__main__':
    main()
