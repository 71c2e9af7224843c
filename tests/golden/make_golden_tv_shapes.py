#!/usr/bin/env python3.9
"""Golden vectors of the "TV" prox and the noise estimate at the shapes the 64 / 256 fixtures of make_golden.py do not
reach, produced by RUNNING THE REAL REFERENCE (harness conventions of make_golden.py: modules imported by path, arrays
only; the reference's Python environment: NumPy 1.26.4, scikit-image 0.18.3, PyWavelets 1.1.1).

    python3.9 tests/golden/make_golden_tv_shapes.py REFERENCE_ROOT

Writes tests/golden/tv_shapes.npz for (H, W) in {(16, 48), (128, 32), (32, 256)}: H = 16 (one Haar level), non-square
images, and widths that are not a multiple of 64 (an odd number of 16-column waves).  Per shape `h{H}w{W}`:
  *_z0         : the input, a smoothed image plus noise quantised to multiples of 2^-16 (exact in float32 too)
  *_sigma_est  : estimate_sigma(z0, multichannel=True, average_sigmas=True)
  *_tv         : TVDenoiser().denoise(noisy=z0, sigma_est=sigma_est)
  *_tv_mod     : TVDenoiser(sigma_modifier=1.7).denoise(noisy=z0, sigma_est=sigma_est)
  *_tv_strength: TVDenoiser(denoise_strength=0.07, decay=0.9).denoise(noisy=z0, sigma_est=0)   (the sigma_est <= 0 branch)
and nonfinite_{z0, sigma_est, tv}: three 64 x 64 images with a NaN, +inf or -inf pixel, their estimates (NaN: the median
sees a NaN coefficient) and TVDenoiser(denoise_strength=0.05).denoise(noisy=z0, sigma_est=estimate).

The GPU box never runs this script; tests read the .npz file only.
"""
import os
import sys
import warnings
import numpy as np

warnings.filterwarnings('ignore')
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [REF, REF + '/denoisers']

from TV import TVDenoiser                                    # noqa: E402
from skimage.restoration import estimate_sigma               # noqa: E402

SHAPES = ((16, 48), (128, 32), (32, 256))


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
        z0 = test_image(H, W, 700 + k)
        s = estimate_sigma(z0, multichannel=True, average_sigmas=True)
        out[f'{tag}_z0'] = z0
        out[f'{tag}_sigma_est'] = np.array(s)
        out[f'{tag}_tv'] = TVDenoiser().denoise(noisy=z0, sigma_est=s)
        out[f'{tag}_tv_mod'] = TVDenoiser(sigma_modifier=1.7).denoise(noisy=z0, sigma_est=s)
        out[f'{tag}_tv_strength'] = TVDenoiser(denoise_strength=0.07, decay=0.9).denoise(noisy=z0, sigma_est=0)
    # non-finite pixels (64 x 64): NaN inside a column; +inf on row 0, where the symmetric edge puts two taps on one pixel
    # (inf - inf = NaN coefficient); -inf inside a column (finite estimate: the median ignores one large coefficient)
    z = test_image(64, 64, 710)[None].repeat(3, 0)
    z[0, 30, 7] = np.nan
    z[1, 0, 9] = np.inf
    z[2, 33, 40] = -np.inf
    out['nonfinite_z0'] = z
    out['nonfinite_sigma_est'] = np.array([estimate_sigma(x, multichannel=True, average_sigmas=True) for x in z])
    out['nonfinite_tv'] = np.stack([TVDenoiser(denoise_strength=0.05).denoise(noisy=x, sigma_est=s)
                                    for x, s in zip(z, out['nonfinite_sigma_est'])])
    np.savez_compressed(os.path.join(HERE, 'tv_shapes.npz'), **out)
    print('wrote tv_shapes.npz', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
