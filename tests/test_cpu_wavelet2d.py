"""CPU side of the 2-D wavelet BayesShrink prox (TVDenoiser(multi=False) -> pnp_prox_wavelet2d): the NumPy restatement
the GPU tests lean on against the real library's outputs, the C ABI surface, and construction without a GPU."""
import ctypes
import os
import re
import numpy as np
import pytest
from conftest import ROOT

import wavelet2d_ref as wr

SHAPES = ((16, 16), (16, 48), (128, 32), (32, 256), (64, 80), (256, 112), (256, 256))


@pytest.fixture(scope='module')
def g():
    return wr.load_fixture()


@pytest.mark.parametrize('H,W', SHAPES)
def test_restatement_is_the_reference_bit_for_bit(g, H, W):
    tag = f'h{H}w{W}'
    z0, s = g[f'{tag}_z0'], float(g[f'{tag}_sigma_est'])
    assert z0.shape == (H, W) and s > 0
    assert np.array_equal(wr.prox(z0, s), g[f'{tag}_w2d'])
    assert np.array_equal(wr.prox(z0, s, sigma_modifier=1.7), g[f'{tag}_w2d_mod'])
    assert np.array_equal(wr.prox(z0, 0.0, fallback_sigma=0.07 * 0.9), g[f'{tag}_w2d_strength'])
    assert np.abs(g[f'{tag}_w2d'] - z0).max() > 1e-3                      # it does denoise


def test_restatement_nonfinite_pixels(g):
    z, s, ref = g['nonfinite_z0'], g['nonfinite_sigma_est'], g['nonfinite_w2d']
    assert np.isnan(ref).any()
    for k in range(3):
        got = wr.prox(z[k], s[k], fallback_sigma=0.05)
        assert np.array_equal(np.isnan(got), np.isnan(ref[k]))
        assert np.array_equal(got, ref[k], equal_nan=True)


def test_fixture_files_are_small():
    for name in ('wavelet2d.npz', 'wavelet2d_h256w256.npz'):
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', name)) < 1 << 20


def test_symbol_declared_exported_and_bound():
    from pnp_svrg_amd import _native as N
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    assert re.search(r'^int\s+pnp_prox_wavelet2d\s*\(', hdr, re.M)
    assert 'pnp_prox_wavelet2d' in N.SIGNATURES
    assert N.SIGNATURES['pnp_prox_wavelet2d'] == N.SIGNATURES['pnp_prox_tv']          # argument for argument
    assert hasattr(ctypes.CDLL(N.LIB_PATH), 'pnp_prox_wavelet2d')


def test_argument_errors_are_reported_without_gpu():
    from pnp_svrg_amd import _native as N
    lib = N.lib()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    args = lambda H, W, dt, zi=p, zo=p, B=1: (zi, zo, H, W, B, dt, None, 1.0, 0.0, None, None, None, None)   # noqa: E731
    assert lib.pnp_prox_wavelet2d(*args(48, 64, N.F64)) == 1                         # PNP_ERR_ARG
    assert b'H must be 16, 32, 64, 128 or 256' in lib.pnp_last_error()
    assert lib.pnp_prox_wavelet2d(*args(64, 40, N.F64)) == 1
    assert b'W must be a multiple of 16 in [16, 256]' in lib.pnp_last_error()
    assert lib.pnp_prox_wavelet2d(*args(64, 64, 7)) == 1
    assert b'bad dtype' in lib.pnp_last_error()
    assert lib.pnp_prox_wavelet2d(*args(64, 64, N.F64, zo=None)) == 1
    assert b'null output' in lib.pnp_last_error()
    assert lib.pnp_prox_wavelet2d(*args(64, 64, N.F64, B=0)) == 1
    assert b'null input / empty batch' in lib.pnp_last_error()
    with pytest.raises(N.NativeError):
        N.call('pnp_prox_wavelet2d', None, None, 48, 64, 1, 0, None, 1.0, 0.0, None, None, None, None)


def test_constructs_without_gpu():
    import denoisers
    from pnp_svrg_amd import ops, sweep
    from pnp_svrg_amd.engine import TVProx
    d = denoisers.TVDenoiser(multi=False, rescale_sigma=False, decay=0.9, denoise_strength=0.07, sigma_modifier=1.7)
    assert d.multi is False and d.t == 0 and d._prox is ops.prox_wavelet2d
    assert d.prox_inplace(None, None, None, probe=True) is False                     # decaying fixed strength: no graph
    assert denoisers.TVDenoiser(multi=False).prox_inplace(None, None, None, probe=True) is True
    assert denoisers.TVDenoiser()._prox is ops.prox_tv
    p = TVProx(multi=False, sigma_modifier=1.3)
    assert p.inplace and not p.fused_denoise and p.multi is False
    assert TVProx().fused_denoise and TVProx().multi
    q = sweep.make_prox('tv', multi=False)
    assert isinstance(q, TVProx) and not q.multi
