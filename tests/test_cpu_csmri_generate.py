"""CPU side of the device-side CSMRI problem generator (pnp_csmri_generate): the NumPy restatement of the published stream
(tests/csmri_generate_ref.py) against known answers and against the statistics a Bernoulli mask and Gaussian noise must
have, and the C ABI surface without a GPU.

The statistical bounds are 5 standard deviations of the binomial count (M0), of the mean of M0 unit normals and of their
variance (chi-square: var of the sample variance = 2/M0).  The (seed, id) pairs are fixed: seeds 0-2 with ids 0-7 were
checked on the CPU to satisfy all three at 64^2 and 256^2 for alpha in 0.1, 0.2, 0.5."""
import ctypes
import numpy as np
import pytest

import csmri_generate_ref as gr

PAIRS = [(s, i) for s in range(3) for i in range(8)]


def test_keys_known_answers():
    """key_k(i) computed with plain Python integers from the header's formulas."""
    for (seed, item_id, k, i), want in (((0, 0, 0, 0), 3625190023), ((0, 0, 1, 1), 3857828524), ((1, 5, 2, 65535), 101152842),
                                        ((2, 7, 0, 4095), 2897500646), ((2 ** 63 + 11, 3, 1, 12345), 537373952)):
        assert int(gr.keys(seed, item_id, k, np.array([i]))[0]) == want


def test_threshold():
    assert gr.threshold(0.0) == 0 and gr.threshold(1.0) == 2 ** 32 and gr.threshold(0.5) == 2 ** 31
    assert gr.threshold(-0.1) == 0 and gr.threshold(1.5) == 2 ** 32
    assert gr.threshold(0.1) == int(np.floor(0.1 * 2.0 ** 32))


@pytest.mark.parametrize('n', [64, 256])
@pytest.mark.parametrize('alpha', [0.1, 0.2, 0.5])
def test_mask_and_noise_statistics(n, alpha):
    N = n * n
    for seed, item_id in PAIRS:
        m = gr.mask(seed, item_id, alpha, n, n).astype(bool)
        M0 = int(m.sum())
        assert abs(M0 - alpha * N) <= 5 * np.sqrt(N * alpha * (1 - alpha)), (seed, item_id, M0)
        g = gr.noise(seed, item_id, n, n)[m]
        assert np.isfinite(g).all()
        assert abs(g.mean()) <= 5 / np.sqrt(M0), (seed, item_id, g.mean())
        assert abs(g.var() - 1) <= 5 * np.sqrt(2 / M0), (seed, item_id, g.var())


def test_masks_differ_between_items_and_edges():
    base = gr.mask(0, 0, 0.2, 64, 64)
    assert not np.array_equal(base, gr.mask(0, 1, 0.2, 64, 64))            # another id
    assert not np.array_equal(base, gr.mask(1, 0, 0.2, 64, 64))            # another seed
    assert not np.array_equal(gr.mask(1, 0, 0.2, 64, 64), gr.mask(0, 1, 0.2, 64, 64))
    assert np.array_equal(base, gr.mask(0, 0, 0.2, 64, 64))
    assert gr.mask(0, 0, 0.0, 64, 64).sum() == 0 and gr.mask(0, 0, 1.0, 64, 64).sum() == 64 * 64
    assert (gr.mask(0, 0, 0.5, 64, 64) >= base).all()                      # one key per position: masks nest in alpha


def test_generate_follows_the_reference_formulas():
    rng = np.random.default_rng(0)
    x = gr.norm01(rng.random((64, 64)))
    it = {'id': 3, 'image': 0, 'alpha': 0.3, 'snr': 20.0, 'seed': 1}
    r = gr.generate(x, it)
    mk = r['mask'].astype(bool)
    assert r['M0'] == mk.sum()
    Y0 = mk * np.fft.fft2(x)
    assert np.isclose(r['sigma'] ** 2, np.linalg.norm(Y0) / 100.0 / 64 / 64, rtol=1e-14)     # the norm, not its square
    assert np.array_equal(r['Y'][~mk], np.zeros((~mk).sum()))
    assert np.allclose((r['Y'] - Y0)[mk].imag, 0.0, atol=1e-12)            # real noise on the support
    assert np.allclose((r['Y'] - Y0)[mk].real, r['sigma'] * r['noise'][mk], rtol=0, atol=1e-9)
    assert r['xinit'].min() == 0.0 and r['xinit'].max() == 1.0


def test_symbol_exported_and_null_plan_is_an_argument_error():
    from pnp_svrg_amd import _native as N
    assert 'pnp_csmri_generate' in N.SIGNATURES
    lib = N.lib()
    args = [None, None, 0] + [None] * 15
    assert lib.pnp_csmri_generate(*args) == 1                             # PNP_ERR_ARG, no GPU touched
    assert b'pnp_csmri_generate' in lib.pnp_last_error() and b'null plan' in lib.pnp_last_error()
    assert hasattr(ctypes.CDLL(N.LIB_PATH), 'pnp_csmri_generate')


def test_device_seeding_is_csmri_only():
    from pnp_svrg_amd import sweep
    for problem in ('deblur', 'pr'):
        with pytest.raises(ValueError, match='csmri'):
            sweep.make_runner([np.zeros((64, 64))], problem, 'svrg', 'tv', eta=1.0, n_inner=4, mini_batch_size=10, T2=2, H=64, W=64,
                              seeding='device')
