"""CPU side of the device-side Deblur / phase-retrieval problem generators (pnp_deblur_generate, pnp_pr_generate,
pnp_pr_spectral_init_batch): the NumPy restatement of the published stream (tests/setup_generate_ref.py) against known answers,
against the statistics a Gaussian matrix must have and against the reference's formulas; the fixed PR test items; the C ABI
surface and make_runner(seeding='counter') without a GPU.

Statistical bounds are 5 standard deviations of the sampling distribution over n = M N elements: mean 1/sqrt(n), variance
sqrt(2/n), correlation of the even and the odd element of a pair 1/sqrt(n/2).  The (seed, id) pairs are those of the PR test
items below plus (1, 5) and (2, 7); all satisfy the bounds (checked here)."""
import ctypes

import numpy as np
import pytest

import csmri_generate_ref as gr
import setup_generate_ref as sr

# The fixed 32 x 32, M = 5120 PR items of the GPU tests (image = index into sr.images(4, 32, seed=11)), found by a scan of ids
# 0-199 x eight SNRs on the CPU (46 of 1600 candidates meet the stop-margin condition below; most do not, because
# |lead - lead_old| usually decays by 0.75-0.9 per step -- these are the items whose lead sequence turns round, so that the
# difference passes through zero).  They stop after 28, 34, 23, 22 and 17 power-iteration steps: a batch of them exercises freezing.
PR_ITEMS_32 = [{'id': 16, 'image': 0, 'alpha': 5.0, 'snr': 10.0, 'seed': 0}, {'id': 50, 'image': 2, 'alpha': 5.0, 'snr': 20.0, 'seed': 0},
               {'id': 72, 'image': 0, 'alpha': 5.0, 'snr': 60.0, 'seed': 0}, {'id': 74, 'image': 2, 'alpha': 5.0, 'snr': 40.0, 'seed': 0},
               {'id': 12, 'image': 0, 'alpha': 5.0, 'snr': 25.0, 'seed': 0}]
PR_ITERS_32 = [28, 34, 23, 22, 17]
PR_IMAGES_32 = dict(n_img=4, n=32, seed=11)

# The 128 x 128, M = 8192 item (on sr.images(1, 128, seed=12)): at snr 5.14 the lead sequence of item 4 turns round at step 60,
# where |lead - lead_old| is 1.1e-3 then 7.9e-8 (||v - v_old|| 9e-2); without such a turn this shape needs ~570 steps whose
# differences shrink by 0.2 % per step and cannot keep the margin.
PR_ITEM_128 = {'id': 4, 'image': 0, 'alpha': 0.5, 'snr': 5.14, 'seed': 0}
PR_ITERS_128 = 60

_cache = {}


def pr_case_128():
    """(x, data dict, spec_init result) of PR_ITEM_128 in float64 (a 1 GiB matrix), computed once per session."""
    if 128 not in _cache:
        x = gr.norm01(sr.images(1, 128, seed=12)[0])
        d = sr.pr_data(x, PR_ITEM_128, 8192)
        _cache[128] = (x, d, sr.spec_init(d['A'], d['Y'], x, max_iters=1000))
    return _cache[128]


def pr_case_32(j):
    """(x, data dict, spec_init result) of PR_ITEMS_32[j] in float64, computed once per session."""
    if j not in _cache:
        it = PR_ITEMS_32[j]
        x = gr.norm01(sr.images(**PR_IMAGES_32)[it['image']])
        d = sr.pr_data(x, it, 5120)
        _cache[j] = (x, d, sr.spec_init(d['A'], d['Y'], x))
    return _cache[j]


def test_keys_known_answers_of_the_new_tags():
    """key_k(i) for tags 3, 4, 5 computed with plain Python integers from the header's formulas."""
    for (seed, item_id, k, i), want in (((0, 0, 3, 0), 1832285373), ((0, 0, 4, 0), 2362548089), ((1, 5, 3, 2621439), 3491859677),
                                        ((2, 7, 4, 2 ** 31 - 1), 1755626784), ((0, 13, 5, 1023), 2371565502),
                                        ((2 ** 63 + 11, 3, 5, 65535), 3649002129)):
        assert int(gr.keys(seed, item_id, k, np.array([i]))[0]) == want
    # the stream's arithmetic on those keys: element 0 / 1 of item (0, 0) and a Deblur Xinit entry
    r = np.sqrt(-2.0 * np.log((1832285373 + 1.0) * 2.0 ** -32))
    a = sr.pr_matrix(0, 0, 2, 2)
    assert a[0, 0] == r * np.cos(2.0 * np.pi * (2362548089 * 2.0 ** -32)) and a[0, 1] == r * np.sin(2.0 * np.pi * (2362548089 * 2.0 ** -32))
    assert sr.uniform(0, 13, 1024)[1023] == 2371565502 * 2.0 ** -32
    u = sr.uniform(2, 7, 4096)
    assert u.min() >= 0.0 and u.max() < 1.0


def test_pr_matrix_layout():
    """Pairs run over the flat element index, across row ends; a block boundary inside pr_matrix changes nothing."""
    a = sr.pr_matrix(1, 5, 6, 5, rows_per_block=256)
    assert np.array_equal(a, sr.pr_matrix(1, 5, 6, 5, rows_per_block=1))
    assert np.array_equal(a.ravel()[:12], sr.pr_matrix(1, 5, 3, 4).ravel())            # element e depends on e alone
    with pytest.raises(AssertionError):
        sr.pr_matrix(0, 0, 2 ** 16 + 1, 2 ** 16)


@pytest.mark.parametrize('seed,item_id', [(0, 16), (0, 50), (0, 72), (0, 74), (0, 12), (1, 5), (2, 7)])
def test_pr_matrix_statistics(seed, item_id):
    a = sr.pr_matrix(seed, item_id, 5120, 1024).ravel()
    n = a.size
    assert np.isfinite(a).all()
    assert abs(a.mean()) <= 5 / np.sqrt(n), a.mean()
    assert abs(a.var() - 1) <= 5 * np.sqrt(2 / n), a.var()
    ev, od = a[0::2], a[1::2]
    corr = np.mean((ev - ev.mean()) * (od - od.mean())) / (ev.std() * od.std())
    assert abs(corr) <= 5 / np.sqrt(n / 2), corr


def test_restatement_follows_the_reference_formulas():
    # sigma: the norm, not its square
    x, d, s = pr_case_32(0)
    assert np.isclose(d['sigma'] ** 2, np.linalg.norm(d['Y0']) / 10.0 / 32 / 32, rtol=1e-14)          # (item 0: snr 10)
    assert np.array_equal(d['Y0'], np.absolute(d['A'] @ x.ravel())) and np.allclose(d['Y'] - d['Y0'], d['sigma'] * d['noise'], rtol=0, atol=1e-12)
    # the power iteration is the loop of PR.py:54-63 on the N x N matrix D
    A, Y = d['A'][:600, :64], d['Y'][:600]
    xs = x.ravel()[:64]
    D = A.T.dot(A * Y[:, None]) / 600
    m, mold = 1, 2
    y_final, y_old = 2 * np.ones(64), np.ones(64)
    n_it = 0
    while abs(m - mold) > 1e-5 and np.linalg.norm(y_final - y_old) > 1e-5:
        mold = m
        y_old = y_final
        y_final = D.dot(y_final)
        m = np.max(y_final)
        y_final = y_final / m
        n_it += 1
    x0 = np.sqrt(m) * y_final / np.linalg.norm(y_final) * np.linalg.norm(xs)
    want = (x0 - x0.min()) / (x0.max() - x0.min())
    got = sr.spec_init(A, Y, xs)
    assert got['iters'] == n_it and np.abs(got['xinit'] - want).max() <= 1e-10
    assert sr.spec_init(A, Y, xs, order='chunked')['iters'] == n_it
    # Deblur: Y0 = fft_blur then the bilinear down-sampler; identity at scale_percent 100
    img = gr.norm01(sr.images(1, 64, seed=3)[0])
    it = {'id': 4, 'image': 0, 'alpha': 0.5, 'snr': 20.0, 'seed': 1}
    Bk = sr.blur_kernel(64, 64)
    blurred = np.real(np.fft.ifft(np.fft.fft(img.ravel()) * np.fft.fft(Bk))) * np.sqrt(4096)
    r100, r50 = sr.deblur_generate(img, it, scale_percent=100), sr.deblur_generate(img, it, scale_percent=50)
    assert np.array_equal(r100['Y0'], blurred) and r50['Y0'].shape == (1024,)
    assert np.array_equal(r50['Y0'], sr.bilinear(blurred, 64, 64, 50))
    from pnp_svrg_amd.problems import _deblur_taps
    idx, wts = _deblur_taps(64, 64, 50)[:2]
    assert np.abs((wts * blurred[idx]).sum(1) - r50['Y0']).max() <= 1e-14                 # the taps the plan is given
    assert np.isclose(r50['sigma'] ** 2, np.linalg.norm(r50['Y0']) / 100.0 / 64 / 64, rtol=1e-14)
    assert np.array_equal(r50['xinit'], sr.uniform(1, 4, 4096)) and np.array_equal(r50['noise'], sr.noise(1, 4, 1024))


@pytest.mark.parametrize('j', range(5))
def test_pr_test_items_iteration_count_survives_float32_rounding(j):
    """The iteration count of every PR test item is the one recorded above, and the same whether A, x, Y are kept in float64
    or rounded to float32 (and with the products summed in another order)."""
    x, d, s = pr_case_32(j)
    assert s['iters'] == PR_ITERS_32[j]
    x32, A32 = sr.r32(x), sr.r32(d['A'])
    d32 = sr.pr_data(x32, PR_ITEMS_32[j], 5120, A=A32)
    assert sr.spec_init(A32, sr.r32(d32['Y']), x32)['iters'] == s['iters']
    assert sr.spec_init(d['A'], d['Y'], x, order='chunked')['iters'] == s['iters']


@pytest.mark.parametrize('j', range(5))
def test_stop_margin_of_the_pr_test_items(j):
    """Neither stop quantity (|lead - lead_old|, ||v - v_old||), at the last iteration or at the one before, lies within a
    factor 2 of tol = 1e-5: |lead - lead_old| falls from >= 2.4e-5 to <= 3.2e-6 in the last step of every item (5.43e-5 -> 2.47e-6,
    2.79e-5 -> 1.64e-6, 2.41e-5 -> 1.87e-7, 1.29e-4 -> 3.08e-7, 7.57e-4 -> 3.19e-6) and ||v - v_old|| is >= 4e-3 throughout."""
    hist = pr_case_32(j)[2]['hist']
    print(PR_ITEMS_32[j]['id'], hist[-2:])
    assert sr.stop_margin_ok(hist), hist[-2:]


def test_the_128_pr_test_item():
    """The same two conditions for the 128 x 128, M = 8192 item: stop margin, and an iteration count that survives float32
    rounding of A, x, Y and another summation order."""
    x, d, s = pr_case_128()
    print(s['hist'][-2:])
    assert s['iters'] == PR_ITERS_128 and sr.stop_margin_ok(s['hist']), s['hist'][-2:]
    assert sr.spec_init(d['A'], d['Y'], x, order='chunked', max_iters=1000)['iters'] == s['iters']
    x32, A32 = sr.r32(x), sr.r32(d['A'])
    d32 = sr.pr_data(x32, PR_ITEM_128, 8192, A=A32)
    assert sr.spec_init(A32, sr.r32(d32['Y']), x32, max_iters=1000)['iters'] == s['iters']


def test_symbols_exported_and_argument_errors_without_a_gpu():
    from pnp_svrg_amd import _native as N
    lib = N.lib()
    names = ('pnp_deblur_generate', 'pnp_pr_generate', 'pnp_pr_spectral_workspace_bytes', 'pnp_pr_spectral_init_batch')
    raw = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert nm in N.SIGNATURES and hasattr(raw, nm)
    assert lib.pnp_deblur_generate(*([None, None, 0] + [None] * 9)) == 1                    # PNP_ERR_ARG: null plan
    assert b'pnp_deblur_generate' in lib.pnp_last_error() and b'null plan' in lib.pnp_last_error()
    one = ctypes.c_void_p(8)                                                               # non-null, never dereferenced
    assert lib.pnp_pr_generate(one, 1, one, one, one, one, 32, 32, 16, 1, 0, None, one, one, one, None) == 1
    assert b'pnp_pr_generate' in lib.pnp_last_error() and b'null A' in lib.pnp_last_error()
    assert lib.pnp_pr_generate(one, 1, one, one, one, one, 256, 256, 65537, 1, 0, one, one, one, one, None) == 1
    assert b'2^32' in lib.pnp_last_error()
    assert lib.pnp_pr_spectral_init_batch(None, one, one, 16, 16, 1, 0, 10, 2, one, one, one, one, None) == 1
    assert b'pnp_pr_spectral_init_batch' in lib.pnp_last_error() and b'null A' in lib.pnp_last_error()
    assert lib.pnp_pr_spectral_init_batch(one, one, one, 16, 16, 1, 0, 0, 2, one, one, one, one, None) == 1
    assert lib.pnp_pr_spectral_workspace_bytes(5120, 1024, 3) == (3 * (2 * 1024 + 5120 + 64 * 1024 + 1) + 1) * 8


def test_counter_seeding_constructs_without_a_gpu():
    from pnp_svrg_amd import sweep
    imgs = [np.zeros((32, 32))]
    for problem in ('csmri', 'deblur', 'pr'):
        run = sweep.make_runner(imgs, problem, 'svrg', 'tv', eta=1.0, n_inner=4, mini_batch_size=10, T2=2, H=32, W=32, seeding='counter')
        assert callable(run) and callable(run.prepare)
    for problem in ('deblur', 'pr'):                                                       # the older spelling stays CSMRI-only
        with pytest.raises(ValueError, match='csmri'):
            sweep.make_runner(imgs, problem, 'svrg', 'tv', eta=1.0, n_inner=4, mini_batch_size=10, T2=2, H=32, W=32, seeding='device')
    assert sweep.deblur_scale_percent(0.5) == 50 and sweep.pr_num_meas(5.0, 32, 32) == 5120
