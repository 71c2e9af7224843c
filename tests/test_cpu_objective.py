"""CPU side of the device objective f(z): the NumPy restatement the GPU tests compare against (tests/objective_ref.py) equals
the oracle's `f` -- which pins the FFT form of CSMRI to the reference's dense-DFT form, and the full-spectrum sum to masks that
are not Hermitian -- the three entry points are declared and bound, and the sweep's new arguments are checked before any device
work."""
import os
import re

import numpy as np
import pytest

import objective_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG64 = os.path.join(ROOT, 'tests', 'golden', 'synth64.png')
SYMBOLS = ('pnp_csmri_objective', 'pnp_deblur_objective', 'pnp_pr_objective')


def _img64():
    from PIL import Image
    return np.array(Image.open(IMG64).resize((64, 64)))


def _points(p, rng, near=True):
    """Where f is compared: two random images and, with `near`, the initialisation and the ground truth (f = the noise's share).
    near=False is for the oracle's CSMRI: it multiplies by a dense DFT matrix built with np.power whose product is off from fft2
    by about 3e-11 (oracle/problems.py), an error that scales with the spectrum, not with the residual.  Near the solution the
    residual is 1e2 .. 1e3 times smaller than the spectrum, and the ORACLE's own f is then good to a few 1e-12 only (seen: 2.1e-12
    at Xinit with alpha = 1.0, 1.01e-12 at the ground truth with alpha = 0.3) -- no yardstick for a 1e-12 comparison there."""
    return [rng.random(p.N), 0.25 + 0.5 * rng.random(p.N)] + ([p.Xinit, p.X] if near else [])


@pytest.mark.parametrize('alpha', [0.3, 1.0])
def test_csmri_restatement_equals_oracle_f(alpha):
    from oracle import problems as op
    np.random.seed(3)
    p = op.CSMRI(None, H=64, W=64, sample_prob=alpha, snr=20., img=_img64())
    assert alpha == 1.0 or not np.array_equal(p.mask, np.roll(p.mask[::-1, ::-1], 1, (0, 1)))      # not a Hermitian mask
    for w in _points(p, np.random.default_rng(0), near=False):
        got, want = oref.csmri_f(w, p.mask, p.Y), p.f(w)
        print(f'csmri alpha={alpha}: restatement {got:.17g} oracle {want:.17g}')
        assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize('scale_percent', [100, 50])
def test_deblur_restatement_equals_oracle_f(scale_percent):
    from oracle import problems as op
    np.random.seed(4)
    p = op.Deblur(None, H=64, W=64, kernel='Minimal', scale_percent=scale_percent, snr=20., img=_img64())
    taps = oref.deblur_taps(64, 64, scale_percent)
    assert np.array_equal(oref.minimal_kernel(64, 64), p.B) and p.Y.size == p.M == (64 * scale_percent // 100) ** 2
    for w in _points(p, np.random.default_rng(1)):
        got, want = oref.deblur_f(w, p.B, p.Y, taps), p.f(w)
        print(f'deblur scale_percent={scale_percent}: restatement {got:.17g} oracle {want:.17g}')
        assert abs(got - want) <= 1e-12 * abs(want)


def test_pr_restatement_equals_oracle_f():
    from oracle import problems as op
    np.random.seed(5)
    img = _img64()[::4, ::4]                                    # 16 x 16
    p = op.PhaseRetrieval(None, H=16, W=16, num_meas=77, snr=20., img=img)
    for w in _points(p, np.random.default_rng(2)):
        got, want = oref.pr_f(w, p.A, p.Y), p.f(w)
        assert abs(got - want) <= 1e-12 * abs(want)


def test_symbols_declared_and_bound():
    from pnp_svrg_amd import _native
    header = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    declared = set(re.findall(r'\b(pnp_\w+)\s*\(', header))
    for name in SYMBOLS + ('pnp_pr_objective_workspace_bytes',):
        assert name in declared, f'{name} is not declared in include/pnp_hip.h'
        assert name in _native.SIGNATURES, f'{name} is not bound in _native.SIGNATURES'
    # the argument lists of the header, counted
    for name in SYMBOLS:
        args = re.search(name + r'\s*\(([^;]*?)\)\s*;', header, re.S).group(1)
        assert len(args.split(',')) == len(_native.SIGNATURES[name][1])
    assert os.path.exists(os.path.join(ROOT, 'pnp_svrg_amd', 'csrc', 'objective.hip'))


def test_batches_engines_and_problems_offer_the_objective():
    import inspect
    from pnp_svrg_amd import engine as E, problems as P
    for cls in (E.CsmriBatch, E.DeblurBatch, E.PrBatch, P.CSMRI, P.Deblur, P.PhaseRetrieval):
        assert callable(getattr(cls, 'objective', None)), cls
    for cls in (E.GdEngine, E.SgdEngine, E.SvrgEngine, E.SagaEngine, E.SarahEngine):
        assert inspect.signature(cls.__init__).parameters['log_objective'].default is False
        assert callable(cls.objective_log)


def _rows(f_finals=None):
    item = {'id': 0, 'image': 0, 'alpha': 0.5, 'snr': 20.0, 'seed': 0}
    rows = []
    for t, loss in enumerate([1.0, -2.0, 0.5]):
        r = {'id': 0, 'item': item, 'loss': loss, 'psnr_init': 10.0, 'psnr_final': 10.0 - loss}
        if f_finals is not None:
            r['f_final'] = f_finals[t]
        rows.append(({'eta': float(t)}, [r]))
    return rows


def test_make_runner_rejects_unknown_objective_values():
    from pnp_svrg_amd import sweep
    for bad in ('yes', 1, None, 'psnr'):
        with pytest.raises(ValueError, match='objective'):
            sweep.make_runner([np.zeros((64, 64))], eta=1.0, n_inner=2, mini_batch_size=8, T2=2, H=64, W=64, objective=bad)
    for ok in (False, True):
        run = sweep.make_runner([np.zeros((64, 64))], eta=1.0, n_inner=2, mini_batch_size=8, T2=2, H=64, W=64, objective=ok)
        assert run.objective is ok


def test_grid_search_rejects_unknown_scores_and_rows_without_f_final():
    from pnp_svrg_amd import sweep
    items = sweep.make_items(1, [0.5], [20.0])
    images = [np.zeros((64, 64))]

    def touches_nothing(**params):
        raise AssertionError('an unknown score must be refused before a runner is made')

    with pytest.raises(ValueError, match='score'):
        sweep.grid_search(items, touches_nothing, {'eta': [1.0]}, score='f')
    with pytest.raises(ValueError, match='score'):
        sweep.best_over_trials(_rows(), score='loss')

    def plain(**params):                                        # a runner made WITHOUT objective: refused before it runs
        return sweep.make_runner(images, eta=params['eta'], n_inner=2, mini_batch_size=8, T2=2, H=64, W=64)

    for kw in ({}, {'batch_trials': True}):
        with pytest.raises(ValueError, match='objective=True'):
            sweep.grid_search(items, plain, {'eta': [1.0, 2.0]}, score='objective', **kw)
    with pytest.raises(ValueError, match='f_final'):
        sweep.best_over_trials(_rows(), score='objective')


def test_best_over_trials_by_score():
    from pnp_svrg_amd import sweep
    by_loss = sweep.best_over_trials(_rows([3.0, 2.0, 1.0]))
    assert by_loss[0]['params'] == {'eta': 1.0} and set(by_loss[0]) == {'id', 'item', 'loss', 'params', 'psnr_init', 'psnr_final'}
    by_f = sweep.best_over_trials(_rows([3.0, 2.0, 1.0]), score='objective')
    assert by_f[0]['params'] == {'eta': 2.0} and by_f[0]['f_final'] == 1.0 and by_f[0]['loss'] == 0.5
    assert sweep.best_over_trials(_rows([np.nan, 2.0, 2.0]), score='objective')[0]['params'] == {'eta': 1.0}   # NaN never wins; ties: first
