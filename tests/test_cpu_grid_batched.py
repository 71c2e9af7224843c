"""CPU-only checks of the trial-batched grid search: the `_pp` symbols, their argument errors, the pure layout functions."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = ['pnp_csmri_draw_thresholds_pp', 'pnp_draw_thresholds_pp', 'pnp_csmri_grad_sel_pp', 'pnp_csmri_svrg_step_pp',
      'pnp_csmri_svrg_outer_step_pp', 'pnp_csmri_svrg_outer_iteration_pp', 'pnp_prox_tv_pp', 'pnp_prox_wavelet2d_pp']


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_pp_symbols_exported_and_declared():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name in PP:
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name


def test_pp_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) for a NULL where a pointer is required: every check below fails before any device work."""
    h = _lib()
    one = ctypes.c_void_p(1)                                     # a non-NULL pointer that is never dereferenced
    assert h.pnp_draw_thresholds_pp(4096, 2, None, None, 1, 0, 1, None, one, None) == 1          # mb_vec is required
    assert b'null' in h.pnp_last_error()
    assert h.pnp_draw_thresholds_pp(4096, 2, one, None, 1, 0, 1, None, None, None) == 1          # so is the output
    assert h.pnp_draw_thresholds_pp(4096, 2, one, None, 1, 0, 0, None, one, None) == 1           # nsteps >= 1
    assert h.pnp_csmri_draw_thresholds_pp(None, one, one, None, 1, 0, 1, None, one, None, None) == 1
    assert h.pnp_csmri_grad_sel_pp(None, one, None, None, one, None, None, 1.0, one, None, 0.0, None, 0.0, None, None, one, None) == 1
    assert h.pnp_csmri_svrg_step_pp(None, one, None, one, 1.0, one, None, 0.0, None, 0.0, None, None, one, 1, 1.0, one, 0.0, None, None,
                                    None, None) == 1
    assert h.pnp_csmri_svrg_outer_step_pp(None, one, one, one, None, 1.0, one, one, one, one, 1, 1.0, None, 0.0, None, None, None, None) == 1
    assert h.pnp_csmri_svrg_outer_iteration_pp(None, one, one, one, one, one, one, one, 2, 1.0, one, 1, one, 1.0, None, 0.0, one, one, 0, 1,
                                               one, None) == 1
    assert h.pnp_prox_tv_pp(one, None, 64, 64, 1, 0, None, 1.0, one, 0.0, None, None, None, None) == 1     # null output
    assert h.pnp_prox_wavelet2d_pp(None, one, 64, 64, 1, 0, None, 1.0, one, 0.0, None, None, None, None) == 1
    assert h.pnp_prox_tv_pp(one, one, 60, 64, 1, 0, None, 1.0, one, 0.0, None, None, None, None) == 1       # bad H


def test_per_problem_minibatch_sizes_are_checked_on_the_host():
    """The sync-free C entry cannot read a device mb_vec: the front end checks its host copy, per problem."""
    from pnp_svrg_amd.engine import _BatchBase
    b = _BatchBase()
    b.B, b.max_mb, b.M0 = 3, 10, np.array([10, 20, 30])
    b._check_mb(np.array([10, 20, 30]))
    b._check_mb(10)
    for bad, who in (([10, 0, 5], 'problem 1'), ([10, 20, 31], 'problem 2'), ([-1, 2, 3], 'problem 0')):
        with pytest.raises(ValueError, match=who):
            b._check_mb(np.array(bad))
    with pytest.raises(ValueError, match='integers'):
        b._check_mb(np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError):
        b._check_mb(11)


def test_trial_grouping_layout_and_draw_ids():
    from pnp_svrg_amd import sweep as S
    grid = {'eta': [1.0, 2.0], 'T2': [2, 3], 'mini_batch_size': [5, 6], 'variant': ['svrg']}
    trials = S.grid_points(grid)
    groups = S.group_trials(trials)
    assert groups == [({'T2': 2, 'variant': 'svrg'}, [0, 1, 4, 5]), ({'T2': 3, 'variant': 'svrg'}, [2, 3, 6, 7])]
    assert sorted(t for _, idx in groups for t in idx) == list(range(8))
    assert S.group_trials([{'eta': 1.0}, {'eta': 2.0}]) == [({}, [0, 1])]
    # slabs: whole trials, at most max_batch_trials problems, at least one trial
    assert S.trial_slabs(5, 3, 7) == [(0, 2), (2, 4), (4, 5)]
    assert S.trial_slabs(4, 15, 1024) == [(0, 4)]
    assert S.trial_slabs(3, 15, 4) == [(0, 1), (1, 2), (2, 3)]
    # layout: b = t * n_items + i, draw_id[b] = i, a missing key takes the runner's own value
    lay = S.trial_layout(3, [{'eta': 1.0, 'mini_batch_size': 7}, {'eta': 2.0}], {'eta': 9.0, 'mini_batch_size': 4, 'sigma_modifier': 1.5})
    assert lay['draw_id'].tolist() == [0, 1, 2, 0, 1, 2]
    assert lay['eta'].tolist() == [1.0] * 3 + [2.0] * 3 and lay['eta'].dtype == np.float64
    assert lay['mini_batch_size'].tolist() == [7] * 3 + [4] * 3 and lay['mini_batch_size'].dtype == np.int32
    assert lay['sigma_modifier'].tolist() == [1.5] * 6
    for t in range(2):
        for i in range(3):
            assert lay['draw_id'][t * 3 + i] == i
    assert S.trial_layout(2, [{'eta': 1.0}], {'eta': 1.0, 'mini_batch_size': None})['mini_batch_size'] is None    # gd


def test_best_over_trials_keeps_the_first_of_tied_losses():
    from pnp_svrg_amd import sweep as S
    it = [{'id': 0}, {'id': 1}]
    row = lambda i, loss: {'id': i, 'item': it[i], 'loss': loss, 'psnr_init': 1.0, 'psnr_final': 1.0 - loss}
    per_trial = [({'eta': 1.0}, [row(0, -2.0), row(1, float('nan'))]),
                 ({'eta': 2.0}, [row(0, -3.0), row(1, -1.0)]),
                 ({'eta': 3.0}, [row(0, -3.0), row(1, -1.0)])]
    best = S.best_over_trials(per_trial)
    assert [(r['id'], r['loss'], r['params']) for r in best] == [(0, -3.0, {'eta': 2.0}), (1, -1.0, {'eta': 2.0})]
    assert S.best_over_trials(per_trial[::-1])[0]['params'] == {'eta': 3.0}      # the order of the trials decides a tie


@pytest.mark.parametrize('kw,word', [(dict(problem='pr'), 'pr'), (dict(algorithm='saga'), 'saga'), (dict(denoiser='nlm'), 'nlm'),
                                     (dict(seeding='legacy'), 'legacy')])
def test_unsupported_trial_batches_are_refused_before_any_device_work(kw, word):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='svrg', denoiser='tv', seeding='counter')
    a.update(kw)
    run = S.make_runner([], a['problem'], a['algorithm'], a['denoiser'], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding=a['seeding'])
    with pytest.raises(ValueError, match=word):
        run.check_trials([{'eta': 1.0}])
    ok = S.make_runner([], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding='counter')
    ok.check_trials([{'eta': 1.0, 'mini_batch_size': 3, 'sigma_modifier': 1.2}])
    with pytest.raises(ValueError, match='T2'):
        ok.check_trials([{'T2': 3}])
