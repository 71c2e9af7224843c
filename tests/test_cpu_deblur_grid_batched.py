"""CPU-only checks of the wider trial-batched grid: the SAGA table cap of a trial slab, what `check_trials` admits with
and without `wide_trials`, the new `_pp` symbols and their argument errors."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP = ['pnp_deblur_grad_pp', 'pnp_deblur_grad_mb_pp', 'pnp_saga_table_update_pp', 'pnp_nlm2d_pp']


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_new_pp_symbols_exported_and_declared():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name in PP:
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name
    # a _pp form is its plain call with a nullable array behind the scalar that has a per-problem form
    for name, pos in (('pnp_deblur_grad', 5), ('pnp_deblur_grad_mb', 5), ('pnp_nlm2d', 10)):
        plain, pp = _native.SIGNATURES[name][1], _native.SIGNATURES[name + '_pp'][1]
        assert pp == plain[:pos] + [ctypes.c_void_p] + plain[pos:], name


def test_new_pp_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work."""
    h = _lib()
    one, al = ctypes.c_void_p(1), ctypes.c_void_p(64)            # non-NULL pointers that are never dereferenced (al: 16-byte aligned)
    assert h.pnp_deblur_grad_pp(None, one, one, None, 1.0, one, one, None) == 1
    assert h.pnp_deblur_grad_mb_pp(None, one, one, one, 1.0, one, one, None) == 1
    assert h.pnp_nlm2d_pp(one, None, 64, 64, 1, 0, 4, 5, None, 1.0, one, 0.1, one, 1.0, None, None, None, None) == 1
    assert h.pnp_nlm2d_pp(one, one, 64, 64, 1, 0, 4, 5, None, 1.0, one, 0.1, one, 1.0, None, None, None, None) == 1     # in place
    ok = (al, al, al, one, one, al, 0.1, None, 0.25, 4, 2, 4096, 0, None)
    bad = {2: None, 3: None, 9: 0, 10: 0, 11: 4098, 12: 7, 0: ctypes.c_void_p(68)}   # table, row, hist, batch, N % 4, dtype, alignment
    for pos, val in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_saga_table_update_pp(*args) == 1, pos


def test_saga_table_cap_of_a_trial_slab():
    from pnp_svrg_amd import sweep as S
    N = 256 * 256
    assert S.MAX_TABLE_BYTES == 8 * 2 ** 30
    # config 4: hist 50, f32, 256 x 256 -> 12.5 MiB per problem; 8 GiB hold 655 problems
    assert S.table_trial_cap(1, 50, N, 4) == 655
    assert S.table_trial_cap(15, 50, N, 4) == 43                  # 43 trials x 15 items = 645 problems <= 655 < 44 x 15
    assert S.table_trial_cap(15, 50, N, 8) == 21                  # float64: half as many
    assert S.table_trial_cap(2, 3, 4096, 4, 2 * 3 * 2 * 4096 * 4) == 2
    assert S.table_trial_cap(2, 3, 4096, 4, 2 * 3 * 2 * 4096 * 4 - 1) == 1
    assert S.table_trial_cap(128, 50, N, 4, 2 ** 20) == 1         # never below one trial per slab
    assert S.table_trial_cap(0, 50, N, 4, 0) == 1
    # the slabs: the smaller of the two bounds, whole trials, at least one
    assert S.trial_slabs(8, 2, 1024, 2) == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert S.trial_slabs(8, 2, 6, 5) == [(0, 3), (3, 6), (6, 8)]
    assert S.trial_slabs(3, 15, 4, 1) == [(0, 1), (1, 2), (2, 3)]
    assert S.trial_slabs(5, 3, 7, None) == S.trial_slabs(5, 3, 7) == [(0, 2), (2, 4), (4, 5)]
    assert S.trial_slabs(4, 2, 1024, 0) == [(0, 1), (1, 2), (2, 3), (3, 4)]


def _runner(wide, **kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='svrg', denoiser='tv', seeding='counter')
    a.update(kw)
    extra = dict(shared_matrix=True) if a.pop('shared', False) else {}
    return S.make_runner([], a['problem'], a['algorithm'], a['denoiser'], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding=a['seeding'],
                         wide_trials=wide, **extra)


@pytest.mark.parametrize('kw', [dict(problem='deblur'), dict(problem='deblur', seeding='generator'), dict(algorithm='saga'),
                                dict(denoiser='nlm'), dict(problem='deblur', algorithm='saga', denoiser='nlm'),
                                dict(algorithm='saga', denoiser='nlm'), dict(problem='deblur', algorithm='gd')])
def test_wide_trials_admits_deblur_saga_nlm(kw):
    _runner(True, **kw).check_trials([{'eta': 1.0, 'mini_batch_size': 3, 'sigma_modifier': 1.2}])
    with pytest.raises(ValueError, match='batch_trials'):          # the same cell without the opt-in
        _runner(False, **kw).check_trials([{'eta': 1.0}])


@pytest.mark.parametrize('kw,trial,word', [(dict(algorithm='sarah'), {'eta': 1.0}, 'sarah'), (dict(seeding='legacy'), {'eta': 1.0}, 'legacy'),
                                           (dict(problem='pr'), {'eta': 1.0}, 'shared_matrix'),
                                           (dict(problem='pr', shared=True, algorithm='saga'), {'eta': 1.0}, 'saga'),
                                           (dict(algorithm='saga'), {'hist_size': 4}, 'hist_size'), (dict(), {'T2': 3}, 'T2')])
def test_wide_trials_refusals_name_the_offender(kw, trial, word):
    with pytest.raises(ValueError, match=word):
        _runner(True, **kw).check_trials([trial])


def test_without_wide_trials_the_answers_are_unchanged():
    cases = [(dict(problem='deblur'), "batch_trials: problem 'deblur' is not supported (only 'csmri', and 'pr' with shared_matrix=True)"),
             (dict(algorithm='saga'), "batch_trials: algorithm 'saga' is not supported (only 'gd', 'sgd', 'svrg')"),
             (dict(denoiser='nlm'), "batch_trials: denoiser 'nlm' is not supported (NLMProx has no per-problem form)")]
    for kw, msg in cases:
        with pytest.raises(ValueError) as e:
            _runner(False, **kw).check_trials([{'eta': 1.0}])
        assert str(e.value) == msg
    _runner(True, problem='pr', shared=True).check_trials([{'eta': 1.0}])       # what shared_matrix admitted stays admitted
