"""pnp_pr_grad_shared (csrc/pr_shared.hip) and the shared-matrix PR grid, without a GPU: the symbols, the argument checks (they
return before anything is launched), the workspace size and what `check_trials` accepts."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pnp_pr_shared_workspace_elems', 'pnp_pr_grad_shared', 'pnp_pr_grad_shared_pp')


def _lib():
    from pnp_svrg_amd import _native
    return _native.lib()


def test_symbols_are_exported_declared_and_bound():
    from pnp_svrg_amd import _native
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _native.SIGNATURES and f' {name}(' in hdr, name
    plain, pp = _native.SIGNATURES['pnp_pr_grad_shared'][1], _native.SIGNATURES['pnp_pr_grad_shared_pp'][1]
    assert len(pp) == len(plain) + 2                            # alpha_pp, gamma_pp
    assert _lib().pnp_pr_grad_shared.argtypes == plain


def _call(lib, A=16, Y=16, W=16, W2=None, mbd=None, ind=None, M=8, N=8, batch=4, items=2, dtype=0, ws=16, out=16, div=1.0):
    return lib.pnp_pr_grad_shared(A, Y, W, W2, mbd, ind, M, N, batch, items, dtype, 1.0, div, 0.0, None, 0.0, None, ws, out, None)


@pytest.mark.parametrize('kw,text', [(dict(A=None), b'null A'), (dict(W=None), b'null argument'), (dict(out=None), b'null argument'),
                                     (dict(ws=None), b'null argument'), (dict(M=0), b'bad sizes'), (dict(N=0), b'bad sizes'),
                                     (dict(batch=0), b'bad sizes'), (dict(items=0), b'bad sizes'),
                                     (dict(batch=5, items=2), b'batch % items != 0'),
                                     (dict(mbd=16, ind=16), b'both selections given'), (dict(dtype=7), b'bad dtype')])
def test_argument_errors_return_before_any_launch(kw, text):
    lib = _lib()
    assert _call(lib, **kw) != 0
    err = lib.pnp_last_error()
    assert text in err and b'pnp_pr_grad_shared' in err, err


def test_pp_form_checks_the_same_arguments():
    lib = _lib()
    rc = lib.pnp_pr_grad_shared_pp(16, 16, 16, None, 16, 16, 8, 8, 4, 2, 0, 1.0, None, 1.0, 0.0, None, 0.0, None, None, 16, 16, None)
    assert rc != 0 and b'both selections given' in lib.pnp_last_error()


def test_workspace_size_has_its_known_value():
    lib = _lib()
    # M = 77 -> 80 padded rows; 3 problems -> 16 padded columns with or without W2; N = 96: three splits of N and of M (float64's)
    assert lib.pnp_pr_shared_workspace_elems(77, 96, 3) == 3 * 16 * 80 + 16 * 80 + 3 * 16 * 96
    # the reference size, 16 trials: 4 splits of N x 32 columns x 8192 rows, 16 x 8192 weights, 8 splits of M x 16 x 16384
    assert lib.pnp_pr_shared_workspace_elems(8192, 16384, 16) == 4 * 32 * 8192 + 16 * 8192 + 8 * 16 * 16384
    assert lib.pnp_pr_shared_workspace_elems(0, 96, 3) == 0


def _runner(problem='pr', seeding='counter', **kw):
    from pnp_svrg_amd import sweep as S
    return S.make_runner([], problem, 'svrg', 'tv', eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding=seeding, **kw)


@pytest.mark.parametrize('seeding', ['counter', 'generator'])
def test_a_shared_matrix_pr_runner_takes_trial_batches(seeding):
    _runner(seeding=seeding, shared_matrix=True).check_trials([{'eta': 1.0, 'mini_batch_size': 3}])
    from pnp_svrg_amd import sweep as S
    for alg in ('gd', 'sgd'):
        S.make_runner([], 'pr', alg, lambda: None, eta=1.0, n_inner=2, mini_batch_size=5, seeding=seeding,
                      shared_matrix=True).check_trials([{'eta': 1.0}])


def test_what_is_still_refused():
    with pytest.raises(ValueError, match='shared_matrix'):
        _runner(problem='csmri', shared_matrix=True)
    with pytest.raises(ValueError, match='legacy'):
        _runner(seeding='legacy', shared_matrix=True).check_trials([{'eta': 1.0}])
    with pytest.raises(ValueError, match="'pr'.*shared_matrix=True"):
        _runner().check_trials([{'eta': 1.0}])
    with pytest.raises(ValueError, match='deblur'):
        _runner(problem='deblur').check_trials([{'eta': 1.0}])
    with pytest.raises(ValueError, match='T2'):
        _runner(shared_matrix=True).check_trials([{'T2': 3}])
