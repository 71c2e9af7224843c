"""CPU-only checks of per-problem pnp_sarah: the `pnp_axpbypcz_pp` symbol, its signature and argument errors, the
scalar / per-problem routing of `ops.axpbypcz`, and what `check_trials` admits with and without `sarah_trials`."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'pnp_axpbypcz_pp'


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_symbol_exported_declared_and_bound():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    assert hasattr(h, NAME) and NAME in _native.SIGNATURES and f'int {NAME}(' in hdr


def test_signature_is_the_plain_one_with_arrays_and_batch():
    """a nullable array (c_void_p) behind each of the three doubles, an int (batch) behind n"""
    from pnp_svrg_amd import _native
    (res, plain), (res_pp, pp) = _native.SIGNATURES['pnp_axpbypcz'], _native.SIGNATURES[NAME]
    want = []
    for t in plain:
        want.append(t)
        if t is ctypes.c_double:
            want.append(ctypes.c_void_p)
        elif t is ctypes.c_size_t:
            want.append(ctypes.c_int)
    assert plain.count(ctypes.c_double) == 3 and plain.count(ctypes.c_size_t) == 1
    assert res_pp is res and pp == want and len(pp) == len(plain) + 4


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work, the call named in pnp_last_error()."""
    h = _lib()
    al = ctypes.c_void_p(64)                                     # a non-NULL pointer that is never dereferenced
    ok = [1.0, None, al, 0.5, None, al, 0.25, None, al, al, 12, 3, 0, None]
    bad = {'x': (2, None), 'out': (9, None), 'batch 0': (11, 0), 'batch < 0': (11, -2), 'n % batch': (10, 13), 'dtype': (12, 7)}
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert getattr(h, NAME)(*args) == 1, what
        assert NAME in h.pnp_last_error().decode(), what


def _mocked(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, 'require_gpu', lambda: None)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    monkeypatch.setattr(ops, '_p', lambda t: None if t is None else ('ptr', t))    # (CPU tensors: no device pointer to take)
    return ops, calls


def test_three_scalars_take_the_plain_call_with_the_old_arguments(monkeypatch):
    ops, calls = _mocked(monkeypatch)
    x, y, w, out = (torch.zeros((3, 4, 5), dtype=torch.float32) for _ in range(4))
    ops.axpbypcz(2, x, -0.5, y, 0.25, w, out=out)
    name, args = calls.pop()
    assert name == 'pnp_axpbypcz' and len(args) == 10
    assert args[0] == 2.0 and args[2] == -0.5 and args[4] == 0.25 and all(type(args[i]) is float for i in (0, 2, 4))
    assert all(args[i][1] is t for i, t in zip((1, 3, 5, 6), (x, y, w, out)))
    assert args[7:] == (60, 0, 'stream')
    ops.axpbypcz(1.5, x.double(), out=out.double())               # defaults: b = c = 0.0, y = w = NULL
    name, args = calls.pop()
    assert name == 'pnp_axpbypcz' and args[2:6] == (0.0, None, 0.0, None) and args[7:] == (60, 1, 'stream')
    assert calls == []


@pytest.mark.parametrize('where', [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)])
def test_a_tensor_in_any_position_takes_the_pp_call(monkeypatch, where):
    ops, calls = _mocked(monkeypatch)
    B = 3
    x, y, w, out = (torch.zeros((B, 4, 5), dtype=torch.float64) for _ in range(4))
    coef = [2.0, -0.5, 0.25]
    vec = {i: torch.full((B,), 1.0 + i, dtype=torch.float64) for i in where}
    a, b, c = (vec.get(i, coef[i]) for i in range(3))
    ops.axpbypcz(a, x, b, y, c, w, out=out)
    name, args = calls.pop()
    assert name == 'pnp_axpbypcz_pp' and len(args) == 14 and calls == []
    for i in range(3):                                           # (scalar, array) pairs at 0, 3, 6
        s, arr = args[3 * i], args[3 * i + 1]
        if i in where:
            assert s == 0.0 and arr[0] == 'ptr' and arr[1] is vec[i]
        else:
            assert s == coef[i] and type(s) is float and arr is None
    assert all(args[i][1] is t for i, t in zip((2, 5, 8, 9), (x, y, w, out)))
    assert args[10:] == (B * 20, B, 1, 'stream') and type(args[11]) is int


def test_a_coefficient_tensor_must_match_the_leading_dimension(monkeypatch):
    ops, calls = _mocked(monkeypatch)
    x = torch.zeros((3, 8), dtype=torch.float32)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float32), torch.zeros((3, 1), dtype=torch.float64)):
        with pytest.raises(AssertionError, match='per-problem values'):
            ops.axpbypcz(1.0, x, bad, x, out=x)
    assert calls == []


# ---------------------------------------------------------------------------------------------------------- check_trials
def _runner(sarah, **kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='sarah', denoiser='tv', seeding='counter', wide=False, shared=False)
    a.update(kw)
    extra = dict(shared_matrix=True) if a['shared'] else {}
    if sarah is not None:
        extra['sarah_trials'] = sarah
    return S.make_runner([], a['problem'], a['algorithm'], a['denoiser'], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding=a['seeding'],
                         wide_trials=a['wide'], **extra)


TRIAL = {'eta': 1.0, 'mini_batch_size': 3, 'sigma_modifier': 1.2}


@pytest.mark.parametrize('kw', [dict(), dict(seeding='generator'), dict(wide=True), dict(problem='deblur', wide=True),
                                dict(problem='deblur', wide=True, denoiser='nlm'), dict(wide=True, denoiser='nlm'),
                                dict(problem='pr', shared=True), dict(problem='pr', shared=True, wide=True)])
def test_sarah_trials_admits(kw):
    _runner(True, **kw).check_trials([TRIAL, {'eta': 2.0}])
    for off in (False, None):                                    # the same cell without the opt-in (None: the default)
        with pytest.raises(ValueError, match='sarah'):
            _runner(off, **kw).check_trials([{'eta': 1.0}])


@pytest.mark.parametrize('kw,trial,word', [(dict(seeding='legacy'), {'eta': 1.0}, 'legacy'), (dict(), {'T2': 3}, 'T2'),
                                           (dict(problem='deblur'), {'eta': 1.0}, 'deblur'),
                                           (dict(problem='pr'), {'eta': 1.0}, 'shared_matrix'),
                                           (dict(denoiser='nlm'), {'sigma_modifier': 1.2}, 'nlm')])
def test_sarah_trials_refusals_name_the_offender(kw, trial, word):
    with pytest.raises(ValueError, match=word) as e:
        _runner(True, **kw).check_trials([trial])
    assert str(e.value).startswith('batch_trials:')


def test_sarah_trials_admits_nothing_else():
    """The other algorithms' answers do not move with the opt-in."""
    for kw in (dict(algorithm='saga'), dict(algorithm='saga', problem='pr', shared=True, wide=True)):
        with pytest.raises(ValueError, match='saga'):
            _runner(True, **kw).check_trials([{'eta': 1.0}])
    _runner(True, algorithm='svrg').check_trials([TRIAL])
    _runner(True, algorithm='saga', wide=True).check_trials([TRIAL])


def test_without_sarah_trials_the_answers_are_unchanged():
    cases = [(dict(problem='deblur', algorithm='svrg'), "batch_trials: problem 'deblur' is not supported (only 'csmri', and 'pr' with shared_matrix=True)"),
             (dict(algorithm='saga'), "batch_trials: algorithm 'saga' is not supported (only 'gd', 'sgd', 'svrg')"),
             (dict(algorithm='svrg', denoiser='nlm'), "batch_trials: denoiser 'nlm' is not supported (NLMProx has no per-problem form)"),
             (dict(), "batch_trials: algorithm 'sarah' is not supported (only 'gd', 'sgd', 'svrg')"),
             (dict(wide=True), "batch_trials: algorithm 'sarah' is not supported on problem 'csmri' (wide_trials: 'gd', 'sgd', 'svrg', and "
                               "'saga' on 'csmri' or 'deblur'; SarahEngine has no per-problem form)")]
    for kw, msg in cases:
        for off in (False, None):
            with pytest.raises(ValueError) as e:
                _runner(off, **kw).check_trials([{'eta': 1.0}])
            assert str(e.value) == msg
