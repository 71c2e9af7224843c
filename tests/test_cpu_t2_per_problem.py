"""CPU-only checks of per-problem T2: grouping and layout of trials, what `check_trials` admits with and without
`t2_trials`, the two symbols and their argument errors, the routing of a scalar and of a [B] T2 through the engine and `ops` (the
library replaced by a recorder, as in test_cpu_front_end.py), and the engine's host-side schedule against a NumPy restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnp_csmri_svrg_span_pp', 'pnp_refresh_pp')


# ------------------------------------------------------------------------------------------------------- trials: groups, layout
def test_group_trials_with_and_without_T2_among_the_keys():
    from pnp_svrg_amd import sweep as S
    trials = S.grid_points({'eta': [1.0, 2.0], 'T2': [2, 3, 5], 'hist_size': [7]})
    assert S.PER_PROBLEM_KEYS == ('eta', 'mini_batch_size', 'sigma_modifier')
    apart = S.group_trials(trials)                               # the default: T2 is structural, as it always was
    assert [g for g, _ in apart] == [{'T2': 2, 'hist_size': 7}, {'T2': 3, 'hist_size': 7}, {'T2': 5, 'hist_size': 7}]
    assert [idx for _, idx in apart] == [[0, 3], [1, 4], [2, 5]]
    assert S.group_trials(trials, S.PER_PROBLEM_KEYS) == apart
    one = S.group_trials(trials, S.PER_PROBLEM_KEYS + ('T2',))
    assert one == [({'hist_size': 7}, [0, 1, 2, 3, 4, 5])]


def test_trial_layout_carries_T2_as_int32_when_asked():
    from pnp_svrg_amd import sweep as S
    trials = [{'eta': 1.0, 'T2': 2}, {'eta': 2.0}, {'T2': 5, 'mini_batch_size': 9}]
    defaults = {'eta': 0.5, 'mini_batch_size': 4, 'sigma_modifier': 1.0, 'T2': 3}
    n = 4
    lay = S.trial_layout(n, trials, defaults, keys=S.PER_PROBLEM_KEYS + ('T2',))
    assert lay['T2'].dtype == np.int32 and lay['T2'].shape == (3 * n,)
    for t, want in enumerate([2, 3, 5]):
        for i in range(n):
            assert lay['T2'][t * n + i] == want and lay['draw_id'][t * n + i] == i
    assert lay['mini_batch_size'].tolist() == [4] * 8 + [9] * 4 and lay['eta'].tolist() == [1.0] * 4 + [2.0] * 4 + [0.5] * 4
    plain = S.trial_layout(n, trials, defaults)                  # not asked: no 'T2' entry, the other vectors the same
    assert 'T2' not in plain and all(np.array_equal(plain[k], lay[k]) for k in plain)


# ---------------------------------------------------------------------------------------------------------------- check_trials
def _runner(t2, **kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='svrg', denoiser='tv', seeding='counter', wide=False, shared=False, sarah=False)
    a.update(kw)
    extra = dict(shared_matrix=True) if a['shared'] else {}
    if t2 is not None:
        extra['t2_trials'] = t2
    return S.make_runner([], a['problem'], a['algorithm'], a['denoiser'], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding=a['seeding'],
                         wide_trials=a['wide'], sarah_trials=a['sarah'], **extra)


OLD_T2 = ("batch_trials: trial key 'T2' has no per-problem form here (per-problem keys: ('eta', 'mini_batch_size', 'sigma_modifier'); "
          'a prox factory takes no sigma_modifier)')


@pytest.mark.parametrize('kw', [dict(), dict(seeding='generator'), dict(wide=True), dict(problem='deblur', wide=True),
                                dict(problem='pr', shared=True), dict(problem='pr', shared=True, wide=True)])
def test_t2_trials_admits_T2_for_svrg_on_the_batches_of_batch_trials(kw):
    _runner(True, **kw).check_trials([{'eta': 1.0, 'T2': 3}, {'T2': 5, 'mini_batch_size': 3, 'sigma_modifier': 1.2}, {'eta': 2.0}])
    for off in (False, None):                                    # without the flag (None: the default): today's text
        with pytest.raises(ValueError) as e:
            _runner(off, **kw).check_trials([{'eta': 1.0, 'T2': 3}])
        assert str(e.value) == OLD_T2


@pytest.mark.parametrize('algo', ['sarah', 'saga', 'sgd', 'gd'])
@pytest.mark.parametrize('kw', [dict(), dict(wide=True, sarah=True)])
def test_t2_trials_refuses_other_algorithms_by_name(algo, kw):
    with pytest.raises(ValueError) as e:
        _runner(True, algorithm=algo, **kw).check_trials([{'eta': 1.0, 'T2': 3}])
    assert str(e.value).startswith("batch_trials: trial key 'T2' has no per-problem form for algorithm " + repr(algo))
    if algo in ('sgd', 'gd') or kw:                              # trials that do not name T2: what the runner always answered
        _runner(True, algorithm=algo, **kw).check_trials([{'eta': 1.0}])


def test_t2_trials_leaves_the_other_refusals_as_they_are():
    cases = [(dict(seeding='legacy'), "batch_trials: seeding 'legacy' is not supported (host index lists; use 'counter' or 'generator')"),
             (dict(problem='deblur'), "batch_trials: problem 'deblur' is not supported (only 'csmri', and 'pr' with shared_matrix=True)"),
             (dict(denoiser='nlm'), "batch_trials: denoiser 'nlm' is not supported (NLMProx has no per-problem form)")]
    for kw, msg in cases:
        for flag in (True, False):
            with pytest.raises(ValueError) as e:
                _runner(flag, **kw).check_trials([{'eta': 1.0, 'T2': 3}])
            assert str(e.value) == msg
    with pytest.raises(ValueError, match="trial key 'hist_size'"):
        _runner(True).check_trials([{'T2': 3, 'hist_size': 4}])


def test_grid_search_batch_T2_needs_batch_trials():
    from pnp_svrg_amd import sweep as S
    with pytest.raises(ValueError, match='batch_trials=True'):
        S.grid_search([], lambda **kw: None, {'T2': [2, 3]}, batch_T2=True)


# -------------------------------------------------------------------------------------------------------------------- symbols
def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_symbols_exported_declared_and_bound():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name in NEW:
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name
    assert len(_native.SIGNATURES[NEW[0]][1]) == 25 and len(_native.SIGNATURES[NEW[1]][1]) == 10


def test_span_kernel_loads_untouched():
    """tools/check_fused_isa.py --pp: the hand-issued loads of the two bodies inside k_svrg_span_pp's loop (and k_svrg_outer_pp's)
    are not named before a wait that covers them, on any path -- the check test_fused_loads_untouched makes for k_svrg_iter and
    k_svrg_outer."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), '--pp'], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    lines = [ln for ln in out.stdout.splitlines() if 'k_svrg_span_pp' in ln or 'k_svrg_outer_pp' in ln]
    assert len(lines) == 2 and all(' 0 violations' in ln and '288 hand-issued loads' in ln for ln in lines), out.stdout[-3000:]
    assert out.stdout.count(' 0 violations') == 14 and 'VIOLATION' not in out.stdout


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work, the call named in pnp_last_error()."""
    h = _lib()
    al, al2, al3, al4 = (ctypes.c_void_p(64 * k) for k in (1, 2, 3, 4))      # non-NULL pointers that are never dereferenced
    ok = [al, al2, al3, al4, al, 0, 12, 3, 0, None]                          # mu_new, z, mu, w, t2_vec, step, n, batch, dtype, stream
    bad = {'mu_new': (0, None), 'z': (1, None), 'mu': (2, None), 'w': (3, None), 't2_vec': (4, None), 'batch 0': (7, 0), 'batch < 0': (7, -1),
           'n % batch': (6, 13), 'dtype': (8, 5), 'mu_new is mu': (0, al3), 'step < 0': (5, -1)}
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_refresh_pp(*args) == 1, what
        assert 'pnp_refresh_pp' in h.pnp_last_error().decode(), what
    # plan, z, w, mu, mask, yh, alpha_vec, selbits, step0, n_steps, T2, t2_vec, lr, lr_pp, mb, mb_vec, sm, sm_pp, fallback, xrec, sse_log,
    # log_row0, n_log, sigma_out, stream -- the plan pointer is not read before the checks below have passed
    ok = [al, al, al2, al3, al, al, al, al, 0, 4, 3, None, 1.0, None, 5, None, 1.0, None, 0.0, al, al, 0, 8, al, None]
    bad = {'n_steps 0': (9, 0), 'n_steps < 0': (9, -3), 'T2 0, no vector': (10, 0), 'T2 < 0, no vector': (10, -2), 'step0 < 0': (8, -1),
           'mb 0, no vector': (14, 0), 'n_log': (22, 0)}
    bad.update({f'null {i}': (i, None) for i in (0, 1, 2, 3, 4, 5, 6, 7, 19, 20, 23)})
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_csmri_svrg_span_pp(*args) == 1, what
        assert 'pnp_csmri_svrg_span_pp' in h.pnp_last_error().decode(), what


# ------------------------------------------------------------------------------------- the engine on a recorder: routing, schedule
class _Prox:
    """what the streaming paths ask of a prox"""
    inplace = True

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        return z


class _Batch:
    """The batch interface the engines use, on CPU tensors, every call recorded instead of launched."""
    per_problem = True

    def __init__(self, B, n=4, dtype=torch.float64, kind='fake'):
        self.B, self.H, self.W, self.N, self.dtype, self.kind, self.max_mb = B, n, n, n * n, dtype, kind, 10 ** 6
        self.xrec, self.xinit = torch.zeros((B, n, n), dtype=dtype), torch.ones((B, n, n), dtype=dtype)
        self.device, self.calls = self.xrec.device, []

    def _check_mb(self, mb):
        pass

    def minibatches(self, n):
        from pnp_svrg_amd.batches import Minibatches
        return Minibatches.zeros(n, self.B, self.device, bits_shape=(self.W, max(1, self.H // 32)))

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        self.calls.append(('draw', step0, nsteps))
        for j in range(nsteps):
            mbs.host[j] = None

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        self.calls.append(('grad_full', out))
        return out

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        self.calls.append(('diff', j, alpha, gamma))
        return out


def _recorder(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, 'require_gpu', lambda: None)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    monkeypatch.setattr(ops, '_p', lambda t: None if t is None else ('ptr', t))    # (CPU tensors: no device pointer to take)
    return ops, calls


def test_scalar_T2_reaches_no_new_entry_point_and_a_vector_reaches_refresh_pp(monkeypatch):
    from pnp_svrg_amd.engine import SvrgEngine
    ops, calls = _recorder(monkeypatch)
    for variant in ('svrg', 'reference'):
        b = _Batch(3)
        e = SvrgEngine(b, _Prox(), 2.0, 2, 5, variant=variant)
        for _ in range(5):
            e.step()
        assert not [c for c in calls if c[0] in NEW]
        assert [c[:3] for c in b.calls if c[0] == 'draw'] == ([('draw', 0, 2), ('draw', 2, 2), ('draw', 4, 2)] if variant == 'svrg' else [])
        calls.clear()
        b = _Batch(3)
        e = SvrgEngine(b, _Prox(), 2.0, np.array([1, 2, 3]), 5, variant=variant)
        for _ in range(3):
            e.step()
        got = [c for c in calls if c[0] in NEW]
        assert [c[0] for c in got] == ['pnp_refresh_pp'] * 3
        for s, (_, a) in enumerate(got):
            mu_new, z, mu, w, t2 = (x[1] for x in a[:5])
            assert t2.dtype == torch.int32 and t2.tolist() == [1, 2, 3]
            assert mu_new is e._mu_new and mu is e.mu and w is e.w and mu_new is not mu
            assert a[5:] == (s, 3 * 16, 3, 1, 'stream') and type(a[5]) is int
        calls.clear()
        assert not e.graph_ok()
        with pytest.raises(ValueError, match='run_span'):
            e.run_outer(1)
        with pytest.raises(ValueError, match='hipGraph'):
            e.capture()


class _Csmri(_Batch):
    """A 256 x 256 f32 'csmri' batch on CPU tensors whose plan is the real front end over the recorder."""

    def __init__(self, B, ops):
        super().__init__(B, 256, torch.float32, 'csmri')
        self.plan = ops.CsmriPlan.__new__(ops.CsmriPlan)
        self.plan.H, self.plan.W, self.plan.B, self.plan.dtype, self.plan._h = 256, 256, B, torch.float32, None
        self.bits = torch.zeros((B, 256, 8), dtype=torch.int32)
        self.yh_full = torch.zeros((B, 128, 256), dtype=torch.complex64)
        self.inv_m0 = torch.ones(B, dtype=torch.float32)


def test_run_span_routes_the_vector_to_the_span_kernel_in_windows(monkeypatch):
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops)
    eta, mb = np.array([3.0, 4.0]), np.array([7, 9], np.int32)
    e = SvrgEngine(b, TVProx(sigma_modifier=1.25), eta, np.array([2, 5]), mb, fused=True, span=2, n_log=4)
    assert e.fused and e.outer_kernel_ok() and not e.graph_ok()
    for _ in range(3):                                           # three eager steps first: n_prox = 3, so the log row wraps below
        e.step()
    assert [c[0] for c in calls if c[0] in NEW] == ['pnp_refresh_pp', 'pnp_refresh_pp']          # s = 0 (both), s = 2 (T2 = 2)
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 0, 2), ('draw', 2, 2)]
    calls.clear(), b.calls.clear()
    e.run_span(5)
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 3, 2), ('draw', 5, 2), ('draw', 7, 1)] and len(b.calls) == 3
    assert [c[0] for c in calls] == ['pnp_csmri_svrg_span_pp'] * 3 and (e.s, e.n_prox, e.prox.t) == (8, 8, 8)
    for (_, a), (s0, m, row) in zip(calls, [(3, 2, 3), (5, 2, 1), (7, 1, 3)]):
        assert len(a) == 25 and a[8:11] == (s0, m, 0) and a[21:23] == (row, 4)
        assert a[11][1] is e._t2_dev and a[11][1].dtype == torch.int32 and a[11][1].tolist() == [2, 5]
        assert a[12] == 0.0 and a[13][1].tolist() == [3.0, 4.0] and a[13][1].dtype == torch.float64          # lr_pp = eta
        assert a[14] == 0 and a[15][1].tolist() == [7, 9] and a[16:19] == (1.25, None, 0.0)
        assert a[1][1] is e.z and a[2][1] is e.w and a[3][1] is e.mu and a[7][1] is e.mbs.selbits
    # a scalar T2 on the same batch: the calls it always made, none of the new ones -- stepping, run_outer, and run_span (eager steps)
    calls.clear()
    e = SvrgEngine(b, TVProx(), 3.0, 2, 7, fused=True)
    e.step(), e.step(), e.run_outer(1), e.run_span(2)
    assert [c[0] for c in calls] == ['pnp_csmri_svrg_outer_step', 'pnp_csmri_svrg_step', 'pnp_csmri_svrg_outer_iteration',
                                     'pnp_csmri_svrg_outer_step', 'pnp_csmri_svrg_step']


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
def test_host_schedule_against_a_numpy_restatement(monkeypatch, lr_decay):
    """Which steps launch a refresh (and a full gradient), and when the coefficient vectors are remade."""
    from pnp_svrg_amd.engine import SvrgEngine
    ops, calls = _recorder(monkeypatch)
    T2, eta, mb, n = np.array([1, 2, 3, 5, 8, 13]), 2.0, 4, 30
    # ---- the restatement
    steps = np.arange(n)
    k = steps[:, None] // T2[None, :]                                            # decay exponent of problem b at step s
    want_refresh = [int(s) for s in steps if (s % T2 == 0).any()]
    want_remade = [int(s) for s in steps if s == 0 or (k[s] != k[s - 1]).any()] if lr_decay != 1.0 else []
    want_gamma = [[-(eta * lr_decay ** int(kb)) for kb in k[s]] for s in steps]
    # ---- the engine
    b = _Batch(6)
    e = SvrgEngine(b, _Prox(), eta, T2, mb, lr_decay=lr_decay, span=4)
    seen, remade, last = [], [], None
    for s in range(n):
        n0 = len(b.calls)
        e.step()
        new = b.calls[n0:]
        assert [c[0] for c in new if c[0] != 'draw'] == (['grad_full', 'diff'] if s in want_refresh else ['diff'])
        _, j, alpha, gamma = new[-1]
        assert j == s % 4                                                        # the slot of step s in its window of `span` steps
        if lr_decay == 1.0:
            assert gamma == -eta and alpha == -eta / mb and type(gamma) is float     # nothing to upload: the scalars of the plain calls
            continue
        if gamma is not last:
            remade.append(s)
            last = gamma
        assert gamma.dtype == torch.float64 and gamma.tolist() == want_gamma[s]
        assert alpha.tolist() == [g / mb for g in want_gamma[s]]
    assert [a[5] for name, a in calls if name == 'pnp_refresh_pp'] == want_refresh
    assert len([c for c in b.calls if c[0] == 'grad_full']) == len(want_refresh)
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', s, 4) for s in range(0, n, 4)]
    assert remade == want_remade
    assert want_refresh == list(range(n)) and (lr_decay == 1.0 or want_remade == list(range(n)))    # (T2 = 1 is in the vector ...)
    # ... so once more without it: steps with no refresh launch nothing extra, steps with no new exponent upload nothing
    T2b = np.array([4, 6])
    b = _Batch(2)
    e = SvrgEngine(b, _Prox(), np.array([2.0, 3.0]), T2b, mb, lr_decay=lr_decay)
    calls.clear()
    ids = []
    for s in range(13):
        e.step()
        ids.append(b.calls[-1][3])
    assert [a[5] for name, a in calls if name == 'pnp_refresh_pp'] == [0, 4, 6, 8, 12]
    changes = [s for s in range(13) if s == 0 or ids[s] is not ids[s - 1]]
    assert changes == ([0, 4, 6, 8, 12] if lr_decay != 1.0 else [0])


def test_T2_vector_is_validated_naming_the_offender(monkeypatch):
    from pnp_svrg_amd.engine import SvrgEngine, SarahEngine
    _recorder(monkeypatch)
    b = _Batch(3)
    for bad, word in (([2, 3], r'shape \(2,\)'), ([[1, 2, 3]], r'shape \(1, 3\)'), ([2.0, 3.0, 4.0], 'float64'), ([2, 0, 3], 'problem 1: T2 0'),
                      ([2, 3, -4], 'problem 2: T2 -4')):
        with pytest.raises(ValueError, match=word):
            SvrgEngine(b, _Prox(), 1.0, np.array(bad), 5)
    b.per_problem = False
    with pytest.raises(ValueError, match="per-problem T2 needs a batch that takes per-problem values \\(got 'fake'\\)"):
        SvrgEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5)
    b.per_problem = True
    with pytest.raises(ValueError, match='span'):
        SvrgEngine(b, _Prox(), 1.0, 3, 5, span=4)
    with pytest.raises(ValueError, match='span'):
        SvrgEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, span=0)
    with pytest.raises(ValueError, match='scalar T2'):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5)


class _ArithBatch(_Batch):
    """`_Batch` with arithmetic: gradients that depend on z, w and on the ABSOLUTE step a slot was drawn for, so a wrong slot, a
    missed or a spurious refresh, or a wrong coefficient changes the numbers."""

    def __init__(self, B):
        super().__init__(B)
        g = torch.Generator().manual_seed(B)
        self.xinit = torch.rand((B, 4, 4), generator=g, dtype=torch.float64)
        self.xrec = torch.rand((B, 4, 4), generator=g, dtype=torch.float64)

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        super().draw(mbs, mb, seed, step0, nsteps)
        for j in range(nsteps):
            mbs.mbd[j, :, 0] = step0 + j

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        return out.copy_(0.5 * z + 0.125)

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        col = lambda v: v.reshape(-1, 1, 1) if isinstance(v, torch.Tensor) else v          # noqa: E731
        g = (z - w) * (1.0 + mbs.mbd[j, :, 0].double()).reshape(-1, 1, 1) * 0.03125
        return out.copy_(col(alpha) * g + beta * c1 + col(gamma) * c2)


class _ArithProx(_Prox):
    def __call__(self, z, xrec, sse_out):
        z.mul_(0.75)
        sse_out.copy_(((z - xrec) ** 2).sum((1, 2)))
        return z


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
@pytest.mark.parametrize('per_problem', [False, True])
def test_engine_with_a_T2_vector_walks_the_scalar_engines_trajectories_on_the_host(monkeypatch, lr_decay, per_problem):
    """The engine's own logic -- draw windows, refresh steps, decay exponents -- on a batch whose arithmetic runs on the host, with
    pnp_refresh_pp restated in three lines: rows with T2[b] == v equal the scalar-T2 = v engine, z, w, mu and the log, exactly."""
    from pnp_svrg_amd import _native
    from pnp_svrg_amd.engine import SvrgEngine
    _recorder(monkeypatch)

    def call(name, *a):
        assert name == 'pnp_refresh_pp'
        (mu_new, z, mu, w, t2), step = (x[1] for x in a[:5]), a[5]
        for p in range(z.shape[0]):
            if step % int(t2[p]) == 0:
                mu[p], w[p] = mu_new[p], z[p]
    monkeypatch.setattr(_native, 'call', call)
    T2, n = np.array([1, 2, 3, 5, 8, 13]), 29
    eta = np.array([0.5, 0.25, 0.75, 0.5, 0.25, 0.75]) if per_problem else 0.5
    mb = np.array([2, 3, 2, 3, 2, 3], np.int32) if per_problem else 2
    b = _ArithBatch(6)
    e = SvrgEngine(b, _ArithProx(), eta, T2, mb, lr_decay=lr_decay, span=5)
    e.mu.zero_(), e.w.zero_()
    for _ in range(n):
        e.step()
    for v in T2.tolist():
        r = SvrgEngine(b, _ArithProx(), eta, v, mb, lr_decay=lr_decay)
        r.mu.zero_(), r.w.zero_()
        for _ in range(n):
            r.step()
        p = T2.tolist().index(v)
        for x, y in ((e.z, r.z), (e.w, r.w), (e.mu, r.mu), (e.sse_log[:n].T, r.sse_log[:n].T)):
            assert torch.equal(x[p], y[p]), v
    assert not torch.equal(e.z[0] - b.xinit[0], e.z[5] - b.xinit[5])
