"""CPU-only checks of per-problem hist_size for pnp_saga: grouping and layout of trials, what `check_trials` admits with
and without `hist_trials`, the table cap of a slab, the three symbols and their argument errors, the routing of a scalar and of a [B]
hist_size through SagaEngine and `ops` (the library replaced by a recorder, as in test_cpu_t2_per_problem.py), the per-distinct-value
row streams, the validation errors, and the engine's logic on a batch whose arithmetic runs on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnp_saga_table_update_hist_pp', 'pnp_csmri_saga_step_hist_pp', 'pnp_csmri_saga_span_hist')
HIST = np.array([1, 2, 3, 5, 8, 13])


# ------------------------------------------------------------------------------------------------------- trials: groups, layout
def test_group_trials_with_and_without_hist_size_among_the_keys():
    from pnp_svrg_amd import sweep as S
    trials = S.grid_points({'eta': [1.0, 2.0], 'hist_size': [5, 8, 12]})
    assert S.PER_PROBLEM_KEYS == ('eta', 'mini_batch_size', 'sigma_modifier')
    apart = S.group_trials(trials)                               # the default: hist_size is structural, as it always was
    assert [g for g, _ in apart] == [{'hist_size': 5}, {'hist_size': 8}, {'hist_size': 12}]
    assert [idx for _, idx in apart] == [[0, 3], [1, 4], [2, 5]]
    assert S.group_trials(trials, S.PER_PROBLEM_KEYS) == apart
    assert S.group_trials(trials, S.PER_PROBLEM_KEYS + ('hist_size',)) == [({}, [0, 1, 2, 3, 4, 5])]


def test_trial_layout_carries_hist_size_as_int32_when_asked():
    from pnp_svrg_amd import sweep as S
    trials = [{'eta': 1.0, 'hist_size': 5}, {'eta': 2.0}, {'hist_size': 15, 'mini_batch_size': 9}]
    defaults = {'eta': 0.5, 'mini_batch_size': 4, 'sigma_modifier': 1.0, 'hist_size': 7}
    n = 4
    lay = S.trial_layout(n, trials, defaults, keys=S.PER_PROBLEM_KEYS + ('hist_size',))
    assert lay['hist_size'].dtype == np.int32 and lay['hist_size'].tolist() == [5] * n + [7] * n + [15] * n
    assert lay['draw_id'].tolist() == list(range(n)) * 3
    assert lay['mini_batch_size'].tolist() == [4] * 8 + [9] * 4 and lay['eta'].tolist() == [1.0] * 4 + [2.0] * 4 + [0.5] * 4
    plain = S.trial_layout(n, trials, defaults)                  # not asked: no 'hist_size' entry, the other vectors the same
    assert 'hist_size' not in plain and all(np.array_equal(plain[k], lay[k]) for k in plain)


# ---------------------------------------------------------------------------------------------------------------- check_trials
def _runner(hist, **kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='saga', denoiser='tv', seeding='counter', wide=True, shared=False)
    a.update(kw)
    extra = dict(shared_matrix=True) if a['shared'] else {}
    if hist is not None:
        extra['hist_trials'] = hist
    return S.make_runner([], a['problem'], a['algorithm'], a['denoiser'], eta=1.0, n_inner=2, mini_batch_size=5, T2=2, hist_size=6,
                         seeding=a['seeding'], wide_trials=a['wide'], **extra)


OLD_HIST = ("batch_trials: trial key 'hist_size' has no per-problem form here (per-problem keys: ('eta', 'mini_batch_size', "
            "'sigma_modifier'); a prox factory takes no sigma_modifier)")


@pytest.mark.parametrize('kw', [dict(), dict(seeding='generator'), dict(problem='deblur'), dict(problem='deblur', denoiser='nlm')])
def test_hist_trials_admits_hist_size_for_saga_on_the_batches_of_batch_trials(kw):
    _runner(True, **kw).check_trials([{'eta': 1.0, 'hist_size': 5}, {'hist_size': 15, 'mini_batch_size': 3, 'sigma_modifier': 1.2},
                                      {'eta': 2.0}])
    for off in (False, None):                                    # without the flag (None: the default): today's text
        with pytest.raises(ValueError) as e:
            _runner(off, **kw).check_trials([{'eta': 1.0, 'hist_size': 5}])
        assert str(e.value) == OLD_HIST


@pytest.mark.parametrize('algo', ['svrg', 'sgd', 'gd'])
def test_hist_trials_refuses_other_algorithms_by_name(algo):
    with pytest.raises(ValueError) as e:
        _runner(True, algorithm=algo).check_trials([{'eta': 1.0, 'hist_size': 5}])
    assert str(e.value).startswith("batch_trials: trial key 'hist_size' has no per-problem form for algorithm " + repr(algo))
    _runner(True, algorithm=algo).check_trials([{'eta': 1.0}])   # trials that do not name it: what the runner always answered


def test_hist_trials_leaves_the_other_refusals_as_they_are():
    cases = [(dict(seeding='legacy'), "batch_trials: seeding 'legacy' is not supported (host index lists; use 'counter' or 'generator')"),
             (dict(wide=False), "batch_trials: algorithm 'saga' is not supported (only 'gd', 'sgd', 'svrg')"),
             (dict(problem='deblur', wide=False),
              "batch_trials: problem 'deblur' is not supported (only 'csmri', and 'pr' with shared_matrix=True)"),
             (dict(problem='pr', shared=True),
              "batch_trials: algorithm 'saga' is not supported on problem 'pr' (wide_trials: 'gd', 'sgd', 'svrg', and 'saga' on 'csmri' "
              "or 'deblur'; SarahEngine has no per-problem form)")]
    for kw, msg in cases:
        for flag in (True, False):
            with pytest.raises(ValueError) as e:
                _runner(flag, **kw).check_trials([{'eta': 1.0, 'hist_size': 5}])
            assert str(e.value) == msg
    with pytest.raises(ValueError, match="trial key 'T2'"):
        _runner(True).check_trials([{'T2': 3, 'hist_size': 4}])


def test_grid_search_batch_hist_needs_batch_trials():
    from pnp_svrg_amd import sweep as S
    with pytest.raises(ValueError, match='batch_trials=True'):
        S.grid_search([], lambda **kw: None, {'hist_size': [5, 8]}, batch_hist=True)


def test_table_trial_cap_takes_the_largest_hist_size_of_the_trials(monkeypatch):
    """The table of a slab is dense over its largest hist_size: with hist_trials the cap is computed from the largest value the trials
    name (the runner's own where a trial names none); without it from the runner's, as always."""
    from pnp_svrg_amd import sweep as S
    seen = []
    real = S.table_trial_cap

    def cap(n_items, hist_size, *a):
        seen.append((n_items, hist_size))
        return real(n_items, hist_size, *a)
    monkeypatch.setattr(S, 'table_trial_cap', cap)

    class _Data:
        items = [{'id': 0}, {'id': 1}, {'id': 2}]
    monkeypatch.setattr(S, 'trial_slabs', lambda *a: [])         # (no slab runs: the cap is what is looked at)
    _runner(True).run_trials([_Data()], [{'eta': 1.0, 'hist_size': 5}, {'hist_size': 15}, {'eta': 2.0}])
    _runner(True).run_trials([_Data()], [{'eta': 1.0, 'hist_size': 5}, {'eta': 2.0}])          # (6: the runner's hist_size)
    _runner(None).run_trials([_Data()], [{'eta': 1.0}])
    assert seen == [(3, 15), (3, 6), (3, 6)]
    assert real(3, 15, 256 * 256, 4, 8 * 2 ** 30) == 728 and real(3, 5, 256 * 256, 4, 8 * 2 ** 30) == 2184


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
    assert [len(_native.SIGNATURES[n][1]) for n in NEW] == [15, 25, 27]
    for old, new in (('pnp_saga_table_update_pp', NEW[0]), ('pnp_csmri_saga_step_pp', NEW[1]), ('pnp_csmri_saga_span', NEW[2])):
        assert len(_native.SIGNATURES[new][1]) == len(_native.SIGNATURES[old][1]) + 1


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work, the call named in pnp_last_error(): everything pnp_saga_table_update_pp rejects."""
    h = _lib()
    al, al2, al3, al4, al5 = (ctypes.c_void_p(64 * k) for k in (1, 2, 3, 4, 5))   # non-NULL aligned pointers that are never dereferenced
    # z, g, table, row, prev_row, sum, lr, lr_pp, inv_hist, inv_hist_pp, hist, batch, N, dtype, stream
    ok = [al, al2, al3, al4, al4, al5, 1.0, None, 0.5, al, 3, 2, 16, 0, None]
    bad = {'z': (0, None), 'g': (1, None), 'table': (2, None), 'row': (3, None), 'prev_row': (4, None), 'sum': (5, None), 'hist 0': (10, 0),
           'batch 0': (11, 0), 'batch > 65535': (11, 65536), 'N 0': (12, 0), 'N % 4': (12, 18), 'dtype': (13, 5),
           'z misaligned': (0, ctypes.c_void_p(68)), 'g misaligned': (1, ctypes.c_void_p(136)), 'table misaligned': (2, ctypes.c_void_p(196)),
           'sum misaligned': (5, ctypes.c_void_p(324))}
    for what, (pos, val) in bad.items():
        for name in ('pnp_saga_table_update_hist_pp', 'pnp_saga_table_update_pp'):           # the same answers as the call it extends
            args = list(ok)
            args[pos] = val
            if name == 'pnp_saga_table_update_pp':
                del args[9]
            assert getattr(h, name)(*args) == 1, (name, what)
            assert name in h.pnp_last_error().decode(), (name, what)
    # the fused forms: what the calls they extend reject before the plan is read (the checks are the shared ones)
    step = [al, al, al, al, 1.0, None, None, al2, al, al, al3, 1.0, None, 0.5, al, 3, al4, 1, 1.0, None, 0.0, al, al, al, None]
    for what, (pos, val) in {**{f'null {i}': (i, None) for i in (0, 1, 2, 3, 7, 8, 9, 10, 16)}}.items():
        args = list(step)
        args[pos] = val
        assert h.pnp_csmri_saga_step_hist_pp(*args) == 1, what
    span = [al, al, al, al, 1.0, None, None, al2, al, al, al3, 1.0, None, 0.5, al, 3, 1, 1.0, None, 0.0, al, 4, al, 0, 8, al, None]
    for what, (pos, val) in {**{f'null {i}': (i, None) for i in (0, 1, 2, 3, 7, 8, 9, 10, 20, 22, 25)}, 'hist 0': (15, 0), 'n_steps 0': (21, 0),
                             'log_row0 < 0': (23, -1), 'n_log 0': (24, 0), 'denoise 0': (16, 0)}.items():
        args = list(span)
        args[pos] = val
        assert h.pnp_csmri_saga_span_hist(*args) == 1, what


def test_fused_hist_kernels_loads_untouched():
    """tools/check_fused_isa.py --hist: the hand-issued loads and stores of k_saga_iter_hist (denoise on and off) and of
    k_saga_span_hist obey the rules the check holds k_saga_iter and k_saga_span to, and there are as many of them."""
    import subprocess
    import sys
    tool = os.path.join(ROOT, 'tools', 'check_fused_isa.py')
    with __import__('tempfile').TemporaryDirectory() as td:
        lst = os.path.join(td, 'fused.s')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'hip_listing.py'), 'csmri_fused.hip', '-o', lst], check=True, timeout=1500)
        out = {f: subprocess.run([sys.executable, tool, f, lst], capture_output=True, text=True, timeout=300) for f in ('--hist', '--steps', '--spans')}
    for f, o in out.items():
        assert o.returncode == 0 and 'VIOLATION' not in o.stdout, f + o.stdout[-3000:] + o.stderr[-1000:]
    counts = lambda text, name: sorted(ln.split(': ', 1)[1].split(' stores,')[0] for ln in text.splitlines() if name in ln)      # noqa: E731
    got = counts(out['--hist'].stdout, 'k_saga_iter_hist')
    assert len(got) == 2 and got == counts(out['--steps'].stdout, '11k_saga_iter')
    got = counts(out['--hist'].stdout, 'k_saga_span_hist')
    assert len(got) == 1 and got == counts(out['--spans'].stdout, '11k_saga_span')
    assert out['--hist'].stdout.count(' 0 violations') == 3


# ------------------------------------------------------------------------------------- the engine on a recorder: routing, rows
class _Prox:
    """what the streaming paths ask of a prox"""
    inplace = True

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        return z


class _Batch:
    """The batch interface SagaEngine uses, on CPU tensors, every call recorded instead of launched."""
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

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        self.calls.append(('grad_stoch', j))
        return out


def _recorder(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, 'require_gpu', lambda: None)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    monkeypatch.setattr(ops, '_p', lambda t: None if t is None else ('ptr', t))    # (CPU tensors: no device pointer to take)
    return ops, calls


def test_scalar_hist_size_makes_the_calls_of_today_and_a_vector_reaches_the_new_entry(monkeypatch):
    from pnp_svrg_amd.engine import SagaEngine
    ops, calls = _recorder(monkeypatch)
    b = _Batch(3)
    e = SagaEngine(b, _Prox(), 2.0, 5, hist_size=4, seed=3)
    assert e.hist == 4 and e.hist_pp is None and tuple(e.table.shape) == (4, 3, 4, 4)
    for _ in range(3):
        e.step()
    e.step(r=np.array([0, 1, 2]))                                # per-problem rows: the batched update, as always
    e.step(r=2)
    assert [c[0] for c in calls] == ['pnp_axpbypcz'] + ['pnp_saga_table_update'] * 3 + ['pnp_saga_table_update_pp'] * 2
    assert calls[0][1][0] == 4.0 and type(calls[0][1][0]) is float
    want = np.random.default_rng(3 + 977)
    prev = 0
    for _, a in calls[1:4]:                                      # z, g, slot, prev, sum, lr, inv_hist, n, dtype, stream
        r = int(want.integers(4))
        assert a[2][1].data_ptr() == e.table[r].data_ptr() and a[3][1].data_ptr() == e.table[prev].data_ptr()
        assert a[5:] == (2.0, 0.25, 48, 1, 'stream') and type(a[6]) is float
        prev = r
    for _, a in calls[4:]:                                       # ..., lr, lr_pp, inv_hist, hist, batch, N, dtype, stream
        assert a[6:] == (2.0, None, 0.25, 4, 3, 16, 1, 'stream')
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 0xFFFFFFFF, 1), ('draw', 0, 16)]
    # ---- the vector
    calls.clear()
    b = _Batch(3)
    e = SagaEngine(b, _Prox(), 2.0, 5, hist_size=np.array([2, 7, 3]), seed=3)
    assert e.hist == 7 and e.hist_pp.tolist() == [2, 7, 3] and tuple(e.table.shape) == (7, 3, 4, 4)
    assert calls[0][0] == 'pnp_axpbypcz_pp' and calls[0][1][1][1].tolist() == [2.0, 7.0, 3.0] and calls[0][1][1][1].dtype == torch.float64
    calls.clear()
    gens = {h: np.random.default_rng(3 + 977) for h in (2, 7, 3)}
    prev = [0, 0, 0]
    for s in range(4):
        e.step()
        (name, a), = calls
        calls.clear()
        rows = [int(gens[h].integers(h)) for h in (2, 7, 3)]
        # z, g, table, row, prev_row, sum, lr, lr_pp, inv_hist, inv_hist_pp, hist, batch, N, dtype, stream
        assert name == 'pnp_saga_table_update_hist_pp' and len(a) == 15
        assert a[2][1] is e.table and a[3][1].dtype == torch.int32 and a[3][1].tolist() == rows and a[4][1].tolist() == prev
        assert a[6:9] == (2.0, None, 1.0 / 7) and a[10:] == (7, 3, 16, 1, 'stream')
        assert a[9][1] is e._inv_hist_pp and a[9][1].dtype == torch.float64 and a[9][1].tolist() == [1.0 / 2, 1.0 / 7, 1.0 / 3]
        prev = rows
    with pytest.raises(NotImplementedError):
        e.reset()


class _Csmri(_Batch):
    """A 256 x 256 f32 'csmri' batch on CPU tensors whose plan is the real front end over the recorder."""

    def __init__(self, B, ops):
        super().__init__(B, 256, torch.float32, 'csmri')
        self.plan = ops.CsmriPlan.__new__(ops.CsmriPlan)
        self.plan.H, self.plan.W, self.plan.B, self.plan.dtype, self.plan._h = 256, 256, B, torch.float32, None
        self.YT = torch.zeros((B, 256, 256), dtype=torch.complex64)


def test_fused_step_and_run_span_route_the_vector_and_a_scalar_as_today(monkeypatch):
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops)
    e = SagaEngine(b, TVProx(sigma_modifier=1.25), 3.0, 7, hist_size=np.array([2, 5]), seed=1, fused=True, n_log=8)
    calls.clear()
    e.step()
    (name, a), = calls
    assert name == 'pnp_csmri_saga_step_hist_pp' and len(a) == 25 and a[13] == 1.0 / 5 and a[15] == 5
    assert a[14][1] is e._inv_hist_pp and a[14][1].tolist() == [0.5, 0.2] and a[7][1] is e.table and a[1][1] is e.z and a[16][1] is e.z
    calls.clear(), b.calls.clear()
    assert e.span_kernel_ok()
    e.run_span(20)                                               # AHEAD = 16: two launches
    assert [c[0] for c in calls] == ['pnp_csmri_saga_span_hist'] * 2 and (e.s, e.n_prox, e.prox.t) == (21, 21, 21)
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 1, 16), ('draw', 17, 4)]
    gens = {h: np.random.default_rng(1 + 977) for h in (2, 5)}
    rows = np.array([[int(gens[h].integers(h)) for h in (2, 5)] for _ in range(21)])
    for (_, a), (i0, m, row0) in zip(calls, [(1, 16, 1), (17, 4, 1)]):
        assert len(a) == 27 and a[8][1].tolist() == rows[i0:i0 + m].tolist() and a[9][1].tolist() == rows[i0 - 1].tolist()
        assert a[14][1] is e._inv_hist_pp and a[13] == 1.0 / 5 and a[15:17] == (5, 1) and a[21] == m and a[23:25] == (row0, 8)
    assert e.r_prev.tolist() == rows[-1].tolist() and e._rows[0] is e.r_prev and e._rows[1].tolist() == rows[-1].tolist()
    # a scalar hist_size on the same batch: the calls it always made, none of the new ones
    calls.clear()
    e = SagaEngine(b, TVProx(), 3.0, 7, hist_size=5, seed=1, fused=True)
    e.step(), e.step(r=np.array([1, 2])), e.run_span(3), e.run_span(2, r=np.array([[0, 1], [2, 3]]))
    assert [c[0] for c in calls] == ['pnp_axpbypcz', 'pnp_csmri_saga_step', 'pnp_csmri_saga_step', 'pnp_csmri_saga_span', 'pnp_csmri_saga_span']
    assert not [c for c in calls if c[0] in NEW]


@pytest.mark.parametrize('fused', [False, True])
def test_row_streams_per_distinct_value_equal_the_scalar_engines(monkeypatch, fused):
    """step() and run_span(r=None): problem b takes, step for step, the row a scalar engine of the same seed with hist_size = hist[b]
    draws -- read from the row vectors that reach the entry points."""
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    hist, n = np.array([5, 1, 13, 5, 8, 13]), 23

    def rows_of(engine_calls, B):
        out = []
        for name, a in engine_calls:
            if name == 'pnp_saga_table_update':                  # scalar row: the slot is a view of table[r]
                out.append([int((a[2][1].data_ptr() - e.table.data_ptr()) // (e.table[0].numel() * e.table.element_size()))] * B)
            elif name in ('pnp_saga_table_update_pp', 'pnp_saga_table_update_hist_pp'):
                out.append(a[3][1].tolist())
            elif name in ('pnp_csmri_saga_step', 'pnp_csmri_saga_step_pp', 'pnp_csmri_saga_step_hist_pp'):
                out.append(a[7 if name == 'pnp_csmri_saga_step' else 8][1].tolist())          # (the plain call has no alpha_pp)
            elif name in ('pnp_csmri_saga_span', 'pnp_csmri_saga_span_hist'):
                out += a[8][1].tolist()
        return np.array(out)

    def walk(hs):
        nonlocal e
        b = _Csmri(6, ops) if fused else _Batch(6)
        e = SagaEngine(b, TVProx() if fused else _Prox(), 2.0, 5, hist_size=hs, seed=11, fused=fused)
        calls.clear()
        for _ in range(3):
            e.step()
        e.run_span(n - 5)                                        # (fused: span launches; streaming: eager steps)
        e.step(), e.step()
        return rows_of(list(calls), 6)
    e = None
    got = walk(hist)
    assert got.shape == (n, 6)
    for h in sorted(set(hist.tolist())):
        want = walk(int(h))
        for p in np.flatnonzero(hist == h):
            assert np.array_equal(got[:, p], want[:, p]), (h, p)
        assert want.max() < h
    assert (got < hist).all() and got[:, 2].max() >= 8           # (every problem stays below its own bound; 13 uses its range)


def test_hist_size_vector_and_rows_are_validated_naming_the_problem(monkeypatch):
    from pnp_svrg_amd.engine import SagaEngine, TVProx, make_engine
    ops, _ = _recorder(monkeypatch)
    b = _Batch(3)
    for bad, word in (([2, 3], r'shape \(2,\)'), ([[1, 2, 3]], r'shape \(1, 3\)'), ([2.0, 3.0, 4.0], 'float64'),
                      ([2, 0, 3], 'problem 1: hist_size 0'), ([2, 3, -4], 'problem 2: hist_size -4')):
        with pytest.raises(ValueError, match=word):
            SagaEngine(b, _Prox(), 1.0, 5, hist_size=np.array(bad))
    b.per_problem = False
    with pytest.raises(ValueError, match="per-problem hist_size needs a batch that takes per-problem values \\(got 'fake'\\)"):
        SagaEngine(b, _Prox(), 1.0, 5, hist_size=np.array([2, 3, 4]))
    b.per_problem = True
    e = make_engine(b, _Prox(), 1.0, None, 5, algorithm='saga', hist_size=np.array([2, 3, 4]))      # make_engine passes the array through
    assert e.hist_pp.tolist() == [2, 3, 4]
    e.step(r=1), e.step(r=np.array([1, 2, 3]))
    for r, word in ((2, r'problem 0: rows in \[0, 2\), got 2'), (np.array([1, 3, 3]), r'problem 1: rows in \[0, 3\), got 3'),
                    (np.array([0, 0, -1]), r'problem 2: rows in \[0, 4\), got -1'), (4, r'problem 0: rows in \[0, 2\), got 4')):
        with pytest.raises(ValueError, match=word):
            e.step(r=r)
    assert e.s == 2
    for fused in (False, True):                                  # run_span: [n] and [n][B] rows, eager and in span launches
        bb = _Csmri(3, ops) if fused else b
        e = SagaEngine(bb, TVProx() if fused else _Prox(), 1.0, 5, hist_size=np.array([2, 3, 4]), fused=fused)
        e.run_span(2, r=np.array([1, 0])), e.run_span(2, r=np.array([[1, 2, 3], [0, 0, 0]]))
        with pytest.raises(ValueError, match=r'problem 0: rows in \[0, 2\), got 2'):
            e.run_span(2, r=np.array([1, 2]))
        with pytest.raises(ValueError, match=r'problem 1: rows in \[0, 3\), got 3'):
            e.run_span(2, r=np.array([[1, 2, 3], [1, 3, 3]]))
        with pytest.raises(ValueError, match='run_span: r holds one row per step'):
            e.run_span(2, r=np.array([[1, 2], [1, 3]]))


# ------------------------------------------------------------------------------------------ the engine's logic, arithmetic on the host
class _ArithBatch(_Batch):
    """`_Batch` with arithmetic: minibatch gradients that depend on z, on the problem and on the ABSOLUTE step a slot was drawn for."""

    def __init__(self, B):
        super().__init__(B)
        g = torch.Generator().manual_seed(7)
        self.xinit = torch.rand((B, 4, 4), generator=g, dtype=torch.float64)
        self.xrec = torch.rand((B, 4, 4), generator=g, dtype=torch.float64)

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        super().draw(mbs, mb, seed, step0, nsteps)
        for j in range(nsteps):
            mbs.mbd[j, :, 0] = (step0 + j) % 1009

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        col = alpha.reshape(-1, 1, 1) if isinstance(alpha, torch.Tensor) else alpha
        return out.copy_(col * (0.5 * z + 0.125 * self.xrec) * (1.0 + mbs.mbd[j, :, 0].double()).reshape(-1, 1, 1) * 0.03125)


class _ArithProx(_Prox):
    def __call__(self, z, xrec, sse_out):
        z.mul_(0.75)
        sse_out.copy_(((z - xrec) ** 2).sum((1, 2)))
        return z


def _host_saga(monkeypatch):
    """`_native.call` restated on CPU tensors: the combine and the three table updates, one expression for all of them."""
    from pnp_svrg_amd import _native

    def update(z, g, slot, prev, tsum, lr, inv):
        old, pv = slot.clone(), prev.clone()
        s = tsum + g - old
        z.sub_(lr * ((g - pv) + s * inv))
        slot.copy_(g), tsum.copy_(s)

    def call(name, *a):
        t = lambda x: x[1]                                                         # noqa: E731
        if name == 'pnp_axpbypcz':
            t(a[6]).copy_(a[0] * t(a[1]))
        elif name == 'pnp_axpbypcz_pp':
            t(a[9]).copy_(t(a[1]).reshape(-1, 1, 1) * t(a[2]))
        elif name == 'pnp_saga_table_update':
            update(t(a[0]), t(a[1]), t(a[2]), t(a[3]), t(a[4]), a[5], a[6])
        elif name in ('pnp_saga_table_update_pp', 'pnp_saga_table_update_hist_pp'):
            z, g, table, row, prev, tsum = (t(x) for x in a[:6])
            inv_pp = a[9] if name.endswith('hist_pp') else None
            for p in range(z.shape[0]):
                lr = a[6] if a[7] is None else float(t(a[7])[p])
                inv = a[8] if inv_pp is None else float(t(inv_pp)[p])
                update(z[p], g[p], table[int(row[p]), p], table[int(prev[p]), p], tsum[p], lr, inv)
        else:
            raise AssertionError(name)
    monkeypatch.setattr(_native, 'call', call)


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
@pytest.mark.parametrize('per_problem', [False, True])
def test_engine_with_a_hist_vector_walks_the_scalar_engines_trajectories_on_the_host(monkeypatch, lr_decay, per_problem):
    """The engine's own logic -- table rows, initial sums, divisors, row streams -- on a batch whose arithmetic runs on the host: problem
    b equals the scalar engine with hist_size = hist[b], z, its log column, its tsum and rows [0, hist[b]) of its table, exactly; the
    rows beyond are never written, and never read (they are poisoned with NaN after the fill)."""
    from pnp_svrg_amd.engine import SagaEngine
    _recorder(monkeypatch)
    _host_saga(monkeypatch)
    n = 29
    eta = np.array([0.5, 0.25, 0.75, 0.5, 0.25, 0.75]) if per_problem else 0.5
    mb = np.array([2, 3, 2, 3, 2, 3], np.int32) if per_problem else 2
    b = _ArithBatch(6)
    e = SagaEngine(b, _ArithProx(), eta, mb, hist_size=HIST, lr_decay=lr_decay, seed=5)
    g0 = e.table[0].clone()
    assert tuple(e.table.shape) == (13, 6, 4, 4)
    for p, h in enumerate(HIST):
        assert torch.equal(e.tsum[p], float(h) * g0[p])
        e.table[h:, p] = float('nan')
    for _ in range(n - 9):
        e.step()
    e.run_span(9)
    assert not torch.isnan(e.z).any() and not torch.isnan(e.tsum).any()
    for p, h in enumerate(HIST.tolist()):
        r = SagaEngine(b, _ArithProx(), eta, mb, hist_size=h, lr_decay=lr_decay, seed=5)
        for _ in range(n):
            r.step()
        assert torch.equal(e.z[p], r.z[p]) and torch.equal(e.tsum[p], r.tsum[p]), h
        assert torch.equal(e.sse_log[:n, p], r.sse_log[:n, p]) and torch.equal(e.table[:h, p], r.table[:, p]), h
        assert torch.isnan(e.table[h:, p]).all()
    assert not torch.equal(e.z[0] - b.xinit[0], e.z[5] - b.xinit[5])
