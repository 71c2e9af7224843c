"""CPU-only checks of the one-kernel pnp_gd / pnp_sgd / pnp_saga iterations: the four symbols, every PNP_ERR_ARG path
(answered before any device work), the static check of the hand-issued accesses of the new kernels, the calls GdEngine, SgdEngine and
SagaEngine make with and without `fused` (the library replaced by a recorder, as in test_cpu_sarah_fused.py), and what
`make_runner(fused_steps=True)` refuses."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'pnp_csmri_grad_step': 17, 'pnp_csmri_grad_step_pp': 19, 'pnp_csmri_saga_step': 21, 'pnp_csmri_saga_step_pp': 24}


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
    for name, n in NEW.items():
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name
        assert len(_native.SIGNATURES[name][1]) == n, name


class _Plan(ctypes.Structure):
    """The fields of csrc/csmri_plan.h, filled on the host: enough for the argument checks, which answer before any of the device
    pointers is used."""
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('batch', ctypes.c_int), ('dtype', ctypes.c_int), ('NL', ctypes.c_int),
                ('work', ctypes.c_void_p), ('twtab', ctypes.c_void_p), ('mbd', ctypes.c_void_p), ('fused_min_batch', ctypes.c_int)]


def _plan(n=256, dtype=None, batch=2):
    from pnp_svrg_amd import _native
    return _Plan(n, n, batch, _native.F32 if dtype is None else dtype, 16 if n == 256 else 12, None, None, None, 192)


def _pp_grad(a):
    return a[:6] + [None] + a[6:12] + [None] + a[12:]


def _pp_saga(a):
    return a[:5] + [None] + a[5:11] + [None] + a[11:16] + [None] + a[16:]


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work, plain and _pp: NULL pointers, both or neither of yh / YT, a 128 x 128 or f64 plan, the
    forbidden aliasings of table and sum, sse_out without xrec."""
    from pnp_svrg_amd import _native
    h = _lib()
    IMG = 2 * 256 * 256 * 4                                      # bytes of one [batch] image array of the plan below
    plan, p128, p64 = _plan(), _plan(128), _plan(dtype=_native.F64)
    P = lambda s: ctypes.cast(ctypes.byref(s), ctypes.c_void_p)                      # noqa: E731
    at = lambda k: ctypes.c_void_p(1 << 20 | k * 16 * IMG)                           # noqa: E731  (disjoint, never dereferenced)
    a, bits, yh, YT, c1, out, xrec, table, row, prev, tsum = (at(k) for k in range(1, 12))
    # plan, a, bitsT, yh, YT, alpha, alpha_vec, beta, c1, out, denoise, sigma_modifier, fallback_sigma, xrec, sse_out, sigma_out, stream
    ok = [P(plan), a, bits, None, YT, 1e-3, None, 1.0, c1, out, 1, 1.0, 0.0, None, None, None, None]
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 8, 9)}
    bad.update({'neither yh nor YT': {4: None}, 'both yh and YT': {3: yh}, '128 x 128 plan': {0: P(p128)}, 'f64 plan': {0: P(p64)},
                'sse without xrec': {14: a}, 'yh form, 128 x 128 plan': {0: P(p128), 3: yh, 4: None}})
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_csmri_grad_step(*args) == 1, what
        assert h.pnp_last_error().decode(), what
        assert h.pnp_csmri_grad_step_pp(*_pp_grad(args)) == 1, what
    h.pnp_csmri_grad_step(*[P(p128)] + ok[1:])
    assert b'f32 plans of 256 x 256' in h.pnp_last_error()       # the refusal text of the other one-kernel entries
    # plan, z, bitsT, YT, alpha, alpha_vec, table, row, prev_row, sum, lr, inv_hist, hist, out, denoise, sigma_modifier, fallback_sigma,
    # xrec, sse_out, sigma_out, stream
    HIST = 4
    ok = [P(plan), a, bits, YT, 1e-3, None, table, row, prev, tsum, 2e3, 0.25, HIST, out, 1, 1.0, 0.0, xrec, None, None, None]
    inside = lambda k: ctypes.c_void_p(table.value + k * IMG)                        # noqa: E731  (row k of the table)
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 3, 6, 7, 8, 9, 13)}
    bad.update({'128 x 128 plan': {0: P(p128)}, 'f64 plan': {0: P(p64)}, 'hist 0': {12: 0}, 'sse without xrec': {17: None, 18: a},
                'table is z': {6: a}, 'table is out': {6: out}, 'table is xrec': {6: xrec}, 'sum is z': {9: a}, 'sum is out': {9: out},
                'sum is xrec': {9: xrec}, 'sum is table': {9: table}, 'sum is the last row of table': {9: inside(HIST - 1)},
                'z is a row of table': {1: inside(2)}, 'out straddles table and what follows': {13: ctypes.c_void_p(table.value + HIST * IMG - 16)},
                'table starts inside z': {6: ctypes.c_void_p(a.value + IMG - 16)}})
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_csmri_saga_step(*args) == 1, what
        assert h.pnp_last_error().decode(), what
        assert h.pnp_csmri_saga_step_pp(*_pp_saga(args)) == 1, what
    h.pnp_csmri_saga_step(*ok[:9] + [table] + ok[10:])
    assert b'must not alias' in h.pnp_last_error()


# ------------------------------------------------------------------------------------------------------------ the static check
def test_new_kernels_loads_and_stores_untouched(tmp_path):
    """tools/check_fused_isa.py --steps: k_grad_step and k_saga_iter, denoise on and off -- no instruction names the destination of
    a hand-issued load before a wait that covers it, every hand-issued store keeps its wait state."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import hip_listing
    finally:
        sys.path.pop(0)
    path = tmp_path / 'csmri_fused.s'
    path.write_text(hip_listing.listing('csmri_fused.hip'))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), '--steps', str(path)], capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    lines = out.stdout.splitlines()
    grad, saga = [ln for ln in lines if 'k_grad_step' in ln], [ln for ln in lines if 'k_saga_iter' in ln]
    assert len(grad) == len(saga) == 2 and out.stdout.count(' 0 violations') == 4 and 'VIOLATION' not in out.stdout, out.stdout[-3000:]
    count = lambda ln, what: int(ln.split(' hand-issued ' + what)[0].split()[-1])  # noqa: E731
    # loads: 32 pieces each of a and c1, and 32 of the second operand b behind the run-time test the k_svrg_iter instantiations have
    # as well (never taken: b is NULL) (grad); 32 of z in phase 1 and of old, pv, sum, z in the epilogue (saga); with the prox 32 more
    # of the ground truth
    assert sorted(count(ln, 'loads') for ln in grad) == [96, 128] and sorted(count(ln, 'loads') for ln in saga) == [160, 192], lines
    # stores: 32 of out in each form of the last phase (one form without the prox); saga: 32 each of the table row and the sum before
    assert sorted(count(ln, 'stores') for ln in grad) == [32, 64] and sorted(count(ln, 'stores') for ln in saga) == [96, 128], lines
    # the switch leaves the other selections as they were
    other = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), str(path)], capture_output=True, text=True,
                           timeout=900)
    assert other.returncode == 0 and other.stdout.count(' 0 violations') == 12 and 'k_grad_step' not in other.stdout


# ------------------------------------------------------------------------------------------------ the engines on a recorder
class _Prox:
    """what the streaming path asks of a prox"""
    inplace = True

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        return z


class _Csmri:
    """A 256 x 256 f32 'csmri' batch on CPU tensors: the gradients recorded instead of launched, the plan the real front end over
    the recorder."""
    per_problem, kind = True, 'csmri'

    def __init__(self, B, ops, calls):
        self.B, self.H, self.W, self.N, self.dtype, self.max_mb = B, 256, 256, 65536, torch.float32, 10 ** 6
        self.xrec, self.xinit = torch.zeros((B, 256, 256)), torch.ones((B, 256, 256))
        self.device, self.calls = self.xrec.device, calls
        self.plan = ops.CsmriPlan.__new__(ops.CsmriPlan)
        self.plan.H, self.plan.W, self.plan.B, self.plan.dtype, self.plan._h = 256, 256, B, torch.float32, None
        self.bits = torch.zeros((B, 256, 8), dtype=torch.int32)
        self.yh_full = torch.zeros((B, 128, 256), dtype=torch.complex64)
        self.YT = torch.zeros((B, 256, 256), dtype=torch.complex64)
        self.inv_m0 = torch.ones(B)

    def _check_mb(self, mb):
        pass

    def minibatches(self, n):
        from pnp_svrg_amd.batches import Minibatches
        return Minibatches.zeros(n, self.B, self.device, bits_shape=(256, 8))

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        self.calls.append(('draw', step0, nsteps))
        for j in range(nsteps):
            mbs.host[j] = None

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        self.calls.append(('grad_full', z, out, alpha, beta, c1))
        return out

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        self.calls.append(('grad_stoch', z, j, out, alpha, beta, c1))
        return out


def _recorder(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, 'require_gpu', lambda: None)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    monkeypatch.setattr(ops, '_p', lambda t: None if t is None else ('ptr', t))    # (CPU tensors: no device pointer to take)
    return ops, calls


def _ptr_is(arg, t):
    return arg[1].data_ptr() == t.data_ptr()


def test_gd_and_sgd_one_call_per_iteration(monkeypatch):
    """fused=True: ONE pnp_csmri_grad_step per inner iteration, in place, with the streaming step's coefficient -- GD on the mask and
    its packed data term with 1 / M0, SGD on the drawn slot and the raw data; fused=False: the gradient through the batch, as ever."""
    from pnp_svrg_amd.engine import GdEngine, SgdEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops, calls)
    eta, mb, decay = 3.0, 7, 0.5
    # ---- streaming: the calls they always made
    g, s = GdEngine(b, _Prox(), eta, lr_decay=decay), SgdEngine(b, _Prox(), eta, mb, lr_decay=decay)
    assert g.fused is False and s.fused is False
    for _ in range(2):
        g.step()
    for _ in range(2):
        s.step()
    assert [c[0] for c in calls] == ['grad_full', 'grad_full', 'draw', 'grad_stoch', 'grad_stoch']
    assert [c[3] for c in calls if c[0] == 'grad_full'] == [-eta, -eta * decay] and calls[2] == ('draw', 0, 16)
    assert [(c[2], c[4], c[5]) for c in calls if c[0] == 'grad_stoch'] == [(0, -eta / mb, 1.0), (1, -eta * decay / mb, 1.0)]
    # ---- fused GD
    del calls[:]
    g = GdEngine(b, TVProx(sigma_modifier=1.25), eta, lr_decay=decay, fused=True, n_log=8)
    for _ in range(3):
        g.step()
    assert [c[0] for c in calls] == ['pnp_csmri_grad_step'] * 3 and (g.s, g.n_prox, g.prox.t) == (3, 3, 3)
    for k, (_, a) in enumerate(calls):   # plan, a, bitsT, yh, YT, alpha, alpha_vec, beta, c1, out, denoise, sm, fb, xrec, sse, sigma_out, stream
        assert len(a) == 17 and a[1][1] is g.z and a[8][1] is g.z and a[9][1] is g.z and a[2][1] is b.bits and a[3][1] is b.yh_full
        assert a[4] is None and a[5] == -(eta * decay ** k) and a[6][1] is b.inv_m0 and a[7] == 1.0 and a[10:12] == (1, 1.25)
        assert a[13][1] is b.xrec and _ptr_is(a[14], g.sse_log[k])
    # ---- fused SGD: device draws in windows of AHEAD steps, the slot of the step
    del calls[:]
    s = SgdEngine(b, TVProx(sigma_modifier=1.25), eta, mb, lr_decay=decay, fused=True, n_log=8)
    for _ in range(3):
        s.step()
    assert [c if c[0] == 'draw' else c[0] for c in calls] == [('draw', 0, 16)] + ['pnp_csmri_grad_step'] * 3
    for k, (_, a) in enumerate(calls[1:]):
        assert len(a) == 17 and a[1][1] is s.z and a[8][1] is s.z and a[9][1] is s.z and a[3] is None and a[4][1] is b.YT
        assert _ptr_is(a[2], s.mbs.selbits[k]) and a[5] == -(eta * decay ** k) / mb and a[6] is None and a[7] == 1.0
        assert _ptr_is(a[14], s.sse_log[k])
    # per-problem values go to the _pp entry point as float64 vectors
    del calls[:]
    s = SgdEngine(b, TVProx(sigma_modifier=np.array([1.0, 1.5])), np.array([2.0, 3.0]), np.array([4, 5], np.int32), fused=True)
    s.step()
    assert [c[0] for c in calls] == ['draw', 'pnp_csmri_grad_step_pp']
    a = calls[1][1]
    assert len(a) == 19 and a[6][1].tolist() == [-0.5, -0.6] and a[13][1].tolist() == [1.0, 1.5]


def test_saga_one_call_per_iteration(monkeypatch):
    """fused=True: after the streaming table initialisation ONE pnp_csmri_saga_step per inner iteration -- 1 / mb, lr, 1 / hist and the
    rows (this step's, the previous step's) of the streaming step; fused=False: gradient + pnp_saga_table_update[_pp], as ever."""
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops, calls)
    eta, mb, hist, decay = 3.0, 7, 5, 0.5
    rows = [2, 4, np.array([1, 3]), np.array([0, 0])]
    e = SagaEngine(b, _Prox(), eta, mb, hist_size=hist, lr_decay=decay)
    assert e.fused is False
    for r in rows:
        e.step(r=r)
    names = [c[0] for c in calls]
    assert names == (['draw', 'grad_stoch', 'pnp_axpbypcz'] + ['draw', 'grad_stoch', 'pnp_saga_table_update'] + ['grad_stoch', 'pnp_saga_table_update']
                     + ['grad_stoch', 'pnp_saga_table_update_pp'] * 2)
    # ---- fused
    del calls[:]
    e = SagaEngine(b, TVProx(sigma_modifier=1.25), eta, mb, hist_size=hist, lr_decay=decay, fused=True, n_log=8)
    assert [c[0] for c in calls] == ['draw', 'grad_stoch', 'pnp_axpbypcz']          # the table initialisation stays as it is
    del calls[:]
    for r in rows:
        e.step(r=r)
    assert [c if c[0] == 'draw' else c[0] for c in calls] == [('draw', 0, 16)] + ['pnp_csmri_saga_step'] * 4
    assert (e.s, e.n_prox, e.prox.t) == (4, 4, 4)
    prev = 0
    for k, (_, a) in enumerate(calls[1:]):
        # plan, z, bitsT, YT, alpha, alpha_vec, table, row, prev_row, sum, lr, inv_hist, hist, out, denoise, sm, fb, xrec, sse, sigma_out, stream
        assert len(a) == 21 and a[1][1] is e.z and a[13][1] is e.z and a[3][1] is b.YT and a[6][1] is e.table and a[9][1] is e.tsum
        assert _ptr_is(a[2], e.mbs.selbits[k]) and a[4] == 1.0 / mb and a[5] is None
        assert a[10] == eta * decay ** k and a[11] == 1.0 / hist and a[12] == hist and a[14:16] == (1, 1.25)
        assert a[7][1].dtype == torch.int32 and a[7][1].tolist() == np.broadcast_to(rows[k], (2,)).tolist()
        assert a[8][1].tolist() == np.broadcast_to(prev, (2,)).tolist()
        assert _ptr_is(a[18], e.sse_log[k])
        prev = rows[k]
    with pytest.raises(ValueError, match=r'SAGA row outside the table: rows in \[0, 5\)'):
        e.step(r=5)
    del calls[:]
    e = SagaEngine(b, TVProx(sigma_modifier=np.array([1.0, 1.5])), np.array([2.0, 3.0]), np.array([4, 5], np.int32), hist_size=hist, fused=True)
    e.step(r=1)
    assert calls[-1][0] == 'pnp_csmri_saga_step_pp'
    a = calls[-1][1]
    assert len(a) == 24 and a[5][1].tolist() == [0.25, 0.2] and a[12][1].tolist() == [2.0, 3.0] and a[18][1].tolist() == [1.0, 1.5]


class _Fake:
    kind, B, H, W, N, dtype, per_problem, max_mb = 'fake', 2, 4, 4, 16, torch.float64, True, 10 ** 6
    xrec = xinit = torch.zeros((2, 4, 4), dtype=torch.float64)


def test_fused_names_what_is_missing(monkeypatch):
    from pnp_svrg_amd.engine import GdEngine, SgdEngine, SagaEngine, TVProx, make_engine
    ops, calls = _recorder(monkeypatch)
    for cls, args in ((GdEngine, (1.0,)), (SgdEngine, (1.0, 5)), (SagaEngine, (1.0, 5))):
        name = cls.__name__
        with pytest.raises(ValueError, match=name + r"\(fused=True\) needs a CsmriBatch \(got 'fake'\), a prox with fused_args"):
            cls(_Fake(), _Prox(), *args, fused=True)
        b = _Csmri(2, ops, calls)
        with pytest.raises(ValueError, match=name + r'\(fused=True\) needs log_objective=False$'):
            cls(b, TVProx(), *args, fused=True, log_objective=True)
        b.dtype, b.H = torch.float64, 128
        with pytest.raises(ValueError, match=r'needs float32 \(got torch.float64\), 256 x 256 images \(got 128 x 256\)$'):
            cls(b, TVProx(), *args, fused=True)
    with pytest.raises(TypeError):
        GdEngine(_Csmri(2, ops, calls), TVProx(), 1.0, 1.0, 4096, 0, False, True)    # keyword-only
    b = _Csmri(2, ops, calls)
    for algo in ('gd', 'sgd', 'saga'):                                              # make_engine passes it through
        assert make_engine(b, TVProx(), 1.0, None, 5, algorithm=algo, hist_size=2, fused=True).fused is True
        assert make_engine(b, TVProx(), 1.0, None, 5, algorithm=algo, hist_size=2).fused is False


# ---------------------------------------------------------------------------------------------------------------- make_runner
def _runner(**kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='sgd', denoiser='tv', eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding='counter')
    a.update(kw)
    return S.make_runner([], a.pop('problem'), a.pop('algorithm'), a.pop('denoiser'), **a)


@pytest.mark.parametrize('kw,word', [(dict(problem='deblur'), "'deblur'"), (dict(problem='pr'), "'pr'"), (dict(algorithm='svrg'), "'svrg'"),
                                     (dict(algorithm='sarah'), "'sarah'"), (dict(H=128), 'H = 128'), (dict(W=64), 'W = 64'),
                                     (dict(denoiser='nlm'), "'nlm'"), (dict(dtype=torch.float64), 'torch.float64'),
                                     (dict(objective=True), 'objective=False')])
def test_fused_steps_refuses_by_name(kw, word):
    with pytest.raises(ValueError) as e:
        _runner(fused_steps=True, **kw)
    assert str(e.value).startswith('fused_steps=True') and word in str(e.value)
    _runner(**kw)                                                # without the option: the runner is made as it always was


def test_fused_steps_covers_the_three_loops_and_off_changes_nothing():
    for algo in ('gd', 'sgd', 'saga'):
        _runner(fused_steps=True, algorithm=algo)
        _runner(fused_steps=True, algorithm=algo, denoiser=lambda **kw: None)
    _runner(fused_steps=True, algorithm='sgd').check_trials([{'eta': 1.0, 'mini_batch_size': 3, 'sigma_modifier': 1.2}])
    _runner(fused_steps=True, algorithm='saga', wide_trials=True).check_trials([{'eta': 1.0, 'mini_batch_size': 3}])
    with pytest.raises(ValueError, match='fused_steps: True or False'):
        _runner(fused_steps=1)
    for off in (dict(), dict(fused_steps=False)):
        with pytest.raises(ValueError) as e:
            _runner(algorithm='saga', **off).check_trials([{'eta': 1.0}])
        assert str(e.value) == "batch_trials: algorithm 'saga' is not supported (only 'gd', 'sgd', 'svrg')"
        with pytest.raises(ValueError) as e:
            _runner(algorithm='sarah', **off).check_trials([{'eta': 1.0}])
        assert str(e.value) == "batch_trials: algorithm 'sarah' is not supported (only 'gd', 'sgd', 'svrg')"
        with pytest.raises(ValueError) as e:
            _runner(sarah_fused=True, **off)
        assert str(e.value) == "sarah_fused=True is for algorithm='sarah' (got 'sgd')"
