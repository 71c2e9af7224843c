"""CPU-only checks of the one-launch forms -- pnp_csmri_sarah_outer_iteration[_pp], pnp_csmri_grad_span and
pnp_csmri_saga_span: the four symbols, every PNP_ERR_ARG path (answered before any device work), the static check of the hand-issued
accesses of the new kernels, the calls SarahEngine.run_outer(one_launch=True) and the run_span of GdEngine, SgdEngine and SagaEngine
make (the library replaced by a recorder, as in test_cpu_sarah_fused.py), that the default paths make the calls they made, and
what `make_runner(one_launch=True)` refuses."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'pnp_csmri_sarah_outer_iteration': 21, 'pnp_csmri_sarah_outer_iteration_pp': 25, 'pnp_csmri_grad_span': 20,
       'pnp_csmri_saga_span': 26}


# -------------------------------------------------------------------------------------------------------------------- symbols
def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_symbols_exported_declared_and_bound():
    from pnp_svrg_amd import _native, ops
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name, n in NEW.items():
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name
        assert len(_native.SIGNATURES[name][1]) == n, name
    for m in ('sarah_outer_iteration', 'grad_span', 'saga_span'):
        assert callable(getattr(ops.CsmriPlan, m))


class _Plan(ctypes.Structure):
    """The fields of csrc/csmri_plan.h, filled on the host: enough for the argument checks, which answer before any of the device
    pointers is used."""
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('batch', ctypes.c_int), ('dtype', ctypes.c_int), ('NL', ctypes.c_int),
                ('work', ctypes.c_void_p), ('twtab', ctypes.c_void_p), ('mbd', ctypes.c_void_p), ('fused_min_batch', ctypes.c_int)]


def _plan(n=256, dtype=None, batch=2):
    from pnp_svrg_amd import _native
    return _Plan(n, n, batch, _native.F32 if dtype is None else dtype, 16 if n == 256 else 12, None, None, None, 192)


def _each(ok, bad, *calls):
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        for fn, shape in calls:
            assert fn(*shape(args)) == 1, what
            assert _lib().pnp_last_error().decode(), what


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work: NULL required pointers, T2 / n_steps <= 0, n_log < 1, mini_batch_size <= 0 with a NULL
    mb_vec, hist < 1, both or neither of yh / YT, a 128 x 128 or f64 plan, SARAH buffers that are not four, the SAGA overlaps."""
    from pnp_svrg_amd import _native
    h = _lib()
    IMG = 2 * 256 * 256 * 4                                      # bytes of one [batch] image array of the plan below
    plan, p128, p64 = _plan(), _plan(128), _plan(dtype=_native.F64)
    P = lambda s: ctypes.cast(ctypes.byref(s), ctypes.c_void_p)                      # noqa: E731
    at = lambda k: ctypes.c_void_p(1 << 20 | k * 16 * IMG)                           # noqa: E731  (disjoint, never dereferenced)
    z, wp, wn, vp, mask, yh, av, sel, xrec, log, sig, YT, table, rows, prev, tsum = (at(k) for k in range(1, 17))
    # ---- SARAH: plan, z, w_prev, w_next, v_prev, mask_bitsT, yh, alpha_vec, selbits, T2, eta, lr, mb, sm, fb, xrec, sse_log, log_row0,
    # n_log, sigma_out, stream
    ok = [P(plan), z, wp, wn, vp, mask, yh, av, sel, 3, 2e3, 1.8e3, 100, 1.0, 0.0, xrec, log, 0, 8, sig, None]
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 19)}
    bad.update({'T2 0': {9: 0}, 'T2 -1': {9: -1}, 'n_log 0': {18: 0}, 'log_row0 -1': {17: -1}, 'mb 0': {12: 0}, '128 x 128 plan': {0: P(p128)},
                'f64 plan': {0: P(p64)}, 'w_prev is z': {2: z}, 'w_next is z': {3: z}, 'v_prev is z': {4: z}, 'w_next is w_prev': {3: wp},
                'v_prev is w_prev': {4: wp}, 'v_prev is w_next': {4: wn}})
    pp = lambda a: a[:11] + [None] + a[11:12] + [None] + a[12:13] + [None] + a[13:14] + [None] + a[14:]      # noqa: E731
    _each(ok, bad, (h.pnp_csmri_sarah_outer_iteration, list), (h.pnp_csmri_sarah_outer_iteration_pp, pp))
    a = pp(ok)
    assert len(a) == 25
    a[14], a[15] = 0, at(20)                                     # mini_batch_size 0 is fine beside an mb_vec ... up to the plan check
    a[0] = P(p128)
    assert h.pnp_csmri_sarah_outer_iteration_pp(*a) == 1 and b'f32 plans of 256 x 256' in h.pnp_last_error()
    a[0], a[15] = P(plan), None
    assert h.pnp_csmri_sarah_outer_iteration_pp(*a) == 1 and b'mini_batch_size' in h.pnp_last_error()
    h.pnp_csmri_sarah_outer_iteration(*ok[:3] + [z] + ok[4:])
    assert b'buffers of their own' in h.pnp_last_error()
    # ---- grad_span: plan, z, bitsT, yh, YT, alpha, alpha_pp, alpha_vec, beta, denoise, sm, sm_pp, fb, xrec, n_steps, sse_log, log_row0,
    # n_log, sigma_out, stream
    ok = [P(plan), z, sel, None, YT, -1e-3, None, None, 1.0, 1, 1.0, None, 0.0, xrec, 5, log, 0, 8, sig, None]
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 13, 15, 18)}
    bad.update({'neither yh nor YT': {4: None}, 'both yh and YT': {3: yh}, 'n_steps 0': {14: 0}, 'n_steps -2': {14: -2}, 'n_log 0': {17: 0},
                'log_row0 -1': {16: -1}, 'denoise 0': {9: 0}, '128 x 128 plan': {0: P(p128)}, 'f64 plan': {0: P(p64)},
                'yh form, f64 plan': {0: P(p64), 3: yh, 4: None}})
    _each(ok, bad, (h.pnp_csmri_grad_span, list))
    # ---- saga_span: plan, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, rows, prev_row0, sum, lr, lr_pp, inv_hist, hist, denoise, sm,
    # sm_pp, fb, xrec, n_steps, sse_log, log_row0, n_log, sigma_out, stream
    HIST = 4
    ok = [P(plan), z, sel, YT, 1e-3, None, None, table, rows, prev, tsum, 2e3, None, 0.25, HIST, 1, 1.0, None, 0.0, xrec, 5, log, 0, 8, sig,
          None]
    inside = lambda k: ctypes.c_void_p(table.value + k * IMG)                        # noqa: E731  (row k of the table)
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 3, 7, 8, 9, 10, 19, 21, 24)}
    bad.update({'hist 0': {14: 0}, 'n_steps 0': {20: 0}, 'n_log 0': {23: 0}, 'log_row0 -1': {22: -1}, 'denoise 0': {15: 0},
                '128 x 128 plan': {0: P(p128)}, 'f64 plan': {0: P(p64)}, 'table is z': {7: z}, 'table is xrec': {7: xrec}, 'sum is z': {10: z},
                'sum is xrec': {10: xrec}, 'sum is table': {10: table}, 'sum is the last row of table': {10: inside(HIST - 1)},
                'z is a row of table': {1: inside(2)}, 'table starts inside z': {7: ctypes.c_void_p(z.value + IMG - 16)}})
    _each(ok, bad, (h.pnp_csmri_saga_span, list))
    h.pnp_csmri_saga_span(*ok[:10] + [table] + ok[11:])
    assert b'must not alias' in h.pnp_last_error()


# ------------------------------------------------------------------------------------------------------------ the static check
def test_span_kernels_loads_and_stores_untouched(tmp_path):
    """tools/check_fused_isa.py --spans: k_sarah_outer, k_grad_span (GD and SGD) and k_saga_span -- no instruction names the destination
    of a hand-issued load before a wait that covers it, every hand-issued store keeps its wait state; the other walks list what they
    listed."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import hip_listing
    finally:
        sys.path.pop(0)
    path = tmp_path / 'csmri_fused.s'
    path.write_text(hip_listing.listing('csmri_fused.hip'))
    tool = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), *a, str(path)],   # noqa: E731
                                     capture_output=True, text=True, timeout=900)
    out = tool('--spans')
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    lines = out.stdout.splitlines()
    count = lambda ln, what: int(ln.split(' hand-issued ' + what)[0].split()[-1])  # noqa: E731
    pick = lambda word: [ln for ln in lines if word in ln]                         # noqa: E731
    assert len(lines) == 4 and out.stdout.count(' 0 violations') == 4 and 'VIOLATION' not in out.stdout, out.stdout[-3000:]
    assert len(pick('k_sarah_outer')) == 1 and len(pick('k_grad_span')) == 2 and len(pick('k_saga_span')) == 1
    # the loop bodies are those of the per-iteration kernels: their counts, the outer step's and an inner iteration's added up for SARAH
    # (k_svrg_iter<0, true, 0>: 128 loads, 64 + 2 x 32 stores; k_sarah_iter<0, true>: 160 and 160)
    assert [count(ln, 'loads') for ln in pick('k_sarah_outer')] == [288] and [count(ln, 'stores') for ln in pick('k_sarah_outer')] == [288]
    assert [count(ln, 'loads') for ln in pick('k_grad_span')] == [128, 128] and [count(ln, 'stores') for ln in pick('k_grad_span')] == [64, 64]
    assert [count(ln, 'loads') for ln in pick('k_saga_span')] == [192] and [count(ln, 'stores') for ln in pick('k_saga_span')] == [128]
    # the switch leaves the other selections as they were
    for flag, n in (((), 12), (('--pp',), 14), (('--sarah',), 6), (('--steps',), 4)):
        other = tool(*flag)
        assert other.returncode == 0 and other.stdout.count(' 0 violations') == n == len(other.stdout.splitlines()), (flag, other.stdout[-2000:])
        assert not any(w in other.stdout for w in ('k_sarah_outer', 'k_grad_span', 'k_saga_span')), flag


# ------------------------------------------------------------------------------------------------ the engines on a recorder
class _Csmri:
    """A 256 x 256 f32 'csmri' batch on CPU tensors: draws and streaming gradients recorded instead of launched, the plan the real
    front end over the recorder."""
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

    def set_host(self, mbs, j, idx):
        mbs.host[j] = idx

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


def _names(calls):
    return [c if c[0] == 'draw' else c[0] for c in calls]


def test_sarah_one_draw_and_one_launch_per_outer_iteration(monkeypatch):
    """run_outer(n, one_launch=True): per outer iteration one draw of T2 steps and ONE pnp_csmri_sarah_outer_iteration -- eta for the
    outer step, eta * lr_decay ** k for the inner ones, the draw's minibatch size, T2 + 1 log rows; per-problem values take the _pp
    entry.  The default run_outer replays the captured graph, and stepping makes the calls it made."""
    from pnp_svrg_amd.engine import LoopEngine, SarahEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops, calls)
    eta, mb, T2, decay = 3.0, 7, 3, 0.5
    e = SarahEngine(b, TVProx(sigma_modifier=1.25), eta, T2, mb, lr_decay=decay, fused=True, n_log=8)
    assert e.outer_kernel_ok()
    e.run_outer(3, one_launch=True)
    assert _names(calls) == [('draw', 0, 3), 'pnp_csmri_sarah_outer_iteration', ('draw', 3, 3), 'pnp_csmri_sarah_outer_iteration',
                             ('draw', 6, 3), 'pnp_csmri_sarah_outer_iteration']
    assert (e.s, e.n_prox, e.prox.t) == (9, 12, 12)
    for k, (_, a) in enumerate(calls[1::2]):
        # plan, z, w_prev, w_next, v_prev, mask, yh, alpha_vec, selbits, T2, eta, lr, mb, sm, fb, xrec, sse_log, log_row0, n_log, sigma_out, stream
        assert len(a) == 21 and a[1][1] is e.z and a[2][1] is e.w_prev and a[3][1] is e.w_next and a[4][1] is e.v_prev
        assert a[5][1] is b.bits and a[6][1] is b.yh_full and a[7][1] is b.inv_m0 and a[8][1] is e.mbs.selbits and a[9] == T2
        assert a[10] == eta and a[11] == eta * decay ** k and a[12] == mb and a[13:15] == (1.25, 0.0)     # (F6: eta does not decay)
        assert a[15][1] is b.xrec and a[16][1] is e.sse_log and a[17:19] == ((4 * k) % 8, 8) and a[19][1] is e.prox.sig
    # eager steps go on from there with the calls of the fused path
    del calls[:]
    for _ in range(4):
        e.step()
    assert _names(calls) == [('draw', 9, 3), 'pnp_csmri_svrg_outer_step'] + ['pnp_csmri_sarah_step'] * 3 + [('draw', 12, 3),
                                                                                                          'pnp_csmri_svrg_outer_step',
                                                                                                          'pnp_csmri_sarah_step']
    with pytest.raises(ValueError, match=r'run_outer\(one_launch=True\) needs a step count that is a multiple of T2 \(s = 13, T2 = 3\)'):
        e.run_outer(1, one_launch=True)
    # per-problem eta, mini_batch_size and sigma_modifier: float64 / int32 vectors to the _pp entry
    del calls[:]
    e = SarahEngine(b, TVProx(sigma_modifier=np.array([1.0, 1.5])), np.array([2.0, 3.0]), T2, np.array([4, 5], np.int32), lr_decay=decay,
                    fused=True)
    e.run_outer(2, one_launch=True)
    assert [c[0] for c in calls] == ['draw', 'pnp_csmri_sarah_outer_iteration_pp'] * 2
    for k, (_, a) in enumerate(calls[1::2]):
        assert len(a) == 25 and a[11][1].tolist() == [2.0, 3.0] and a[13][1].tolist() == [2.0 * decay ** k, 3.0 * decay ** k]
        assert a[15][1].dtype == torch.int32 and a[15][1].tolist() == [4, 5] and a[17][1].tolist() == [1.0, 1.5]
    # ---- the default: a captured graph, replayed; no one-launch call
    del calls[:]
    graphs = []

    class _Graph:
        n = 0

        def replay(self):
            self.n += 1

    def fake_capture(self, body, state):
        graphs.append(_Graph())
        return graphs[-1]
    monkeypatch.setattr(LoopEngine, '_capture_graph', fake_capture)
    e = SarahEngine(b, TVProx(), eta, T2, mb, fused=True)
    e.run_outer(2)
    assert len(graphs) == 1 and graphs[0].n == 2 and (e.s, e.n_prox, e.prox.t) == (6, 8, 8)
    assert not any(c[0].startswith('pnp_csmri_sarah_outer') for c in calls)


def test_sarah_one_launch_names_what_is_missing(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine, TVProx, DnCNNProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops, calls)

    class _Net(DnCNNProx):                                       # the DnCNN prox's interface without its plan
        def __init__(self):
            self.t = 0

        def bind(self, batch):
            self.sig = torch.empty(batch.B)

    e = SarahEngine(b, _Net(), 1.0, 2, 5, fused=True)
    assert not e.outer_kernel_ok()
    with pytest.raises(ValueError, match=r'run_outer\(one_launch=True\) needs a prox that runs inside the kernel: TVProx \(got _Net\)$'):
        e.run_outer(1, one_launch=True)
    e = SarahEngine(b, TVProx(denoise_strength=0.1), 1.0, 2, 5, fused=True)
    with pytest.raises(ValueError, match='needs denoise_strength == 0$'):
        e.run_outer(1, one_launch=True)
    e = SarahEngine(b, TVProx(), 1.0, 2, 5, fused=True)
    e.mbs.host[1] = torch.zeros(1)                               # a host-fed minibatch in a slot
    assert not e.outer_kernel_ok()
    with pytest.raises(ValueError, match='needs device-drawn minibatches'):
        e.run_outer(1, one_launch=True)
    assert not calls


def test_run_span_one_draw_and_one_launch_per_window(monkeypatch):
    """run_span: launches of at most AHEAD = 16 steps -- GD: ONE pnp_csmri_grad_span on the mask and its packed data term; SGD: one draw
    of m steps from the absolute step id + ONE pnp_csmri_grad_span on the drawn slots and the raw data; SAGA: the same with ONE
    pnp_csmri_saga_span and the rows of the window.  lr_decay != 1 steps eagerly.  Stepping makes the calls it made."""
    from pnp_svrg_amd.engine import GdEngine, SgdEngine, SagaEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops, calls)
    eta, mb, hist = 3.0, 7, 5
    # ---- GD
    g = GdEngine(b, TVProx(sigma_modifier=1.25), eta, fused=True, n_log=40)
    assert g.span_kernel_ok() and g.AHEAD == 16
    g.run_span(35)
    assert [c[0] for c in calls] == ['pnp_csmri_grad_span'] * 3 and (g.s, g.n_prox, g.prox.t) == (35, 35, 35)
    for (_, a), (row, m) in zip(calls, ((0, 16), (16, 16), (32, 3))):
        # plan, z, bitsT, yh, YT, alpha, alpha_pp, alpha_vec, beta, denoise, sm, sm_pp, fb, xrec, n_steps, sse_log, log_row0, n_log, sigma_out, stream
        assert len(a) == 20 and a[1][1] is g.z and a[2][1] is b.bits and a[3][1] is b.yh_full and a[4] is None
        assert a[5] == -eta and a[6] is None and a[7][1] is b.inv_m0 and a[8:11] == (1.0, 1, 1.25) and a[11] is None and a[12] == 0.0
        assert a[13][1] is b.xrec and a[14] == m and a[15][1] is g.sse_log and a[16:18] == (row, 40) and a[18][1] is g.prox.sig
    del calls[:]
    g.step()
    assert [c[0] for c in calls] == ['pnp_csmri_grad_step']
    # ---- SGD, from an unaligned step count
    del calls[:]
    s = SgdEngine(b, TVProx(), eta, mb, fused=True, n_log=64)
    for _ in range(3):
        s.step()
    assert _names(calls) == [('draw', 0, 16)] + ['pnp_csmri_grad_step'] * 3
    del calls[:]
    s.run_span(18)
    assert _names(calls) == [('draw', 3, 16), 'pnp_csmri_grad_span', ('draw', 19, 2), 'pnp_csmri_grad_span']
    assert (s.s, s.n_prox, s.prox.t) == (21, 21, 21) and s._drawn_base is None
    for (_, a), (row, m) in zip(calls[1::2], ((3, 16), (19, 2))):
        assert a[1][1] is s.z and a[2][1] is s.mbs.selbits and a[3] is None and a[4][1] is b.YT and a[5] == -eta / mb and a[7] is None
        assert a[14] == m and a[16:18] == (row, 64)
    del calls[:]
    s.step()                                                     # a later eager step redraws its own window
    assert _names(calls) == [('draw', 16, 16), 'pnp_csmri_grad_step']
    # per-problem values: the arrays of the _pp steps
    del calls[:]
    s = SgdEngine(b, TVProx(sigma_modifier=np.array([1.0, 1.5])), np.array([2.0, 3.0]), np.array([4, 5], np.int32), fused=True)
    s.run_span(2)
    a = calls[1][1]
    assert a[6][1].tolist() == [-0.5, -0.6] and a[11][1].tolist() == [1.0, 1.5]
    # lr_decay != 1: eager steps
    del calls[:]
    s = SgdEngine(b, TVProx(), eta, mb, lr_decay=0.5, fused=True)
    assert not s.span_kernel_ok()
    s.run_span(3)
    assert _names(calls) == [('draw', 0, 16)] + ['pnp_csmri_grad_step'] * 3
    # ---- SAGA
    del calls[:]
    e = SagaEngine(b, TVProx(sigma_modifier=1.25), eta, mb, hist_size=hist, fused=True, n_log=64, seed=3)
    twin = np.random.default_rng(3 + 977)
    del calls[:]
    e.step(r=2)
    rows = [1, 1, 4] + [0] * 14 + [3]
    del calls[:]
    e.run_span(18, r=rows)
    assert _names(calls) == [('draw', 1, 16), 'pnp_csmri_saga_span', ('draw', 17, 2), 'pnp_csmri_saga_span']
    assert (e.s, e.n_prox, e.prox.t, e.r_prev) == (19, 19, 19, 3) and type(e.r_prev) is int and e._drawn_base is None
    for (_, a), (i0, m, prev) in zip(calls[1::2], ((0, 16, 2), (16, 2, 0))):
        # plan, z, bitsT, YT, alpha, alpha_pp, alpha_vec, table, rows, prev_row0, sum, lr, lr_pp, inv_hist, hist, denoise, sm, sm_pp, fb, xrec,
        # n_steps, sse_log, log_row0, n_log, sigma_out, stream
        assert len(a) == 26 and a[1][1] is e.z and a[2][1] is e.mbs.selbits and a[3][1] is b.YT and a[4] == 1.0 / mb and a[5] is None
        assert a[7][1] is e.table and a[10][1] is e.tsum and a[11] == eta and a[12] is None and a[13:17] == (1.0 / hist, hist, 1, 1.25)
        assert a[8][1].dtype == torch.int32 and a[8][1].tolist() == [[r, r] for r in rows[i0:i0 + m]] and a[9][1].tolist() == [prev, prev]
        assert a[20] == m and a[21][1] is e.sse_log and a[22:24] == (1 + i0, 64)
    # r=None: the engine's own stream, in the order step() takes it
    del calls[:]
    e.run_span(3)
    want = [int(twin.integers(hist)) for _ in range(3)]
    assert calls[1][1][8][1][:, 0].tolist() == want and calls[1][1][9][1].tolist() == [3, 3] and e.r_prev == want[-1]
    # per-problem rows: r_prev and the device vector of the last step, as a batched step leaves them
    del calls[:]
    per = np.array([[0, 1], [2, 2], [4, 3]])
    e.run_span(3, r=per)
    assert calls[1][1][8][1].tolist() == per.tolist() and e.r_prev.tolist() == [4, 3] and e.r_prev.dtype == np.int64
    assert e._rows[0] is e.r_prev and e._rows[1].tolist() == [4, 3]
    del calls[:]
    e.step(r=0)
    assert calls[-1][0] == 'pnp_csmri_saga_step' and calls[-1][1][8][1].tolist() == [4, 3]
    with pytest.raises(ValueError, match=r'SAGA row outside the table: rows in \[0, 5\)'):
        e.run_span(2, r=[0, 5])
    with pytest.raises(ValueError, match=r'run_span: r holds one row per step'):
        e.run_span(2, r=[0, 1, 2])


# ---------------------------------------------------------------------------------------------------------------- make_runner
def _runner(**kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='sgd', denoiser='tv', eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding='counter')
    a.update(kw)
    return S.make_runner([], a.pop('problem'), a.pop('algorithm'), a.pop('denoiser'), **a)


def test_one_launch_refuses_by_name_and_off_changes_nothing():
    for kw in (dict(), dict(algorithm='sarah'), dict(algorithm='svrg'), dict(problem='deblur')):
        with pytest.raises(ValueError) as e:
            _runner(one_launch=True, **kw)
        assert str(e.value).startswith('one_launch=True needs sarah_fused=True or fused_steps=True')
        _runner(**kw)
        _runner(one_launch=False, **kw)
    with pytest.raises(ValueError, match='one_launch: True or False'):
        _runner(one_launch=1, fused_steps=True)
    for algo in ('gd', 'sgd', 'saga'):
        _runner(one_launch=True, fused_steps=True, algorithm=algo)
    _runner(one_launch=True, sarah_fused=True, algorithm='sarah')
    with pytest.raises(ValueError) as e:                         # the refusals beside it come first, in their own words
        _runner(one_launch=True, sarah_fused=True)
    assert str(e.value) == "sarah_fused=True is for algorithm='sarah' (got 'sgd')"
