"""CPU-only checks of per-problem T2 for pnp_sarah: the two symbols and their argument errors, the routing of a scalar
and of a [B] T2 through `SarahEngine` and `ops` (the library replaced by the recorder of test_cpu_t2_per_problem.py), the engine's
host-side schedule against a NumPy restatement, its trajectory on a batch whose arithmetic runs on the host, the refusals, and what
`check_trials` / `_TrialSlab` do with and without `sarah_t2_trials`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_cpu_t2_per_problem import OLD_T2, _ArithBatch, _ArithProx, _Batch, _Csmri, _Prox, _lib, _recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnp_csmri_sarah_span_pp', 'pnp_select_pp')


# -------------------------------------------------------------------------------------------------------------------- symbols
def test_symbols_exported_declared_and_bound():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name in NEW:
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name
    assert len(_native.SIGNATURES[NEW[0]][1]) == 29 and len(_native.SIGNATURES[NEW[1]][1]) == 10


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work, the call named in pnp_last_error()."""
    h = _lib()
    al, al2, al3, al4, al5 = (ctypes.c_void_p(64 * k) for k in (1, 2, 3, 4, 5))    # non-NULL pointers that are never dereferenced
    ok = [al, al2, al3, al4, al5, 0, 12, 3, 0, None]                         # src, dst, row_in, row_out, t2_vec, step, n, batch, dtype, stream
    bad = {'src': (0, None), 'dst': (1, None), 't2_vec': (4, None), 'row_in alone NULL': (2, None), 'row_out alone NULL': (3, None),
           'batch 0': (7, 0), 'batch < 0': (7, -1), 'n % batch': (6, 13), 'dtype': (8, 5), 'step < 0': (5, -1), 'dst is src': (1, al)}
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_select_pp(*args) == 1, what
        assert 'pnp_select_pp' in h.pnp_last_error().decode(), what
    # plan, z, w_prev, w_next, v_prev, mask, yh, alpha_vec, selbits, step0, n_steps, T2, t2_vec, eta, eta_pp, lr, lr_pp, mb, mb_vec, sm,
    # sm_pp, fallback, xrec, sse_log, outer_log, log_row0, n_log, sigma_out, stream -- the plan is not read before these checks passed
    ok = [al, al, al2, al3, al4, al, al, al, al, 0, 4, 3, None, 1.0, None, 1.0, None, 5, None, 1.0, None, 0.0, al, al, al2, 0, 8, al, None]
    bad = {'n_steps 0': (10, 0), 'n_steps < 0': (10, -3), 'T2 0, no vector': (11, 0), 'T2 < 0, no vector': (11, -2), 'step0 < 0': (9, -1),
           'mb 0, no vector': (17, 0), 'n_log': (26, 0), 'log_row0 < 0': (25, -1)}
    bad.update({f'null {i}': (i, None) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 22, 23, 24, 27)})
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_csmri_sarah_span_pp(*args) == 1, what
        assert 'pnp_csmri_sarah_span_pp' in h.pnp_last_error().decode(), what


def test_sarah_span_kernel_loads_untouched():
    """tools/check_fused_isa.py --sarah-span: the hand-issued loads of the two bodies inside k_sarah_span_pp's loop are not named before
    a wait that covers them, on any path, and every hand-issued store keeps its wait state."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), '--sarah-span'], capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    lines = [ln for ln in out.stdout.splitlines() if 'k_sarah_span_pp' in ln]
    assert len(lines) == 1 and ' 0 violations' in lines[0], out.stdout[-3000:]
    n_loads = int(lines[0].split(':')[1].split('hand-issued loads')[0])
    assert n_loads > 0 and 'VIOLATION' not in out.stdout and out.stdout.count('violations') == 1


# ------------------------------------------------------------------------------------- the engine on a recorder: routing, schedule
def test_scalar_T2_reaches_no_new_entry_point_and_makes_the_calls_it_made(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Batch(3)
    e = SarahEngine(b, _Prox(), 2.0, 2, 5)
    for _ in range(5):
        e.step()
    assert [c[0] for c in calls] == ['pnp_axpbypcz'] * 8                     # 3 outer steps + 5 inner steps, nothing else native
    assert [c[0] for c in b.calls] == ['grad_full', 'draw', 'diff', 'diff', 'grad_full', 'diff', 'diff', 'grad_full', 'diff']
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 0, 16)]        # the AHEAD window of the scalar engine
    assert e.outer_log is None and e.n_prox == 8
    e.run_span(1)                                                            # a scalar T2: an eager step
    assert e.s == 6 and not [c for c in calls if c[0] in NEW + ('pnp_refresh_pp',)]
    with pytest.raises(ValueError, match='per-problem T2'):
        e.outer_trace()
    # ... and on the one-kernel path
    calls.clear()
    b = _Csmri(2, ops)
    e = SarahEngine(b, TVProx(), 3.0, 2, 7, fused=True)
    e.step(), e.step(), e.step(), e.step(), e.run_outer(1, one_launch=True), e.run_span(1)
    assert [c[0] for c in calls] == ['pnp_csmri_svrg_outer_step', 'pnp_csmri_sarah_step', 'pnp_csmri_sarah_step',
                                     'pnp_csmri_svrg_outer_step', 'pnp_csmri_sarah_step', 'pnp_csmri_sarah_step',
                                     'pnp_csmri_sarah_outer_iteration', 'pnp_csmri_svrg_outer_step', 'pnp_csmri_sarah_step']
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 0, 2), ('draw', 2, 2), ('draw', 4, 2), ('draw', 6, 2)]


def test_vector_T2_reaches_refresh_pp_and_select_pp(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine
    ops, calls = _recorder(monkeypatch)
    b = _Batch(3)
    e = SarahEngine(b, _Prox(), 2.0, np.array([1, 2, 3]), 5, split_log=True, n_log=2)
    for _ in range(3):
        e.step()
    got = [c for c in calls if c[0] != 'pnp_axpbypcz']
    assert [c[0] for c in got] == ['pnp_refresh_pp', 'pnp_select_pp'] * 3
    for s in range(3):
        a = got[2 * s][1]
        v_new, z, v_prev, w_prev, t2 = (x[1] for x in a[:5])
        assert t2 is e._t2_dev and t2.dtype == torch.int32 and t2.tolist() == [1, 2, 3]
        assert v_new is e._v_new and a[5:] == (s, 3 * 16, 3, 1, 'stream') and type(a[5]) is int
        a = got[2 * s + 1][1]
        src, dst, row_in, row_out, t2 = (x[1] for x in a[:5])
        assert dst is e.w_next and src is not dst and row_in is e.sse_tmp and t2 is e._t2_dev
        assert row_out.data_ptr() == e.outer_log[s % 2].data_ptr() and a[5:] == (s, 3 * 16, 3, 1, 'stream')
    assert (e.s, e.n_prox) == (3, 3) and not e.graph_ok() and not e.outer_kernel_ok()
    assert e.psnr_trace().shape == (2, 3) and e.outer_trace().shape == (2, 3)
    with pytest.raises(ValueError, match='run_span'):
        e.run_outer(1)
    with pytest.raises(ValueError, match='hipGraph'):
        e.capture()


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
def test_host_schedule_against_a_numpy_restatement(monkeypatch, lr_decay, fused):
    """Which steps launch grad_full (streaming) / pnp_csmri_svrg_outer_step (fused), pnp_refresh_pp and pnp_select_pp, the draw
    windows, and when the coefficient vectors are remade."""
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    ops, calls = _recorder(monkeypatch)

    def run(B, T2, eta, n, span):
        calls.clear()
        b = _Csmri(B, ops) if fused else _Batch(B)
        e = SarahEngine(b, TVProx() if fused else _Prox(), eta, T2, 4, lr_decay=lr_decay, split_log=True, fused=fused,
                        **({} if span is None else dict(span=span)))
        per_step = []
        for s in range(n):
            n0, m0 = len(calls), len(b.calls)
            e.step()
            per_step.append(([c for c in calls[n0:]], [c for c in b.calls[m0:]]))
        return e, b, per_step

    T2, eta, n = np.array([1, 2, 3, 5, 8, 13]), 2.0, 30
    steps = np.arange(n)
    k = steps[:, None] // T2[None, :]                                            # decay exponent of problem b at step s
    want_refresh = [int(s) for s in steps if (s % T2 == 0).any()]
    want_remade = [int(s) for s in steps if s == 0 or (k[s] != k[s - 1]).any()] if lr_decay != 1.0 else []
    want_gamma = [[-(eta * lr_decay ** int(kb)) for kb in k[s]] for s in steps]
    e, b, per_step = run(6, T2, eta, n, 4)
    inner_name = 'pnp_csmri_sarah_step' + ('' if lr_decay == 1.0 else '_pp') if fused else 'pnp_axpbypcz' + ('' if lr_decay == 1.0 else '_pp')
    remade, last, eta_coefs = [], None, []
    for s, (nat, bat) in enumerate(per_step):
        names = [c[0] for c in nat]
        extra = ((['pnp_csmri_svrg_outer_step'] if fused else []) + ['pnp_refresh_pp'] + ([] if fused else ['pnp_axpbypcz']) + ['pnp_select_pp']
                 if s in want_refresh else [])
        assert names == extra + [inner_name], s
        assert [c[0] for c in bat if c[0] != 'draw'] == ([] if fused else (['grad_full', 'diff'] if s in want_refresh else ['diff']))
        if s in want_refresh:
            c = nat[0][1][5] if fused else nat[1][1][2]                          # the outer step's coefficient: eta / -eta, a Python float
            eta_coefs.append(c)
        # the inner step's coefficient gamma = -lr: sarah_step's argument 8 (_pp: the array at 10), axpbypcz's b at 2 (_pp: the array at 4)
        a = nat[-1][1]
        if lr_decay == 1.0:
            assert (a[8] if fused else a[2]) == -eta and type(a[8] if fused else a[2]) is float
            continue
        gamma = a[10][1] if fused else a[4][1]
        if gamma is not last:
            remade.append(s)
            last = gamma
        assert gamma.dtype == torch.float64 and gamma.tolist() == want_gamma[s]
    assert eta_coefs == [eta if fused else -eta] * len(want_refresh)             # F6: the outer step's eta never decays, never remade
    assert [c for _, bat in per_step for c in bat if c[0] == 'draw'] == [('draw', s, 4) for s in range(0, n, 4)]
    assert remade == want_remade and want_refresh == list(range(n))             # (T2 = 1 is in the vector ...)
    # ... so once more without it, with per-problem eta and the default window: steps with no refresh launch nothing extra
    e, b, per_step = run(2, np.array([4, 6]), np.array([2.0, 3.0]), 13, None)
    ref = [s for s, (nat, _) in enumerate(per_step) if 'pnp_refresh_pp' in [c[0] for c in nat]]
    assert ref == [0, 4, 6, 8, 12] == [s for s, (nat, _) in enumerate(per_step) if 'pnp_select_pp' in [c[0] for c in nat]]
    for s, (nat, bat) in enumerate(per_step):
        assert len(nat) == (1 if s not in ref else 4 if not fused else 4) and ('grad_full' in [c[0] for c in bat]) == (s in ref and not fused)
    assert [c for _, bat in per_step for c in bat if c[0] == 'draw'] == [('draw', 0, 16)]
    # the '-eta' / 'eta' vector of the outer step is made once; the '-lr' vector whenever an exponent changes
    outer = [nat[0][1][6][1] if fused else nat[1][1][4][1] for s, (nat, _) in enumerate(per_step) if s in ref]
    assert all(t is outer[0] for t in outer) and outer[0].tolist() == ([2.0, 3.0] if fused else [-2.0, -3.0])
    inner = [nat[-1][1][10][1] if fused else nat[-1][1][4][1] for nat, _ in per_step]
    changes = [s for s in range(13) if s == 0 or inner[s] is not inner[s - 1]]
    assert changes == ([0, 4, 6, 8, 12] if lr_decay != 1.0 else [0])


def test_run_span_routes_the_vector_to_the_span_kernel_in_windows(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops)
    eta, mb = np.array([3.0, 4.0]), np.array([7, 9], np.int32)
    e = SarahEngine(b, TVProx(sigma_modifier=1.25), eta, np.array([2, 5]), mb, fused=True, split_log=True, span=2, n_log=4)
    assert e.fused and e.outer_kernel_ok() and not e.graph_ok()
    for _ in range(3):                                           # three eager steps first: the log row wraps below
        e.step()
    assert [c[0] for c in calls if c[0] in NEW + ('pnp_refresh_pp',)] == ['pnp_refresh_pp', 'pnp_select_pp'] * 2      # s = 0, s = 2
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 0, 2), ('draw', 2, 2)]
    calls.clear(), b.calls.clear()
    e.run_span(5)
    assert [c for c in b.calls if c[0] == 'draw'] == [('draw', 3, 2), ('draw', 5, 2), ('draw', 7, 1)] and len(b.calls) == 3
    assert [c[0] for c in calls] == ['pnp_csmri_sarah_span_pp'] * 3 and (e.s, e.n_prox, e.prox.t) == (8, 8, 3 + 2 + 5)
    for (_, a), (s0, m, row) in zip(calls, [(3, 2, 3), (5, 2, 1), (7, 1, 3)]):
        assert len(a) == 29 and a[9:12] == (s0, m, 0) and a[25:27] == (row, 4)
        assert a[12][1] is e._t2_dev and a[12][1].dtype == torch.int32 and a[12][1].tolist() == [2, 5]
        assert a[13] == 0.0 and a[14][1].tolist() == [3.0, 4.0] and a[14][1].dtype == torch.float64
        assert a[15] == 0.0 and a[16][1] is a[14][1]                                                        # lr_pp == eta_pp
        assert a[17] == 0 and a[18][1].tolist() == [7, 9] and a[19:22] == (1.25, None, 0.0)
        assert a[1][1] is e.z and a[2][1] is e.w_prev and a[3][1] is e.w_next and a[4][1] is e.v_prev and a[8][1] is e.mbs.selbits
        assert a[23][1] is e.sse_log and a[24][1] is e.outer_log
    # lr_decay != 1, the 2-D prox inside the kernel, a network behind it: eager steps
    for kw, px in ((dict(lr_decay=0.9), TVProx()), ({}, TVProx(multi=False, in_kernel=True)), ({}, TVProx(multi=False))):
        calls.clear()
        e = SarahEngine(b, px, 3.0, np.array([2, 5]), 7, fused=True, split_log=True, **kw)
        e.run_span(3)
        assert e.s == 3 and 'pnp_csmri_sarah_span_pp' not in [c[0] for c in calls] and [c[0] for c in calls].count('pnp_select_pp') == 2


# ------------------------------------------------------------------------------------------------- host-arithmetic trajectories
class _SarahArith(_ArithBatch):
    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        col = lambda v: v.reshape(-1, 1, 1) if isinstance(v, torch.Tensor) else v          # noqa: E731
        g = (z - w) * (1.0 + mbs.mbd[j, :, 0].double()).reshape(-1, 1, 1) * 0.03125
        return out.copy_(col(alpha) * g + beta * c1)


def _host_natives(monkeypatch):
    """pnp_axpbypcz(_pp), pnp_refresh_pp and pnp_select_pp restated on the host tensors the recorder hands through."""
    from pnp_svrg_amd import _native

    def coef(scalar, arr):
        return scalar if arr is None else arr[1].reshape(-1, 1, 1)

    def call(name, *a):
        if name == 'pnp_axpbypcz':
            ca, x, cb, y, cc, w, out = a[:7]
            out[1].copy_(ca * x[1] + cb * y[1])
        elif name == 'pnp_axpbypcz_pp':
            ca, ca_pp, x, cb, cb_pp, y, cc, cc_pp, w, out = a[:10]
            out[1].copy_(coef(ca, ca_pp) * x[1] + coef(cb, cb_pp) * y[1])
        elif name == 'pnp_refresh_pp':
            (mu_new, z, mu, w, t2), step = (x[1] for x in a[:5]), a[5]
            for p in range(z.shape[0]):
                if step % int(t2[p]) == 0:
                    mu[p], w[p] = mu_new[p], z[p]
        elif name == 'pnp_select_pp':
            (src, dst, row_in, row_out, t2), step = (x[1] for x in a[:5]), a[5]
            for p in range(src.shape[0]):
                if step % int(t2[p]) == 0:
                    dst[p], row_out[p] = src[p], row_in[p]
                else:
                    row_out[p] = float('nan')
        else:
            raise AssertionError(name)
    monkeypatch.setattr(_native, 'call', call)


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
@pytest.mark.parametrize('per_problem', [False, True])
def test_engine_with_a_T2_vector_walks_the_scalar_engines_trajectories_on_the_host(monkeypatch, lr_decay, per_problem):
    """The engine's own logic -- draw windows, refresh steps, decay exponents, the two rings -- on a batch whose arithmetic runs on the
    host: problem b equals the scalar-T2 = T2[b] engine on that problem, z, w_prev, w_next, v_prev and the logs, exactly.  n_log = 16
    < 29 steps: both rings wrap."""
    from pnp_svrg_amd.engine import SarahEngine
    _recorder(monkeypatch)
    _host_natives(monkeypatch)
    T2, n, n_log = np.array([1, 2, 3, 5, 8, 13]), 29, 16
    eta = np.array([0.5, 0.25, 0.75, 0.5, 0.25, 0.75]) if per_problem else 0.5
    mb = np.array([2, 3, 2, 3, 2, 3], np.int32) if per_problem else 2
    b = _SarahArith(6)
    e = SarahEngine(b, _ArithProx(), eta, T2, mb, lr_decay=lr_decay, split_log=True, span=5, n_log=n_log)
    for t in (e.w_prev, e.w_next, e.v_prev, e.v_next):
        t.zero_()
    for _ in range(n):
        e.step()
    inner, outer = e.sse_log.clone(), e.outer_log.clone()
    tr, otr = e.psnr_trace(), e.outer_trace()
    assert tr.shape == otr.shape == (n_log, 6) and not np.isnan(tr).any()
    for p, v in enumerate(T2.tolist()):
        r = SarahEngine(b, _ArithProx(), eta, v, mb, lr_decay=lr_decay, n_log=4096)
        for t in (r.w_prev, r.w_next, r.v_prev, r.v_next):
            t.zero_()
        for _ in range(n):
            r.step()
        for x, y in ((e.z, r.z), (e.w_prev, r.w_prev), (e.w_next, r.w_next), (e.v_prev, r.v_prev)):
            assert torch.equal(x[p], y[p]), v
        # the scalar engine's single log, split by step: at s % v == 0 the outer row, then the inner row
        rows, ref_in, ref_out = iter(r.sse_log[:r.n_prox, p].tolist()), [], []
        for s in range(n):
            ref_out.append(next(rows) if s % v == 0 else float('nan'))
            ref_in.append(next(rows))
        for s in range(n - n_log, n):                            # the rows that survive in the rings
            assert inner[s % n_log, p].item() == ref_in[s], (v, s)
            o = outer[s % n_log, p].item()
            assert (np.isnan(o) and np.isnan(ref_out[s])) or o == ref_out[s], (v, s)
        assert np.array_equal(np.isnan(otr[:, p]), [s % v != 0 for s in range(n - n_log, n)])
    assert not torch.equal(e.z[0] - b.xinit[0], e.z[5] - b.xinit[5])
    # psnr_trace_of on an unwrapped run: element for element the scalar engine's trace
    e = SarahEngine(b, _ArithProx(), eta, T2, mb, lr_decay=lr_decay, split_log=True, span=5)
    for _ in range(n):
        e.step()
    for p, v in enumerate(T2.tolist()):
        r = SarahEngine(b, _ArithProx(), eta, v, mb, lr_decay=lr_decay)
        for _ in range(n):
            r.step()
        assert np.array_equal(e.psnr_trace_of(p), r.psnr_trace()[:, p]) and len(e.psnr_trace_of(p)) == n + (n + v - 1) // v
    e.reset()
    assert (e.s, e.n_prox) == (0, 0) and torch.isnan(e.outer_log).all()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_T2_vector_is_validated_and_the_refusals_name_their_reason(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine, TVProx, make_engine
    ops, _ = _recorder(monkeypatch)
    b = _Batch(3)
    with pytest.raises(ValueError, match='scalar T2.*split_log=True'):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5)
    with pytest.raises(ValueError, match='split_log=True is the log layout of a per-problem T2'):
        SarahEngine(b, _Prox(), 1.0, 3, 5, split_log=True)
    with pytest.raises(TypeError):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, 1.0, 4096, 0, None, False, False, True)      # (split_log is keyword-only)
    for bad, word in (([2, 3], r'shape \(2,\)'), ([[1, 2, 3]], r'shape \(1, 3\)'), ([2.0, 3.0, 4.0], 'float64'), ([2, 0, 3], 'problem 1: T2 0'),
                      ([2, 3, -4], 'problem 2: T2 -4')):
        with pytest.raises(ValueError, match=word):
            SarahEngine(b, _Prox(), 1.0, np.array(bad), 5, split_log=True)
    b.per_problem = False
    with pytest.raises(ValueError, match="per-problem T2 needs a batch that takes per-problem values \\(got 'fake'\\)"):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, split_log=True)
    b.per_problem = True
    with pytest.raises(ValueError, match='span'):
        SarahEngine(b, _Prox(), 1.0, 3, 5, span=4)
    with pytest.raises(ValueError, match='span'):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, split_log=True, span=0)
    with pytest.raises(ValueError, match='log_objective'):
        SarahEngine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, split_log=True, log_objective=True)
    with pytest.raises(ValueError, match='call count'):
        SarahEngine(b, TVProx(denoise_strength=0.1, decay=0.9), 1.0, np.array([2, 3, 4]), 5, split_log=True)
    SarahEngine(b, TVProx(denoise_strength=0.1), 1.0, np.array([2, 3, 4]), 5, split_log=True)       # (decay == 1: no call count in it)
    e = make_engine(b, _Prox(), 1.0, np.array([2, 3, 4]), 5, algorithm='sarah', split_log=True, span=3)
    assert type(e) is SarahEngine and e.span == 3 and e.outer_log.shape == (4096, 3) and torch.isnan(e.outer_log).all()
    with pytest.raises(ValueError, match='row_in and row_out'):
        ops.select_pp(e.z, e.w_next, e._t2_dev, 0, row_in=e.sse_tmp)


# ---------------------------------------------------------------------------------------------------------------- check_trials
def _runner(**kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='sarah', denoiser='tv', seeding='counter')
    a.update(kw)
    problem, algorithm, denoiser = a.pop('problem'), a.pop('algorithm'), a.pop('denoiser')
    return S.make_runner([], problem, algorithm, denoiser, eta=1.0, n_inner=2, mini_batch_size=5, T2=2, **a)


def test_sarah_t2_trials_needs_sarah_trials_and_sarah():
    for kw in (dict(), dict(sarah_trials=True, algorithm='svrg'), dict(algorithm='svrg', t2_trials=True)):
        with pytest.raises(ValueError, match='sarah_t2_trials=True needs sarah_trials=True and algorithm='):
            _runner(sarah_t2_trials=True, **kw)
    with pytest.raises(ValueError, match='sarah_t2_trials: True or False'):
        _runner(sarah_trials=True, sarah_t2_trials=1)


@pytest.mark.parametrize('kw', [dict(), dict(seeding='generator'), dict(problem='deblur', wide_trials=True), dict(problem='pr', shared_matrix=True),
                                dict(wide_trials=True), dict(t2_trials=True)])
def test_check_trials_with_and_without_sarah_t2_trials(kw):
    trials = [{'eta': 1.0, 'T2': 3}, {'T2': 5, 'mini_batch_size': 3, 'sigma_modifier': 1.2}, {'eta': 2.0}]
    _runner(sarah_trials=True, sarah_t2_trials=True, **kw).check_trials(trials)
    with pytest.raises(ValueError) as e:                         # without the flag: the texts the runner always used
        _runner(sarah_trials=True, **kw).check_trials(trials)
    if kw.get('t2_trials'):
        assert str(e.value).startswith("batch_trials: trial key 'T2' has no per-problem form for algorithm 'sarah' (t2_trials: 'svrg' only; "
                                       'SarahEngine logs its outer prox in a row of its own')
    else:
        assert str(e.value) == OLD_T2
    _runner(sarah_trials=True, **kw).check_trials([{'eta': 1.0}])
    # the other refusals stay as they are, flag or no flag
    for flag in (True, False):
        with pytest.raises(ValueError) as e:
            _runner(sarah_trials=True, sarah_t2_trials=flag, seeding='legacy').check_trials(trials)
        assert str(e.value) == "batch_trials: seeding 'legacy' is not supported (host index lists; use 'counter' or 'generator')"
        with pytest.raises(ValueError) as e:
            _runner(sarah_trials=True, sarah_t2_trials=flag, problem='deblur').check_trials(trials)
        assert str(e.value) == "batch_trials: problem 'deblur' is not supported (only 'csmri', and 'pr' with shared_matrix=True)"
    with pytest.raises(ValueError, match="trial key 'hist_size'"):
        _runner(sarah_trials=True, sarah_t2_trials=True).check_trials([{'T2': 3, 'hist_size': 4}])


def test_trial_slab_lays_out_T2_and_asks_for_the_split_log(monkeypatch):
    """Through the runner: group_trials with 'T2' among the keys is one group, and the slab's engine gets the int32-valued T2 vector of
    `trial_layout` with split_log=True -- and neither without the flag's key in the trials."""
    from pnp_svrg_amd import engine as E, sweep as S
    made = []

    class _Eng:
        T2 = np.array([1])

        def run_span(self, n):
            made[-1]['ran'] = n

    def fake(batch, prox, eta, T2, mb, **kw):
        made.append(dict(eta=eta, T2=T2, mb=mb, kw=kw))
        return _Eng()
    monkeypatch.setattr(E, 'make_engine', fake)
    monkeypatch.setattr(S, 'make_prox', lambda *a, **k: None)
    trials = S.grid_points({'eta': [1.0, 2.0], 'T2': [2, 3, 5]})
    assert S.group_trials(trials, S.PER_PROBLEM_KEYS + ('T2',)) == [({}, [0, 1, 2, 3, 4, 5])]
    run = _runner(sarah_trials=True, sarah_t2_trials=True)

    class _Base:
        items, streams, tiles = [{'id': 4}, {'id': 9}], None, {}

        class batch:
            @staticmethod
            def tile(n):
                return ('tiled', n)
    monkeypatch.setattr(run, 'run_trials', run.run_trials)
    try:
        run.run_trials([_Base()], trials)
    except AttributeError:
        pass                                                     # (the fake engine has no results: the construction is what is checked)
    assert len(made) == 1 and made[0]['ran'] == 2
    m = made[0]
    assert m['T2'].dtype == np.int32 and m['T2'].tolist() == [2, 2, 3, 3, 5, 5, 2, 2, 3, 3, 5, 5]
    assert m['eta'].tolist() == [1.0] * 6 + [2.0] * 6 and m['kw']['split_log'] is True and m['kw']['algorithm'] == 'sarah'
    assert m['kw']['draw_id'].tolist() == [0, 1] * 6 and m['kw']['seed'] == 5
    made.clear()
    try:
        run.run_trials([_Base()], [{'eta': 1.0}, {'eta': 2.0}])  # no trial names T2: the scalar, no split log
    except AttributeError:
        pass
    assert made[0]['T2'] == 2 and 'split_log' not in made[0]['kw']
