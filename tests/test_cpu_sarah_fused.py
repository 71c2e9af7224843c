"""CPU-only checks of the one-kernel pnp_sarah iteration: the two symbols, the static check of the hand-issued
accesses of the new instantiations (and that the existing ones are checked as before), the calls SarahEngine makes with and without
`fused` (the library replaced by a recorder, as in test_cpu_t2_per_problem.py), and what `make_runner(sarah_fused=True)` refuses."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnp_csmri_sarah_step', 'pnp_csmri_sarah_step_pp')


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
    assert len(_native.SIGNATURES[NEW[0]][1]) == 20 and len(_native.SIGNATURES[NEW[1]][1]) == 23


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) before any device work: NULL pointers, out2 without the prox, v_out aliasing anything but c1."""
    h = _lib()
    p0, a, b, bits, c1, c2, v, out, out2 = (ctypes.c_void_p(64 * k) for k in range(1, 10))      # never dereferenced
    ok = [p0, a, b, bits, 1e-3, None, 1.0, c1, -2e3, c2, v, out, out2, 1, 1.0, 0.0, None, None, None, None]
    bad = {f'null {i}': {i: None} for i in (0, 1, 2, 3, 7, 9, 10, 11)}
    bad.update({'out2 with denoise 0': {13: 0}, 'sse without xrec': {17: a}})
    bad.update({f'v_out aliases {i}': {10: ok[i]} for i in (1, 2, 9, 11, 12)})
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_csmri_sarah_step(*args) == 1, what
        assert h.pnp_last_error().decode(), what
        pp = args[:5] + [None] + args[5:9] + [None] + args[9:15] + [None] + args[15:]
        assert h.pnp_csmri_sarah_step_pp(*pp) == 1, what


# ------------------------------------------------------------------------------------------------------------ the static check
@pytest.fixture(scope='module')
def listing_path(tmp_path_factory):
    """csmri_fused.hip compiled to assembly once for the checks below (the tool compiles it itself when given no listing)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import hip_listing
    finally:
        sys.path.pop(0)
    path = tmp_path_factory.mktemp('isa') / 'csmri_fused.s'
    path.write_text(hip_listing.listing('csmri_fused.hip'))
    return str(path)


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_fused_isa.py'), *args], capture_output=True, text=True, timeout=900)


def test_sarah_instantiations_loads_and_stores_untouched(listing_path):
    """tools/check_fused_isa.py --sarah: plain and _pp, denoise on and off, with and without out2 -- no instruction names the
    destination of a hand-issued load before a wait that covers it, every hand-issued store keeps its wait state."""
    out = _tool('--sarah', listing_path)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    lines = [ln for ln in out.stdout.splitlines() if 'k_sarah_iter' in ln]
    assert len(lines) == 6 and sum('k_sarah_iter_pp' in ln for ln in lines) == 3, out.stdout[-3000:]
    assert out.stdout.count(' 0 violations') == 6 and 'VIOLATION' not in out.stdout
    # loads per instantiation: 32 pieces each of a, b, c1, c2 and -- with the prox -- of the ground truth; stores: 32 of v_out, then 32
    # of out (and 32 of out2) in each of the two forms of the last phase (with and without the error sum; one form without the prox)
    count = lambda ln, what: int(ln.split(' hand-issued ' + what)[0].split()[-1])  # noqa: E731
    assert sorted(count(ln, 'loads') for ln in lines) == [128, 128, 160, 160, 160, 160], lines
    assert sorted(count(ln, 'stores') for ln in lines) == [64, 64, 96, 96, 160, 160], lines


def test_existing_instantiations_checked_as_before(listing_path):
    """Without the flag, and with --pp: the instantiation counts of test_fused_loads_untouched / test_span_kernel_loads_untouched."""
    out = _tool(listing_path)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert out.stdout.count(' 0 violations') == 12 and 'VIOLATION' not in out.stdout and 'k_sarah' not in out.stdout
    out = _tool('--pp', listing_path)
    assert out.returncode == 0 and out.stdout.count(' 0 violations') == 14 and 'k_sarah' not in out.stdout


# ------------------------------------------------------------------------------------------------ the engine on a recorder
class _Prox:
    """what the streaming path asks of a prox"""
    inplace = True

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        return z


class _Batch:
    """The batch interface SarahEngine uses, on CPU tensors, every call recorded instead of launched."""
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
        self.calls.append(('diff', z, w, j, out, alpha, beta, c1))
        return out


class _Csmri(_Batch):
    """A 256 x 256 f32 'csmri' batch on CPU tensors whose plan is the real front end over the recorder."""

    def __init__(self, B, ops):
        super().__init__(B, 256, torch.float32, 'csmri')
        self.plan = ops.CsmriPlan.__new__(ops.CsmriPlan)
        self.plan.H, self.plan.W, self.plan.B, self.plan.dtype, self.plan._h = 256, 256, B, torch.float32, None
        self.bits = torch.zeros((B, 256, 8), dtype=torch.int32)
        self.yh_full = torch.zeros((B, 128, 256), dtype=torch.complex64)
        self.inv_m0 = torch.ones(B, dtype=torch.float32)


def _recorder(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(ops, 'require_gpu', lambda: None)
    monkeypatch.setattr(ops, '_stream', lambda: 'stream')
    monkeypatch.setattr(ops, '_p', lambda t: None if t is None else ('ptr', t))    # (CPU tensors: no device pointer to take)
    return ops, calls


def test_default_engine_makes_the_calls_it_always_made(monkeypatch):
    """SarahEngine without `fused`, call for call in order (written down from the engine as it was before the option existed): per
    outer iteration the copy w_prev <- z, grad_full into v_prev, ONE pnp_axpbypcz into w_next, the prox; per inner iteration the
    windowed draw, the difference of minibatch gradients into v_next, ONE pnp_axpbypcz into z, the prox, the buffer swap and the copy
    w_prev <- z.  No pnp_csmri_sarah_step."""
    from pnp_svrg_amd.engine import SarahEngine
    ops, calls = _recorder(monkeypatch)
    b = _Batch(3)
    b.calls = calls                                              # one chronological list for the batch, the library and the copies
    eta, mb, T2 = 2.0, 5, 2
    e = SarahEngine(b, _Prox(), eta, T2, mb, lr_decay=0.5)
    assert e.fused is False and not e.graph_ok()
    bufs = {'w_prev': e.w_prev, 'w_next': e.w_next, 'v_prev': e.v_prev, 'v_next': e.v_next, 'z': e.z}
    name = lambda t: next((k for k, v in bufs.items() if v is t), '?')             # noqa: E731
    orig = torch.Tensor.copy_

    def copy_(self, src, *a, **k):
        calls.append(('copy_', self, src))
        return orig(self, src, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'copy_', copy_)
    for s in range(5):
        e.step()
    monkeypatch.setattr(torch.Tensor, 'copy_', orig)
    seen = []
    for c in calls:
        if c[0] == 'pnp_axpbypcz':
            a = c[1]
            seen.append((c[0], a[0], name(a[1][1]), a[2], name(a[3][1]), a[4], a[5], name(a[6][1])))
        elif c[0] == 'diff':
            seen.append((c[0], name(c[1]), name(c[2]), c[3], name(c[4]), c[5], c[6], name(c[7])))
        elif c[0] in ('copy_', 'grad_full'):
            seen.append((c[0],) + tuple(name(t) for t in c[1:]))
        else:
            seen.append(c)
    want = []
    v = ['v_prev', 'v_next']                                     # (the names the two direction buffers had at construction)
    for s in range(5):
        if s % T2 == 0:
            want += [('copy_', 'w_prev', 'z'), ('grad_full', v[0]), ('pnp_axpbypcz', 1.0, 'w_prev', -eta, v[0], 0.0, None, 'w_next')]
        if s == 0:
            want.append(('draw', 0, 16))
        want += [('diff', 'w_next', 'w_prev', s, v[1], 1.0 / mb, 1.0, v[0]),
                 ('pnp_axpbypcz', 1.0, 'z', -(eta * 0.5 ** (s // T2)), v[1], 0.0, None, 'z'), ('copy_', 'w_prev', 'z')]
        v.reverse()                                              # the swap
    assert seen == want
    assert (e.s, e.n_prox) == (5, 8)
    with pytest.raises(ValueError, match='hipGraph'):
        e.capture()


def test_fused_engine_makes_one_call_per_iteration(monkeypatch):
    """fused=True: ONE pnp_csmri_svrg_outer_step per outer iteration, ONE pnp_csmri_sarah_step per inner iteration, in place --
    no pnp_axpbypcz, no gradient through the batch, no copy and no buffer swap; the draws of an outer iteration are one launch."""
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    ops, calls = _recorder(monkeypatch)
    b = _Csmri(2, ops)
    eta, mb, T2 = 3.0, 7, 3
    e = SarahEngine(b, TVProx(sigma_modifier=1.25), eta, T2, mb, lr_decay=0.5, fused=True, n_log=8)
    assert e.fused and not hasattr(e, 'v_next')
    ids = {k: id(getattr(e, k)) for k in ('z', 'w_prev', 'w_next', 'v_prev')}
    copies, orig = [], torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, 'copy_', lambda self, *a, **k: copies.append(self))
    for _ in range(7):
        e.step()
    monkeypatch.setattr(torch.Tensor, 'copy_', orig)
    assert not copies and ids == {k: id(getattr(e, k)) for k in ids}
    assert [c[0] for c in calls] == (['pnp_csmri_svrg_outer_step'] + ['pnp_csmri_sarah_step'] * 3) * 2 + ['pnp_csmri_svrg_outer_step',
                                                                                                           'pnp_csmri_sarah_step']
    assert b.calls == [('draw', 0, 3), ('draw', 3, 3), ('draw', 6, 3)]
    assert (e.s, e.n_prox, e.prox.t) == (7, 10, 10)
    row = 0
    for nm, a in calls:
        if nm == 'pnp_csmri_svrg_outer_step':                    # plan, z, mask, yh, alpha_vec, lr, w_out, mu_out, out, denoise, sm, fb, xrec, sse, ...
            assert a[1][1] is e.z and a[6][1] is e.w_prev and a[7][1] is e.v_prev and a[8][1] is e.w_next
            assert a[5] == eta and a[9] == 1 and a[10] == 1.25                        # (F6: the outer step size does not decay)
        else:   # plan, a, b, bits, alpha, alpha_vec, beta, c1, gamma, c2, v_out, out, out2, denoise, sm, fb, xrec, sse, sigma_out, stream
            s = row - row // (T2 + 1) - 1
            assert len(a) == 20 and a[1][1] is e.w_next and a[2][1] is e.w_prev and a[7][1] is e.v_prev and a[9][1] is e.z
            assert a[10][1] is e.v_prev and a[11][1] is e.z and a[12][1] is e.w_prev
            assert a[4] == 1.0 / mb and a[5] is None and a[6] == 1.0 and a[8] == -(eta * 0.5 ** (s // T2)) and a[13:15] == (1, 1.25)
            assert a[3][1].data_ptr() == e.mbs.selbits[s % T2].data_ptr()
        assert a[13 if nm == 'pnp_csmri_svrg_outer_step' else 17][1].data_ptr() == e.sse_log[row % 8].data_ptr()
        row += 1
    # per-problem values go to the _pp entry points as float64 vectors
    calls.clear()
    e = SarahEngine(b, TVProx(sigma_modifier=np.array([1.0, 1.5])), np.array([2.0, 3.0]), T2, np.array([4, 5], np.int32), fused=True)
    e.step()
    assert [c[0] for c in calls] == ['pnp_csmri_svrg_outer_step_pp', 'pnp_csmri_sarah_step_pp']
    a = calls[1][1]
    assert len(a) == 23 and a[5][1].tolist() == [0.25, 0.2] and a[10][1].tolist() == [-2.0, -3.0] and a[17][1].tolist() == [1.0, 1.5]
    assert calls[0][1][6][1].tolist() == [2.0, 3.0]


def test_fused_names_what_is_missing(monkeypatch):
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    ops, _ = _recorder(monkeypatch)
    with pytest.raises(ValueError, match=r"SarahEngine\(fused=True\) needs a CsmriBatch \(got 'fake'\), a prox with fused_args"):
        SarahEngine(_Batch(2), _Prox(), 1.0, 2, 5, fused=True)
    b = _Csmri(2, ops)
    with pytest.raises(ValueError, match='needs log_objective=False$'):
        SarahEngine(b, TVProx(), 1.0, 2, 5, fused=True, log_objective=True)
    b.dtype, b.H = torch.float64, 128
    with pytest.raises(ValueError, match=r'needs float32 \(got torch.float64\), 256 x 256 images \(got 128 x 256\)$'):
        SarahEngine(b, TVProx(), 1.0, 2, 5, fused=True)
    with pytest.raises(TypeError):
        SarahEngine(_Batch(2), _Prox(), 1.0, 2, 5, 1.0, 4096, 0, None, False, True)      # keyword-only


# ---------------------------------------------------------------------------------------------------------------- make_runner
def _runner(**kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='csmri', algorithm='sarah', denoiser='tv', eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding='counter')
    a.update(kw)
    return S.make_runner([], a.pop('problem'), a.pop('algorithm'), a.pop('denoiser'), **a)


@pytest.mark.parametrize('kw,word', [(dict(problem='deblur'), "'deblur'"), (dict(problem='pr'), "'pr'"), (dict(algorithm='svrg'), "'svrg'"),
                                     (dict(H=128), 'H = 128'), (dict(denoiser='nlm'), "'nlm'"), (dict(dtype=torch.float64), 'torch.float64')])
def test_sarah_fused_refuses_by_name(kw, word):
    with pytest.raises(ValueError) as e:
        _runner(sarah_fused=True, **kw)
    assert str(e.value).startswith('sarah_fused=True') and word in str(e.value)
    _runner(**kw)                                                # without the option: the runner is made as it always was


def test_sarah_fused_goes_with_sarah_trials_and_off_changes_nothing():
    _runner(sarah_fused=True, sarah_trials=True).check_trials([{'eta': 1.0, 'mini_batch_size': 3, 'sigma_modifier': 1.2}])
    _runner(sarah_fused=True, denoiser=lambda **kw: None)
    for off in (dict(), dict(sarah_fused=False)):
        with pytest.raises(ValueError) as e:
            _runner(**off).check_trials([{'eta': 1.0}])
        assert str(e.value) == "batch_trials: algorithm 'sarah' is not supported (only 'gd', 'sgd', 'svrg')"
        with pytest.raises(ValueError) as e:
            _runner(sarah_trials=True, **off).check_trials([{'T2': 3}])
        assert str(e.value) == ("batch_trials: trial key 'T2' has no per-problem form here (per-problem keys: ('eta', 'mini_batch_size', "
                                "'sigma_modifier'); a prox factory takes no sigma_modifier)")
        with pytest.raises(ValueError) as e:
            _runner(sarah_trials=True, wide_trials=True, problem='pr', **off).check_trials([{'eta': 1.0}])
        assert 'shared_matrix=True' in str(e.value)
