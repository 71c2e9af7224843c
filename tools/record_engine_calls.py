#!/usr/bin/env python3
"""Record, call for call, what the engines of pnp_svrg_amd/engine.py ask of the library and of their batch -- on the CPU, with the
library replaced by a recorder (the arrangement of tests/test_cpu_t2_per_problem.py: `_native.call` recorded, a fake batch on CPU
tensors whose plan is the real front end of `ops`).

    python tools/record_engine_calls.py tests/golden/engine_calls.json      # write the traces of every configuration
    python tools/record_engine_calls.py --list

tests/test_cpu_engine_calls.py compares the traces of the code under test, entry for entry, with the committed file: a refactor of
the engines that makes another call, the same call with another argument, or leaves another counter behind shows up as the first
differing entry of a configuration.

A trace is the ordered list of every `_native.call`, every method call on the fake batch (draw, set_host, grad_full, grad_stoch,
grad_stoch_diff, objective), every call of the fake prox and every `Tensor.copy_` / `fill_` made from Python.  Arguments are
normalised so that a trace does not depend on addresses or on the order of allocations:
  * a tensor is the string `t<label>@<storage offset>[shape]<dtype>`, the label numbering the storages by first appearance in the trace of its
    configuration (every storage seen is kept alive, so an address is never seen twice);
  * a tensor of at most two dimensions and 64 elements whose storage was filled on the host (made by torch.from_numpy, torch.full or
    torch.zeros: coefficient, T2, mb, draw-id, row and divisor vectors, counters, log rows) carries its values as well;
  * a Python float is its `float.hex()`.
After its calls a trace ends with the counters the run left behind: s, n_prox, prox.t, r_prev, _drawn_base, _outer_dirty, and --
where the fake prox wrote the log -- the PSNR traces read back from the rings.
The last configuration, 'refusals', is the exact text of every ValueError the constructors, capture, run_outer, run_span and the
row checks raise on the CPU."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 3
N_LOG = 5                                                       # both rings wrap in every configuration
HEAD = 40                                                       # entries kept per configuration beside the SHA-256 of all of them
ETA_V = np.array([0.5, 0.25, 0.75])
MB_V = np.array([2, 3, 4], np.int32)
DRAW_ID = [7, 2 ** 32 + 5, 11]
T2_V = np.array([2, 3, 5])
HIST_V = np.array([2, 3, 4])


# ------------------------------------------------------------------------------------------------------------------ the recorder
def _flat(v):
    """Host values as one compact string: lists nested in brackets, floats as float.hex(), booleans as 0 / 1."""
    if isinstance(v, list):
        return '[' + ','.join(_flat(x) for x in v) + ']'
    if isinstance(v, bool):
        return str(int(v))
    return v.hex() if isinstance(v, float) else str(v)


class Trace:
    def __init__(self):
        self.entries, self._labels, self._keep, self._filled = [], {}, [], set()

    def filled(self, t):
        """t's storage was filled on the host: its small views go into the trace with their values."""
        if isinstance(t, torch.Tensor):
            self._filled.add(t.untyped_storage().data_ptr())
            self._keep.append(t)
        return t

    def tensor(self, t):
        key = t.untyped_storage().data_ptr()
        if key not in self._labels:
            self._labels[key] = len(self._labels)
            self._keep.append(t)
        d = f't{self._labels[key]}@{t.storage_offset()}{_flat(list(t.shape))}{str(t.dtype)[6:]}'
        if key in self._filled and t.dim() <= 2 and t.numel() <= 64:
            d += '=' + _flat(t.detach().cpu().numpy().tolist())
        return d

    def norm(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v).hex()
        if v is None or isinstance(v, str):
            return v
        if isinstance(v, np.ndarray):
            return f'a{_flat(list(v.shape))}{v.dtype}={_flat(v.tolist())}'
        if isinstance(v, (tuple, list)):
            return [self.norm(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.norm(x) for k, x in sorted(v.items())}
        if type(v).__name__ == 'Minibatches':
            return f'mbs({self.norm(v.mbd)},{self.norm(v.selbits)},host={_flat([h is not None for h in v.host])})'
        return f'<{type(v).__name__}>'

    def add(self, name, *args, **kw):
        self.entries.append([name] + [self.norm(a) for a in args] + ([self.norm(kw)] if kw else []))


@contextlib.contextmanager
def recording(tr):
    """The library, the stream, the pointers and the Python-level copies of torch replaced by the recorder `tr`; put back on exit."""
    from pnp_svrg_amd import _native, ops
    saved = [(_native, 'call', _native.call), (ops, 'require_gpu', ops.require_gpu), (ops, '_stream', ops._stream), (ops, '_p', ops._p),
             (torch.Tensor, 'copy_', torch.Tensor.copy_), (torch.Tensor, 'fill_', torch.Tensor.fill_),
             (torch, 'from_numpy', torch.from_numpy), (torch, 'full', torch.full), (torch, 'zeros', torch.zeros)]
    orig = {name: f for _, name, f in saved}

    def copy_(self, src, *a, **k):
        tr.add('copy_', self, src)
        return orig['copy_'](self, src, *a, **k)

    def fill_(self, value):
        tr.add('fill_', self, value)
        return orig['fill_'](self, value)

    def maker(name):
        return lambda *a, **k: tr.filled(orig[name](*a, **k))
    new = dict(call=lambda name, *args: tr.add(name, *args), require_gpu=lambda: None, _stream=lambda: 'stream',
               _p=lambda t: None if t is None else t, copy_=copy_, fill_=fill_, from_numpy=maker('from_numpy'), full=maker('full'),
               zeros=maker('zeros'))
    try:
        for obj, name, _ in saved:
            setattr(obj, name, new[name])
        yield
    finally:
        for obj, name, f in saved:
            setattr(obj, name, f)


class Prox:
    """What the streaming paths ask of a prox, recorded; it writes its call count into the log row, so the rings hold distinct
    rows.  pingpong: the result is handed back in another buffer (as NLMProx does)."""

    def __init__(self, tr, pingpong=False):
        self.tr, self.t, self.inplace, self._other = tr, 0, not pingpong, None

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        self.t += 1
        self.tr.add('prox', z, xrec, sse_out)
        sse_out.zero_().add_(float(self.t))
        if self.inplace:
            return z
        if self._other is None:
            self._other = torch.empty_like(z)
        out, self._other = self._other, z
        return out


class Batch:
    """The batch interface the engines use, on CPU tensors, every call recorded instead of launched."""
    per_problem = True

    def __init__(self, tr, n=4, dtype=torch.float64, kind='fake'):
        self.tr = tr
        self.B, self.H, self.W, self.N, self.dtype, self.kind, self.max_mb = B, n, n, n * n, dtype, kind, 10 ** 6
        self.xrec, self.xinit = torch.zeros((B, n, n), dtype=dtype), torch.ones((B, n, n), dtype=dtype)
        self.device = self.xrec.device
        self._sel = torch.zeros((B, n, n), dtype=torch.uint8)    # what a host-fed slot holds (CSMRI: the transposed selector)

    def _check_mb(self, mb):
        pass

    def minibatches(self, n):
        from pnp_svrg_amd.batches import Minibatches
        return Minibatches.zeros(n, self.B, self.device, bits_shape=(self.W, max(1, self.H // 32)))

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        self.tr.add('draw', mbs, mb, seed, step0, nsteps, step_dev, draw_id)
        for j in range(nsteps):
            mbs.host[j] = None

    def set_host(self, mbs, j, idx):
        self.tr.add('set_host', mbs, j, idx)
        mbs.host[j] = self._sel

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        self.tr.add('grad_full', z, out, alpha, beta, c1)
        return out

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        self.tr.add('grad_stoch', z, mbs, j, out, alpha, beta, c1)
        return out

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        self.tr.add('grad_stoch_diff', z, w, mbs, j, out, alpha, beta, c1, gamma, c2)
        return out

    def objective(self, z, out=None):
        self.tr.add('objective', z, out)
        return out


class Csmri(Batch):
    """A 256 x 256 float32 'csmri' batch on CPU tensors whose plan is the real front end over the recorder."""

    def __init__(self, tr):
        from pnp_svrg_amd import ops
        super().__init__(tr, 256, torch.float32, 'csmri')
        self.plan = ops.CsmriPlan.__new__(ops.CsmriPlan)
        self.plan.H, self.plan.W, self.plan.B, self.plan.dtype, self.plan._h = 256, 256, B, torch.float32, None
        self.bits = torch.zeros((B, 256, 8), dtype=torch.int32)
        self.yh_full = torch.zeros((B, 128, 256), dtype=torch.complex64)
        self.YT = torch.zeros((B, 256, 256), dtype=torch.complex64)
        self.inv_m0 = torch.ones(B, dtype=torch.float32)


def _prox(tr, kind):
    from pnp_svrg_amd.engine import TVProx
    if kind == 'fake':
        return Prox(tr)
    if kind == 'pingpong':
        return Prox(tr, pingpong=True)
    if kind == 'tv':                                            # inside the kernel, span-capable
        return TVProx(sigma_modifier=1.25)
    if kind == 'tv_pp':
        return TVProx(sigma_modifier=np.array([1.0, 1.25, 1.5]))
    if kind == 'tv_strength':                                   # inside the kernel, with host-side per-call state
        return TVProx(denoise_strength=0.5, decay=0.9)
    if kind == 'w2d':                                           # follows the kernel
        return TVProx(sigma_modifier=1.25, multi=False)
    if kind == 'w2d_in':                                        # the 2-D prox inside the kernel
        return TVProx(sigma_modifier=1.25, multi=False, in_kernel=True)
    raise KeyError(kind)


def _idx(s):
    return (np.arange(B * 2, dtype=np.int32).reshape(B, 2) + s)


# --------------------------------------------------------------------------------------------------------------- configurations
def _steps(n, host=()):
    """n steps; those named in `host` are fed host index lists."""
    def run(e):
        for s in range(n):
            e.step(_idx(s)) if s in host else e.step()
    return run


def _span(n, **kw):
    return lambda e: e.run_span(n, **kw)


def _outer(n, **kw):
    return lambda e: e.run_outer(n, **kw)


def configurations():
    """[(name, algorithm, fused, prox kind, engine keywords, run)]: the matrix of the engines' paths."""
    from pnp_svrg_amd.engine import GdEngine
    ahead = GdEngine.AHEAD
    out = []

    def add(name, algo, fused, prox, kw, run):
        assert name not in [c[0] for c in out], name
        out.append((name, algo, fused, prox, kw, run))
    # ---- Gd, Sgd
    for algo in ('gd', 'sgd'):
        for fused in (False, True):
            px = 'tv' if fused else 'fake'
            f = f'{algo}-{"fused" if fused else "stream"}'
            for case, kw in (('scalar', dict(eta=0.5)), ('eta_pp', dict(eta=ETA_V)), ('decay', dict(eta=0.5, lr_decay=0.9)),
                             ('decay_pp', dict(eta=ETA_V, lr_decay=0.9))):
                add(f'{f}-{case}', algo, fused, px, kw, _steps(7))
            add(f'{f}-span', algo, fused, px, dict(eta=ETA_V), _span(ahead + 3))
            if fused:
                add(f'{f}-span_prox_follows', algo, fused, 'w2d', dict(eta=0.5), _span(ahead + 3))
                add(f'{f}-prox_follows', algo, fused, 'w2d', dict(eta=0.5), _steps(7))
                add(f'{f}-prox_2d_inside', algo, fused, 'w2d_in', dict(eta=0.5), _steps(3))
                add(f'{f}-span_decay', algo, fused, px, dict(eta=0.5, lr_decay=0.9), _span(3))
            if algo == 'sgd':
                add(f'{f}-mb_pp_draw_id', algo, fused, px, dict(eta=ETA_V, mini_batch_size=MB_V, draw_id=DRAW_ID), _steps(7))
                add(f'{f}-host_mix', algo, fused, px, dict(eta=0.5), _steps(7, host=(2, 5)))
    # ---- Svrg
    modes = [('stream', dict(fused=False), 'fake'), ('fused_fold', dict(fused=True, fold_outer=True), 'tv'),
             ('fused_nofold', dict(fused=True, fold_outer=False), 'tv')]
    for variant in ('svrg', 'reference'):
        for mode, mkw, px in modes:
            if variant == 'reference' and mkw['fused']:
                continue                                        # (refused: among the refusals)
            for t2name, t2kw, n in (('T2_3', dict(T2=3), 7), ('T2_vec', dict(T2=T2_V, span=4), 11)):
                for decay in (1.0, 0.9):
                    for pp, hkw in (('scalar', dict(eta=0.5, mini_batch_size=2)), ('pp', dict(eta=ETA_V, mini_batch_size=MB_V))):
                        add(f'svrg-{variant}-{mode}-{t2name}-decay{decay}-{pp}', 'svrg', mkw['fused'], px,
                            dict(variant=variant, lr_decay=decay, **mkw, **t2kw, **hkw), _steps(n))
    for mode, mkw, px in modes:
        f = mkw['fused']
        add(f'svrg-{mode}-host_fed_then_device', 'svrg', f, px, dict(T2=3, **mkw), _steps(7, host=(0, 1, 3)))
        add(f'svrg-{mode}-T2_vec-host_mix', 'svrg', f, px, dict(T2=T2_V, span=4, **mkw), _steps(7, host=(1, 4)))
        add(f'svrg-{mode}-T2_vec-run_span', 'svrg', f, px, dict(T2=T2_V, span=4, eta=ETA_V, mini_batch_size=MB_V, **mkw), _span(11))
        add(f'svrg-{mode}-T2_3-run_span', 'svrg', f, px, dict(T2=3, **mkw), _span(4))
    add('svrg-fused-T2_vec-run_span_2d_inside', 'svrg', True, 'w2d_in', dict(T2=T2_V, span=4, fused=True), _span(5))
    add('svrg-fused-T2_vec-run_span_decay', 'svrg', True, 'tv', dict(T2=T2_V, span=4, fused=True, lr_decay=0.9), _span(5))
    add('svrg-fused-prox_follows', 'svrg', True, 'w2d', dict(T2=3, fused=True), _steps(7))
    add('svrg-fused-T2_vec-prox_follows', 'svrg', True, 'w2d', dict(T2=T2_V, span=4, fused=True), _steps(7))
    add('svrg-fused-run_outer_one_launch', 'svrg', True, 'tv', dict(T2=3, fused=True, eta=ETA_V, lr_decay=0.9), _outer(2, one_launch=True))
    add('svrg-fused-run_outer_default', 'svrg', True, 'tv_pp', dict(T2=3, fused=True, mini_batch_size=MB_V), _outer(2))
    add('svrg-fused-run_outer_2d_inside', 'svrg', True, 'w2d_in', dict(T2=3, fused=True), _outer(2, one_launch=True))
    add('svrg-fused-auto_small_batch', 'svrg', True, 'tv', dict(T2=3, fused=None), _steps(4))
    add('svrg-stream-log_objective', 'svrg', False, 'fake', dict(T2=3, log_objective=True), _steps(7))
    add('svrg-stream-T2_vec-log_objective', 'svrg', False, 'fake', dict(T2=T2_V, span=4, log_objective=True), _steps(7))
    # ---- Sarah
    for mode, fused, proxes in (('stream', False, ('fake',)), ('fused', True, ('tv', 'w2d'))):
        for px in proxes:
            f = f'sarah-{mode}-{px}'
            for decay in (1.0, 0.9):
                for pp, hkw in (('scalar', dict(eta=0.5, mini_batch_size=2)), ('pp', dict(eta=ETA_V, mini_batch_size=MB_V))):
                    add(f'{f}-T2_3-decay{decay}-{pp}', 'sarah', fused, px, dict(T2=3, lr_decay=decay, fused=fused, **hkw), _steps(7))
                    add(f'{f}-T2_vec-decay{decay}-{pp}', 'sarah', fused, px,
                        dict(T2=T2_V, split_log=True, span=4, lr_decay=decay, fused=fused, **hkw), _steps(11))
            add(f'{f}-T2_vec-run_span', 'sarah', fused, px,
                dict(T2=T2_V, split_log=True, span=4, eta=ETA_V, mini_batch_size=MB_V, fused=fused), _span(11))
            add(f'{f}-T2_3-run_span', 'sarah', fused, px, dict(T2=3, fused=fused), _span(4))
            add(f'{f}-host_fed_then_device', 'sarah', fused, px, dict(T2=3, fused=fused), _steps(7, host=(0, 1, 3)))
            add(f'{f}-T2_vec-host_mix', 'sarah', fused, px, dict(T2=T2_V, split_log=True, span=4, fused=fused), _steps(7, host=(1, 4)))
    add('sarah-stream-pingpong-T2_3', 'sarah', False, 'pingpong', dict(T2=3), _steps(7))
    add('sarah-stream-pingpong-T2_vec', 'sarah', False, 'pingpong', dict(T2=T2_V, split_log=True, span=4), _steps(11))
    add('sarah-stream-log_objective', 'sarah', False, 'fake', dict(T2=3, log_objective=True), _steps(7))
    add('sarah-fused-w2d_in-T2_3', 'sarah', True, 'w2d_in', dict(T2=3, fused=True), _steps(7))
    add('sarah-fused-w2d_in-T2_vec-run_span', 'sarah', True, 'w2d_in', dict(T2=T2_V, split_log=True, span=4, fused=True), _span(5))
    add('sarah-fused-run_outer_one_launch', 'sarah', True, 'tv', dict(T2=3, fused=True, eta=ETA_V, mini_batch_size=MB_V, lr_decay=0.9),
        _outer(2, one_launch=True))
    add('sarah-fused-draw_id', 'sarah', True, 'tv_pp', dict(T2=3, fused=True, draw_id=DRAW_ID), _steps(4))
    # ---- Saga
    for mode, fused, px in (('stream', False, 'fake'), ('fused', True, 'tv')):
        for hname, hist in (('hist4', 4), ('hist_vec', HIST_V)):
            f = f'saga-{mode}-{hname}'
            for rname, r in (('r_none', None), ('r_scalar', 1), ('r_pp', np.array([1, 0, 1]))):
                for pp, eta in (('scalar', 0.5), ('eta_pp', ETA_V)):
                    def run(e, r=r):
                        for s in range(7):
                            e.step(r=r) if s % 2 else e.step()   # (every other step from the engine's own stream)
                    add(f'{f}-{rname}-{pp}', 'saga', fused, px, dict(hist_size=hist, eta=eta, fused=fused), run)
            rows = np.array([[(i + p) % 2 for p in range(B)] for i in range(ahead + 3)])
            add(f'{f}-run_span', 'saga', fused, px, dict(hist_size=hist, fused=fused), _span(ahead + 3))
            add(f'{f}-run_span_rows', 'saga', fused, px, dict(hist_size=hist, fused=fused, eta=ETA_V), _span(ahead + 3, r=rows))
            add(f'{f}-run_span_row_per_step', 'saga', fused, px, dict(hist_size=hist, fused=fused), _span(3, r=np.array([1, 0, 1])))
            add(f'{f}-span_then_step', 'saga', fused, px, dict(hist_size=hist, fused=fused, mini_batch_size=MB_V, draw_id=DRAW_ID),
                lambda e: (e.step(), e.run_span(2), e.step(), e.run_span(0)))
        add(f'saga-{mode}-decay-host', 'saga', fused, px, dict(hist_size=4, fused=fused, lr_decay=0.9, idx0=_idx(9)), _steps(4, host=(1,)))
    add('saga-fused-prox_follows', 'saga', True, 'w2d', dict(hist_size=4, fused=True), _steps(4))
    add('saga-fused-hist_vec-prox_follows', 'saga', True, 'w2d', dict(hist_size=HIST_V, fused=True), _span(3))
    add('saga-fused-w2d_in', 'saga', True, 'w2d_in', dict(hist_size=4, fused=True), _span(3))
    add('saga-stream-log_objective', 'saga', False, 'fake', dict(hist_size=4, log_objective=True), _steps(6))
    return out


def _engine(tr, algo, fused, prox, kw):
    from pnp_svrg_amd.engine import make_engine
    kw = dict(kw)
    batch = Csmri(tr) if fused else Batch(tr)
    return make_engine(batch, _prox(tr, prox), kw.pop('eta', 0.5), kw.pop('T2', None), kw.pop('mini_batch_size', 2), algorithm=algo,
                       n_log=N_LOG, seed=3, **kw)


def _state(tr, e):
    st = dict(s=e.s, n_prox=e.n_prox, prox_t=getattr(e.prox, 't', None), r_prev=getattr(e, 'r_prev', None),
              drawn_base=getattr(e, '_drawn_base', None), outer_dirty=getattr(e, '_outer_dirty', None))
    if isinstance(e.prox, Prox):                                # the rings hold what the fake prox wrote
        st['psnr_trace'] = e.psnr_trace()
        if e.log_objective:
            st['objective_log_shape'] = list(e.objective_log().shape)
        if getattr(e, 'outer_log', None) is not None:
            st['outer_trace'] = e.outer_trace()
            st['psnr_trace_of_1'] = e.psnr_trace_of(1)
    return tr.norm(st)


def record(config):
    name, algo, fused, prox, kw, run = config
    tr = Trace()
    with recording(tr):
        e = _engine(tr, algo, fused, prox, kw)
        tr.add('constructed')
        run(e)
    tr.entries.append(['state', _state(tr, e)])
    return tr.entries


# --------------------------------------------------------------------------------------------------------------------- refusals
def refusals():
    """[(what, thunk)]: every ValueError the engines raise on the CPU."""
    from pnp_svrg_amd import engine as E
    tr = Trace()
    fake, csm = (lambda **k: _mk(Batch(tr), **k)), (lambda **k: _mk(Csmri(tr), **k))

    def _mk(b, **k):
        for key, v in k.items():
            setattr(b, key, v)
        return b
    P, TV = (lambda: Prox(tr)), (lambda **k: E.TVProx(**k))
    out = []

    def add(what, thunk):
        out.append((what, thunk))

    def after(e, n, then):
        for _ in range(n):
            e.step()
        return then(e)
    # ---- the hyper-parameters every engine takes
    add('eta shape', lambda: E.GdEngine(fake(), P(), np.array([1.0, 2.0])))
    add('eta on a batch without per-problem values', lambda: E.GdEngine(fake(per_problem=False), P(), ETA_V))
    add('mb on a batch without per-problem values', lambda: E.SgdEngine(fake(per_problem=False), P(), 0.5, MB_V))
    add('draw_id on a batch without per-problem values', lambda: E.SgdEngine(fake(per_problem=False), P(), 0.5, 2, draw_id=DRAW_ID))
    add('draw_id shape', lambda: E.SgdEngine(fake(), P(), 0.5, 2, draw_id=[1, 2]))
    add('objective_log without log_objective', lambda: E.GdEngine(fake(), P(), 0.5).objective_log())
    add('make_engine: unknown algorithm', lambda: E.make_engine(fake(), P(), 0.5, 3, 2, algorithm='adam'))
    # ---- fused=True
    mk = dict(gd=lambda b, p, **k: E.GdEngine(b, p, 0.5, **k), sgd=lambda b, p, **k: E.SgdEngine(b, p, 0.5, 2, **k),
              saga=lambda b, p, **k: E.SagaEngine(b, p, 0.5, 2, hist_size=4, **k), sarah=lambda b, p, **k: E.SarahEngine(b, p, 0.5, 3, 2, **k),
              svrg=lambda b, p, **k: E.SvrgEngine(b, p, 0.5, 3, 2, **k))
    for algo, make in mk.items():
        add(f'{algo} fused: a fake batch and prox', lambda make=make: make(fake(), P(), fused=True))
        add(f'{algo} fused: float64, 128 rows', lambda make=make: make(csm(dtype=torch.float64, H=128), TV(), fused=True))
        add(f'{algo} fused: 256 x 128, no fused_args', lambda make=make: make(csm(W=128), P(), fused=True))
        add(f'{algo} fused: log_objective', lambda make=make: make(csm(), TV(), fused=True, log_objective=True))
    add('svrg fused: variant reference', lambda: E.SvrgEngine(csm(), TV(), 0.5, 3, 2, variant='reference', fused=True))
    # ---- T2, span
    for algo, make in (('svrg', lambda b, T2, **k: E.SvrgEngine(b, P(), 0.5, T2, 2, **k)),
                       ('sarah', lambda b, T2, **k: E.SarahEngine(b, P(), 0.5, T2, 2, split_log=np.ndim(T2) != 0, **k))):
        for what, bad in (('short', [2, 3]), ('2-D', [[1, 2, 3]]), ('float', [2.0, 3.0, 4.0]), ('zero', [2, 0, 3]), ('negative', [2, 3, -4]),
                          ('beyond int32', [2, 2 ** 31, 3])):
            add(f'{algo} T2 vector: {what}', lambda make=make, bad=bad: make(fake(), np.array(bad)))
        add(f'{algo} T2 vector on a batch without per-problem values', lambda make=make: make(fake(per_problem=False), T2_V))
        add(f'{algo} span with a scalar T2', lambda make=make: make(fake(), 3, span=4))
        add(f'{algo} span 0', lambda make=make: make(fake(), T2_V, span=0))
        add(f'{algo} run_outer with a T2 vector', lambda make=make: make(fake(), T2_V).run_outer(1))
        add(f'{algo} capture with a T2 vector', lambda make=make: make(fake(), T2_V).capture())
    add('sarah T2 vector without split_log', lambda: E.SarahEngine(fake(), P(), 0.5, T2_V, 2))
    add('sarah T2 vector with log_objective', lambda: E.SarahEngine(fake(), P(), 0.5, T2_V, 2, split_log=True, log_objective=True))
    add('sarah T2 vector with a prox that counts its calls',
        lambda: E.SarahEngine(fake(), TV(denoise_strength=0.5, decay=0.9), 0.5, T2_V, 2, split_log=True))
    add('sarah split_log with a scalar T2', lambda: E.SarahEngine(fake(), P(), 0.5, 3, 2, split_log=True))
    add('sarah outer_trace with a scalar T2', lambda: E.SarahEngine(fake(), P(), 0.5, 3, 2).outer_trace())
    # ---- capture, run_outer
    add('svrg capture: lr_decay', lambda: E.SvrgEngine(fake(), P(), 0.5, 3, 2, lr_decay=0.9).capture())
    add('svrg capture: log_objective', lambda: E.SvrgEngine(fake(), P(), 0.5, 3, 2, log_objective=True).capture())
    add('svrg capture: mid outer iteration', lambda: after(E.SvrgEngine(fake(), P(), 0.5, 3, 2), 1, lambda e: e.capture()))
    add('svrg run_outer(one_launch=True): streaming', lambda: E.SvrgEngine(fake(), P(), 0.5, 3, 2, fused=False).run_outer(1, one_launch=True))
    add('svrg run_outer(one_launch=True): mid outer iteration',
        lambda: after(E.SvrgEngine(csm(), TV(), 0.5, 3, 2, fused=True), 1, lambda e: e.run_outer(1, one_launch=True)))
    add('svrg run_outer(): mid outer iteration', lambda: after(E.SvrgEngine(csm(), TV(), 0.5, 3, 2, fused=True), 1, lambda e: e.run_outer(1, one_launch=False)))
    add('sarah capture: streaming', lambda: E.SarahEngine(fake(), P(), 0.5, 3, 2).capture())
    add('sarah capture: mid outer iteration', lambda: after(E.SarahEngine(csm(), TV(), 0.5, 3, 2, fused=True), 1, lambda e: e.capture()))
    add('sarah run_outer(one_launch=True): streaming, mid outer iteration',
        lambda: after(E.SarahEngine(fake(), P(), 0.5, 3, 2, log_objective=True), 1, lambda e: e.run_outer(1, one_launch=True)))
    add('sarah run_outer(one_launch=True): the 2-D prox inside', lambda: E.SarahEngine(csm(), TV(multi=False, in_kernel=True), 0.5, 3, 2, fused=True).run_outer(1, one_launch=True))
    add('sarah run_outer(one_launch=True): denoise_strength', lambda: E.SarahEngine(csm(), TV(denoise_strength=0.5), 0.5, 3, 2, fused=True).run_outer(1, one_launch=True))

    def host_fed():
        e = E.SarahEngine(csm(), TV(), 0.5, 3, 2, fused=True)
        for s in range(3):
            e.step(_idx(s))
        e.run_outer(1, one_launch=True)
    add('sarah run_outer(one_launch=True): a host-fed slot', host_fed)

    def replay_mid():
        e = E.SarahEngine(csm(), TV(), 0.5, 3, 2, fused=True)
        e.step()
        e.graph = object()                                      # (as if captured: the step count is checked before any replay)
        e.run_outer(1)
    add('sarah run_outer(): mid outer iteration', replay_mid)
    # ---- hist_size, SAGA rows
    saga = lambda b=None, p=None, **k: E.SagaEngine(b or fake(), p or P(), 0.5, 2, **k)     # noqa: E731
    for what, bad in (('short', [2, 3]), ('2-D', [[1, 2, 3]]), ('float', [2.0, 3.0, 4.0]), ('zero', [2, 0, 3]), ('negative', [2, 3, -4]),
                      ('beyond int32', [2, 2 ** 31, 3])):
        add(f'saga hist_size vector: {what}', lambda bad=bad: saga(hist_size=np.array(bad)))
    add('saga hist_size vector on a batch without per-problem values', lambda: saga(fake(per_problem=False), hist_size=HIST_V))
    add('saga hist_size vector with the 2-D prox inside', lambda: saga(csm(), TV(multi=False, in_kernel=True), hist_size=HIST_V, fused=True))
    for mode, b, p, f in (('stream', fake, P, False), ('fused', csm, TV, True)):
        add(f'saga {mode} step: row vector out of range', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=4, fused=f).step(r=np.array([0, 4, 1])))
        add(f'saga {mode} step: negative row', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=4, fused=f).step(r=np.array([0, -1, 1])))
        add(f'saga {mode} step hist vector: scalar row', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=HIST_V, fused=f).step(r=2))
        add(f'saga {mode} step hist vector: row vector', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=HIST_V, fused=f).step(r=np.array([1, 3, 3])))
        add(f'saga {mode} step hist vector: negative', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=HIST_V, fused=f).step(r=np.array([0, 0, -1])))
        add(f'saga {mode} run_span: shape of r', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=4, fused=f).run_span(3, r=np.array([1, 2])))
        add(f'saga {mode} run_span: row out of range', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=4, fused=f).run_span(3, r=np.array([1, 4, 0])))
        add(f'saga {mode} run_span: rows out of range', lambda b=b, p=p, f=f: saga(b(), p(), hist_size=4, fused=f).run_span(2, r=np.array([[1, 2, 0], [0, -1, 1]])))
        add(f'saga {mode} run_span hist vector: rows out of range',
            lambda b=b, p=p, f=f: saga(b(), p(), hist_size=HIST_V, fused=f).run_span(2, r=np.array([[1, 2, 0], [0, 1, 4]])))
        add(f'saga {mode} run_span hist vector: row per step out of range',
            lambda b=b, p=p, f=f: saga(b(), p(), hist_size=HIST_V, fused=f).run_span(2, r=np.array([1, 2])))
    add('saga fused step: scalar row out of range', lambda: saga(csm(), TV(), hist_size=4, fused=True).step(r=4))
    add('saga fused step: negative scalar row', lambda: saga(csm(), TV(), hist_size=4, fused=True).step(r=-1))
    return tr, out


def record_refusals():
    tr, cases = refusals()
    entries = []
    with recording(tr):
        for what, thunk in cases:
            try:
                thunk()
                entries.append([what, 'no ValueError'])
            except ValueError as e:
                entries.append([what, str(e)])
            except Exception as e:                              # (not a refusal of the engine's: its type alone)
                entries.append([what, type(e).__name__])
    return entries


# -------------------------------------------------------------------------------------------------------------------- the file
def digest(entries):
    return hashlib.sha256(json.dumps(entries, separators=(',', ':'), sort_keys=True).encode()).hexdigest()


def names():
    return [c[0] for c in configurations()] + ['refusals']


def record_one(name):
    """One configuration as the file holds it: the number of entries, the SHA-256 of all of them and the first HEAD in full (the
    refusals in full)."""
    if name == 'refusals':
        entries = record_refusals()
        return dict(n=len(entries), sha256=digest(entries), head=entries)
    entries = record(next(c for c in configurations() if c[0] == name))
    entries = json.loads(json.dumps(entries))                   # (tuples -> lists: what a reader of the file gets)
    return dict(n=len(entries), sha256=digest(entries), head=entries[:HEAD])


def save(path, configs):
    """Write {name: record_one(name)}.  The traces repeat themselves step after step and from one configuration to the next, so the
    file holds every distinct argument once (`values`), every distinct entry once as indices into them (`entries`), and per
    configuration its count, its SHA-256 and its head as indices into the entries; `load` undoes it."""
    values, entries, packed = {}, {}, []
    for name, c in configs.items():
        head = [entries.setdefault(tuple(values.setdefault(json.dumps(a, sort_keys=True), len(values)) for a in e), len(entries))
                for e in c['head']]
        packed.append(json.dumps(name) + ':' + json.dumps(dict(n=c['n'], sha256=c['sha256'], head=head), separators=(',', ':'), sort_keys=True))
    values = list(values)
    with open(path, 'w') as f:
        f.write('{"values":[' + ',\n'.join(','.join(values[i:i + 10]) for i in range(0, len(values), 10)) + '],\n"entries":' + json.dumps([list(e) for e in entries], separators=(',', ':'))
                + ',\n"configs":{\n' + ',\n'.join(packed) + '\n}}\n')


def load(path):
    """{name: {n, sha256, head}} with the heads in full, as `record_one` gives them."""
    with open(path) as f:
        d = json.load(f)
    entries = [[d['values'][i] for i in e] for e in d['entries']]
    return {name: dict(c, head=[entries[i] for i in c['head']]) for name, c in d['configs'].items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('out', nargs='?', help='the JSON file to write')
    ap.add_argument('--list', action='store_true', help='print the names of the configurations')
    ap.add_argument('--show', help='print the whole trace of one configuration, one entry per line')
    a = ap.parse_args()
    if a.list:
        print('\n'.join(names()))
        return
    if a.show:
        entries = record_refusals() if a.show == 'refusals' else record(next(c for c in configurations() if c[0] == a.show))
        for i, e in enumerate(entries):
            print(i, json.dumps(e, separators=(',', ':')))
        return
    if not a.out:
        ap.error('name the file to write')
    all_names = names()
    save(a.out, {name: record_one(name) for name in all_names})
    print(f'{len(all_names)} configurations -> {a.out} ({os.path.getsize(a.out)} bytes)')


if __name__ == '__main__':
    main()
