"""CPU-only checks of the one-pass Deblur step (pnp_deblur_grad_step): the symbol and what it refuses before any device
work, what the Python layers refuse and hand down (the plan and the batch replaced by recorders), the identity the one-pass form
rests on in float64 NumPy, and that the float32 bound of tests/test_gpu_deblur_step.py holds for a float32 rendering of the
reference itself (margin 1 where the device gets deblur_ref.F32_MARGIN)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import deblur_ref as dr
import deblur_step_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = 'pnp_deblur_grad_step'


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


# -------------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_exported_declared_and_bound():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    assert hasattr(h, NEW) and NEW in _native.SIGNATURES and f'int {NEW}(' in hdr
    res, args = _native.SIGNATURES[NEW]
    vp, d = ctypes.c_void_p, ctypes.c_double
    assert res is ctypes.c_int and args == [vp] * 6 + [d, vp, d, vp, d, vp, vp, vp, vp]


def test_argument_errors_without_gpu():
    """PNP_ERR_ARG (1) with a message, before any device work (the pointers are never dereferenced)."""
    h = _lib()
    plan, a, b, Y, sel, mbd, spp, c1, gpp, c2, out = (ctypes.c_void_p(64 * k) for k in range(1, 12))
    #       0     1  2  3  4     5     6    7    8    9   10   11   12  13   14
    ok = [plan, a, b, Y, None, None, 1.0, None, 1.0, c1, 0.5, None, c2, out, None]
    bad = {'null plan': {0: None}, 'null a': {1: None}, 'null out': {13: None}, 'sel and mbd': {4: sel, 5: mbd},
           'beta without c1': {9: None}, 'gamma without c2': {12: None}, 'gamma_pp without c2': {10: 0.0, 11: gpp, 12: None}}
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_deblur_grad_step(*args) == 1, what
        msg = h.pnp_last_error().decode()
        assert msg.startswith('pnp_deblur_grad_step: ') and len(msg) > len('pnp_deblur_grad_step: '), (what, msg)
    for change, word in (({4: sel, 5: mbd}, 'sel and mbd'), ({9: None}, 'c1'), ({12: None}, 'c2'), ({0: None}, 'null')):
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_deblur_grad_step(*args) == 1 and word in h.pnp_last_error().decode(), word


# ------------------------------------------------------------------------------------------------------------ Python refusals
class _Prox:
    inplace = True

    def bind(self, batch):
        pass

    def __call__(self, z, xrec, sse_out):
        return z


def test_engines_refuse_one_pass_off_its_ground():
    from pnp_svrg_amd import engine as E
    from pnp_svrg_amd.batches import CsmriBatch, DeblurBatch
    csmri = CsmriBatch.__new__(CsmriBatch)                       # (refused before anything of the batch is read)
    mixed = DeblurBatch.__new__(DeblurBatch)
    mixed.M_vec = np.array([4096, 1024], np.int32)
    deblur = DeblurBatch.__new__(DeblurBatch)
    for make in (lambda b, **kw: E.SvrgEngine(b, _Prox(), 1.0, 4, 10, one_pass=True, **kw),
                 lambda b, **kw: E.SarahEngine(b, _Prox(), 1.0, 4, 10, one_pass=True, **kw),
                 lambda b, **kw: E.make_engine(b, _Prox(), 1.0, 4, 10, algorithm='svrg', one_pass=True, **kw),
                 lambda b, **kw: E.make_engine(b, _Prox(), 1.0, 4, 10, algorithm='sarah', one_pass=True, **kw)):
        with pytest.raises(ValueError, match='uniform DeblurBatch'):
            make(csmri)
        with pytest.raises(ValueError, match='mixed scales'):
            make(mixed)
        with pytest.raises(ValueError, match='fused=True'):
            make(deblur, fused=True)


IMAGES = []                                                  # (one list: data_key holds its id)


def _runner(**kw):
    from pnp_svrg_amd import sweep as S
    a = dict(problem='deblur', algorithm='svrg', denoiser='tv', eta=1.0, n_inner=2, mini_batch_size=5, T2=2, seeding='counter')
    a.update(kw)
    return S.make_runner(IMAGES, a.pop('problem'), a.pop('algorithm'), a.pop('denoiser'), **a)


def test_make_runner_refusals_and_default():
    with pytest.raises(ValueError, match="one_pass_diff=True is for problem='deblur' \\(got 'csmri'\\)"):
        _runner(problem='csmri', one_pass_diff=True)
    with pytest.raises(ValueError, match="one_pass_diff=True is for problem='deblur' \\(got 'pr'\\)"):
        _runner(problem='pr', one_pass_diff=True)
    for alg in ('saga', 'sgd', 'gd'):
        with pytest.raises(ValueError, match=f"one_pass_diff=True is for algorithm in \\('svrg', 'sarah'\\) \\(got '{alg}'\\)"):
            _runner(algorithm=alg, one_pass_diff=True)
    with pytest.raises(ValueError, match='mixed_scales=False'):
        _runner(one_pass_diff=True, mixed_scales=True)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='one_pass_diff: True or False'):
            _runner(one_pass_diff=bad)
    for alg in ('svrg', 'sarah'):
        _runner(algorithm=alg, one_pass_diff=True)
        # off: the runner is the one made without the keyword
        plain, off = _runner(algorithm=alg), _runner(algorithm=alg, one_pass_diff=False)
        assert plain.data_key == off.data_key and plain.names == off.names and plain.objective == off.objective
        assert sorted(vars(plain)) == sorted(vars(off))
    for prob, alg in (('csmri', 'svrg'), ('deblur', 'saga'), ('pr', 'sarah')):
        _runner(problem=prob, algorithm=alg, one_pass_diff=False)


def test_runner_hands_one_pass_to_the_engines_only_when_asked(monkeypatch):
    """`prepare` on a stubbed batch: make_engine gets one_pass=True with the flag and exactly today's keywords without it."""
    from pnp_svrg_amd import engine as E
    seen = []

    class _Stop(Exception):
        pass

    def make_engine(batch, prox, *a, **kw):
        seen.append(kw)
        raise _Stop

    monkeypatch.setattr(E, 'make_engine', make_engine)
    monkeypatch.setattr(E.CsmriBatch, 'upload_images', staticmethod(lambda *a, **k: None))
    monkeypatch.setattr(E.DeblurBatch, 'generate', classmethod(lambda cls, *a, **k: object()))
    items = [dict(id=0, image=0, alpha=1.0, snr=20.0, seed=0)]
    for kw in ({}, dict(one_pass_diff=False), dict(one_pass_diff=True)):
        with pytest.raises(_Stop):
            _runner(**kw).prepare(items)
    assert 'one_pass' not in seen[0] and seen[0] == seen[1]
    assert seen[2] == dict(seen[0], one_pass=True)


# ------------------------------------------------------------------------------------------------ what the layers hand down
class _Plan:
    """A DeblurPlan that records its calls."""
    M_vec = None

    def __init__(self):
        self.calls = []

    def grad_step(self, a, **kw):
        self.calls.append(('grad_step', a, kw))
        return kw['out']

    def grad(self, *a, **kw):
        self.calls.append(('grad', a, kw))
        return kw['out']


def test_batch_one_pass_is_one_grad_step_and_nothing_else(monkeypatch):
    from pnp_svrg_amd import batches
    from pnp_svrg_amd.batches import DeblurBatch, Minibatches
    b = DeblurBatch.__new__(DeblurBatch)
    b.plan, b.Y, b._tmp = _Plan(), torch.zeros(2, 16), None
    z, w, mu = (torch.full((2, 4, 4), float(k)) for k in (1, 2, 3))
    mbs = Minibatches.zeros(2, 2, 'cpu')
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: pytest.fail('one_pass=True allocates nothing'))
    monkeypatch.setattr(batches.ops, 'axpbypcz', lambda *a, **k: pytest.fail('one_pass=True launches nothing else'))
    gam = torch.tensor([0.5, 0.25], dtype=torch.float64)
    out = b.grad_stoch_diff(z, w, mbs, 1, out=z, alpha=-0.1, beta=1.0, c1=z, gamma=gam, c2=mu, one_pass=True)
    assert out is z and len(b.plan.calls) == 1
    name, a, kw = b.plan.calls[0]
    assert name == 'grad_step' and a is z and kw['b'] is w and kw['c1'] is z and kw['c2'] is mu and kw['out'] is z
    assert kw['scale'] == -0.1 and kw['beta'] == 1.0 and kw['gamma'] is gam and kw.get('Y') is None
    assert kw['mbd'] is mbs.mbd[1] or torch.equal(kw['mbd'], mbs.mbd[1])
    sel = torch.ones(2, 16, dtype=torch.uint8)
    mbs.host[0] = sel
    b.grad_stoch_diff(z, w, mbs, 0, out=mu, one_pass=True)
    assert b.plan.calls[1][2]['sel'] is sel and 'mbd' not in b.plan.calls[1][2]
    mixed = DeblurBatch.__new__(DeblurBatch)
    mixed.M_vec, mixed.plan = np.array([16, 4], np.int32), _Plan()
    with pytest.raises(ValueError, match='mixed-scale'):
        mixed.grad_stoch_diff(z, w, mbs, 0, out=mu, one_pass=True)
    assert not mixed.plan.calls


class _Batch:
    """The batch interface the streaming paths of SvrgEngine and SarahEngine use, on CPU tensors, every call recorded."""
    per_problem = True
    kind = 'deblur'
    M_vec = None

    def __init__(self, B=2, n=4, dtype=torch.float64, takes_flag=True):
        self.B, self.H, self.W, self.N, self.dtype, self.max_mb = B, n, n, n * n, dtype, 10 ** 6
        self.xrec, self.xinit = torch.zeros((B, n, n), dtype=dtype), torch.ones((B, n, n), dtype=dtype)
        self.device, self.calls, self.takes_flag = self.xrec.device, [], takes_flag

    def _check_mb(self, mb):
        pass

    def minibatches(self, n):
        from pnp_svrg_amd.batches import Minibatches
        return Minibatches.zeros(n, self.B, self.device)

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        for j in range(nsteps):
            mbs.host[j] = None

    def set_host(self, mbs, j, idx):
        mbs.host[j] = idx

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        return out

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None, **kw):
        if not self.takes_flag:
            assert not kw, 'the default engine passes grad_stoch_diff the arguments it always passed'
        self.calls.append(kw)
        return out


@pytest.mark.parametrize('algorithm', ['svrg', 'sarah'])
def test_engine_passes_the_flag_to_every_difference(monkeypatch, algorithm):
    from pnp_svrg_amd import engine as E
    monkeypatch.setattr(E.ops, 'axpbypcz', lambda *a, out=None, **k: out)
    idx = torch.zeros((2, 3), dtype=torch.int32)
    for one_pass in (False, True):
        b = _Batch(takes_flag=one_pass)
        eng = E.make_engine(b, _Prox(), 1.0, 2, 3, algorithm=algorithm, **(dict(one_pass=True) if one_pass else {}))
        assert eng.one_pass is one_pass
        for _ in range(5):
            eng.step(idx)
        assert len(b.calls) == 5 and all(kw == (dict(one_pass=True) if one_pass else {}) for kw in b.calls)


# ------------------------------------------------------------------------------------------------ the identity, float64 NumPy
@pytest.mark.parametrize('scale', [100, 50, 75])
def test_difference_of_minibatch_gradients_is_one_gradient_of_the_difference(scale):
    """gs(z, mb) - gs(w, mb) == grad(z - w, Y = 0, mb): the terms in y cancel.  1e-12 in deblur_ref's metric."""
    n = 64
    inp = sr.inputs(n, scale, 'edge')
    z, w, Y, kern, pts, M = inp['a'], inp['b'], inp['Y'], inp['kern'], inp['pts'], inp['M']
    for what, sel in (('selection', dr.selection(M, 3)), ('all', None)):
        gs = lambda x: dr.grad(x, Y, sel, 1.0, kern, pts, n, n)                               # noqa: E731
        one, S = dr.grad(z - w, np.zeros((3, M)), sel, 1.0, kern, pts, n, n, parts=True)
        e = dr.err(gs(z) - gs(w), one, S)
        print(f'scale {scale}, {what}: err {e:.3e}')
        assert e <= 1e-12, (scale, what, e)


# ------------------------------------------------------------------------------------ the float32 bound, on the reference itself
def _render_step32(n, scale, kname, a, b, Y, sel, sc, beta, c1, gamma, c2):
    """The one-pass operation in float32 on the CPU: the difference in float32, the two blurs of deblur_ref._render32 (torch
    complex64 FFT, float32 taps), the two addends added in float32 in the stated order."""
    f32 = np.float32
    r32 = dr._render32(n, n, scale, kname)
    M = dr.n_meas(n, n, scale) if scale != 100 else n * n
    d = a.astype(f32) if b is None else a.astype(f32) - b.astype(f32)
    Y0 = np.zeros((3, M), f32) if Y is None else Y.astype(f32)
    s1 = np.ones((3, M), np.uint8) if sel is None else sel
    o = np.stack([r32['grad'](d[i:i + 1], Y0[i:i + 1], s1[i:i + 1], np.atleast_1d(sc)[i % np.size(sc)]) for i in range(3)]).reshape(3, -1)
    o = o.astype(f32)
    if c1 is not None:
        o = o + f32(beta) * c1.astype(f32)
    if c2 is not None:
        o = o + np.asarray(gamma, f32).reshape(-1, 1) * c2.astype(f32)
    assert o.dtype == f32
    return o


@pytest.mark.parametrize('n,scale,kname', sr.CASES)
def test_float32_rendering_of_the_reference_is_within_the_bound(n, scale, kname):
    """Every (size, scale, kernel) case of the GPU file and its forms, with margin 1 in place of F32_MARGIN."""
    f32 = np.float32
    inp = sr.inputs(n, scale, kname)
    a, b, Y, c1, c2 = (inp[k] for k in ('a', 'b', 'Y', 'c1', 'c2'))
    ra, rb, rY, rc1, rc2 = (sr.rounded(x, f32) for x in (a, b, Y, c1, c2))
    M = inp['M']
    base = sr.base_bound(f32, n, scale, kname, margin=1.0)
    sels = dict(all=None, selection=dr.selection(M, 3), edges=sr.edge_selection(M))
    forms = [('diff', True, False), ('plain', False, True), ('both', True, True)]
    for name, with_b, with_Y in forms:
        for sname, sel in sels.items():
            for sc, ga in ((sr.SCALE, sr.GAMMA), (sr.SCALE_PP, sr.GAMMA_PP)):
                got = _render_step32(n, scale, kname, a, b if with_b else None, Y if with_Y else None, sel, sc, sr.BETA, c1, ga, c2)
                ref, S = sr.gradient_term(inp, n, ra, rb if with_b else None, rY if with_Y else None, sel, sc)
                add = sr.addends(sr.BETA, rc1, ga, rc2, f32, ref.shape)
                errs = sr.check(f'{n} {scale} {kname} {name} {sname} {"pp" if sc is sr.SCALE_PP else "scalar"}', got, add, ref, S, base, f32)
                assert len(errs) == (2 if sname == 'edges' else 3)
                if sname == 'edges':                                # nothing selected: the addends, exactly
                    g = np.asarray(ga, f32).reshape(-1, 1)[-1]
                    assert np.array_equal(got[2], f32(sr.BETA) * c1[2].astype(f32) + g * c2[2].astype(f32))
