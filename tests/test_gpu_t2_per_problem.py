"""Per-problem T2 for pnp_svrg: `SvrgEngine` with a [B] T2 on the streaming paths and in the span kernel
(`pnp_csmri_svrg_span_pp`), `pnp_refresh_pp` alone, and `grid_search(batch_trials=True, batch_T2=True)`.

Everything here is "equal bit for bit": the per-problem engine executes the scalar engine's arithmetic on the same operands.  The
comparison is always the same: one engine gets the T2 vector; for each distinct value v a scalar-T2 = v engine runs on the same
tiled batch, seed and draw_id; the rows b with T2[b] == v are compared for z, w, mu and the PSNR trace."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(v, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(v, dtype)).cuda()


def _same(x, y):
    """bit for bit, NaNs included"""
    if isinstance(x, np.ndarray):
        return x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}[x.dtype]
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(iv), y.contiguous().view(iv))


def _force_path(monkeypatch, min_batch):
    """The same kernel path on both sides of a comparison, whatever the batch sizes (1: the one-kernel gradient for every batch,
    which is what the folded refresh of the span kernel equals bit for bit; 10 ** 6: the streaming kernels)."""
    from pnp_svrg_amd.engine import SvrgEngine
    monkeypatch.setenv('PNP_CSMRI_FUSED_MIN_BATCH', str(min_batch))
    monkeypatch.setattr(SvrgEngine, 'FUSED_MIN_BATCH', min_batch)


def _state(eng):
    torch.cuda.synchronize()
    return eng.z.clone(), eng.w.clone(), eng.mu.clone(), eng.psnr_trace()


def _check_against_scalars(got, T2, make_scalar, advance, what=''):
    """got: (z, w, mu, trace) of the engine that took the vector; make_scalar(v) -> the scalar-T2 = v engine on the same batch."""
    for v in sorted(set(int(t) for t in T2)):
        ref = make_scalar(v)
        advance(ref)
        rows = np.flatnonzero(np.asarray(T2) == v)
        zr, wr, mur, trr = _state(ref)
        for name, x, y in (('z', got[0], zr), ('w', got[1], wr), ('mu', got[2], mur)):
            assert _same(x[rows], y[rows]), (what, 'T2', v, name)
        assert _same(got[3][:, rows], trr[:, rows]), (what, 'T2', v, 'trace')


def _steps(n):
    def go(eng):
        for _ in range(n):
            eng.step()
    return go


# ------------------------------------------------------------------------------------------------------------ streaming paths
_T2_6 = np.array([1, 2, 3, 5, 8, 13])
_PP = dict(eta=np.array([500.0, 90.0, 500.0, 90.0, 300.0, 300.0]), mb=np.array([150, 400, 400, 150, 250, 250], np.int32),
           sm=np.array([1.0, 1.4, 1.4, 1.0, 1.2, 0.9]))


@pytest.mark.parametrize('variant', ['svrg', 'reference'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ['plain', 'per-problem', 'decay'])
def test_streaming_csmri(case, dtype, variant, monkeypatch):
    """CSMRI 64 x 64, B = 6, T2 = [1, 2, 3, 5, 8, 13], 12 steps: T2 = 1 refreshes at every step, T2 = 13 only at s = 0."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    _force_path(monkeypatch, 10 ** 6)
    B, steps = 6, 12
    base = CsmriBatch.synthetic(B, 64, 64, 0.3, 20.0, seed=41, dtype=dtype)
    eta, mb, sm = (_PP['eta'], _PP['mb'], _PP['sm']) if case == 'per-problem' else (400.0, 200, 1.1)
    kw = dict(variant=variant, seed=7, lr_decay=0.9 if case == 'decay' else 1.0)
    eng = SvrgEngine(base, TVProx(sigma_modifier=sm), eta, _T2_6, mb, **kw)
    assert not eng.fused and not eng.graph_ok()
    _steps(steps)(eng)
    got = _state(eng)
    _check_against_scalars(got, _T2_6, lambda v: SvrgEngine(base, TVProx(sigma_modifier=sm), eta, v, mb, **kw), _steps(steps), case)
    assert not _same(got[0][0], got[0][5]) and not _same(got[2][0], got[2][5])          # (the problems do differ)


@pytest.mark.parametrize('kind', ['deblur', 'pr'])
def test_streaming_deblur_and_pr_tiles(kind):
    """DeblurBatch.tile (64 x 64: the smallest image a Deblur plan takes) / PrBatch.tile (32 x 32), f64, B = 4, T2 = [1, 2, 3, 7],
    8 steps, both variants."""
    from pnp_svrg_amd.engine import DeblurBatch, PrBatch, SvrgEngine, TVProx
    T2, steps, n = np.array([1, 2, 3, 7]), 8, 32
    if kind == 'deblur':
        base = DeblurBatch.synthetic(2, 64, 64, 'Minimal', 20.0, seed=3, dtype=torch.float64).tile(2)
        eta, mb = 3e3, 500
    else:
        rng = np.random.default_rng(9)
        x = rng.random((2, n, n))
        A = rng.standard_normal((2, 2 * n * n, n * n))
        Y = np.abs(np.einsum('bmn,bn->bm', A, x.reshape(2, -1)))
        base = PrBatch(x, A, Y, rng.random((2, n * n)), dtype=torch.float64).tile(2)
        eta, mb = 0.15, 512
    assert base.per_problem and base.B == 4
    for variant in ('svrg', 'reference'):
        kw = dict(variant=variant, seed=2, draw_id=np.tile(np.arange(2), 2))
        eng = SvrgEngine(base, TVProx(), eta, T2, mb, **kw)
        _steps(steps)(eng)
        _check_against_scalars(_state(eng), T2, lambda v: SvrgEngine(base, TVProx(), eta, v, mb, **kw), _steps(steps), (kind, variant))


# ---------------------------------------------------------------------------------------------------------- pnp_refresh_pp alone
def _sentinel(shape, dtype, word):
    """a NaN-free bit pattern no copy could produce by accident"""
    it = {torch.float32: (torch.int32, word), torch.float64: (torch.int64, (word << 32) | 0x1234567)}[dtype]
    return torch.full(shape, it[1], dtype=it[0], device='cuda').view(dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('len_', [4, 4 * 37 + 4, 4 * 700 + 4, 4 * 37 + 3])
def test_refresh_pp_alone(dtype, len_):
    """B = 5, n / B = 4 k + 4 elements (and one odd length: the element-by-element path), steps 0, 1, 6 with T2 = [1, 2, 3, 4, 7]:
    selected rows equal mu_new / z, the others keep the sentinel."""
    from pnp_svrg_amd import ops
    B, T2 = 5, np.array([1, 2, 3, 4, 7])
    g = torch.Generator().manual_seed(len_)
    mu_new, z = (torch.rand((B, len_), generator=g, dtype=torch.float64).to('cuda', dtype) for _ in range(2))
    t2 = _dev(T2, np.int32)
    for step in (0, 1, 6):
        mu, w = _sentinel((B, len_), dtype, 0x3DA5C3E1), _sentinel((B, len_), dtype, 0x3E5A3C1E)
        keep_mu, keep_w = mu.clone(), w.clone()
        ops.refresh_pp(mu_new, z, mu, w, t2, step)
        torch.cuda.synchronize()
        sel = step % T2 == 0
        assert sel.tolist() == {0: [True] * 5, 1: [True, False, False, False, False], 6: [True, True, True, False, False]}[step]
        for p in range(B):
            assert _same(mu[p], mu_new[p] if sel[p] else keep_mu[p]), (step, p)
            assert _same(w[p], z[p] if sel[p] else keep_w[p]), (step, p)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_refresh_pp_argument_errors_leave_the_arrays_alone(dtype):
    from pnp_svrg_amd import _native as N, ops
    B, len_ = 5, 8
    mu_new, z = (torch.rand((B, len_), dtype=torch.float64).to('cuda', dtype) for _ in range(2))
    mu, w = _sentinel((B, len_), dtype, 0x3DA5C3E1), _sentinel((B, len_), dtype, 0x3E5A3C1E)
    keep_mu, keep_w = mu.clone(), w.clone()
    t2 = _dev([1, 1, 1, 1, 1], np.int32)
    h = N.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                 # noqa: E731
    ok = [p(mu_new), p(z), p(mu), p(w), p(t2), 0, B * len_, B, ops._DT[dtype], None]
    bad = {'mu_new': (0, None), 'z': (1, None), 'mu': (2, None), 'w': (3, None), 't2_vec': (4, None), 'batch 0': (7, 0), 'batch < 0': (7, -5),
           'n % batch': (6, B * len_ - 1), 'dtype': (8, 2), 'mu_new aliases mu': (0, p(mu))}
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_refresh_pp(*args) == 1, what                # PNP_ERR_ARG
        torch.cuda.synchronize()
        assert _same(mu, keep_mu) and _same(w, keep_w), what
    assert h.pnp_refresh_pp(*ok) == 0
    torch.cuda.synchronize()
    assert _same(mu, mu_new) and _same(w, z)


# ------------------------------------------------------------------------------------------------------------------ span kernel
_T2_SPAN = np.array([1, 2, 3, 5, 7, 40])


@pytest.fixture(scope='module')
def span_base():
    """The 256 x 256 f32 batch of the span tests (B = 6) and the scalar engines' states after 14 steps, computed once: {T2: state}."""
    import os
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    old = os.environ.get('PNP_CSMRI_FUSED_MIN_BATCH')
    os.environ['PNP_CSMRI_FUSED_MIN_BATCH'] = '1'              # (read when a plan is created)
    try:
        base = CsmriBatch.synthetic(6, 256, 256, 0.3, 20.0, seed=51)
        one = CsmriBatch(base.xrec[3:4].cpu().numpy(), base.mask_np[3:4], np.swapaxes(base.YT[3:4].cpu().numpy(), 1, 2),
                         base.xinit[3:4].cpu().numpy().reshape(1, -1))
    finally:
        if old is None:
            del os.environ['PNP_CSMRI_FUSED_MIN_BATCH']
        else:
            os.environ['PNP_CSMRI_FUSED_MIN_BATCH'] = old
    refs = {}
    for v in sorted(set(_T2_SPAN.tolist())):
        e = SvrgEngine(base, TVProx(sigma_modifier=1.1), 2e3, v, 1000, seed=4, fused=True)
        _steps(14)(e)
        refs[v] = _state(e)
    return base, one, refs


def _span_engine(base, T2=_T2_SPAN, eta=2e3, mb=1000, sm=1.1, **kw):
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    e = SvrgEngine(base, TVProx(sigma_modifier=sm), eta, T2, mb, seed=4, fused=True, **kw)
    assert e.fused and (np.ndim(T2) == 0 or (e.outer_kernel_ok() and not e.graph_ok()))
    return e


def test_span_equals_stepping_and_the_scalar_engines(span_base, monkeypatch):
    """B = 6, T2 = [1, 2, 3, 5, 7, 40], span = 4, run_span(14): spans end inside outer iterations and the last one is short."""
    from pnp_svrg_amd import _native as N
    base, _, refs = span_base
    names = []
    real = N.call
    monkeypatch.setattr(N, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    e = _span_engine(base, span=4)
    e.run_span(14)
    got = _state(e)
    assert names.count('pnp_csmri_svrg_span_pp') == 4 and names.count('pnp_csmri_draw_thresholds') == 4 and len(names) == 8, names
    assert (e.s, e.n_prox, e.prox.t) == (14, 14, 14)
    names.clear()
    st = _span_engine(base, span=4)
    _steps(14)(st)
    assert names.count('pnp_refresh_pp') == 14 and 'pnp_csmri_svrg_span_pp' not in names      # (T2 = 1: a refresh at every step)
    for x, y in zip(got, _state(st)):
        assert _same(x, y)
    for v, ref in refs.items():
        rows = np.flatnonzero(_T2_SPAN == v)
        for name, x, y in zip(('z', 'w', 'mu'), got, ref):
            assert _same(x[rows], y[rows]), (v, name)
        assert _same(got[3][:, rows], ref[3][:, rows]), v
    assert not _same(got[0][0], got[0][5])


def test_span_log_row_wraps(span_base):
    base, _, refs = span_base
    e = _span_engine(base, span=4, n_log=8)
    e.run_span(14)
    z, w, mu, tr = _state(e)
    assert tr.shape == (8, 6)
    for v, ref in refs.items():
        rows = np.flatnonzero(_T2_SPAN == v)
        assert _same(z[rows], ref[0][rows]) and _same(tr[:, rows], ref[3][-8:, rows]), v


def test_span_from_a_non_zero_start(span_base):
    """3 eager steps, then run_span(9): the first span starts inside every outer iteration but T2 = 1's and T2 = 3's."""
    base, _, _ = span_base
    e = _span_engine(base, span=4)
    _steps(3)(e)
    e.run_span(9)
    _check_against_scalars(_state(e), _T2_SPAN, lambda v: _span_engine(base, T2=v), _steps(12), 'start 3')


def test_span_with_per_problem_eta_mb_and_sigma_modifier(span_base):
    base, _, _ = span_base
    eta, mb, sm = np.array([2e3, 900.0, 2e3, 900.0, 1500.0, 1500.0]), np.array([1000, 300, 300, 1000, 600, 600], np.int32), _PP['sm']
    e = _span_engine(base, eta=eta, mb=mb, sm=sm, span=4)
    e.run_span(14)
    got = _state(e)
    st = _span_engine(base, eta=eta, mb=mb, sm=sm, span=4)
    _steps(14)(st)
    for x, y in zip(got, _state(st)):
        assert _same(x, y)
    _check_against_scalars(got, _T2_SPAN, lambda v: _span_engine(base, T2=v, eta=eta, mb=mb, sm=sm), _steps(14), 'per-problem')


def test_span_image_does_not_depend_on_the_batch(span_base):
    """Image 3 of the batch (T2 = 5) == the same image in a batch of one (draw_id = 3: its stream in the batch)."""
    base, one, _ = span_base
    e = _span_engine(base, span=4)
    e.run_span(14)
    z, w, mu, tr = _state(e)
    e1 = _span_engine(one, T2=np.array([5]), span=4, draw_id=[3])
    e1.run_span(14)
    z1, w1, mu1, tr1 = _state(e1)
    assert _same(z[3], z1[0]) and _same(w[3], w1[0]) and _same(mu[3], mu1[0]) and _same(tr[:, 3], tr1[:, 0])


# ------------------------------------------------------------------------------------------------------------------------ sweep
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def test_grid_search_batch_T2_equals_serial(monkeypatch):
    """2 items x {eta: 2 values, T2: [2, 3, 5]}, n_inner = 10, 64 x 64, TV, counter seeding: one batch of 12 problems, the rows of
    batch_trials=False."""
    import functools
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import SvrgEngine
    _force_path(monkeypatch, 10 ** 6)
    items = sweep.make_items(2, [0.4], [20.0])
    mk = functools.partial(sweep.make_runner, _images(2, 64), 'csmri', 'svrg', 'tv', n_inner=10, mini_batch_size=200, H=64, W=64,
                           seeding='counter', t2_trials=True)
    grid = {'eta': [500.0, 60.0], 'T2': [2, 3, 5]}
    key = lambda rows: [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]      # noqa: E731
    serial = sweep.grid_search(items, mk, grid)
    made = []
    init = SvrgEngine.__init__
    monkeypatch.setattr(SvrgEngine, '__init__', lambda self, batch, prox, eta, T2, *a, **k: (made.append((batch.B, np.ndim(T2))),
                                                                                            init(self, batch, prox, eta, T2, *a, **k))[1])
    batched = sweep.grid_search(items, mk, grid, batch_trials=True, batch_T2=True)
    assert made == [(12, 1)]                                     # ONE engine: 2 items x 6 trials, T2 a vector
    assert key(batched) == key(serial)
    made.clear()
    assert key(sweep.grid_search(items, mk, grid, batch_trials=True)) == key(serial)
    assert made == [(4, 0)] * 3                                  # without batch_T2: grouped by T2, as before
