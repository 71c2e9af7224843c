"""Per-problem hist_size for pnp_saga: `SagaEngine` with a [B] hist_size on the streaming path
(`pnp_saga_table_update_hist_pp`), in the one-kernel step (`pnp_csmri_saga_step_hist_pp`) and in the span kernel
(`pnp_csmri_saga_span_hist`), the update kernel alone, and `grid_search(batch_trials=True, batch_hist=True)`.

Everything here is "equal bit for bit" unless it says otherwise: the per-problem engine executes the scalar engine's arithmetic on the
same operands.  The comparison is always the same: one engine gets the hist_size vector; for each distinct value h a scalar engine with
hist_size = h runs on the same batch, seed and draw_id; the problems b with hist[b] == h are compared for z, the log column, tsum[b]
and rows [0, h) of the table.  The one comparison across kernels -- fused against streaming -- holds the bounds
tests/test_gpu_fused_steps.py holds fused engines to: 5e-5 * max(1, |ref|) and 0.01 dB."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIST = np.array([1, 2, 3, 5, 8, 13])
_PP = dict(eta=np.array([300.0, 90.0, 300.0, 90.0, 200.0, 200.0]), mb=np.array([150, 400, 400, 150, 250, 250], np.int32),
           sm=np.array([1.0, 1.4, 1.4, 1.0, 1.2, 0.9]))


def _same(x, y):
    """bit for bit, NaNs included"""
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}[x.dtype]
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(iv), y.contiguous().view(iv))


def _steps(n):
    def go(eng):
        for _ in range(n):
            eng.step()
    return go


def _state(eng):
    torch.cuda.synchronize()
    n = min(eng.n_prox, eng.n_log)
    return eng.z.clone(), eng._ring(eng.sse_log)[:n].clone(), eng.tsum.clone(), eng.table.clone()


def _check_against_scalars(got, hist, make_scalar, advance, what=''):
    """got: (z, log, tsum, table) of the engine that took the vector; make_scalar(h) -> the scalar engine with hist_size = h."""
    seen = []
    for h in sorted(set(int(v) for v in hist)):
        ref = make_scalar(h)
        advance(ref)
        zr, lr, sr, tr = _state(ref)
        assert tr.shape[0] == h and not any(_same(zr, other) for other in seen), (what, h)      # (hist_size does change the walk)
        seen.append(zr)
        for p in np.flatnonzero(np.asarray(hist) == h):
            assert _same(got[0][p], zr[p]), (what, 'hist', h, 'z')
            assert _same(got[1][:, p], lr[:, p]), (what, 'hist', h, 'log')
            assert _same(got[2][p], sr[p]), (what, 'hist', h, 'tsum')
            assert _same(got[3][:h, p], tr[:, p]), (what, 'hist', h, 'table')


def _dead_rows_untouched(eng, hist, g0):
    """rows at or beyond hist[b] of problem b still hold the initial fill"""
    for p, h in enumerate(hist):
        for r in range(int(h), eng.table.shape[0]):
            assert _same(eng.table[r, p], g0[p]), (p, r)


# ------------------------------------------------------------------------------------------------------------ streaming paths
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ['plain', 'per-problem', 'decay'])
def test_streaming_csmri(case, dtype):
    """CSMRI 64 x 64, B = 6, hist = [1, 2, 3, 5, 8, 13], 12 steps: hist = 1 has row == prev_row at every step."""
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.engine import CsmriBatch, SagaEngine, TVProx
    steps = 12
    base = CsmriBatch.synthetic(6, 64, 64, 0.3, 20.0, seed=41, dtype=dtype)
    eta, mb, sm = (_PP['eta'], _PP['mb'], _PP['sm']) if case == 'per-problem' else (250.0, 200, 1.1)
    kw = dict(seed=7, lr_decay=0.9 if case == 'decay' else 1.0)
    eng = SagaEngine(base, TVProx(sigma_modifier=sm), eta, mb, hist_size=HIST, **kw)
    assert not eng.fused and tuple(eng.table.shape) == (13, 6, 64, 64)
    g0 = eng.table[0].clone()
    for p, h in enumerate(HIST):
        assert _same(eng.tsum[p], ops.axpbypcz(float(h), g0)[p])                 # the scalar path's float(hist_size) * g
    _steps(steps)(eng)
    got = _state(eng)
    _check_against_scalars(got, HIST, lambda h: SagaEngine(base, TVProx(sigma_modifier=sm), eta, mb, hist_size=h, **kw), _steps(steps), case)
    _dead_rows_untouched(eng, HIST, g0)
    assert bool(torch.isfinite(got[0]).all()) and not _same(got[0][0] - base.xinit[0], got[0][5] - base.xinit[5])


@pytest.mark.parametrize('kind', ['deblur', 'pr'])
def test_streaming_deblur_and_pr_tiles(kind):
    """DeblurBatch.tile (64 x 64: the smallest image a Deblur plan takes) / PrBatch.tile (32 x 32), f64, B = 4, hist = [1, 2, 3, 7],
    8 steps."""
    from pnp_svrg_amd.engine import DeblurBatch, PrBatch, SagaEngine, TVProx
    hist, steps, n = np.array([1, 2, 3, 7]), 8, 32
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
    kw = dict(seed=2, draw_id=np.tile(np.arange(2), 2))
    eng = SagaEngine(base, TVProx(), eta, mb, hist_size=hist, **kw)
    g0 = eng.table[0].clone()
    _steps(steps)(eng)
    _check_against_scalars(_state(eng), hist, lambda h: SagaEngine(base, TVProx(), eta, mb, hist_size=h, **kw), _steps(steps), kind)
    _dead_rows_untouched(eng, hist, g0)


# ------------------------------------------------------------------------------------------------------ the update kernel alone
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _distinct(shape, dtype, seed):
    """finite values, no two alike: a sentinel in every element"""
    n = int(np.prod(shape))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).double()
    return ((perm + 1.0) / 1024.0 + seed).reshape(shape).to('cuda', dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('n', [4, 4 * 37, 4 * 70001])
def test_update_kernel_alone(dtype, n):
    """B = 5, hist = [1, 2, 4, 4, 7] in a table of 7 rows, N = 4, 148 and 280004 elements (the last: more than one pass of the 256
    workgroups a problem gets at most): problem b equals pnp_saga_table_update_pp called with its own
    divisor; every row of the table but row[b] of problem b -- the rows beyond hist[b] among them -- keeps its sentinels; a NULL
    inv_hist_pp equals pnp_saga_table_update_pp."""
    from pnp_svrg_amd import _native as N, ops
    B, hist = 5, np.array([1, 2, 4, 4, 7])
    row, prev = _dev([0, 1, 3, 2, 6], np.int32), _dev([0, 0, 3, 1, 5], np.int32)      # (row == prev for problems 0 and 2)
    lr = _dev([0.5, 0.25, 0.75, 1.5, 0.125], np.float64)
    inv = _dev([1.0 / int(h) for h in hist], np.float64)
    z0, g, s0 = (_distinct((B, n), dtype, k) for k in (1, 2, 3))
    t0 = _distinct((7, B, n), dtype, 4)
    z, s, t = z0.clone(), s0.clone(), t0.clone()
    ops.saga_table_update_pp(z, g, t, row, prev, s, lr, 1.0 / 7, inv_hist_pp=inv)
    torch.cuda.synchronize()
    for p in range(B):
        zr, sr, tr = z0.clone(), s0.clone(), t0.clone()
        ops.saga_table_update_pp(zr, g, tr, row, prev, sr, lr, 1.0 / int(hist[p]))
        torch.cuda.synchronize()
        assert _same(z[p], zr[p]) and _same(s[p], sr[p]) and _same(t[:, p], tr[:, p]), p
        for r in range(7):
            assert _same(t[r, p], g[p] if r == int(row[p]) else t0[r, p]), (p, r)
    assert not _same(z, z0)
    # NULL inv_hist_pp: the scalar for every problem, i.e. pnp_saga_table_update_pp
    P = lambda x: ctypes.c_void_p(x.data_ptr())                 # noqa: E731
    z1, s1, t1 = z0.clone(), s0.clone(), t0.clone()
    N.call('pnp_saga_table_update_hist_pp', P(z1), P(g), P(t1), P(row), P(prev), P(s1), 0.0, P(lr), 1.0 / 7, None, 7, B, n, ops._DT[dtype], None)
    z2, s2, t2 = z0.clone(), s0.clone(), t0.clone()
    ops.saga_table_update_pp(z2, g, t2, row, prev, s2, lr, 1.0 / 7)
    torch.cuda.synchronize()
    assert _same(z1, z2) and _same(s1, s2) and _same(t1, t2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_update_kernel_argument_errors_leave_the_arrays_alone(dtype):
    from pnp_svrg_amd import _native as N, ops
    B, n = 3, 16
    z, g, s = (_distinct((B, n), dtype, k) for k in (1, 2, 3))
    t = _distinct((2, B, n), dtype, 4)
    keep = [x.clone() for x in (z, s, t)]
    row, prev, inv = _dev([0, 1, 1], np.int32), _dev([0, 0, 1], np.int32), _dev([1.0, 0.5, 0.5], np.float64)
    h = N.lib()
    P = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)    # noqa: E731
    ok = [P(z), P(g), P(t), P(row), P(prev), P(s), 0.5, None, 0.5, P(inv), 2, B, n, ops._DT[dtype], None]
    es = z.element_size()
    bad = {'N % 4': (12, n - 2), 'N 0': (12, 0), 'z misaligned': (0, P(z, es)), 'g misaligned': (1, P(g, es)), 'table misaligned': (2, P(t, es)),
           'sum misaligned': (5, P(s, es)), 'null row': (3, None), 'hist 0': (10, 0), 'batch 0': (11, 0), 'dtype': (13, 2)}
    for what, (pos, val) in bad.items():
        args = list(ok)
        args[pos] = val
        assert h.pnp_saga_table_update_hist_pp(*args) == 1, what     # PNP_ERR_ARG
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip((z, s, t), keep)), what
    assert h.pnp_saga_table_update_hist_pp(*ok) == 0
    torch.cuda.synchronize()
    assert not _same(z, keep[0])


# ------------------------------------------------------------------------------------------------------- fused step and span
N_SPAN = 20


def _fused_engine(base, hist=HIST, eta=2e3, mb=1000, sm=1.1, fused=True, **kw):
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    return SagaEngine(base, TVProx(sigma_modifier=sm), eta, mb, hist_size=hist, seed=4, fused=fused, **kw)


@pytest.fixture(scope='module')
def fused_base():
    """The 256 x 256 f32 batch of the fused tests (B = 6) and the state of the fused vector engine after 20 eager steps, computed once."""
    from pnp_svrg_amd.engine import CsmriBatch
    base = CsmriBatch.synthetic(6, 256, 256, 0.3, 20.0, seed=51)
    e = _fused_engine(base)
    _steps(N_SPAN)(e)
    return base, _state(e), (np.array(e.r_prev), e._rows[0].copy(), e._rows[1].clone())


def test_fused_step_equals_scalar_fused_engines_and_the_streaming_engine(fused_base, monkeypatch):
    """256 x 256, B = 6, f32, TV, hist = [1, 2, 3, 5, 8, 13], 6 steps, fused=True: bit for bit the scalar fused engines; against the
    streaming vector engine 5e-5 * max(1, |ref|) on z, tsum and the live table rows, 0.01 dB on every PSNR."""
    from pnp_svrg_amd import _native as N
    base, _, _ = fused_base
    steps = 6
    names = []
    real = N.call
    monkeypatch.setattr(N, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    ef = _fused_engine(base)
    g0 = ef.table[0].clone()
    names.clear()
    _steps(steps)(ef)
    assert names.count('pnp_csmri_saga_step_hist_pp') == steps and 'pnp_csmri_saga_step_pp' not in names and 'pnp_csmri_saga_step' not in names
    got = _state(ef)
    monkeypatch.setattr(N, 'call', real)
    _check_against_scalars(got, HIST, lambda h: _fused_engine(base, hist=h), _steps(steps), 'fused')
    _dead_rows_untouched(ef, HIST, g0)
    eu = _fused_engine(base, fused=False)
    _steps(steps)(eu)
    torch.cuda.synchronize()
    rel = lambda x, y: (x - y).abs().max().item() / max(1.0, y.abs().max().item())        # noqa: E731
    dp = np.abs(ef.psnr_trace() - eu.psnr_trace()).max()
    live = torch.stack([torch.arange(13, device='cuda') < int(h) for h in HIST], 1)[:, :, None, None]
    dt = rel(torch.where(live, ef.table, 0.0), torch.where(live, eu.table, 0.0))
    print(f'fused vs streaming: |z| {rel(ef.z, eu.z):.3e}, tsum {rel(ef.tsum, eu.tsum):.3e}, table {dt:.3e} (bound 5e-5), PSNR {dp:.4f} dB')
    assert rel(ef.z, eu.z) <= 5e-5 and rel(ef.tsum, eu.tsum) <= 5e-5 and dt <= 5e-5
    assert dp <= 0.01 + 1e-9


def test_span_equals_stepping(fused_base, monkeypatch):
    """run_span(20) crosses one AHEAD = 16 launch boundary: two launches, the bits of 20 eager fused steps, r_prev and _rows left as
    stepping leaves them."""
    from pnp_svrg_amd import _native as N
    base, ref, (r_prev, rows_host, rows_dev) = fused_base
    names = []
    real = N.call
    e = _fused_engine(base)
    assert e.span_kernel_ok()
    monkeypatch.setattr(N, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    e.run_span(N_SPAN)
    assert names.count('pnp_csmri_saga_span_hist') == 2 and len(names) == 4 and not [n for n in names if 'saga_step' in n], names
    assert (e.s, e.n_prox, e.prox.t) == (N_SPAN, N_SPAN, N_SPAN)
    for x, y in zip(_state(e), ref):
        assert _same(x, y)
    assert np.array_equal(e.r_prev, r_prev) and e.r_prev.dtype == r_prev.dtype and e._rows[0] is e.r_prev
    assert np.array_equal(e._rows[0], rows_host) and torch.equal(e._rows[1], rows_dev) and e._rows[1].dtype == torch.int32
    e.step()                                                     # ... and an eager step goes on from there as from stepping
    st = _fused_engine(base)
    _steps(N_SPAN + 1)(st)
    for x, y in zip(_state(e), _state(st)):
        assert _same(x, y)


def test_span_log_row_wraps(fused_base):
    base, ref, _ = fused_base
    e = _fused_engine(base, n_log=8)
    e.run_span(N_SPAN)
    z, log, tsum, table = _state(e)
    assert log.shape == (8, 6)
    assert _same(z, ref[0]) and _same(log, ref[1][-8:]) and _same(tsum, ref[2]) and _same(table, ref[3])


def test_span_with_explicit_rows_and_from_a_non_zero_start(fused_base):
    """3 eager steps, then run_span(17, r=[17][B]); and the engine's own rows from a non-zero start against the 20 eager steps."""
    base, ref, _ = fused_base
    rng = np.random.default_rng(3)
    rows = np.stack([rng.integers(0, HIST) for _ in range(N_SPAN)])              # [20][B], every problem below its own bound
    assert rows.shape == (N_SPAN, 6) and (rows < HIST).all() and rows[:, 5].max() >= 8
    e = _fused_engine(base)
    for s in range(3):
        e.step(r=rows[s])
    e.run_span(N_SPAN - 3, r=rows[3:])
    st = _fused_engine(base)
    for s in range(N_SPAN):
        st.step(r=rows[s])
    for x, y in zip(_state(e), _state(st)):
        assert _same(x, y)
    assert np.array_equal(e.r_prev, st.r_prev) and torch.equal(e._rows[1], st._rows[1])
    _check_against_scalars(_state(e), HIST, lambda h: _fused_engine(base, hist=h),
                           lambda eng: [eng.step(r=np.minimum(rows[s], eng.hist - 1)) for s in range(N_SPAN)], 'explicit rows')
    e = _fused_engine(base)                                      # the engine's own row streams, a span that starts at step 3
    _steps(3)(e)
    e.run_span(N_SPAN - 3)
    for x, y in zip(_state(e), ref):
        assert _same(x, y)
    with pytest.raises(ValueError, match=r'problem 0: rows in \[0, 1\), got 1'):
        e.run_span(2, r=np.ones((2, 6), np.int64))


def test_span_with_per_problem_eta_mb_and_sigma_modifier(fused_base):
    base, _, _ = fused_base
    eta, mb = np.array([2e3, 900.0, 2e3, 900.0, 1500.0, 1500.0]), np.array([1000, 300, 300, 1000, 600, 600], np.int32)
    kw = dict(eta=eta, mb=mb, sm=_PP['sm'])
    e = _fused_engine(base, **kw)
    e.run_span(N_SPAN)
    _check_against_scalars(_state(e), HIST, lambda h: _fused_engine(base, hist=h, **kw), _steps(N_SPAN), 'per-problem')


@pytest.mark.parametrize('fused', [False, True], ids=['streaming', 'fused'])
def test_a_batch_of_one_with_a_length_one_vector_equals_the_scalar_engine(fused):
    from pnp_svrg_amd.engine import CsmriBatch
    n = 256 if fused else 64
    one = CsmriBatch.synthetic(1, n, n, 0.3, 20.0, seed=19)
    eta, mb = (2e3, 1000) if fused else (250.0, 200)
    e = _fused_engine(one, hist=np.array([3]), eta=eta, mb=mb, fused=fused)
    r = _fused_engine(one, hist=3, eta=eta, mb=mb, fused=fused)
    for eng in (e, r):
        _steps(5)(eng)
        eng.run_span(4)
    for x, y in zip(_state(e), _state(r)):
        assert _same(x, y)


# ------------------------------------------------------------------------------------------------------------------------ sweep
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


@pytest.mark.parametrize('cell', ['csmri-tv', 'deblur-nlm'])
def test_grid_search_batch_hist_equals_serial(cell, monkeypatch):
    """2 items x {eta: 2 values, hist_size: [2, 3, 5]}, n_inner = 8, 64 x 64, counter seeding: ONE batch of 12 problems, the rows of
    batch_trials=False; without batch_hist the grid splits by hist_size, as before."""
    import functools
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import SagaEngine
    if cell == 'csmri-tv':
        items = sweep.make_items(2, [0.4], [20.0])
        mk = functools.partial(sweep.make_runner, _images(2, 64), 'csmri', 'saga', 'tv', n_inner=8, mini_batch_size=200, H=64, W=64,
                               seeding='counter', wide_trials=True, hist_trials=True)
        grid = {'eta': [300.0, 60.0], 'hist_size': [2, 3, 5]}
    else:
        items = sweep.make_items(2, [1.0], [20.0])
        mk = functools.partial(sweep.make_runner, _images(2, 64), 'deblur', 'saga', 'nlm', n_inner=8, mini_batch_size=500, H=64, W=64,
                               seeding='counter', wide_trials=True, hist_trials=True)
        grid = {'eta': [2e4, 3e3], 'hist_size': [2, 3, 5]}
    key = lambda rows: [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]      # noqa: E731
    serial = sweep.grid_search(items, mk, grid)
    assert len(serial) == 2 and all(np.isfinite(r['loss']) for r in serial)
    made = []
    init = SagaEngine.__init__
    monkeypatch.setattr(SagaEngine, '__init__', lambda self, batch, *a, hist_size=50, **k: (
        made.append((batch.B, np.ndim(hist_size))), init(self, batch, *a, hist_size=hist_size, **k))[1])
    batched = sweep.grid_search(items, mk, grid, batch_trials=True, batch_hist=True)
    assert made == [(12, 1)]                                     # ONE engine: 2 items x 6 trials, hist_size a vector
    assert key(batched) == key(serial)
    made.clear()
    assert key(sweep.grid_search(items, mk, grid, batch_trials=True)) == key(serial)
    assert made == [(4, 0)] * 3                                  # without batch_hist: grouped by hist_size, as before
