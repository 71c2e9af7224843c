"""Per-problem T2 for pnp_sarah: `pnp_select_pp` alone, `SarahEngine(T2=[B] ints, split_log=True)` on the streaming
path, on the per-step one-kernel path and in the span kernel (`pnp_csmri_sarah_span_pp`), and
`grid_search(batch_trials=True, batch_T2=True)` on a `sarah_t2_trials` runner.

Everything here is "equal bit for bit": the per-problem engine executes the scalar engine's arithmetic on the same operands.  The
judge is always a scalar `SarahEngine` with T2[b] (and b's eta, mini_batch_size, sigma_modifier, draw_id) -- on problem b ALONE, a
batch of one, for CSMRI; on the same tiled batch for the Deblur and PR tiles, whose problems share one plan / one matrix kernel (bit
equality can be asked of the same kernel only, as in test_gpu_sarah_per_problem.py)."""
import functools

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


def _steps(n):
    def go(eng):
        for _ in range(n):
            eng.step()
    return go


def _state(eng):
    torch.cuda.synchronize()
    return eng.z.clone(), eng.w_prev.clone(), eng.w_next.clone(), eng.v_prev.clone()


def _at(v, b):
    return v if np.ndim(v) == 0 else v[b].item()


def _one(base, b):
    """Problem b of a CsmriBatch as a batch of one."""
    from pnp_svrg_amd.engine import CsmriBatch
    return CsmriBatch(base.xrec[b:b + 1].cpu().numpy(), base.mask_np[b:b + 1], np.swapaxes(base.YT[b:b + 1].cpu().numpy(), 1, 2),
                      base.xinit[b:b + 1].cpu().numpy().reshape(1, -1), dtype=base.dtype)


def _check_alone(eng, base, T2, eta, mb, sm, advance, what='', **kw):
    """eng took the vector on `base`; for every problem b a scalar engine with b's values runs on b alone."""
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    got = _state(eng)
    for b in range(base.B):
        ref = SarahEngine(_one(base, b), TVProx(sigma_modifier=_at(sm, b)), _at(eta, b), int(T2[b]), _at(mb, b), draw_id=[b], **kw)
        advance(ref)
        for name, x, y in zip(('z', 'w_prev', 'w_next', 'v_prev'), got, _state(ref)):
            assert _same(x[b], y[0]), (what, 'problem', b, name)
        assert _same(eng.psnr_trace_of(b), ref.psnr_trace()[:, 0]), (what, 'problem', b, 'trace')
    return got


# ---------------------------------------------------------------------------------------------------------- pnp_select_pp alone
def _sentinel(shape, dtype, word):
    """a NaN-free bit pattern no copy could produce by accident"""
    it = {torch.float32: (torch.int32, word), torch.float64: (torch.int64, (word << 32) | 0x1234567)}[dtype]
    return torch.full(shape, it[1], dtype=it[0], device='cuda').view(dtype)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('len_,off', [(4 * 700 + 4, 0), (4 * 37 + 3, 0), (4 * 37 + 4, 1), (4, 0)],
                         ids=['aligned', 'odd-length', 'unaligned', 'one-vector'])
def test_select_pp_alone(dtype, len_, off):
    """B = 5, t2 = [1, 2, 3, 4, 7] at steps 0, 6, 7: adopted problems equal src, the others keep the sentinel bit for bit, row_out
    holds NaN exactly where nothing was adopted, the NaN guard bands around dst stay intact.  `off` shifts src and dst by one element
    off 16-byte alignment (the element-by-element path, as an odd length)."""
    from pnp_svrg_amd import _native as N, ops
    B, T2, G = 5, np.array([1, 2, 3, 4, 7]), 8
    g = torch.Generator().manual_seed(len_)
    src_buf = torch.rand(B * len_ + off, generator=g, dtype=torch.float64).to('cuda', dtype)
    src = src_buf[off:].view(B, len_)
    row_in = torch.rand(B, generator=g, dtype=torch.float64).cuda()
    t2 = _dev(T2, np.int32)
    for step in (0, 6, 7):
        buf = torch.full((G + off + B * len_ + G,), float('nan'), dtype=dtype, device='cuda')
        dst = buf[G + off:G + off + B * len_].view(B, len_)
        dst.copy_(_sentinel((B, len_), dtype, 0x3DA5C3E1))
        keep = dst.clone()
        row_out = torch.full((B,), 7.0, dtype=torch.float64, device='cuda')
        assert (dst.data_ptr() % 16 == 0) == (off == 0)
        if off:                                                  # (views that are no whole tensors: the raw call)
            N.call('pnp_select_pp', src.data_ptr(), dst.data_ptr(), row_in.data_ptr(), row_out.data_ptr(), t2.data_ptr(), step, B * len_, B,
                   ops._DT[dtype], ops._stream())
        else:
            ops.select_pp(src, dst, t2, step, row_in, row_out)
        torch.cuda.synchronize()
        sel = step % T2 == 0
        assert sel.tolist() == {0: [True] * 5, 6: [True, True, True, False, False], 7: [True, False, False, False, True]}[step]
        for p in range(B):
            assert _same(dst[p], src[p] if sel[p] else keep[p]), (step, p)
        assert _same(row_out, torch.where(torch.from_numpy(sel).cuda(), row_in, torch.full_like(row_in, float('nan'))))
        assert bool(torch.isnan(buf[:G + off]).all()) and bool(torch.isnan(buf[G + off + B * len_:]).all())
    dst2 = _sentinel((B, len_), dtype, 0x3E5A3C1E)               # without the rows: the copies alone
    ops.select_pp(src.contiguous(), dst2, t2, 6)
    torch.cuda.synchronize()
    assert _same(dst2[:3], src[:3]) and _same(dst2[3:], _sentinel((2, len_), dtype, 0x3E5A3C1E))


# ------------------------------------------------------------------------------------------------------------ streaming path
_T2_6 = np.array([1, 2, 3, 5, 8, 13])
_PP = dict(eta=np.array([500.0, 90.0, 500.0, 90.0, 300.0, 300.0]), mb=np.array([150, 400, 400, 150, 250, 250], np.int32),
           sm=np.array([1.0, 1.4, 1.4, 1.0, 1.2, 0.9]))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', ['per-problem', 'decay'])
def test_streaming_csmri(case, dtype):
    """CSMRI 64 x 64, B = 6, T2 = [1, 2, 3, 5, 8, 13], 14 steps: T2 = 1 takes an outer step at every step, T2 = 13 at s = 0 and 13."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    steps = 14
    base = CsmriBatch.synthetic(6, 64, 64, 0.3, 20.0, seed=41, dtype=dtype)
    eta, mb, sm = (_PP['eta'], _PP['mb'], _PP['sm']) if case == 'per-problem' else (400.0, 200, 1.1)
    kw = dict(seed=7, lr_decay=0.9 if case == 'decay' else 1.0)
    eng = SarahEngine(base, TVProx(sigma_modifier=sm), eta, _T2_6, mb, split_log=True, **kw)
    assert not eng.fused and not eng.graph_ok() and not eng.outer_kernel_ok()
    _steps(steps)(eng)
    assert (eng.s, eng.n_prox) == (steps, steps)
    got = _check_alone(eng, base, _T2_6, eta, mb, sm, _steps(steps), case, **kw)
    otr = eng.outer_trace()
    assert np.array_equal(np.isnan(otr), np.arange(steps)[:, None] % _T2_6[None, :] != 0) and not np.isnan(eng.psnr_trace()).any()
    assert not _same(got[0][0], got[0][5]) and not _same(got[2][0], got[2][5])          # (the problems do differ)


@pytest.mark.parametrize('kind', ['deblur', 'pr'])
def test_streaming_deblur_and_pr_tiles(kind):
    """DeblurBatch.tile (64 x 64: the smallest image a Deblur plan takes) / PrBatch.tile (32 x 32), f64, B = 4, T2 = [1, 2, 3, 7],
    8 steps: rows with T2[b] == v against the scalar-T2 = v engine on the same tiled batch."""
    from pnp_svrg_amd.engine import DeblurBatch, PrBatch, SarahEngine, TVProx
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
    kw = dict(seed=2, draw_id=np.tile(np.arange(2), 2))
    eng = SarahEngine(base, TVProx(), eta, T2, mb, split_log=True, **kw)
    _steps(steps)(eng)
    got = _state(eng)
    for b, v in enumerate(T2.tolist()):
        ref = SarahEngine(base, TVProx(), eta, v, mb, **kw)
        _steps(steps)(ref)
        for name, x, y in zip(('z', 'w_prev', 'w_next', 'v_prev'), got, _state(ref)):
            assert _same(x[b], y[b]), (kind, 'T2', v, name)
        assert _same(eng.psnr_trace_of(b), ref.psnr_trace()[:, b]), (kind, 'T2', v)


# ---------------------------------------------------------------------------------- the one-kernel paths: per step, and the span
_T2_SPAN = np.array([1, 2, 3, 5, 7, 40])
_ETA = np.array([2e3, 900.0, 2e3, 900.0, 1500.0, 1500.0])
_MB = np.array([1000, 300, 300, 1000, 600, 600], np.int32)


@pytest.fixture(scope='module')
def span_base():
    """The 256 x 256 f32 batch of the one-kernel tests (B = 6) and, computed once, the scalar fused=True engines on every problem
    alone with the per-problem coefficients: b -> {steps: (state, trace)} after 9 and after 14 steps."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    base = CsmriBatch.synthetic(6, 256, 256, 0.3, 20.0, seed=51)
    refs = {}
    for b in range(6):
        e = SarahEngine(_one(base, b), TVProx(sigma_modifier=_PP['sm'][b].item()), _ETA[b].item(), int(_T2_SPAN[b]), _MB[b].item(), seed=4,
                        draw_id=[b], fused=True)
        _steps(9)(e)
        refs[b] = {9: (_state(e), e.psnr_trace()[:, 0].copy())}
        _steps(5)(e)
        refs[b][14] = (_state(e), e.psnr_trace()[:, 0].copy())
    return base, refs


def _fused_engine(base, T2=_T2_SPAN, eta=_ETA, mb=_MB, sm=_PP['sm'], **kw):
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    e = SarahEngine(base, TVProx(sigma_modifier=sm), eta, T2, mb, seed=4, fused=True, split_log=True, **kw)
    assert e.fused and e.outer_kernel_ok() and not e.graph_ok()
    return e


def _check_refs(eng, refs, steps, what):
    got = _state(eng)
    for b, ref in refs.items():
        st, tr = ref[steps]
        for name, x, y in zip(('z', 'w_prev', 'w_next', 'v_prev'), got, st):
            assert _same(x[b], y[0]), (what, 'problem', b, name)
        assert _same(eng.psnr_trace_of(b), tr), (what, 'problem', b, 'trace')
    return got


def test_fused_per_step_path(span_base, monkeypatch):
    """256 x 256, B = 6, T2 = [1, 2, 3, 5, 7, 40], 9 steps of `step()` with fused=True: T2 = 1 takes an outer step at every step, T2 =
    40 only the initial one.  ONE pnp_csmri_svrg_outer_step + pnp_refresh_pp + pnp_select_pp where any problem refreshes."""
    from pnp_svrg_amd import _native as N
    base, refs = span_base
    names, real = [], N.call
    monkeypatch.setattr(N, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    e = _fused_engine(base)
    _steps(9)(e)
    got = _check_refs(e, refs, 9, 'per step')
    assert names.count('pnp_csmri_svrg_outer_step_pp') == names.count('pnp_refresh_pp') == names.count('pnp_select_pp') == 9
    assert names.count('pnp_csmri_sarah_step_pp') == 9 and 'pnp_csmri_sarah_span_pp' not in names
    assert not _same(got[0][0], got[0][5])


def test_span_equals_stepping_and_the_scalar_engines(span_base, monkeypatch):
    """span = 4, n_log = 8 (both rings wrap): three eager steps, then run_span(11) -- launches of 4, 4 and 3 steps from s = 3, 7 and 11:
    starts inside the outer iterations of T2 = 2, 5, 7 and 40, exactly on a refresh of T2 = 3 (s = 3) and of T2 = 7 (s = 7) -- against
    14 eager steps of a twin engine, both rings row for row with their NaNs, and against the scalar engines."""
    from pnp_svrg_amd import _native as N
    base, refs = span_base
    names, real = [], N.call
    monkeypatch.setattr(N, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    e = _fused_engine(base, span=4, n_log=8)
    _steps(3)(e)
    names.clear()
    e.run_span(11)
    got = _state(e)
    assert names.count('pnp_csmri_sarah_span_pp') == 3 and names.count('pnp_csmri_draw_thresholds_pp') == 3 and len(names) == 6, names
    assert (e.s, e.n_prox, e.prox.t) == (14, 14, 6 + 11)
    twin = _fused_engine(base, span=4, n_log=8)
    _steps(14)(twin)
    for x, y in zip(got, _state(twin)):
        assert _same(x, y)
    assert _same(e.sse_log, twin.sse_log) and _same(e.outer_log, twin.outer_log)
    want_nan = np.array([[(s % t) != 0 for t in _T2_SPAN] for s in range(6, 14)])
    assert np.array_equal(np.isnan(e.outer_trace()), want_nan) and not np.isnan(e.psnr_trace()).any()
    for b, ref in refs.items():                                  # the scalar engines: states, and the rows that survive in the rings
        for name, x, y in zip(('z', 'w_prev', 'w_next', 'v_prev'), got, ref[14][0]):
            assert _same(x[b], y[0]), (b, name)
        tr, v, rows = ref[14][1], int(_T2_SPAN[b]), []
        it = iter(tr)
        for s in range(14):
            o = next(it) if s % v == 0 else None
            i = next(it)
            if s >= 6:
                rows += ([o] if o is not None else []) + [i]
        assert _same(e.psnr_trace_of(b), np.array(rows)), b
    assert not _same(got[0][0], got[0][5])


def test_span_unwrapped_traces_and_a_batch_of_one(span_base):
    """run_span(14) from step 0 (default n_log): psnr_trace_of(b) equals the scalar engines' traces element for element; and image 3 of
    the batch (T2 = 5) equals the same image in a batch of one (draw_id = 3: its stream in the batch)."""
    base, refs = span_base
    e = _fused_engine(base, span=4)
    e.run_span(14)
    got = _check_refs(e, refs, 14, 'span')
    e1 = _fused_engine(_one(base, 3), T2=np.array([5]), eta=_ETA[3:4], mb=_MB[3:4], sm=_PP['sm'][3:4], span=4, draw_id=[3])
    e1.run_span(14)
    for x, y in zip(got, _state(e1)):
        assert _same(x[3], y[0])
    assert _same(e.psnr_trace()[:, 3], e1.psnr_trace()[:, 0]) and _same(e.outer_trace()[:, 3], e1.outer_trace()[:, 0])


# ------------------------------------------------------------------------------------------------------------------------ sweep
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def test_grid_search_batch_T2_equals_serial(monkeypatch):
    """2 items x {eta: 2 values, T2: [2, 3, 5]}, n_inner = 6, CSMRI 256 x 256 with the one-kernel forms (the span kernel), TV, counter
    seeding: ONE engine of 12 problems; the best rows are those of batch_trials=False, and every trial's rows -- 'psnr_trace'
    included -- are those of the per-trial runner."""
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import SarahEngine
    items = sweep.make_items(2, [0.4], [20.0])
    mk = functools.partial(sweep.make_runner, _images(2, 256), 'csmri', 'sarah', 'tv', n_inner=6, mini_batch_size=1000, seeding='counter',
                           sarah_trials=True, sarah_t2_trials=True, sarah_fused=True, keep_trace=True, graph=False)
    grid = {'eta': [2e3, 900.0], 'T2': [2, 3, 5]}
    key = lambda rows: [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]      # noqa: E731
    serial = sweep.grid_search(items, mk, grid)
    made, spans = [], []
    init, span = SarahEngine.__init__, SarahEngine.run_span
    monkeypatch.setattr(SarahEngine, '__init__', lambda self, batch, prox, eta, T2, *a, **k: (made.append((batch.B, np.ndim(T2))),
                                                                                             init(self, batch, prox, eta, T2, *a, **k))[1])
    monkeypatch.setattr(SarahEngine, 'run_span', lambda self, n: (spans.append((n, self.outer_kernel_ok())), span(self, n))[1])
    batched = sweep.grid_search(items, mk, grid, batch_trials=True, batch_T2=True)
    assert made == [(12, 1)] and spans == [(6, True)]            # ONE engine: 2 items x 6 trials, T2 a vector, the launch form
    assert key(batched) == key(serial)
    made.clear()
    assert key(sweep.grid_search(items, mk, grid, batch_trials=True)) == key(serial)
    assert made == [(4, 0)] * 3                                  # without batch_T2: grouped by T2, as before
    # trial by trial, with the traces
    trials = sweep.grid_points(grid)
    run = mk(eta=2e3, T2=2)
    rows = run.run_trials(run.prepare_data(items), trials)
    for tr, got in zip(trials, rows):
        want = mk(**tr)(items)
        assert [r['id'] for r in got] == [r['id'] for r in want]
        for g, w in zip(got, want):
            assert (g['psnr_final'], g['loss'], g['psnr_init']) == (w['psnr_final'], w['loss'], w['psnr_init']), tr
            assert _same(g['psnr_trace'], w['psnr_trace']) and np.array_equal(g['z'], w['z']), tr
