"""GPU side of the device objective f(z) = ||Y - forward_model(z)||^2 / 2 / M: pnp_csmri_objective, pnp_deblur_objective and
pnp_pr_objective behind `batch.objective`, the engines' `log_objective`, the sweep's `objective` / `score`, and the drop-in
problems' `objective`, against the float64 restatement of tests/objective_ref.py.

Tolerances.  f64: |f - ref| <= 1e-12 * max(1, |ref|).  f32: no bound fixed in advance -- the yardstick is an independent pipeline
on the same f32 inputs (complex64 torch.fft.fft2 for CSMRI, complex64 1-D torch.fft for Deblur, a float32 torch.matmul for PR,
each reduced in float64), and over the problems of a case the kernel's largest relative error against the restatement may be at
most 4 x the yardstick's (the margin of test_gpu_csmri_generate.py, for the same reason: both sit on the f32 rounding of the
largest spectrum entries / dot products).  Every case prints both errors."""
import gc

import numpy as np
import pytest
import torch

import objective_ref as oref

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _free_plans():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _r32(a):
    """Round to what an f32 batch holds, so that f32 and f64 batches and the restatement all see the same numbers."""
    a = np.asarray(a)
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


def _smooth(rng, n):
    p = np.pad(rng.random((n, n)), 2, mode='wrap')
    y = sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0
    return _r32((y - y.min()) / (y.max() - y.min()))


def _check(name, dtype, got, ref, yard=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if dtype == F64:
        err = np.abs(got - ref)
        tol = 1e-12 * np.maximum(1.0, np.abs(ref))
        print(f'{name} f64: f {ref.tolist()} |err| {err.tolist()} (tol {tol.tolist()}), rel {(err / np.abs(ref)).max():.3e}')
        assert (err <= tol).all()
        # and relative to f itself (the Deblur values are about 1e-6, where the absolute bound says little): a float64 transform
        # of at most 128 x 128 points is good to about 1e-14 of its largest entry, and at the iterates used here the residuals are
        # not below 1e-3 of those entries -- 1e-11, with a factor ten to spare
        assert (err <= 1e-10 * np.abs(ref)).all()
        return
    e_k, e_y = (np.abs(got - ref) / np.abs(ref)).max(), (np.abs(np.asarray(yard, np.float64) - ref) / np.abs(ref)).max()
    print(f'{name} f32: f {ref.tolist()} kernel rel err {e_k:.3e}, yardstick rel err {e_y:.3e} (ratio {e_k / e_y if e_y else np.inf:.2f})')
    assert e_k <= 4 * e_y


# ------------------------------------------------------------------------------------------------ CSMRI
_CS = {}


def _csmri_data(n, alphas=(0.1, 0.5, 1.0), seed=0):
    """(xrec, mask, Y, z) of len(alphas) problems: Bernoulli masks, COMPLEX noise on the support (no symmetry left in Y), z = an
    |ifft2 Y|-like initialisation; everything rounded to f32 values.  Built once per key and left unchanged."""
    key = (n, alphas, seed)
    if key not in _CS:
        rng = np.random.default_rng(100 * n + seed)
        B = len(alphas)
        xrec = np.stack([_smooth(rng, n) for _ in range(B)])
        mask = np.stack([(rng.random((n, n)) < a).astype(np.uint8) for a in alphas])
        Y = np.empty((B, n, n), np.complex128)
        z = np.empty((B, n, n))
        for b in range(B):
            noise = rng.normal(0, 0.3, (n, n)) + 1j * rng.normal(0, 0.3, (n, n))
            Y[b] = _r32(mask[b] * (np.fft.fft2(xrec[b]) + noise))
            xi = np.abs(np.fft.ifft2(Y[b]))
            z[b] = _r32((xi - xi.min()) / (xi.max() - xi.min()))
        _CS[key] = (xrec, mask, Y, z)
    return _CS[key]


def _csmri_batch(data, dtype, sl=slice(None)):
    from pnp_svrg_amd.engine import CsmriBatch
    xrec, mask, Y, z = data
    return CsmriBatch(xrec[sl], mask[sl], Y[sl], z[sl].reshape(len(xrec[sl]), -1), dtype=dtype)


def _csmri_yard(mask, Y, z):
    out = []
    for b in range(len(z)):
        Z = torch.fft.fft2(torch.from_numpy(z[b].astype(np.float32)).cuda().to(torch.complex64))
        r = torch.from_numpy(Y[b].astype(np.complex64)).cuda() - torch.from_numpy(mask[b].astype(np.float32)).cuda() * Z
        r = r.to(torch.complex128)
        out.append(float((r.real ** 2 + r.imag ** 2).sum() / 2 / z[b].size))
    return out


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('n', [64, 128])
def test_csmri_objective_mixed_sampling_ratios(n, dtype):
    data = _csmri_data(n)
    xrec, mask, Y, z = data
    b = _csmri_batch(data, dtype)
    got = b.objective(b.xinit).cpu().numpy()
    ref = [oref.csmri_f(z[j], mask[j], Y[j]) for j in range(3)]
    _check(f'csmri {n}', dtype, got, ref, _csmri_yard(mask, Y, z) if dtype == F32 else None)
    out = torch.full((3,), -1.0, dtype=F64, device='cuda')
    assert b.objective(b.xinit, out=out) is out and np.array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('n', [64, 128])
def test_csmri_objective_packed_column_and_mirrored_pair(n, dtype):
    """A hand-made mask: the four self-conjugate entries (the packed column kx = 0 / W/2 at ky = 0 / H/2) and the mirrored pair
    (1, W-1), (H-1, 1), with complex Y on it -- each entry alone as well, so that a slip at one of them cannot hide in the sum."""
    rng = np.random.default_rng(7 + n)
    pts = [(0, 0), (0, n // 2), (n // 2, 0), (n // 2, n // 2), (1, n - 1), (n - 1, 1)]
    sets = [pts] + [[p] for p in pts]
    B = len(sets)
    x = _smooth(rng, n)
    mask = np.zeros((B, n, n), np.uint8)
    Y = np.zeros((B, n, n), np.complex128)
    for j, ps in enumerate(sets):
        for ky, kx in ps:
            mask[j, ky, kx] = 1
            Y[j, ky, kx] = _r32(np.complex128(rng.normal(0, 30.0) + 1j * rng.normal(0, 30.0)))
    z = np.stack([_r32(rng.random((n, n))) for _ in range(B)])
    b = _csmri_batch((np.stack([x] * B), mask, Y, z), dtype)
    got = b.objective(b.xinit).cpu().numpy()
    ref = [oref.csmri_f(z[j], mask[j], Y[j]) for j in range(B)]
    _check(f'csmri {n} hand-made mask', dtype, got, ref, _csmri_yard(mask, Y, z) if dtype == F32 else None)


# ------------------------------------------------------------------------------------------------ Deblur
_DB = {}


def _deblur_data(scale_percent, B=3, n=64):
    key = (scale_percent, B, n)
    if key not in _DB:
        rng = np.random.default_rng(11 + scale_percent)
        Bk = _r32(oref.minimal_kernel(n, n))
        taps = oref.deblur_taps(n, n, scale_percent)
        xrec = np.stack([_smooth(rng, n) for _ in range(B)])
        Y = np.stack([_r32(oref.deblur_forward(x, Bk, taps)) for x in xrec])
        Y = _r32(Y + rng.normal(0, 2e-4, Y.shape))
        z = _r32(rng.uniform(0.0, 1.0, (B, n * n)))
        _DB[key] = (xrec, Bk, Y, z, taps)
    return _DB[key]


def _deblur_batch(data, dtype, sl=slice(None), n=64):
    from pnp_svrg_amd.engine import DeblurBatch
    from pnp_svrg_amd.problems import _deblur_taps
    xrec, Bk, Y, z, taps = data
    sp = 100 if taps is None else 50
    return DeblurBatch(xrec[sl], Bk, Y[sl], z[sl], dtype=dtype, bilinear=_deblur_taps(n, n, sp))


def _taps32(taps):
    """The taps as an f32 plan holds them (weights rounded to f32)."""
    return None if taps is None else (taps[0], _r32(taps[1]))


def _deblur_yard(Bk, Y, z, taps):
    out = []
    FB = torch.fft.fft(torch.from_numpy(Bk.astype(np.float32)).cuda().to(torch.complex64))
    for b in range(len(z)):
        zc = torch.from_numpy(z[b].astype(np.float32)).cuda().to(torch.complex64)
        y = torch.fft.ifft(torch.fft.fft(zc) * FB).real * np.float32(np.sqrt(z[b].size))
        if taps is not None:
            idx, w = torch.from_numpy(taps[0]).cuda(), torch.from_numpy(taps[1].astype(np.float32)).cuda()
            y = (w * y[idx]).sum(1)
        r = (torch.from_numpy(Y[b].astype(np.float32)).cuda() - y).double()
        out.append(float((r ** 2).sum() / 2 / r.numel()))
    return out


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('scale_percent', [100, 50])
def test_deblur_objective(scale_percent, dtype):
    data = _deblur_data(scale_percent)
    xrec, Bk, Y, z, taps = data
    b = _deblur_batch(data, dtype)
    assert b.M == (64 * scale_percent // 100) ** 2
    got = b.objective(b.xinit).cpu().numpy()
    t = taps if dtype == F64 else _taps32(taps)
    ref = [oref.deblur_f(z[j], Bk, Y[j], t) for j in range(3)]
    _check(f'deblur scale_percent={scale_percent}', dtype, got, ref, _deblur_yard(Bk, Y, z, t) if dtype == F32 else None)


# ------------------------------------------------------------------------------------------------ phase retrieval
_PR = {}


def _pr_data(M, B=3, n=16):
    key = (M, B, n)
    if key not in _PR:
        rng = np.random.default_rng(23 + M)
        N = n * n
        xrec = np.stack([_smooth(rng, n) for _ in range(B)])
        A = _r32(rng.standard_normal((B, M, N)))
        Y = _r32(np.stack([np.abs(A[b] @ xrec[b].ravel()) for b in range(B)]) + rng.normal(0, 0.05, (B, M)))
        z = _r32(rng.uniform(0.0, 1.0, (B, N)))
        _PR[key] = (xrec, A, Y, z)
    return _PR[key]


def _pr_batch(data, dtype, sl=slice(None)):
    from pnp_svrg_amd.engine import PrBatch
    xrec, A, Y, z = data
    return PrBatch(xrec[sl], A[sl], Y[sl], z[sl], dtype=dtype)


def _pr_yard(A, Y, z):
    out = []
    for b in range(len(z)):
        t = torch.matmul(torch.from_numpy(A[b].astype(np.float32)).cuda(), torch.from_numpy(z[b].astype(np.float32)).cuda())
        r = (torch.from_numpy(Y[b].astype(np.float32)).cuda() - t.abs()).double()
        out.append(float((r ** 2).sum() / 2 / r.numel()))
    return out


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('M', [128, 77])
def test_pr_objective_own_matrices(M, dtype):
    data = _pr_data(M)
    xrec, A, Y, z = data
    b = _pr_batch(data, dtype)
    got = b.objective(b.xinit).cpu().numpy()
    ref = [oref.pr_f(z[j], A[j], Y[j]) for j in range(3)]
    _check(f'pr M={M}', dtype, got, ref, _pr_yard(A, Y, z) if dtype == F32 else None)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_pr_objective_rows_that_are_no_multiple_of_16_bytes(dtype):
    """N = 15 x 15 = 225 elements per row: no row but the first is 16-byte aligned -- the scalar-load path; M = 77 leaves a
    workgroup with one row of its four."""
    rng = np.random.default_rng(5)
    n, M = 15, 77
    xrec = np.stack([_smooth(rng, n) for _ in range(2)])
    A = _r32(rng.standard_normal((2, M, n * n)))
    Y = _r32(np.abs(np.einsum('bmn,bn->bm', A, xrec.reshape(2, -1))) + rng.normal(0, 0.05, (2, M)))
    z = _r32(rng.uniform(0.0, 1.0, (2, n * n)))
    b = _pr_batch((xrec, A, Y, z), dtype)
    ref = [oref.pr_f(z[j], A[j], Y[j]) for j in range(2)]
    _check('pr N=225', dtype, b.objective(b.xinit).cpu().numpy(), ref, _pr_yard(A, Y, z) if dtype == F32 else None)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_pr_objective_shared_matrices(dtype):
    """A tiled batch, 2 items x 3 trials: problem t * 2 + i reads the matrix of item i, with an iterate of its own."""
    rng = np.random.default_rng(9)
    xrec, A, Y, z = (a[:2] for a in _pr_data(77))
    tiled = _pr_batch((xrec, A, Y, z), dtype).tile(3)
    assert tiled.shared and tiled.B == 6 and tiled.A.shape[0] == 2
    zs = _r32(rng.uniform(0.0, 1.0, (6, 256)))
    zd = torch.from_numpy(zs).cuda().to(dtype).reshape(6, 16, 16)
    got = tiled.objective(zd).cpu().numpy()
    ref = [oref.pr_f(zs[p], A[p % 2], Y[p % 2]) for p in range(6)]
    yard = _pr_yard(np.stack([A[p % 2] for p in range(6)]), np.stack([Y[p % 2] for p in range(6)]), zs) if dtype == F32 else None
    _check('pr shared 2 x 3', dtype, got, ref, yard)


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize('kind', ['csmri', 'deblur', 'pr'])
def test_value_does_not_depend_on_batch_size_or_position(kind):
    """A problem's f at B = 1, inside B = 5 and inside the reversed batch: the same bits (f32, the production type)."""
    if kind == 'csmri':
        data = _csmri_data(128, alphas=(0.1, 0.3, 0.5, 0.7, 1.0), seed=1)
        mk = _csmri_batch
    elif kind == 'deblur':
        data = _deblur_data(50, B=5)
        mk = _deblur_batch
    else:
        data = _pr_data(77, B=5)
        mk = _pr_batch
    rev = tuple(a[::-1].copy() if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a for a in data)
    whole, flipped = mk(data, F32), mk(rev, F32)
    f, fr = whole.objective(whole.xinit), flipped.objective(flipped.xinit)
    assert torch.equal(f, fr.flip(0))
    for j in (0, 3):
        one = mk(data, F32, slice(j, j + 1))
        assert torch.equal(one.objective(one.xinit), f[j:j + 1])


# ------------------------------------------------------------------------------------------------ engines
def _step_and_save(eng, n):
    saved = []
    for _ in range(n):
        eng.step()
        saved.append(eng.z.clone())
    return saved


def test_svrg_engine_logs_the_objective_and_changes_nothing_else():
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    batch = _csmri_batch(_csmri_data(64), F32)
    kw = dict(seed=3, n_log=16)
    off = SvrgEngine(batch, TVProx(), 5e2, 3, 100, **kw)
    on = SvrgEngine(batch, TVProx(), 5e2, 3, 100, log_objective=True, **kw)
    assert off.obj_log is None and not on.graph_ok() and not on.outer_kernel_ok() and off.graph_ok()
    with pytest.raises(ValueError, match='log_objective'):
        off.objective_log()
    saved = _step_and_save(off, 7)
    _step_and_save(on, 7)
    assert torch.equal(on.z, off.z) and torch.equal(on.sse_log, off.sse_log) and on.n_prox == off.n_prox == 7
    assert np.array_equal(on.psnr_trace(), off.psnr_trace())
    want = torch.stack([batch.objective(z) for z in saved]).cpu().numpy()
    log = on.objective_log()
    assert log.shape == (7, 3) and log.dtype == np.float64 and np.array_equal(log, want)
    assert (log > 0).all() and np.isfinite(log).all()


def test_objective_log_ring_wraps_like_the_sse_log():
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    batch = _csmri_batch(_csmri_data(64), F32)
    big = SvrgEngine(batch, TVProx(), 5e2, 3, 100, seed=3, log_objective=True)
    small = SvrgEngine(batch, TVProx(), 5e2, 3, 100, seed=3, n_log=4, log_objective=True)
    for _ in range(7):
        big.step()
        small.step()
    assert small.objective_log().shape == (4, 3)
    assert np.array_equal(small.objective_log(), big.objective_log()[-4:])
    assert np.array_equal(small.psnr_trace(), big.psnr_trace()[-4:])


def test_saga_engine_logs_the_objective_and_changes_nothing_else():
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    batch = _deblur_batch(_deblur_data(100), F32)
    mk = lambda **kw: SagaEngine(batch, TVProx(), 1.0, 500, hist_size=4, seed=5, n_log=16, **kw)
    off, on = mk(), mk(log_objective=True)
    saved = _step_and_save(off, 5)
    _step_and_save(on, 5)
    assert torch.equal(on.z, off.z) and torch.equal(on.sse_log, off.sse_log)
    want = torch.stack([batch.objective(z) for z in saved]).cpu().numpy()
    assert np.array_equal(on.objective_log(), want)


def test_sarah_engine_logs_one_row_per_prox_the_outer_one_included():
    from pnp_svrg_amd.engine import SarahEngine, TVProx
    batch = _csmri_batch(_csmri_data(64), F32)
    mk = lambda **kw: SarahEngine(batch, TVProx(), 5e2, 2, 100, seed=4, n_log=16, **kw)
    off, on = mk(), mk(log_objective=True)
    rows = []                                                   # the iterate behind every log row, from the engine that does not log
    for s in range(4):
        off.step()
        if s % off.T2 == 0:                                     # this step began an outer iteration: w_next holds the outer prox
            rows.append(off.w_next.clone())
        rows.append(off.z.clone())
        on.step()
    assert on.n_prox == off.n_prox == 6 and len(rows) == 6
    assert torch.equal(on.z, off.z) and torch.equal(on.sse_log, off.sse_log)
    want = torch.stack([batch.objective(z) for z in rows]).cpu().numpy()
    assert np.array_equal(on.objective_log(), want)


# ------------------------------------------------------------------------------------------------ sweep
def _sweep_images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    return [_smooth(rng, n) for _ in range(k)]


def test_grid_search_by_objective_on_a_trial_batched_runner():
    import functools
    from pnp_svrg_amd import sweep
    imgs = _sweep_images(2, 64)
    items = sweep.make_items(2, [0.4], [20.0])
    mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'svrg', 'tv', n_inner=4, mini_batch_size=150, T2=2, H=64, W=64,
                           seeding='counter', objective=True)
    grid = {'eta': [500.0, 120.0, 30.0, 5.0]}
    rows = sweep.grid_search(items, mk, grid, batch_trials=True, score='objective')
    # what every trial gives, from the runner's own trial-batched pieces
    run = mk(eta=grid['eta'][0])
    per_trial = run.run_trials(run.prepare_data(items), [{'eta': e} for e in grid['eta']])
    assert len(per_trial) == 4 and all('f_final' in r and 'f_trace' not in r for res in per_trial for r in res)
    for j, row in enumerate(rows):
        f = [res[j]['f_final'] for res in per_trial]
        print(f'item {j}: f_final per trial {f}')
        assert len(set(f)) == 4 and np.isfinite(f).all()
        assert row['id'] == items[j]['id'] and row['params'] == {'eta': grid['eta'][int(np.argmin(f))]} and row['f_final'] == min(f)
    # the serial grid picks the same trials with the same values; by PSNR the rows keep today's keys
    serial = sweep.grid_search(items, mk, grid, score='objective')
    assert [(r['id'], r['params'], r['f_final'], r['loss']) for r in serial] == [(r['id'], r['params'], r['f_final'], r['loss']) for r in rows]
    assert set(sweep.grid_search(items, mk, grid, batch_trials=True)[0]) == {'id', 'item', 'loss', 'params', 'psnr_init', 'psnr_final'}


def test_runner_rows_with_and_without_the_objective():
    from pnp_svrg_amd import sweep
    imgs = _sweep_images(2, 64, seed=1)
    items = sweep.make_items(2, [0.4], [20.0])
    kw = dict(eta=500.0, n_inner=4, mini_batch_size=150, T2=2, H=64, W=64, seeding='counter')
    plain = sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', **kw)(items)
    assert all(set(r) == {'id', 'item', 'psnr_init', 'psnr_final', 'loss', 'z', 'M0'} for r in plain)
    traced = sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', keep_trace=True, **kw)(items)
    assert all(set(r) == {'id', 'item', 'psnr_init', 'psnr_final', 'loss', 'z', 'M0', 'psnr_trace'} for r in traced)
    with_f = sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', objective=True, keep_trace=True, **kw)(items)
    for r, p in zip(with_f, traced):
        assert set(r) == set(p) | {'f_final', 'f_trace'}
        assert np.array_equal(r['z'], p['z']) and np.array_equal(r['psnr_trace'], p['psnr_trace'])      # eager steps = graph replays
        assert r['f_trace'].shape == r['psnr_trace'].shape and r['f_final'] == r['f_trace'][-1]


# ------------------------------------------------------------------------------------------------ drop-in problems
def test_drop_in_problems_objective_equals_their_host_f():
    """`objective(w)` (device) against `f(w)` (host float64 forward model on the same f32-rounded iterate) for the three drop-in
    problems in f64, NumPy and device-tensor arguments alike."""
    import os
    import problems
    img = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'synth64.png')
    np.random.seed(2)
    ps = [problems.CSMRI(img, H=64, W=64, sample_prob=0.3, snr=20., dtype=F64),
          problems.Deblur(img, H=64, W=64, kernel='Minimal', scale_percent=50, snr=20., dtype=F64),
          problems.PhaseRetrieval(img, H=16, W=16, num_meas=77, snr=20., dtype=F64)]
    for p in ps:
        w = np.random.default_rng(0).random(p.N)
        want = p.f(w)
        got, got_dev = p.objective(w), p.objective(p.to_device(w))
        print(f'{p.pname}: f {want:.17g} objective {got:.17g}')
        assert isinstance(got, np.float64) and got == got_dev
        # (the host f of Deblur goes through the device forward model and the host norm: the same 1e-12 class)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
