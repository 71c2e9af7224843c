"""A Deblur grid as one batch: the per-problem forms of the Deblur gradients, of the SAGA table update and of the NLM
prox, the engines that drive them on `DeblurBatch.tile`, and `sweep.grid_search(batch_trials=True)` on a `wide_trials` runner.
Everything is "equal bit for bit (torch.equal) to the scalar call made with that problem's values": the arithmetic is the same."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _dev(v, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(v, dtype)).cuda()


def _rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64).to('cuda', dtype)


# ------------------------------------------------------------------------------------------------------- 1. Deblur gradients
def _plan(n, B, dtype, scale_percent):
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.problems import _deblur_taps
    from pnp_svrg_amd.sweep import _minimal_kernel
    return ops.DeblurPlan(n, n, B, dtype, _minimal_kernel(n, n, 'Minimal'), bilinear=_deblur_taps(n, n, scale_percent))


def _check_deblur_pp(n, B, dtype, scale_percent, scales, mbs):
    from pnp_svrg_amd import ops
    plan, one = _plan(n, B, dtype, scale_percent), _plan(n, 1, dtype, scale_percent)
    M = plan.M
    assert (M == n * n) == (scale_percent == 100)
    z, Y = _rand((B, n, n), dtype, 10 + n), _rand((B, M), dtype, 11 + n)
    sel = (_rand((B, M), F64, 12 + n) < 0.3).to(torch.uint8).contiguous()
    for s in (None, sel):                                              # all measurements, a host indicator
        got = plan.grad(z, Y, sel=s, scale=_dev(scales))
        for b in range(B):
            assert torch.equal(got[b], plan.grad(z, Y, sel=s, scale=float(scales[b]))[b]), (n, dtype, scale_percent, s is None, b)
    assert not torch.equal(got[0] * 0, got[0])                         # (not all zero)
    # device-drawn minibatches: per-problem mb and a permuted draw_id; problem b == the scalar _mb call on a one-problem draw
    ids = np.roll(np.arange(B), 1)
    seed, step = 77, 5
    mbd = ops.draw_thresholds(M, B, _dev(mbs, np.int32), seed, step, 1, draw_id=_dev(ids, np.int32))[0]
    got = plan.grad(z, Y, mbd=mbd, scale=_dev(scales))
    for b in range(B):
        d1 = ops.draw_thresholds(M, 1, _dev([mbs[b]], np.int32), seed, step, 1, draw_id=_dev([ids[b]], np.int32))[0]
        assert torch.equal(d1[0], mbd[b])
        assert int(ops.indicator_from_thresholds(M, d1).sum()) == mbs[b]
        ref = one.grad(z[b:b + 1].contiguous(), Y[b:b + 1].contiguous(), mbd=d1, scale=float(scales[b]))
        assert torch.equal(got[b], ref[0]), (n, dtype, scale_percent, 'mb', b)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('scale_percent', [100, 50], ids=['identity', 'bilinear50'])
def test_deblur_grad_pp(dtype, scale_percent):
    """B = 3, three scales: output b of deblur_grad_pp / deblur_grad_mb_pp == the scalar call with scale_b (64 x 64)."""
    _check_deblur_pp(64, 3, dtype, scale_percent, np.array([-0.37, 1.9e-3 / 7, 311.0]), [100, 700, 333])


@pytest.mark.parametrize('n', [128, 256])
def test_deblur_grad_pp_other_fft_sizes(n):
    """The other two FFT instantiations: B = 2, f32."""
    _check_deblur_pp(n, 2, F32, 100, np.array([-1.0 / 3, 2.5e-4]), [1000, 77])


# ------------------------------------------------------------------------------------------------------- 2. SAGA table update
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_saga_table_update_pp(dtype):
    """B = 4, hist = 4, rows with and without row == prev_row, distinct lr_b: z, table, sum == B scalar calls on the views;
    a second step on the result (a stale `prev` would show)."""
    from pnp_svrg_amd import ops
    B, hist, n = 4, 4, 64
    z, ts = _rand((B, n, n), dtype, 1), _rand((B, n, n), dtype, 2)
    table = _rand((hist, B, n, n), dtype, 3)
    zr, tsr, tr = z.clone(), ts.clone(), table.clone()
    lr = np.array([0.7, 1e-3, 123.0, 0.05])
    steps = [([1, 2, 0, 3], [1, 0, 0, 2]), ([1, 3, 2, 3], [1, 2, 0, 3])]      # (row, prev_row): equal for problems 0, 2 / 0, 3
    for k, (row, prev) in enumerate(steps):
        g = _rand((B, n, n), dtype, 20 + k)
        ops.saga_table_update_pp(z, g, table, _dev(row, np.int32), _dev(prev, np.int32), ts, _dev(lr), 0.25)
        for b in range(B):
            ops.saga_table_update(zr[b], g[b], tr[row[b], b], tr[prev[b], b], tsr[b], float(lr[b]), 0.25)
        assert torch.equal(z, zr) and torch.equal(table, tr) and torch.equal(ts, tsr), k
    # one step size for the batch, per-problem rows: the scalar lr of the plain call
    g = _rand((B, n, n), dtype, 30)
    ops.saga_table_update_pp(z, g, table, _dev([0, 0, 1, 2], np.int32), _dev([1, 3, 2, 3], np.int32), ts, 0.3, 0.25)
    for b, (r, p) in enumerate(zip([0, 0, 1, 2], [1, 3, 2, 3])):
        ops.saga_table_update(zr[b], g[b], tr[r, b], tr[p, b], tsr[b], 0.3, 0.25)
    assert torch.equal(z, zr) and torch.equal(table, tr) and torch.equal(ts, tsr)


# ------------------------------------------------------------------------------------------------------- 3. NLM
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('form,dist', [('k_nlm_strip', 5), ('k_nlm', 3)])
def test_nlm2d_pp(dtype, form, dist):
    """B = 3, three modifiers, sigma_in given: image b and sse b == the scalar call with modifier_b, for both kernel forms.
    csrc/nlm.hip runs k_nlm_strip for patch side 5, patch_distance 5 and (f32 or batch <= 4), k_nlm otherwise.  24 x 40: more
    than one 16 x 16 tile each way, neither side a multiple of the tile."""
    from pnp_svrg_amd import ops
    B, H, W, patch = 3, 24, 40, 4
    side = patch + 1
    ran = 'k_nlm_strip' if (side == 5 and dist == 5 and (dtype == F32 or B <= 4) and 'PNP_NLM_GENERIC' not in os.environ) else 'k_nlm'
    assert ran == form
    z, xr = _rand((B, H, W), dtype, 4), _rand((B, H, W), dtype, 5)
    sig = _dev([0.08, 0.11, 0.2]).to(dtype)
    sm = np.array([0.8, 1.0, 1.7])
    out, sse = ops.nlm2d(z, sigma_in=sig, sigma_modifier=_dev(sm), patch_size=patch, patch_distance=dist, xrec=xr)
    for b in range(B):
        ro, rs = ops.nlm2d(z, sigma_in=sig, sigma_modifier=float(sm[b]), patch_size=patch, patch_distance=dist, xrec=xr)
        assert torch.equal(out[b], ro[b]) and torch.equal(sse[b], rs[b]), (form, dtype, b)
    assert not torch.equal(out[0], z[0])


# ------------------------------------------------------------------------------------------------------- 4, 5. engines
_ETA, _MB, _SM = [2e4, 3e3, 9e3], [500, 150, 1200], [1.0, 1.4, 0.8]           # three trials of (eta, mb, sigma_modifier)
_R = [2, 0, 2, 1, 1]                                                          # the replaced SAGA rows (hist 3), a repeat included


def _run(eng, algo, steps):
    for s in range(steps):
        if algo == 'saga':
            eng.step(r=_R[s])
        else:
            eng.step()
    torch.cuda.synchronize()
    return eng.z.clone(), eng.psnr_trace()


def _check_engine(base, algo, prox_cls, eta_scale=1.0, steps=5, **kw):
    from pnp_svrg_amd.engine import make_engine
    ni = base.B
    eta = np.repeat(_ETA, ni) * eta_scale
    mb = np.repeat(_MB, ni).astype(np.int32)
    eng = make_engine(base.tile(3), prox_cls(sigma_modifier=np.repeat(_SM, ni)), eta, 2, mb, algorithm=algo, hist_size=3, seed=5,
                      draw_id=np.tile(np.arange(ni), 3), **kw)
    assert eng.b.B == 3 * ni
    z, tr = _run(eng, algo, steps)
    for t in range(3):
        ref = make_engine(base, prox_cls(sigma_modifier=_SM[t]), _ETA[t] * eta_scale, 2, _MB[t], algorithm=algo, hist_size=3, seed=5, **kw)
        zr, trr = _run(ref, algo, steps)
        assert torch.equal(z[t * ni:(t + 1) * ni], zr), (algo, t)
        assert np.array_equal(tr[:, t * ni:(t + 1) * ni], trr, equal_nan=True), (algo, t)
    assert not torch.equal(z[0], z[ni]) and bool(torch.isfinite(z).all())


@pytest.fixture(scope='module', params=[F32, F64], ids=['f32', 'f64'])
def deblur_base(request):
    from pnp_svrg_amd.engine import DeblurBatch
    return DeblurBatch.synthetic(2, 64, 64, 'Minimal', 20.0, seed=2, dtype=request.param)


@pytest.mark.parametrize('prox', ['nlm', 'tv'])
def test_saga_engine_on_tiled_deblur(deblur_base, prox):
    """SagaEngine on DeblurBatch.synthetic(2, 64, 64).tile(3): each of the 6 problems == its item in the scalar engine of its trial."""
    from pnp_svrg_amd.engine import NLMProx, TVProx
    _check_engine(deblur_base, 'saga', NLMProx if prox == 'nlm' else TVProx)


@pytest.mark.parametrize('algo', ['sgd', 'gd', 'svrg'])
def test_sgd_gd_svrg_engines_on_tiled_deblur(deblur_base, algo):
    """(svrg: T2 = 2, the non-fused path.)"""
    from pnp_svrg_amd.engine import TVProx
    _check_engine(deblur_base, algo, TVProx, steps=4)


def test_saga_engine_on_tiled_csmri():
    from pnp_svrg_amd.engine import CsmriBatch, TVProx
    _check_engine(CsmriBatch.synthetic(2, 64, 64, 0.4, 20.0, seed=21), 'saga', TVProx, eta_scale=1e-2)


def test_saga_rows_outside_the_table_are_refused(deblur_base):
    from pnp_svrg_amd.engine import SagaEngine, TVProx
    eng = SagaEngine(deblur_base, TVProx(), np.array([1e3, 2e3]), 100, hist_size=3, seed=1)
    with pytest.raises(ValueError, match='outside the table'):
        eng.step(r=np.array([0, 3]))


# ------------------------------------------------------------------------------------------------------- 6. grid_search
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def _rows_key(rows):
    return [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]


@pytest.mark.parametrize('alpha', [1.0, 0.5], ids=['identity', 'bilinear50'])
def test_grid_search_deblur_saga_nlm_batched_equals_serial(alpha, monkeypatch):
    """Deblur + NLM + pnp_saga, seeding='counter', 3 items in chunks of 2, 8 trials: batch_trials=True gives the rows of the serial
    run, also in several slabs (max_batch_trials, max_table_bytes).  alpha = 0.5: the bilinear down-sampler (scale_percent 50)."""
    from pnp_svrg_amd import ops, sweep
    n = 64
    imgs = _images(3, n)
    items = sweep.make_items(3, [alpha], [20.0])
    mk = functools.partial(sweep.make_runner, imgs, 'deblur', 'saga', 'nlm', n_inner=4, hist_size=3, H=n, W=n, seeding='counter',
                           max_batch=2, wide_trials=True)
    grid = {'eta': [2e4, 3e3], 'mini_batch_size': [500, 150], 'sigma_modifier': [1.0, 1.4]}
    serial = sweep.grid_search(items, mk, grid)
    assert len(serial) == 3 and all(np.isfinite(r['loss']) for r in serial)
    sizes = []
    real = ops.saga_table_update_pp
    monkeypatch.setattr(ops, 'saga_table_update_pp', lambda z, *a, **k: (sizes.append(z.shape[0]), real(z, *a, **k))[1])
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True)) == _rows_key(serial)
    assert set(sizes) == {16, 8}                                       # 8 trials x (2 items, 1 item): one slab per chunk
    if alpha != 1.0:
        return
    del sizes[:]
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True, max_batch_trials=7)) == _rows_key(serial)
    assert set(sizes) == {6, 4, 7, 1}                                  # 3 + 3 + 2 trials of 2 items; 7 + 1 trials of 1 item
    del sizes[:]
    two_trials = 2 * 3 * 2 * n * n * 4                                 # table bytes of 2 trials of the 2-item chunk (hist 3, f32)
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True, max_table_bytes=two_trials)) == _rows_key(serial)
    assert set(sizes) == {4}                                           # 2 trials x 2 items, 4 trials x 1 item


# ------------------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize('kw,trial,word', [(dict(algorithm='sarah'), {'eta': 1.0}, 'sarah'), (dict(seeding='legacy'), {'eta': 1.0}, 'legacy'),
                                           (dict(), {'hist_size': 4}, 'hist_size')])
def test_wide_trials_still_refuses(kw, trial, word):
    from pnp_svrg_amd import sweep
    a = dict(problem='deblur', algorithm='saga', denoiser='nlm', seeding='counter')
    a.update(kw)
    items = sweep.make_items(1, [1.0], [20.0])

    def mk(**p):
        p.setdefault('eta', 1.0)
        return sweep.make_runner(_images(1, 64), a['problem'], a['algorithm'], a['denoiser'], n_inner=2, mini_batch_size=50, T2=2, H=64, W=64,
                                 seeding=a['seeding'], wide_trials=True, **p)
    with pytest.raises(ValueError, match=word):
        mk().check_trials([trial])
    if 'eta' in trial:
        with pytest.raises(ValueError, match=word):
            sweep.grid_search(items, mk, {'eta': [1.0, 2.0]}, batch_trials=True)


def test_nlm_prox_wrong_length_modifier(deblur_base):
    from pnp_svrg_amd.engine import NLMProx, SagaEngine
    with pytest.raises(ValueError, match='per-problem sigma_modifier: 2 values'):
        SagaEngine(deblur_base, NLMProx(sigma_modifier=np.array([1.0, 1.2, 1.4])), 1e3, 100, hist_size=3)
