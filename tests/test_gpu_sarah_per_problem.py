"""pnp_sarah per problem: SarahEngine with [B] eta / mini_batch_size / draw_id against scalar SarahEngines, the two
per-problem loops of launches replaced by one `pnp_axpbypcz_pp` launch each, `grid_search(batch_trials=True)` on a `sarah_trials`
runner, and one tiled problem against the oracle.  Every engine comparison is `torch.equal`: problem b of a tiled batch walks the
trajectory of the scalar engine made with b's values, bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

from test_gpu_pr_shared import _pr_batch
from test_gpu_round3 import GOLDEN, ol                          # (what test_per_step_engines_device_draws_vs_oracle works with)

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
T2, NI, NT = 3, 3, 4                                            # 3 items x 4 trials: problem b = t * 3 + i, draw_id[b] = i
STEPS = 2 * T2 + 1
_SM = [1.0, 1.4, 0.8, 1.2]
CELLS = {'csmri': dict(eta=[500.0, 60.0, 200.0, 350.0], mb=[150, 400, 250, 90]),
         'pr': dict(eta=[0.3, 0.15, 0.05, 0.1], mb=[512, 1024, 256, 700]),
         'deblur': dict(eta=[2e4, 3e3, 9e3, 5e3], mb=[500, 150, 1200, 800])}


def _base(cell, dtype):
    """-> (the batch the tiled engine is tiled from, the batch the scalar engines run on)."""
    from pnp_svrg_amd.engine import CsmriBatch, DeblurBatch
    if cell == 'csmri':
        b = CsmriBatch.synthetic(NI, 64, 64, 0.4, 20.0, seed=21, dtype=dtype)            # Bernoulli masks: M0 differs per item
        assert len(set(b.M0.tolist())) > 1
        return b, b
    if cell == 'deblur':
        b = DeblurBatch.synthetic(NI, 64, 64, 'Minimal', 20.0, seed=2, dtype=dtype)
        return b, b
    # PR: the scalar engines run on tile(1) -- the same problems on the same shared-matrix kernel (csrc/pr_shared.hip), which is
    # what bit equality can be asked of; the untiled batch runs pr.hip's per-problem kernel, another summation order.
    b = _pr_batch(dtype, items=NI)
    return b, b.tile(1)


def _prox(name, sm):
    from pnp_svrg_amd.engine import NLMProx, TVProx
    return (NLMProx if name == 'nlm' else TVProx)(sigma_modifier=sm)


def _run(eng, steps=STEPS):
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    assert eng.n_prox == steps + (steps + T2 - 1) // T2          # one log row per prox: the outer ones included
    return eng.z.clone(), eng.sse_log[:eng.n_prox].clone()


def _check_cell(cell, dtype, prox='tv', lr_decay=1.0, algorithm='sarah', steps=STEPS, **kw):
    from pnp_svrg_amd.engine import make_engine
    base, ref_base = _base(cell, dtype)
    c = CELLS[cell]
    eng = make_engine(base.tile(NT), _prox(prox, np.repeat(_SM, NI)), np.repeat(c['eta'], NI), T2, np.repeat(c['mb'], NI).astype(np.int32),
                      lr_decay=lr_decay, algorithm=algorithm, seed=5, draw_id=np.tile(np.arange(NI), NT), **kw)
    assert eng.b.B == NI * NT
    if algorithm == 'sarah':
        z, log = _run(eng, steps)
    else:
        for _ in range(steps):
            eng.step()
        z, log = eng.z.clone(), eng.sse_log[:eng.n_prox].clone()
    for t in range(NT):
        ref = make_engine(ref_base, _prox(prox, _SM[t]), c['eta'][t], T2, c['mb'][t], lr_decay=lr_decay, algorithm=algorithm, seed=5, **kw)
        for _ in range(steps):
            ref.step()
        sl = slice(t * NI, (t + 1) * NI)
        assert torch.equal(z[sl], ref.z), (cell, t)
        assert ref.n_prox == log.shape[0] and torch.equal(log[:, sl], ref.sse_log[:ref.n_prox]), (cell, t)
    assert not torch.equal(z[0], z[NI]) and bool(torch.isfinite(z).all()) and bool((log > 0).all())
    return eng


# ------------------------------------------------------------------------------------------ 1. engine against scalar engines
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('cell', ['csmri', 'pr', 'deblur'])
def test_sarah_engine_per_problem_equals_scalar_engines(cell, dtype):
    """3 items x 4 trials (distinct eta, mini_batch_size and sigma_modifier per trial, one seed) over 2 * T2 + 1 steps, TVProx:
    z and every logged sse row of trial t == the scalar SarahEngine with t's values."""
    _check_cell(cell, dtype)


def test_sarah_engine_per_problem_deblur_nlm():
    _check_cell('deblur', F32, prox='nlm')


def test_sarah_engine_array_eta_alone_and_array_mb_alone():
    """Either one per problem with the other a scalar."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    base = CsmriBatch.synthetic(2, 64, 64, 0.4, 20.0, seed=21)
    tiled, ids = base.tile(2), np.tile(np.arange(2), 2)
    for eta, mb in ((np.repeat([500.0, 60.0], 2), 150), (500.0, np.repeat([150, 400], 2).astype(np.int32))):
        eng = SarahEngine(tiled, TVProx(), eta, T2, mb, seed=5, draw_id=ids)
        z, log = _run(eng)
        for t in range(2):
            ref = SarahEngine(base, TVProx(), float(np.broadcast_to(eta, 4)[2 * t]), T2, int(np.broadcast_to(mb, 4)[2 * t]), seed=5)
            zr, logr = _run(ref)
            assert torch.equal(z[2 * t:2 * t + 2], zr) and torch.equal(log[:, 2 * t:2 * t + 2], logr)


def test_per_problem_values_are_gated_like_the_other_engines():
    """The base classes' refusals: an untiled PrBatch takes no per-problem values; a wrong length is named."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    pr = _pr_batch(F32, items=2)
    with pytest.raises(ValueError, match="on a CsmriBatch.*'pr'"):
        SarahEngine(pr, TVProx(), np.array([0.1, 0.2]), T2, 256)
    with pytest.raises(ValueError, match="need a CsmriBatch.*'pr'"):
        SarahEngine(pr, TVProx(), 0.1, T2, np.array([256, 300], np.int32))
    with pytest.raises(ValueError, match='per-problem eta'):
        SarahEngine(CsmriBatch.synthetic(2, 64, 64, 0.4, 20.0, seed=21), TVProx(), np.array([1.0, 2.0, 3.0]), T2, 100)


# ------------------------------------------------------------------------------------------ 2. decay
def test_outer_coefficient_does_not_decay_and_inner_does():
    """lr_decay = 0.9 (quirk F6: the outer step w_prev - eta * v_prev ignores it): the scalar engines are the judge.  The uploaded
    -eta vector is made once; the -lr vector is remade when the decay exponent moves."""
    for dtype in (F32, F64):
        eng = _check_cell('csmri', dtype, lr_decay=0.9)
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    c = CELLS['csmri']
    eng = SarahEngine(CsmriBatch.synthetic(NI, 64, 64, 0.4, 20.0, seed=21).tile(NT), TVProx(), np.repeat(c['eta'], NI), T2,
                      np.repeat(c['mb'], NI).astype(np.int32), lr_decay=0.9, seed=5, draw_id=np.tile(np.arange(NI), NT))
    eng.step()
    eta0, lr0 = eng._coef['-eta'][1], eng._coef['-lr'][1]
    for _ in range(T2):
        eng.step()
    assert eng._coef['-eta'][1] is eta0 and eng._coef['-lr'][1] is not lr0
    want = -np.repeat(c['eta'], NI)
    assert np.array_equal(eta0.cpu().numpy(), want) and np.array_equal(eng._coef['-lr'][1].cpu().numpy(), want * 0.9 ** 1)


# ------------------------------------------------------------------------------------------ 3. the scalar path is unchanged
def _count_calls(monkeypatch):
    from pnp_svrg_amd import _native
    seen, real = [], _native.call
    monkeypatch.setattr(_native, 'call', lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    return seen


def test_scalar_sarah_engine_makes_no_pp_call(monkeypatch):
    from pnp_svrg_amd.engine import CsmriBatch, DeblurBatch, SarahEngine, TVProx
    for base in (CsmriBatch.synthetic(2, 64, 64, 0.4, 20.0, seed=21), DeblurBatch.synthetic(2, 64, 64, 'Minimal', 20.0, seed=2)):
        eng = SarahEngine(base, TVProx(), 500.0, T2, 150, seed=5)
        seen = _count_calls(monkeypatch)
        _run(eng, T2 + 1)
        names = [n for n, _ in seen]
        assert names.count('pnp_axpbypcz') >= 2 * (T2 + 1) - T2 and not [n for n in names if n.endswith('_pp')], names
        monkeypatch.undo()


# ------------------------------------------------------------------------------------------ 4. the replaced loops of launches
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_svrg_on_tiled_deblur_equals_scalar_engines(dtype):
    """SvrgEngine(variant='svrg'), per-problem eta and mb on DeblurBatch.tile: the combine g + c1 + gamma_p * mu is one launch now."""
    _check_cell('deblur', dtype, algorithm='svrg', variant='svrg')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_svrg_reference_variant_on_tiled_csmri_equals_scalar_engines(dtype):
    """variant='reference' (z <- z - lr_p * mu) with per-problem eta, lr_decay included: one launch per step."""
    _check_cell('csmri', dtype, algorithm='svrg', variant='reference', lr_decay=0.9)


def test_one_inner_step_is_one_combine_launch(monkeypatch):
    from pnp_svrg_amd.engine import CsmriBatch, DeblurBatch, SvrgEngine, TVProx
    c = CELLS['deblur']
    tiled = DeblurBatch.synthetic(NI, 64, 64, 'Minimal', 20.0, seed=2).tile(NT)
    eng = SvrgEngine(tiled, TVProx(), np.repeat(c['eta'], NI), T2, np.repeat(c['mb'], NI).astype(np.int32), seed=5,
                     draw_id=np.tile(np.arange(NI), NT))
    eng.step()                                                  # (the refresh and inner iteration 0)
    seen = _count_calls(monkeypatch)
    eng.step()
    torch.cuda.synchronize()
    pp = [a for n, a in seen if n == 'pnp_axpbypcz_pp']
    plain = [a for n, a in seen if n == 'pnp_axpbypcz']
    assert len(pp) == 1 and pp[0][7] is not None and pp[0][10] == eng.z.numel() and pp[0][11] == NI * NT      # gamma: the tensor
    assert len(plain) == 1 and plain[0][7] == eng.z.numel()     # g1 - g2 for the whole batch; nothing on one problem's views
    monkeypatch.undo()
    # variant='reference': the step along mu
    c = CELLS['csmri']
    eng = SvrgEngine(CsmriBatch.synthetic(NI, 64, 64, 0.4, 20.0, seed=21).tile(NT), TVProx(), np.repeat(c['eta'], NI), T2,
                     np.repeat(c['mb'], NI).astype(np.int32), variant='reference', seed=5, draw_id=np.tile(np.arange(NI), NT))
    eng.step()
    seen = _count_calls(monkeypatch)
    eng.step()
    names = [n for n, _ in seen]
    assert names.count('pnp_axpbypcz_pp') == 1 and names.count('pnp_axpbypcz') == 0, names


# ------------------------------------------------------------------------------------------ 5. grid
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def _rows_key(rows):
    return [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]


def test_grid_search_sarah_batched_equals_serial_csmri(monkeypatch):
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import SarahEngine
    imgs = _images(2, 64)
    items = sweep.make_items(2, [0.4], [20.0])
    mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'sarah', 'tv', n_inner=4, T2=2, H=64, W=64, seeding='counter',
                           sarah_trials=True)
    grid = {'eta': [500.0, 60.0], 'mini_batch_size': [150, 400], 'sigma_modifier': [1.0, 1.4]}
    serial = sweep.grid_search(items, mk, grid)
    assert len(serial) == 2 and all(np.isfinite(r['loss']) for r in serial)
    sizes, real = [], SarahEngine.__init__
    monkeypatch.setattr(SarahEngine, '__init__', lambda self, batch, *a, **k: (sizes.append(batch.B), real(self, batch, *a, **k))[1])
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True)) == _rows_key(serial)
    assert sizes == [16]                                        # 8 trials x 2 items on ONE engine
    del sizes[:]
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True, max_batch_trials=6)) == _rows_key(serial)
    assert sizes == [6, 6, 4]
    with pytest.raises(ValueError, match='sarah'):              # the same grid without the opt-in
        sweep.grid_search(items, functools.partial(sweep.make_runner, imgs, 'csmri', 'sarah', 'tv', n_inner=4, T2=2, H=64, W=64,
                                                   seeding='counter'), grid, batch_trials=True)


def test_grid_search_sarah_batched_equals_serial_pr():
    """PR 32 x 32, M = 2048, every trial of an item on the item's one matrix.  float64: the serial runner's untiled batches run
    pr.hip's per-problem kernel, which agrees with the shared-matrix kernel to rounding only, and the rows hold PSNRs rounded to
    0.01 dB (in float32 tests/test_gpu_pr_shared.py bounds that difference by 0.01 dB; in float64 the rows are equal)."""
    from pnp_svrg_amd import sweep
    imgs = _images(2, 32)
    items = sweep.make_items(2, [2.0], [30.0])
    mk = functools.partial(sweep.make_runner, imgs, 'pr', 'sarah', 'tv', n_inner=4, T2=2, H=32, W=32, dtype=F64, seeding='counter',
                           shared_matrix=True, sarah_trials=True)
    grid = {'eta': [0.3, 0.05], 'mini_batch_size': [512, 1024], 'sigma_modifier': [1.0, 1.4]}
    serial = sweep.grid_search(items, mk, grid)
    assert len(serial) == 2 and all(np.isfinite(r['loss']) for r in serial)
    assert _rows_key(sweep.grid_search(items, mk, grid, batch_trials=True)) == _rows_key(serial)


# ------------------------------------------------------------------------------------------ 6. oracle
def test_tiled_sarah_problem_vs_oracle():
    """float64: problem (trial 1, item 1) of a tiled CSMRI engine with its own eta and mb, lr_decay = 0.9, against
    oracle.loops.pnp_sarah fed the minibatches the device drew (a function of (seed, step, draw_id, mb): re-drawn on the base plan
    with that trial's mb and decoded): identical rounded PSNR traces, |z - z_oracle| <= 1e-9."""
    import problems as P
    from oracle import denoise as od, problems as op
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    img64 = os.path.join(GOLDEN, 'synth64.png')
    n, T2_, seed, decay, steps = 64, 4, 3, 0.9, 2 * 4 + 1
    ratios, etas, mbs_ = (0.3, 0.5, 0.8), [5e2, 3.1e2], [150, 230]
    probs = []
    for k, a in enumerate(ratios):
        np.random.seed(30 + k)
        probs.append(P.CSMRI(img64, H=n, W=n, sample_prob=a, snr=20., dtype=F64, upload=False))
    batch = CsmriBatch.from_problems(probs, dtype=F64)
    eng = SarahEngine(batch.tile(2), TVProx(), np.repeat(etas, 3), T2_, np.repeat(mbs_, 3).astype(np.int32), lr_decay=decay, seed=seed,
                      draw_id=np.tile(np.arange(3), 2))
    for _ in range(steps):
        eng.step()
    t, i = 1, 1
    b = t * 3 + i
    tr = eng.psnr_trace()[:, b]
    z = eng.z[b].cpu().numpy().reshape(-1)
    shifts = np.arange(32, dtype=np.uint32)
    sb = torch.zeros((1, batch.B, n, n // 32), dtype=torch.int32, device='cuda')
    mbs = []
    for st in range(steps):
        batch.plan.draw_thresholds(batch.bits, mbs_[t], seed, st, 1, selbits=sb)
        mbs.append(((sb.cpu().numpy()[0][i].view(np.uint32)[:, :, None] >> shifts) & 1).reshape(n, n).T.astype(int))
    assert all(m.sum() == mbs_[t] and (m <= probs[i].mask).all() for m in mbs)
    np.random.seed(30 + i)
    po = op.CSMRI(img64, H=n, W=n, sample_prob=ratios[i], snr=20.)
    it = iter(mbs)
    po.select_mb = lambda size: next(it)
    o, j = (steps - 1) // T2_, (steps - 1) % T2_
    ro = ol.pnp_sarah(po, od.TVDenoiser(), etas[t], 1 + o * (5 + 5 * T2_) + 5 + 5 * j + 1, T2_, mbs_[t], converge_check=False,
                      clock=ol.CountingClock(), lr_decay=decay)
    ref = np.array(ro['psnr_per_iter'])
    assert len(ref) == len(tr) and np.array_equal(tr, ref), np.abs(tr - ref).max()
    assert np.abs(z - ro['z']).max() <= 1e-9
