"""The one-pass Deblur step (pnp_deblur_grad_step / DeblurPlan.grad_step) on the device
    out = beta*c1 + gamma_b*c2 + scale_b * B^T S^T (sel o (S B (a - b) - Y))
against the float64 reference, metric and bound of tests/deblur_step_ref.py (whose float32 part tests/test_cpu_deblur_step.py holds
for a float32 rendering of the reference itself), the equalities it promises bit for bit, the paths it leaves alone, and
SvrgEngine / SarahEngine / make_runner with the opt-in against their defaults.  Every case is a few launches on batches of 1 to 3."""
import gc

import numpy as np
import pytest
import torch

import deblur_ref as dr
import deblur_step_ref as sr

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
DTYPES = pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
CASES = pytest.mark.parametrize('n,scale,kname', sr.CASES)
FORMS = [('diff', True, False), ('plain', False, True), ('both', True, True)]          # (name, b given, Y given)


@pytest.fixture(autouse=True)
def _free_plans():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, NP[dtype])).cuda()


def _host(t):
    return t.double().cpu().numpy()


def _plan(n, B, dtype, kname, scale):
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.problems import _deblur_taps
    return ops.DeblurPlan(n, n, B, dtype, dr.kernel(kname, n * n).Bk, bilinear=_deblur_taps(n, n, scale))


def _setup(n, scale, kname, dtype, B=3, rows=slice(None)):
    inp = sr.inputs(n, scale, kname)
    dev = {k: _dev(inp[k][rows], dtype) for k in ('a', 'b', 'Y', 'c1', 'c2')}
    return inp, dev, _plan(n, B, dtype, kname, scale)


def _scales(dtype):
    """(scale, gamma) as the reference takes them and as the call does: scalars, then [B] vectors."""
    dev = lambda v: torch.tensor(v, dtype=F64, device='cuda')                                # noqa: E731
    return [('scalar', sr.SCALE, sr.GAMMA, sr.SCALE, sr.GAMMA), ('per-problem', sr.SCALE_PP, sr.GAMMA_PP, dev(sr.SCALE_PP), dev(sr.GAMMA_PP))]


def _addends_dev(d, dtype, beta, gamma, rows=slice(None)):
    """beta*c1 + gamma_b*c2 as the kernel forms them: each product and each sum rounded in `dtype`."""
    g = torch.tensor(np.atleast_1d(gamma), dtype=dtype, device='cuda').view(-1, 1)
    return (beta * d['c1'] + g * d['c2'])[rows]


# ------------------------------------------------------------------------------------------------ the forms against the reference
@CASES
@DTYPES
def test_forms_against_the_reference(n, scale, kname, dtype):
    """b / Y / both; no selector, `selection`, the edge rows (one measurement at 0, one at M-1, none: exactly the addends); scalar
    and [B] scale and gamma; B = 3, so blockIdx.y > 0 is read everywhere."""
    npdt = NP[dtype]
    inp, d, plan = _setup(n, scale, kname, dtype)
    N = inp['N']
    base = sr.base_bound(npdt, n, scale, kname)
    rc1, rc2 = sr.rounded(inp['c1'], npdt), sr.rounded(inp['c2'], npdt)
    for form, with_b, with_Y in FORMS:
        for selname in ('all', 'selection', 'edges'):
            g1, S1, sel = sr.unit_term(n, scale, kname, np.dtype(npdt).name, with_b, with_Y, selname)
            sel_d = None if sel is None else torch.from_numpy(sel).cuda()
            for sname, sc, ga, sc_d, ga_d in _scales(dtype):
                got = plan.grad_step(d['a'], b=d['b'] if with_b else None, Y=d['Y'] if with_Y else None, sel=sel_d, scale=sc_d,
                                     beta=sr.BETA, c1=d['c1'], gamma=ga_d, c2=d['c2'])
                ref, S = sr.scaled(g1, S1, sc)
                add = sr.addends(sr.BETA, rc1, ga, rc2, npdt, (3, N))
                errs = sr.check(f'{n} {scale} {kname} {form} {selname} {sname}', _host(got).reshape(3, N), add, ref, S, base, npdt)
                assert len(errs) == (2 if selname == 'edges' else 3)
                if selname == 'edges':
                    assert torch.equal(got.reshape(3, N)[2], _addends_dev(d, dtype, sr.BETA, ga, 2).reshape(-1))


@pytest.mark.parametrize('n,scale,kname', [(64, 100, 'edge'), (64, 50, 'edge'), (256, 100, 'dense')])
@DTYPES
def test_addend_forms(n, scale, kname, dtype):
    """c1 only, c2 only, neither (both: test_forms_against_the_reference), on the difference form with `selection`."""
    npdt = NP[dtype]
    inp, d, plan = _setup(n, scale, kname, dtype)
    N = inp['N']
    base = sr.base_bound(npdt, n, scale, kname)
    rc1, rc2 = sr.rounded(inp['c1'], npdt), sr.rounded(inp['c2'], npdt)
    g1, S1, sel = sr.unit_term(n, scale, kname, np.dtype(npdt).name, True, False, 'selection')
    sel_d = torch.from_numpy(sel).cuda()
    for sname, sc, ga, sc_d, ga_d in _scales(dtype):
        ref, S = sr.scaled(g1, S1, sc)
        for what, kw, add in (('c1', dict(beta=sr.BETA, c1=d['c1']), sr.addends(sr.BETA, rc1, 0.0, None, npdt, (3, N))),
                              ('c2', dict(gamma=ga_d, c2=d['c2']), sr.addends(0.0, None, ga, rc2, npdt, (3, N))),
                              ('none', {}, np.zeros((3, N))),
                              ('beta 0 with c1', dict(beta=0.0, c1=d['c1']), np.zeros((3, N)))):
            got = plan.grad_step(d['a'], b=d['b'], sel=sel_d, scale=sc_d, **kw)
            sr.check(f'{n} {scale} {kname} addends {what} {sname}', _host(got).reshape(3, N), add, ref, S, base, npdt)


# ------------------------------------------------------------------------------------------------------------ the equalities
@CASES
@DTYPES
def test_equalities(n, scale, kname, dtype):
    from pnp_svrg_amd import ops
    inp, d, plan = _setup(n, scale, kname, dtype)
    M, N = inp['M'], inp['N']
    sc_pp, ga_pp = (torch.tensor(v, dtype=F64, device='cuda') for v in (sr.SCALE_PP, sr.GAMMA_PP))
    full = dict(b=d['b'], beta=sr.BETA, c1=d['c1'], c2=d['c2'])
    # descriptors against the indicator made of them
    mbd = ops.draw_thresholds(M, 3, max(M // 4, 1), 11, 2)[0].contiguous()
    sel = ops.indicator_from_thresholds(M, mbd)
    assert (sel.sum(dim=1) == max(M // 4, 1)).all()
    for kw in (dict(scale=sr.SCALE, gamma=sr.GAMMA), dict(scale=sc_pp, gamma=ga_pp)):
        for Y in (None, d['Y']):
            assert torch.equal(plan.grad_step(d['a'], Y=Y, mbd=mbd, **full, **kw), plan.grad_step(d['a'], Y=Y, sel=sel, **full, **kw))
    # problem b of the per-problem call == problem b of the scalar call with its values
    pp = plan.grad_step(d['a'], sel=sel, scale=sc_pp, gamma=ga_pp, **full).reshape(3, N)
    for b in range(3):
        one = plan.grad_step(d['a'], sel=sel, scale=sr.SCALE_PP[b], gamma=sr.GAMMA_PP[b], **full).reshape(3, N)
        assert torch.equal(pp[b], one[b]), b
    half = plan.grad_step(d['a'], sel=sel, scale=sc_pp, gamma=sr.GAMMA_PP[1], **full).reshape(3, N)      # (one of the two per problem)
    assert torch.equal(half[1], pp[1]) and not torch.equal(half[0], pp[0])
    # two identical calls
    assert torch.equal(plan.grad_step(d['a'], sel=sel, scale=sc_pp, gamma=ga_pp, **full).reshape(3, N), pp)
    # out aliasing a and c1 (the engines' out=z, a=z, c1=z), and b, and c2, against a fresh out
    fresh = plan.grad_step(d['a'], b=d['b'], mbd=mbd, scale=sc_pp, beta=1.0, c1=d['a'], gamma=ga_pp, c2=d['c2'])
    z = d['a'].clone()
    assert plan.grad_step(z, b=d['b'], mbd=mbd, scale=sc_pp, beta=1.0, c1=z, gamma=ga_pp, c2=d['c2'], out=z) is z
    assert torch.equal(z, fresh)
    w = d['b'].clone()
    plan.grad_step(d['a'], b=w, mbd=mbd, scale=sc_pp, beta=1.0, c1=d['a'], gamma=ga_pp, c2=d['c2'], out=w)
    assert torch.equal(w, fresh)
    mu = d['c2'].clone()
    plan.grad_step(d['a'], b=d['b'], mbd=mbd, scale=sc_pp, beta=1.0, c1=d['a'], gamma=ga_pp, c2=mu, out=mu)
    assert torch.equal(mu, fresh)
    # B = 1 against the same problem at index 2 of B = 3
    _, d1, plan1 = _setup(n, scale, kname, dtype, B=1, rows=slice(2, 3))
    got1 = plan1.grad_step(d1['a'], b=d1['b'], Y=d1['Y'], sel=sel[2:3].contiguous(), scale=sr.SCALE_PP[2], beta=sr.BETA, c1=d1['c1'],
                           gamma=sr.GAMMA_PP[2], c2=d1['c2'])
    got3 = plan.grad_step(d['a'], Y=d['Y'], sel=sel, scale=sc_pp, gamma=ga_pp, **full)
    assert torch.equal(got1.reshape(-1), got3.reshape(3, N)[2])


# ------------------------------------------------------------------------------------------------------------ untouched paths
@pytest.mark.parametrize('scale', [100, 50])
@DTYPES
def test_gradient_of_the_same_plan_keeps_its_bits(dtype, scale):
    inp, d, plan = _setup(64, scale, 'edge', dtype)
    sel = torch.from_numpy(dr.selection(inp['M'], 3)).cuda()
    sc_pp = torch.tensor(sr.SCALE_PP, dtype=F64, device='cuda')
    before = [plan.grad(d['a'], d['Y'], scale=sr.SCALE).clone(), plan.grad(d['a'], d['Y'], sel=sel, scale=sc_pp).clone(),
              plan.forward(d['a']).clone()]
    plan.grad_step(d['a'], b=d['b'], sel=sel, scale=sc_pp, beta=1.0, c1=d['c1'], gamma=sr.GAMMA, c2=d['c2'])
    plan.grad_step(d['a'], Y=d['Y'], scale=sr.SCALE)
    after = [plan.grad(d['a'], d['Y'], scale=sr.SCALE), plan.grad(d['a'], d['Y'], sel=sel, scale=sc_pp), plan.forward(d['a'])]
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_mixed_scale_plan_is_refused():
    import ctypes
    from pnp_svrg_amd import _native, ops
    from pnp_svrg_amd.problems import deblur_operator_sets
    sets, set_of, M_vec = deblur_operator_sets(64, 64, [100, 50])
    plan = ops.DeblurPlan.mixed(64, 64, F32, dr.kernel('edge', 4096).Bk, sets, set_of, M_vec)
    a = torch.zeros((2, 4096), dtype=F32, device='cuda')
    with pytest.raises(ValueError, match='mixed-scale'):
        plan.grad_step(a)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                              # noqa: E731
    h = _native.lib()
    assert h.pnp_deblur_grad_step(plan._h, p(a), None, None, None, None, 1.0, None, 0.0, None, 0.0, None, None, p(a), None) == 1
    assert b'mixed-scale plan' in h.pnp_last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(a) == 0


# ------------------------------------------------------------------------------------------------------------ the engines
def _batch(dtype):
    from pnp_svrg_amd.engine import DeblurBatch
    return DeblurBatch.synthetic(2, 64, 64, 'Minimal', 20.0, seed=2, dtype=dtype)


def _run(batch, algo, steps, idx=None, **kw):
    from pnp_svrg_amd.engine import TVProx, make_engine
    eng = make_engine(batch, TVProx(), kw.pop('eta', 1e3), kw.pop('T2', 4), kw.pop('mb', 150), algorithm=algo, **kw)
    for s in range(steps):
        eng.step(None if idx is None else idx[s])
    torch.cuda.synchronize()
    return eng, eng.z.clone(), eng.psnr_trace()


@pytest.mark.parametrize('algo', ['svrg', 'sarah'])
@DTYPES
def test_engine_one_pass_against_the_default(algo, dtype):
    """TVProx, eta 1e3, T2 = 4, mb = 150, host-fed minibatches, 9 steps (two refreshes crossed).  The tolerances of the project's
    engine-against-loop parity (tests/test_gpu_round2.py): float64 max|dz| <= 1e-9 and the (rounded) PSNR traces equal; float32 the
    PSNR traces within 0.01 + 1e-9."""
    batch = _batch(dtype)
    idx = batch.draw_minibatches(9, 150, seed=6)
    _, z0, tr0 = _run(batch, algo, 9, idx)
    eng, z1, tr1 = _run(batch, algo, 9, idx, one_pass=True)
    assert eng.one_pass and tr0.shape == tr1.shape and np.isfinite(tr1).all()
    dz, dtr = float((z1 - z0).abs().max()), float(np.abs(tr1 - tr0).max())
    print(f'{algo} {dtype}: max|dz| {dz:.3e}, max|dPSNR| {dtr:.3e}')
    if dtype == F64:
        assert dz <= 1e-9 and np.array_equal(tr1, tr0)
    else:
        assert dtr <= 0.01 + 1e-9


@pytest.mark.parametrize('algo', ['svrg', 'sarah'])
def test_engine_one_pass_device_draws(algo):
    """Deterministic in its seed; the final PSNR above psnr_init()."""
    batch = _batch(F32)
    _, za, tra = _run(batch, algo, 9, seed=3, one_pass=True)
    _, zb, trb = _run(batch, algo, 9, seed=3, one_pass=True)
    _, zc, _ = _run(batch, algo, 9, seed=4, one_pass=True)
    assert torch.equal(za, zb) and np.array_equal(tra, trb) and not torch.equal(za, zc)
    print(f'{algo}: psnr_init {batch.psnr_init()}, final {tra[-1]}')
    assert (tra[-1] > batch.psnr_init()).all()


@pytest.mark.parametrize('algo', ['svrg', 'sarah'])
def test_engine_one_pass_per_problem_values(algo):
    """Per-problem eta and mini_batch_size (the '-lr/mb', '-lr', '1/mb' vectors) and, for svrg, a per-problem T2: every problem of
    the tiled batch walks the scalar one-pass engine of its trial, bit for bit (the equality tests/test_gpu_deblur_grid_batched.py
    demands of the default path)."""
    base = _batch(F32)
    ni, etas, mbs, t2s = base.B, [2e3, 3e2], [500, 150], [2, 3]
    t2 = dict(T2=np.repeat(t2s, ni)) if algo == 'svrg' else dict(T2=2)
    _, z, tr = _run(base.tile(2), algo, 6, eta=np.repeat(etas, ni), mb=np.repeat(mbs, ni).astype(np.int32), seed=5,
                    draw_id=np.tile(np.arange(ni), 2), one_pass=True, **t2)
    for t in range(2):
        _, zr, trr = _run(base, algo, 6, eta=etas[t], mb=mbs[t], seed=5, one_pass=True, T2=t2s[t] if algo == 'svrg' else 2)
        assert torch.equal(z[t * ni:(t + 1) * ni], zr), (algo, t)
        assert np.array_equal(tr[:, t * ni:(t + 1) * ni], trr, equal_nan=True), (algo, t)
    assert not torch.equal(z[0], z[ni])


def test_engine_one_pass_allocates_nothing():
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    eng = SvrgEngine(_batch(F32), TVProx(), 1e3, 4, 150, seed=3, one_pass=True)
    for _ in range(5):                                              # (past a refresh: every buffer and cached coefficient exists)
        eng.step()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for _ in range(4):
        eng.step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0


def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def test_runner_one_pass_trial_slab_equals_the_trials_alone():
    """make_runner(problem='deblur', algorithm='svrg', wide_trials=True, one_pass_diff=True): a 2-trial slab over eta against each
    trial run alone with one_pass_diff=True.  Equality: the rows' id, psnr_init, psnr_final and loss equal (==) and z equal bit for
    bit -- what tests/test_gpu_deblur_grid_batched.py demands of the default path (_rows_key; torch.equal of z for the engines)."""
    import functools
    from pnp_svrg_amd import sweep
    n = 64
    imgs = _images(2, n)
    items = sweep.make_items(2, [1.0], [20.0])
    mk = functools.partial(sweep.make_runner, imgs, 'deblur', 'svrg', 'tv', n_inner=4, mini_batch_size=150, T2=2, H=n, W=n,
                           seeding='counter', wide_trials=True, one_pass_diff=True, graph=False)
    trials = [{'eta': 2e4}, {'eta': 3e3}]
    run = mk(eta=1.0)
    slab = run.run_trials(run.prepare_data(items), trials)
    assert len(slab) == 2
    key = lambda rows: [(r['id'], r['psnr_init'], r['psnr_final'], r['loss']) for r in rows]      # noqa: E731
    for tr, rows in zip(trials, slab):
        alone = mk(eta=tr['eta'])(items)
        assert key(rows) == key(alone) and all(np.isfinite(r['loss']) for r in rows)
        assert all(np.array_equal(r['z'], s['z']) for r, s in zip(rows, alone))
    assert not np.array_equal(slab[0][0]['z'], slab[1][0]['z'])       # (the trials differ: eta reached the engines per problem)
    default = sweep.make_runner(imgs, 'deblur', 'svrg', 'tv', eta=2e4, n_inner=4, mini_batch_size=150, T2=2, H=n, W=n, seeding='counter',
                                graph=False)(items)
    assert all(abs(r['psnr_final'] - s['psnr_final']) <= 0.01 + 1e-9 for r, s in zip(slab[0], default))
