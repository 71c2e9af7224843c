"""Mixed-scale Deblur batches on the GPU: a DeblurBatch whose problems each have a down-sampler and a measurement
count of their own, against the same problems in uniform batches of their scale and against the oracle.

64 x 64, the "Minimal" kernel, scales {10, 50, 75, 100}: M = 36 (less than a wavefront: the tails), 1024, 2304 (adjoint rows with
up to 4 entries: the CSR sum has an order), 4096 (the identity set).  B = 6 in a scrambled order, two problems share scale 50.
Members WITH a down-sampler must be bit-equal to the uniform batch (torch.equal); identity members take "- Y" behind the blur's
rounding, so they are held to the oracle with the bounds tests/test_gpu_deblur_pr.py applies to the 64 x 64 scale-100 gradient
(1e-10 of max|ref| in f64, 2e-4 in f32)."""
import gc

import numpy as np
import pytest
import torch

import setup_generate_ref as sr
from oracle import problems as op

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
N_ = 64
SCALES = [75, 50, 100, 10, 50, 100]
M_VEC = [2304, 1024, 4096, 36, 1024, 4096]
IDS = [11, 4, 7, 0, 9, 2]
MB, SEED = 30, 5
REL = {F64: 1e-10, F32: 2e-4}
_cache = {}


@pytest.fixture(autouse=True)
def _free_plans():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _items():
    return [{'id': IDS[b], 'image': b % 3, 'alpha': SCALES[b] / 100.0, 'snr': 20.0, 'seed': 3} for b in range(6)]


def _data(dtype):
    """(images, items, mixed batch, the same items alone in uniform batches of their scale), generated once per dtype."""
    from pnp_svrg_amd.engine import DeblurBatch
    if dtype not in _cache:
        imgs = sr.images(3, N_, seed=7)
        up = DeblurBatch.upload_images(imgs, N_, N_, dtype)
        items = _items()
        mixed = DeblurBatch.generate(up, items, N_, N_, dtype, scale_percent=SCALES)
        singles = [DeblurBatch.generate(up, [it], N_, N_, dtype, scale_percent=sp) for it, sp in zip(items, SCALES)]
        _cache[dtype] = (imgs, up, items, mixed, singles)
    return _cache[dtype]


def _reordered(dtype, order):
    """The mixed batch with its problems in `order` (built from the generated tensors: same data, other places)."""
    from pnp_svrg_amd.engine import DeblurBatch
    _, up, items, mixed, _ = _data(dtype)
    if list(order) == list(range(6)):
        return mixed
    return DeblurBatch.generate(up, [items[b] for b in order], N_, N_, dtype, scale_percent=[SCALES[b] for b in order])


def _ids(order, dev='cuda'):
    return torch.tensor([IDS[b] for b in order], dtype=torch.int32, device=dev)


def _oracle(dtype, b):
    """oracle.problems.Deblur on member b's operator, holding the generated data of that member (as float64)."""
    imgs, _, _, mixed, _ = _data(dtype)
    np.random.seed(0)
    po = op.Deblur(None, H=N_, W=N_, kernel='Minimal', scale_percent=SCALES[b], snr=20., img=imgs[b % 3])
    assert po.M == M_VEC[b]
    po.Y = mixed.Y[b, :M_VEC[b]].double().cpu().numpy()
    return po


def _z(dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((6, N_, N_), generator=g, dtype=torch.float64).to('cuda', dtype)


def _host_idx(order):
    rng = np.random.default_rng(2)
    rows = [np.sort(rng.choice(M_VEC[b], MB, replace=False)) for b in range(6)]
    return torch.from_numpy(np.stack([rows[b] for b in order]).astype(np.int32)).cuda()


def _all_results(batch, z, w, ids, idx):
    """Every quantity of test 1 on `batch` (mixed, or a uniform batch of one problem)."""
    B = batch.B
    out = {}
    out['grad_full'] = batch.grad_full(z, out=torch.empty_like(z)).clone()
    out['grad_full_a'] = batch.grad_full(z, out=torch.empty_like(z), alpha=-0.7, beta=1.0, c1=w).clone()
    mbs = batch.minibatches(2)
    batch.draw(mbs, MB, SEED, 3, 2, draw_id=ids)
    out['grad_stoch'] = batch.grad_stoch(z, mbs, 1, out=torch.empty_like(z), alpha=0.25).clone()
    out['grad_stoch_diff'] = batch.grad_stoch_diff(z, w, mbs, 1, out=torch.empty_like(z), alpha=0.5, beta=1.0, c1=z, gamma=-0.3,
                                                   c2=w).clone()
    batch.set_host(mbs, 0, idx)
    out['grad_stoch_host'] = batch.grad_stoch(z, mbs, 0, out=torch.empty_like(z)).clone()
    out['objective'] = batch.objective(z).clone()
    fwd = batch.plan.forward(z).reshape(B, batch.M)
    out['forward'] = fwd.clone()
    return out


@pytest.mark.parametrize('order', [list(range(6)), list(range(5, -1, -1))], ids=['order', 'reversed'])
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_member_equals_uniform_batch(dtype, order):
    """grad_full, grad_stoch (descriptor and set_host forms), grad_stoch_diff, objective and the forward pass of every member with
    a down-sampler equal, bit for bit, the same problem alone in a uniform batch -- wherever it sits; identity members agree with
    the oracle (f64 and f32 bounds of the module docstring)."""
    _, _, _, _, singles = _data(dtype)
    batch = _reordered(dtype, order)
    assert batch.M == 4096 and batch.M_vec.tolist() == [M_VEC[b] for b in order]
    z, w, idx = _z(dtype)[order], _z(dtype, 2)[order], _host_idx(order)
    got = _all_results(batch, z.contiguous(), w.contiguous(), _ids(order), idx)
    for k, b in enumerate(order):
        Mb = M_VEC[b]
        ref = _all_results(singles[b], z[k:k + 1].contiguous(), w[k:k + 1].contiguous(), _ids([b]), idx[k:k + 1].contiguous())
        for name, r in ref.items():
            g = got[name][k:k + 1]
            if name == 'forward':
                assert torch.count_nonzero(g[:, Mb:]) == 0, (name, b)          # the padding is written as zero
                g = g[:, :Mb]
            if SCALES[b] != 100:
                assert torch.equal(g, r), (name, b, SCALES[b])
            else:                                                              # identity: "- Y" behind the blur's rounding
                bound = REL[dtype] * float(r.abs().max())
                assert float((g.double() - r.double()).abs().max()) <= bound, (name, b)
        if SCALES[b] == 100:                                                   # ... and the oracle itself
            po = _oracle(dtype, b)
            zb = z[k].double().cpu().numpy().ravel()
            ref = po.grad_full(zb)
            assert np.abs(got['grad_full'][k].double().cpu().numpy().ravel() - ref).max() <= REL[dtype] * np.abs(ref).max()
            ind = np.zeros(Mb)
            ind[idx[k].cpu().numpy()] = 1
            ref = po.grad_stoch(zb, ind)
            assert np.abs(got['grad_stoch_host'][k].double().cpu().numpy().ravel() - ref).max() <= REL[dtype] * np.abs(ref).max()


def test_per_problem_alpha_equals_scalar():
    """grad_full with a [B] alpha: problem b is the scalar call with alpha_b (alpha_b / M_b on the host, as a uniform batch does)."""
    _, _, _, mixed, singles = _data(F32)
    z = _z(F32)
    a = np.array([0.5, -1.25, 2.0, 1e-3, -3.0, 0.75])
    got = mixed.grad_full(z, out=torch.empty_like(z), alpha=torch.from_numpy(a).cuda())
    for b in (0, 1, 3, 4):
        ref = singles[b].grad_full(z[b:b + 1].contiguous(), out=torch.empty_like(z[b:b + 1]), alpha=float(a[b]))
        assert torch.equal(got[b:b + 1], ref), b


def test_oracle_f64():
    """Every member's grad_full, grad_stoch and f against oracle.problems.Deblur / Bilinear of that member's scale."""
    from pnp_svrg_amd import ops
    _, _, _, mixed, _ = _data(F64)
    z = _z(F64)
    mbs = mixed.minibatches(1)
    mixed.draw(mbs, MB, SEED, 0, 1, draw_id=_ids(range(6)))
    ind = ops.indicator_from_thresholds_m(mixed.plan.M_dev, mixed.M, mbs.mbd[0]).cpu().numpy()
    gf = mixed.grad_full(z, out=torch.empty_like(z)).cpu().numpy().reshape(6, -1)
    gs = mixed.grad_stoch(z, mbs, 0, out=torch.empty_like(z)).cpu().numpy().reshape(6, -1)
    f = mixed.objective(z).cpu().numpy()
    for b in range(6):
        po = _oracle(F64, b)
        zb = z[b].cpu().numpy().ravel()
        assert ind[b].sum() == MB and ind[b, M_VEC[b]:].sum() == 0
        for got, ref in ((gf[b], po.grad_full(zb)), (gs[b], po.grad_stoch(zb, ind[b, :M_VEC[b]]))):
            assert np.abs(got - ref).max() <= REL[F64] * np.abs(ref).max(), b
        assert abs(f[b] - po.f(zb)) <= REL[F64] * po.f(zb), b


@pytest.mark.parametrize('mb', [20, [100, 36, 4096, 7, 1, 2304]], ids=['scalar', 'per-problem'])
def test_draws_equal_per_problem_draws(mb):
    from pnp_svrg_amd import ops
    Mv = torch.tensor(M_VEC, dtype=torch.int32, device='cuda')
    ids = _ids(range(6))
    mbv = np.broadcast_to(np.asarray(mb, np.int32), (6,)).copy()
    mb_arg = mb if np.ndim(mb) == 0 else torch.from_numpy(np.ascontiguousarray(mbv)).cuda()
    got = ops.draw_thresholds_mpp(Mv, mb_arg, 77, 5, nsteps=3, draw_id=ids)
    assert tuple(got.shape) == (3, 6, 2)
    for b in range(6):
        one = torch.tensor([int(mbv[b])], dtype=torch.int32, device='cuda')
        ref = ops.draw_thresholds(M_VEC[b], 1, one, 77, 5, nsteps=3, draw_id=ids[b:b + 1].contiguous())
        assert torch.equal(got[:, b], ref[:, 0]), b
    for s in range(3):
        ind = ops.indicator_from_thresholds_m(Mv, 4096, got[s]).cpu().numpy()
        for b in range(6):
            assert ind[b].sum() == mbv[b] and ind[b, M_VEC[b]:].sum() == 0, (s, b)   # mb_b == M_b: everything, nothing beyond
            ref = ops.indicator_from_thresholds(M_VEC[b], got[s, b:b + 1].contiguous()).cpu().numpy()
            assert np.array_equal(ind[b, :M_VEC[b]], ref[0])


def test_larger_sample_than_population_names_the_problem():
    from pnp_svrg_amd.engine import SgdEngine, TVProx
    _, _, _, mixed, _ = _data(F32)
    mbs = mixed.minibatches(1)
    with pytest.raises(ValueError, match=r'larger sample than population.*problem 3: mini_batch_size 37, population 36'):
        mixed.draw(mbs, 37, 1, 0)
    with pytest.raises(ValueError, match=r'larger sample than population.*problem 1: mini_batch_size 1025, population 1024'):
        mixed.draw(mbs, [2304, 1025, 4096, 36, 1024, 4096], 1, 0)
    with pytest.raises(ValueError, match=r'larger sample than population.*problem 3'):
        SgdEngine(mixed, TVProx(), 0.1, 37)
    with pytest.raises(ValueError, match='one per problem'):
        mixed.draw_minibatches(1, 8)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_generation_equals_uniform_generation(dtype):
    from pnp_svrg_amd.engine import DeblurBatch
    _, up, items, mixed, singles = _data(dtype)
    assert tuple(mixed.Y.shape) == (6, 4096)
    for b in range(6):
        Mb, one = M_VEC[b], singles[b]
        assert torch.equal(mixed.Y[b, :Mb], one.Y[0]), b
        assert torch.count_nonzero(mixed.Y[b, Mb:]) == 0, b
        for nm in ('xinit', 'xrec', 'sigma'):
            assert torch.equal(getattr(mixed, nm)[b], getattr(one, nm)[0]), (nm, b)
    pair = DeblurBatch.generate(up, [items[4], items[1]], N_, N_, dtype, scale_percent=50)       # other neighbours, other places
    assert torch.equal(pair.Y[0], mixed.Y[4, :1024]) and torch.equal(pair.Y[1], mixed.Y[1, :1024])
    rev = _reordered(dtype, list(range(5, -1, -1)))
    for nm in ('Y', 'xinit', 'xrec', 'sigma'):
        assert torch.equal(getattr(rev, nm).flip(0), getattr(mixed, nm)), nm


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_guard_bands(dtype):
    """Forward, gradient and objective on caller-provided Y / out buffers with NaN bands before and after them and NaN in the
    padding m >= M_b of every row of Y: outputs finite and unchanged, bands intact (a check that passes, not a provoked fault)."""
    _, _, _, mixed, _ = _data(dtype)
    z = _z(dtype)
    B, M, Nn, G = 6, mixed.M, N_ * N_, 1024
    mbs = mixed.minibatches(1)
    mixed.draw(mbs, MB, SEED, 0, 1, draw_id=_ids(range(6)))
    plan = mixed.plan
    want = dict(g=plan.grad(z, mixed.Y, scale=0.5), gm=plan.grad(z, mixed.Y, scale=0.5, mbd=mbs.mbd[0]), f=plan.forward(z).clone(),
                o=plan.objective(z, mixed.Y, 0.5))
    nan = float('nan')
    ybuf = torch.full((G + B * M + G,), nan, dtype=dtype, device='cuda')
    Y = ybuf[G:G + B * M].view(B, M)
    for b in range(B):
        Y[b, :M_VEC[b]] = mixed.Y[b, :M_VEC[b]]                                # the padding keeps its NaN
    sel_buf = torch.full((G + B * M + G,), 255, dtype=torch.uint8, device='cuda')
    sel = sel_buf[G:G + B * M].view(B, M)
    for b in range(B):
        sel[b, :M_VEC[b]] = 1
    gbuf = torch.full((G + B * Nn + G,), nan, dtype=dtype, device='cuda')
    gout = gbuf[G:G + B * Nn].view(B, N_, N_)
    fbuf = torch.full((G + B * M + G,), nan, dtype=dtype, device='cuda')
    fout = fbuf[G:G + B * M]
    obuf = torch.full((8 + B + 8,), nan, dtype=F64, device='cuda')
    oout = obuf[8:8 + B]

    def bands_ok(buf, g, n):
        return bool(torch.isnan(buf[:g]).all()) and bool(torch.isnan(buf[g + n:]).all())

    plan.grad(z, Y, scale=0.5, out=gout)
    assert torch.isfinite(gout).all() and torch.equal(gout, want['g']) and bands_ok(gbuf, G, B * Nn)
    gbuf[G:G + B * Nn] = nan
    plan.grad(z, Y, sel=sel, scale=0.5, out=gout)                              # an all-ones indicator, 255 in its padding
    assert torch.equal(gout, want['g']) and bands_ok(gbuf, G, B * Nn)
    gbuf[G:G + B * Nn] = nan
    plan.grad(z, Y, scale=0.5, out=gout, mbd=mbs.mbd[0])
    assert torch.isfinite(gout).all() and torch.equal(gout, want['gm']) and bands_ok(gbuf, G, B * Nn)
    plan.forward(z, out=fout)
    assert torch.isfinite(fout).all() and torch.equal(fout, want['f']) and bands_ok(fbuf, G, B * M)
    plan.objective(z, Y, 0.5, out=oout)
    assert torch.isfinite(oout).all() and torch.equal(oout, want['o']) and bands_ok(obuf, 8, B)
    assert bands_ok(ybuf, G, B * M) and all(bool(torch.isnan(Y[b, M_VEC[b]:]).all()) for b in range(B))
    assert bool((sel_buf[:G] == 255).all()) and bool((sel_buf[G + B * M:] == 255).all())


def _engine(kind, batch, ids):
    from pnp_svrg_amd.engine import SvrgEngine, SagaEngine, TVProx, NLMProx
    if kind == 'svrg-tv':
        return SvrgEngine(batch, TVProx(), 0.8, 3, MB, seed=SEED, draw_id=ids)
    return SagaEngine(batch, NLMProx(), 0.8, MB, hist_size=4, seed=SEED, draw_id=ids)


@pytest.mark.parametrize('kind', ['svrg-tv', 'saga-nlm'])
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_engines_on_the_mixed_batch(dtype, kind):
    """2 outer x 3 inner iterations with device draws keyed by the item ids: iterates and squared-error logs of the members with a
    down-sampler equal those of the same items run alone in uniform batches; identity members stay within 0.01 dB; where the
    engine offers hipGraph replay, the replayed run equals the eager one."""
    _, _, _, mixed, singles = _data(dtype)
    eng = _engine(kind, mixed, IDS)
    for _ in range(6):
        eng.step()
    tr = eng.psnr_trace()
    assert tr.shape == (6, 6) and np.isfinite(tr).all()
    for b in range(6):
        one = _engine(kind, singles[b], [IDS[b]])
        for _ in range(6):
            one.step()
        if SCALES[b] != 100:
            assert torch.equal(eng.z[b], one.z[0]), (kind, b)
            assert torch.equal(eng.sse_log[:6, b], one.sse_log[:6, 0]), (kind, b)
        else:
            assert np.abs(tr[:, b] - one.psnr_trace()[:, 0]).max() <= 0.01 + 1e-9, (kind, b)
    if hasattr(eng, 'graph_ok') and eng.graph_ok():
        rep = _engine(kind, mixed, IDS)
        rep.run_outer(2)                                                       # captures one outer iteration, replays it twice
        assert rep.graph is not None
        assert torch.equal(rep.z, eng.z) and torch.equal(rep.sse_log[:6], eng.sse_log[:6])
    else:
        assert kind == 'saga-nlm'                                              # (no hipGraph form: the NLM prox ping-pongs)


def test_tile_repeats_the_mixed_batch():
    _, _, _, mixed, _ = _data(F32)
    t = mixed.tile(2)
    assert t.B == 12 and t.M_vec.tolist() == M_VEC * 2 and torch.equal(t.Y[6:], mixed.Y)
    z = _z(F32)
    g = t.grad_full(torch.cat([z, z]), out=torch.empty((12, N_, N_), dtype=F32, device='cuda'))
    ref = mixed.grad_full(z, out=torch.empty_like(z))
    assert torch.equal(g[:6], ref) and torch.equal(g[6:], ref)


def test_svrg_tv_trace_equals_oracle_loop_f64():
    """f64: the rounded PSNR trace of SvrgEngine + TVProx on the mixed batch is identical, for all six members (identity ones
    included), to oracle.loops.pnp_svrg fed the decoded device draws (as test_timed_path_device_draws_vs_oracle does)."""
    from oracle import denoise as od, loops as ol
    from pnp_svrg_amd import ops
    _, _, _, mixed, _ = _data(F64)
    T2, n_outer, eta = 3, 2, 0.8
    eng = _engine('svrg-tv', mixed, IDS)
    inds = []
    for s in range(n_outer * T2):
        eng.step()
        inds.append(ops.indicator_from_thresholds_m(mixed.plan.M_dev, mixed.M, eng.mbs.mbd[s % T2]).cpu().numpy())
    tr = eng.psnr_trace()
    z = eng.z.cpu().numpy().reshape(6, -1)
    for b in range(6):
        po = _oracle(F64, b)
        po.Xrec = mixed.xrec[b].cpu().numpy().copy()
        po.Xinit = mixed.xinit[b].cpu().numpy().ravel().copy()
        it = iter([ind[b, :M_VEC[b]] for ind in inds])
        po.select_mb = lambda size: next(it)
        ro = ol.pnp_svrg(po, od.TVDenoiser(), eta, 2 + n_outer * (3 + 5 * T2) - 1, T2, MB, converge_check=False, clock=ol.CountingClock(),
                         variant='svrg')
        ref = np.asarray(ro['psnr_per_iter'])
        assert len(ref) == 1 + n_outer * (T2 + 1), b
        ref = np.concatenate([ref[1 + o * (T2 + 1) + 1: 1 + (o + 1) * (T2 + 1)] for o in range(n_outer)])
        assert list(tr[:, b]) == list(ref), (b, tr[:, b], ref)
        assert np.abs(z[b] - ro['z'].ravel()).max() <= 1e-3, b                 # (the iterate bound of the test named above)


@pytest.mark.parametrize('how', ['list', 'padded', 'from_problems'])
def test_constructor_and_from_problems_build_the_generated_batch(how):
    """The NumPy constructor (Y as per-problem arrays or padded) and from_problems on problems of different scales give the batch
    `generate` gives: same Y, M_vec and gradients."""
    from types import SimpleNamespace
    from pnp_svrg_amd.engine import DeblurBatch
    _, _, _, mixed, _ = _data(F64)
    Y = mixed.Y.cpu().numpy()
    xrec, xinit = mixed.xrec.cpu().numpy(), mixed.xinit.cpu().numpy().reshape(6, -1)
    Bk = sr.blur_kernel(N_, N_)
    if how == 'from_problems':
        probs = [SimpleNamespace(Xrec=xrec[b], B=Bk, Y=Y[b, :M_VEC[b]], Xinit=xinit[b], scale_percent=SCALES[b]) for b in range(6)]
        b2 = DeblurBatch.from_problems(probs, dtype=F64)
    else:
        Yarg = [Y[b, :M_VEC[b]] for b in range(6)] if how == 'list' else Y
        b2 = DeblurBatch(xrec, Bk, Yarg, xinit, dtype=F64, scale_percent=SCALES)
    assert b2.M_vec.tolist() == M_VEC and torch.equal(b2.Y, mixed.Y) and torch.equal(b2.xinit, mixed.xinit)
    z = _z(F64)
    assert torch.equal(b2.grad_full(z, out=torch.empty_like(z)), mixed.grad_full(z, out=torch.empty_like(z)))
    assert torch.equal(b2.objective(z), mixed.objective(z))
    same = DeblurBatch(xrec[1:2], Bk, Y[1:2, :1024], xinit[1:2], dtype=F64, scale_percent=50)       # an int: the uniform batch
    assert same.M_vec is None and same.M == 1024


def _sweep_kw(alg):
    kw = dict(problem='deblur', seeding='counter', eta=0.8, n_inner=6, mini_batch_size=MB, T2=3, H=N_, W=N_, keep_trace=True)
    if alg == 'saga-nlm':
        kw.update(algorithm='saga', denoiser='nlm', hist_size=4, max_batch=5)          # (8 items: slabs of 5 and 3)
    return kw


@pytest.mark.parametrize('alg,dtype,objective', [('svrg-tv', F64, True), ('svrg-tv', F32, True), ('svrg-tv', F32, False),
                                                 ('saga-nlm', F32, True)])
def test_sweep_mixed_scales_rows_equal_default_runner(alg, dtype, objective):
    """make_runner(mixed_scales=True) on 2 images x alpha {0.1, 0.5, 0.75, 1.0}: one batch (or slabs of max_batch) whose rows equal
    the default, grouped runner's for alpha != 1.0 (z, traces, f_final) and lie within 0.01 dB for alpha == 1.0; objective=False
    replays hipGraphs in both runners."""
    from pnp_svrg_amd import sweep
    imgs = sr.images(2, N_, seed=5)
    items = sweep.make_items(2, [0.1, 0.5, 0.75, 1.0], [20.0])
    kw = dict(_sweep_kw(alg), dtype=dtype, objective=objective)
    ref = sweep.make_runner(imgs, **kw)(items)
    run = sweep.make_runner(imgs, mixed_scales=True, **kw)
    state = run.prepare(items)
    assert [len(c.items) for c in state] == ([8] if alg == 'svrg-tv' else [5, 3])
    run.advance(state, 6)
    got = run.collect(state)
    assert [r['id'] for r in got] == [it['id'] for it in items] == [r['id'] for r in ref]
    for g, r in zip(got, ref):
        if g['item']['alpha'] != 1.0:
            assert np.array_equal(g['z'], r['z']) and np.array_equal(g['psnr_trace'], r['psnr_trace']), g['id']
            assert g['psnr_init'] == r['psnr_init'] and g['loss'] == r['loss']
            if objective:
                assert g['f_final'] == r['f_final'] and np.array_equal(g['f_trace'], r['f_trace'])
        else:
            assert np.abs(g['psnr_trace'] - r['psnr_trace']).max() <= 0.01 + 1e-9, g['id']


def test_grid_search_batch_trials_on_the_tiled_mixed_batch():
    """grid_search(batch_trials=True) over two eta on make_runner(mixed_scales=True, wide_trials=True): the rows of trial-at-a-time."""
    from pnp_svrg_amd import sweep
    imgs = sr.images(2, N_, seed=5)
    items = sweep.make_items(2, [0.1, 0.5, 0.75, 1.0], [20.0])
    kw = dict(_sweep_kw('svrg-tv'), dtype=F32, wide_trials=True, mixed_scales=True)
    mk = lambda **p: sweep.make_runner(imgs, **{**kw, **p})
    a = sweep.grid_search(items, mk, {'eta': [0.4, 0.8]}, batch_trials=True)
    b = sweep.grid_search(items, mk, {'eta': [0.4, 0.8]})
    assert len(a) == len(b) == 8
    for ra, rb in zip(a, b):
        assert ra['id'] == rb['id'] and ra['loss'] == rb['loss'] and ra['params'] == rb['params'] and ra['psnr_final'] == rb['psnr_final']
    k1 = sweep.make_runner(imgs, **kw).data_key
    assert k1 != sweep.make_runner(imgs, **dict(kw, mixed_scales=False)).data_key


def test_saga_nlm_trace_equals_oracle_loop_f64():
    """f64: the rounded PSNR trace of SagaEngine + NLMProx (hist_size = 4) on the mixed batch is identical, for all six members
    (identity ones included), to oracle.loops.pnp_saga with od.NLMDenoiser fed the decoded device draws (the table-filling draw
    first) and the table rows the engine was given; the iterate within the 1e-3 of test_timed_path_device_draws_vs_oracle."""
    from oracle import denoise as od, loops as ol
    from pnp_svrg_amd import ops
    _, _, _, mixed, _ = _data(F64)
    n, eta, hist = 6, 0.8, 4
    np.random.seed(123)
    rows = [np.random.choice(hist, 1).item() for _ in range(n)]                # the stream the oracle loop reads its rows from
    eng = _engine('saga-nlm', mixed, IDS)
    decode = lambda j: ops.indicator_from_thresholds_m(mixed.plan.M_dev, mixed.M, eng.mbs.mbd[j]).cpu().numpy()
    inds = [decode(0)]                                                         # the draw that filled the table (pnp_saga.py:25-29)
    for s in range(n):
        eng.step(r=rows[s])
        inds.append(decode(s % eng.AHEAD))
    tr = eng.psnr_trace()
    assert tr.shape == (n, 6)
    z = eng.z.cpu().numpy().reshape(6, -1)
    for b in range(6):
        po = _oracle(F64, b)
        po.Xrec = mixed.xrec[b].cpu().numpy().copy()
        po.Xinit = mixed.xinit[b].cpu().numpy().ravel().copy()
        assert all(ind[b].sum() == MB and ind[b, M_VEC[b]:].sum() == 0 for ind in inds)
        it = iter([ind[b, :M_VEC[b]] for ind in inds])
        po.select_mb = lambda size: next(it)
        d = od.NLMDenoiser()
        d.sigma = 1.0
        np.random.seed(123)
        # CountingClock: 3 ticks before the loop, 5 per iteration -> tt = 3 + 5 n runs exactly n iterations
        ro = ol.pnp_saga(po, d, eta, 3 + 5 * n, MB, hist_size=hist, converge_check=False, clock=ol.CountingClock())
        ref = np.asarray(ro['psnr_per_iter'])
        assert len(ref) == 1 + n, b
        assert list(tr[:, b]) == list(ref[1:]), (b, tr[:, b], ref[1:])
        assert np.abs(z[b] - ro['z'].ravel()).max() <= 1e-3, b


def test_sweep_mixed_scales_legacy_seeding_rows_equal_default_runner():
    """seeding='legacy' with mixed_scales=True (problems.Deblur objects of different scales through from_problems, host index
    lists): rows equal the default runner's for alpha != 1.0, within 0.01 dB for alpha == 1.0."""
    from pnp_svrg_amd import sweep
    imgs = sr.images(2, N_, seed=5)
    items = sweep.make_items(2, [0.1, 0.5, 1.0], [20.0])
    kw = dict(problem='deblur', seeding='legacy', eta=0.8, n_inner=4, mini_batch_size=MB, T2=2, H=N_, W=N_, keep_trace=True,
              dtype=F64)
    ref = sweep.make_runner(imgs, **kw)(items)
    run = sweep.make_runner(imgs, mixed_scales=True, **kw)
    state = run.prepare(items)
    assert len(state) == 1 and state[0].batch.M_vec.tolist() == [36, 1024, 4096] * 2
    run.advance(state, 4)
    got = run.collect(state)
    assert [r['id'] for r in got] == [r['id'] for r in ref] == [it['id'] for it in items]
    for g, r in zip(got, ref):
        if g['item']['alpha'] != 1.0:
            assert np.array_equal(g['z'], r['z']) and np.array_equal(g['psnr_trace'], r['psnr_trace']), g['id']
        else:
            assert np.abs(g['psnr_trace'] - r['psnr_trace']).max() <= 0.01 + 1e-9, g['id']
