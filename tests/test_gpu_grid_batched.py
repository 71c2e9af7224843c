"""A hyper-parameter grid as one batch: the per-problem (`_pp`) kernels, the engines that drive them and
`sweep.grid_search(batch_trials=True)`.  Everything here is "equal bit for bit to the scalar call made with that problem's
values": the kernels convert a per-problem value exactly as the host converts the scalar."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev(v, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(v, dtype)).cuda()


def _same(x, y):
    """bit for bit, NaNs included (a diverging trial must still equal its scalar twin)"""
    if isinstance(x, np.ndarray):
        return np.array_equal(x, y, equal_nan=True)
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}.get(x.dtype)
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(iv) if iv else x, y.contiguous().view(iv) if iv else y)


def _force_path(monkeypatch, min_batch):
    """The same kernel path on both sides of a comparison, whatever the batch sizes: the streaming and the one-kernel forms
    agree to the loop tolerance only."""
    from pnp_svrg_amd.engine import SvrgEngine
    monkeypatch.setenv('PNP_CSMRI_FUSED_MIN_BATCH', str(min_batch))
    monkeypatch.setattr(SvrgEngine, 'FUSED_MIN_BATCH', min_batch)


# ------------------------------------------------------------------------------------------------------------ 1. draw
def _mix64(x):
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _keys_np(seed, step, ident, pos):
    """The published key (include/pnp_hip.h) with the stream absorbing `ident` where the plain draw absorbs the batch index."""
    with np.errstate(over='ignore'):
        st = _mix64(_mix64(_mix64(np.uint64(seed)) + np.uint64(step)) + np.uint64(ident))
        x = (np.uint32(int(st) & 0xFFFFFFFF) ^ pos.astype(np.uint32)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
        x ^= x >> np.uint32(15)
        x = (x * np.uint32(0x846ca68b)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        return (x ^ np.uint32(int(st) >> 32)).astype(np.uint32)


def _unpack(selbits, n):
    """bit-packed transposed selectors [..., W, H/32] -> bool [..., W, H]"""
    w = selbits.cpu().numpy().view(np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[:-1] + (n,))


def test_draw_per_problem_mb_and_id():
    from pnp_svrg_amd import ops
    n, B, seed, step0, nsteps = 64, 6, 0xC0FFEE123, 40, 3
    rng = np.random.default_rng(5)
    m3 = (rng.random((3, n, n)) < np.array([0.3, 0.4, 0.5])[:, None, None]).astype(np.uint8)
    plan3, plan6 = ops.CsmriPlan(n, n, 3, torch.float32), ops.CsmriPlan(n, n, B, torch.float32)
    bits3 = plan3.pack_mask(plan3.sel_from_dense(torch.from_numpy(m3).cuda()))
    bits6 = bits3.repeat(2, 1, 1).contiguous()
    sb3 = torch.zeros((nsteps, 3, n, n // 32), dtype=torch.int32, device='cuda')
    sb3b = torch.zeros_like(sb3)
    sb6 = torch.zeros((nsteps, B, n, n // 32), dtype=torch.int32, device='cuda')
    d200 = plan3.draw_thresholds(bits3, 200, seed, step0, nsteps, selbits=sb3)
    plan3.draw_thresholds(bits3, 300, seed, step0, nsteps, selbits=sb3b)
    ids = _dev([0, 1, 2, 0, 1, 2], np.int32)
    mbv = _dev([200, 200, 200, 200, 50, 300], np.int32)
    d6 = plan6.draw_thresholds(bits6, mbv, seed, step0, nsteps, selbits=sb6, draw_id=ids)
    # problems 0..2: the plain draw, descriptors and selections; problem 3 is problem 0 again
    assert torch.equal(d6[:, :3], d200) and torch.equal(sb6[:, :3], sb3)
    assert torch.equal(d6[:, 3], d6[:, 0]) and torch.equal(sb6[:, 3], sb6[:, 0])
    s6, s300 = _unpack(sb6, n), _unpack(sb3b, n)
    for t in range(nsteps):
        assert s6[t, 4].sum() == 50 and not (s6[t, 4] & ~s6[t, 1]).any()          # 50 of problem 1's 200
        assert s6[t, 1].sum() == 200 and not (s6[t, 1] & ~s300[t, 1]).any()       # which are 200 of the scalar 300
        assert s6[t, 5].sum() == 300 and np.array_equal(s6[t, 5], s300[t, 2])
    # known answer: problem 4 (id 1, mb 50), step 1, against the published key
    pos = np.flatnonzero(m3[1])
    keys = _keys_np(seed, step0 + 1, 1, pos)
    order = np.lexsort((pos, keys))[:50]
    d = d6[1, 4].cpu().numpy().view(np.uint32)
    assert (int(d[2]), int(d[3])) == (int(keys[order[-1]]), int(pos[order[-1]]))
    want = np.zeros(n * n, bool)
    want[pos[order]] = True
    assert np.array_equal(s6[1, 4], want.reshape(n, n).T)
    # an entry above the support size selects the whole support; draw_id = None is the batch index
    big = _dev([200, int(m3[1].sum()) + 7, 200], np.int32)
    sbb = torch.zeros_like(sb3)
    db = plan3.draw_thresholds(bits3, big, seed, step0, nsteps, selbits=sbb)
    assert torch.equal(sbb[:, 1], bits3[1].expand(nsteps, -1, -1)) and torch.equal(db[:, 0], d200[:, 0]) and torch.equal(sbb[:, 2], sb3[:, 2])


def test_draw_thresholds_m_candidates_per_problem():
    from pnp_svrg_amd import ops
    M, seed = 4096, 99
    plain = {mb: ops.draw_thresholds(M, 3, mb, seed, 7, 2) for mb in (100, 700)}
    d = ops.draw_thresholds(M, 4, _dev([100, 700, 100, 5000], np.int32), seed, 7, 2, draw_id=_dev([0, 1, 2, 1], np.int32))
    assert torch.equal(d[:, 0], plain[100][:, 0]) and torch.equal(d[:, 1], plain[700][:, 1]) and torch.equal(d[:, 2], plain[100][:, 2])
    sel = ops.indicator_from_thresholds(M, d[0]).cpu().numpy()
    assert sel.sum(1).tolist() == [100, 700, 100, M]
    keys = _keys_np(seed, 7, 1, np.arange(M))
    order = np.lexsort((np.arange(M), keys))[:700]
    assert np.array_equal(np.flatnonzero(sel[1]), np.sort(order))


# ------------------------------------------------------------------------------------------------------------ 2. kernels
@pytest.mark.parametrize('dtype,n,min_batch', [(torch.float32, 64, 10 ** 6), (torch.float64, 64, 10 ** 6), (torch.float32, 128, 10 ** 6),
                                               (torch.float64, 128, 10 ** 6), (torch.float32, 256, 1)])
def test_grad_sel_per_problem(dtype, n, min_batch, monkeypatch):
    """grad_sel with per-problem alpha and gamma == the scalar call per value (streaming kernels; at 256 x 256 the one-kernel
    gradient too)."""
    from pnp_svrg_amd.engine import CsmriBatch
    _force_path(monkeypatch, min_batch)
    B = 4
    b = CsmriBatch.synthetic(B, n, n, 0.3, 20.0, seed=n, dtype=dtype)
    g = torch.Generator().manual_seed(1)
    z, w, mu = (torch.rand((B, n, n), generator=g, dtype=torch.float64).to('cuda', dtype) for _ in range(3))
    al, ga = np.array([-0.37, -1.9e-3, -0.37, -1.9e-3]), np.array([-3.1e2, -3.1e2, -7.7, -7.7])
    got = b.plan.grad(z, b=w, bits=b.bits, alpha=_dev(al), alpha_vec=b.inv_m0, beta=1.0, c1=z, gamma=_dev(ga), c2=mu)
    full = b.plan.grad(z, bits=b.bits, yh=b.yh_full, alpha=_dev(al), alpha_vec=b.inv_m0, beta=1.0, c1=z)
    for k in range(B):
        ref = b.plan.grad(z, b=w, bits=b.bits, alpha=float(al[k]), alpha_vec=b.inv_m0, beta=1.0, c1=z, gamma=float(ga[k]), c2=mu)
        assert torch.equal(got[k], ref[k])
        assert torch.equal(full[k], b.plan.grad(z, bits=b.bits, yh=b.yh_full, alpha=float(al[k]), alpha_vec=b.inv_m0, beta=1.0, c1=z)[k])
    only_alpha = b.plan.grad(z, b=w, bits=b.bits, alpha=_dev(al), beta=1.0, c1=z, gamma=-2.5, c2=mu)
    assert torch.equal(only_alpha[1], b.plan.grad(z, b=w, bits=b.bits, alpha=float(al[1]), beta=1.0, c1=z, gamma=-2.5, c2=mu)[1])


def test_one_kernel_calls_per_problem():
    """svrg_step, svrg_outer_step and svrg_outer_iteration (f32 256 x 256, B = 4, T2 = 3) with two values each of lr, mb and
    sigma_modifier == the scalar calls."""
    from pnp_svrg_amd.engine import CsmriBatch
    B, n, T2 = 4, 256, 3
    b = CsmriBatch.synthetic(B, n, n, 0.3, 20.0, seed=3)
    lr, mb, sm = np.array([500.0, 123.4, 500.0, 123.4]), np.array([300, 300, 1000, 1000], np.int32), np.array([1.0, 1.3, 1.3, 1.0])
    mbs = b.minibatches(T2)
    b.draw(mbs, mb, 11, 0, T2)
    sel = mbs.selbits

    def run(lr_, mb_, sm_, al_, ga_):
        o = {}
        z = b.xinit.clone()
        w, mu = torch.empty_like(z), torch.empty_like(z)
        sse, sig = torch.zeros(B, dtype=torch.float64, device='cuda'), torch.zeros(B, device='cuda')
        b.plan.svrg_outer_step(z, b.bits, b.yh_full, b.inv_m0, lr_, w, mu, out=z, xrec=b.xrec, sse=sse, sigma_modifier=sm_, sigma_out=sig)
        o['outer'] = (z.clone(), w.clone(), mu.clone(), sse.clone(), sig.clone())
        b.plan.svrg_step(z, w, sel[1], alpha=al_, beta=1.0, c1=z, gamma=ga_, c2=mu, out=z, xrec=b.xrec, sse=sse, sigma_modifier=sm_,
                         sigma_out=sig)
        o['step'] = (z.clone(), sse.clone(), sig.clone())
        nd = b.plan.svrg_step(z, w, sel[2], alpha=al_, beta=1.0, c1=z, gamma=ga_, c2=mu, denoise=False, sigma_out=sig)[0]
        o['step_nd'] = (nd.clone(), sig.clone())
        z2 = b.xinit.clone()
        log = torch.zeros((5, B), dtype=torch.float64, device='cuda')
        b.plan.svrg_outer_iteration(z2, w, mu, b.bits, b.yh_full, b.inv_m0, sel, T2, lr_, mb_, b.xrec, log, 1, sig, sigma_modifier=sm_)
        o['iter'] = (z2, w.clone(), mu.clone(), log, sig.clone())
        return o

    got = run(_dev(lr), _dev(mb, np.int32), _dev(sm), _dev(-lr / mb), _dev(-lr))
    for k in range(B):
        ref = run(float(lr[k]), int(mb[k]), float(sm[k]), -float(lr[k]) / int(mb[k]), -float(lr[k]))
        for name in got:
            for x, y in zip(got[name], ref[name]):
                assert torch.equal(x[..., k] if x.dim() == 2 and x.shape[0] == 5 else x[k], y[..., k] if y.dim() == 2 and y.shape[0] == 5 else y[k]), (name, k)
    assert not torch.equal(got['iter'][0][0], got['iter'][0][1])


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('H,W,B', [(64, 48, 3), (256, 256, 3), (64, 48, 40)])
def test_prox_per_problem_sigma_modifier(dtype, H, W, B):
    """prox_tv and prox_wavelet2d (small-batch split form and one-workgroup form) with a per-problem sigma_modifier."""
    from pnp_svrg_amd import ops
    g = torch.Generator().manual_seed(H + B)
    z = torch.rand((B, H, W), generator=g, dtype=torch.float64).to('cuda', dtype)
    xr = torch.rand((B, H, W), generator=g, dtype=torch.float64).to('cuda', dtype)
    vals = [0.8, 1.0, 1.7]
    sm = np.array([vals[k % 3] for k in range(B)])
    for prox in (ops.prox_tv, ops.prox_wavelet2d):
        out, sse, sig = prox(z, sigma_modifier=_dev(sm), xrec=xr)
        for v in vals:
            ro, rs, rg = prox(z, sigma_modifier=v, xrec=xr)
            k = np.flatnonzero(sm == v)
            assert torch.equal(out[k], ro[k]) and torch.equal(sse[k], rs[k]) and torch.equal(sig[k], rg[k])
        sig_in = ops.sigma_est(z)
        o2 = prox(z, sigma_in=sig_in, sigma_modifier=_dev(sm), xrec=xr)[0]
        assert torch.equal(o2, out)


# ------------------------------------------------------------------------------------------------------------ 3. engines
_ETA, _MB, _SM = [500.0, 90.0], [150, 400], [1.0, 1.4]
_TRIALS = [(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0)]             # (eta, mb, sigma_modifier) index per trial


def _trial_vectors(n_items):
    rep = lambda vals, col: np.repeat([vals[t[col]] for t in _TRIALS], n_items)
    return rep(_ETA, 0).astype(np.float64), rep(_MB, 1).astype(np.int32), rep(_SM, 2).astype(np.float64)


def _run_engine(eng, steps, T2, mode):
    if mode == 'outer':
        eng.run_outer(steps // T2)
    elif mode == 'graph':
        eng.run_outer(steps // T2, one_launch=False)
    else:
        for _ in range(steps):
            eng.step()
    torch.cuda.synchronize()
    return eng.z.clone(), eng.psnr_trace()


_CONFIGS = [
    ('f64-64', torch.float64, 64, 10 ** 6, {}, 'step'),
    ('f32-64', torch.float32, 64, 10 ** 6, {}, 'step'),
    ('f32-64-graph', torch.float32, 64, 10 ** 6, {}, 'graph'),
    ('f32-256-one-kernel', torch.float32, 256, 1, {}, 'step'),
    ('f32-256-unfolded', torch.float32, 256, 1, {'fold_outer': False}, 'step'),
    ('f32-256-graph', torch.float32, 256, 1, {}, 'graph'),
    ('f32-256-outer', torch.float32, 256, 1, {}, 'outer'),
]


@pytest.mark.parametrize('name,dtype,n,min_batch,kw,mode', _CONFIGS, ids=[c[0] for c in _CONFIGS])
def test_svrg_engine_tiled_trials(name, dtype, n, min_batch, kw, mode, monkeypatch):
    """SvrgEngine on 2 items x 4 trials (tiled batch, per-problem eta, mb, sigma_modifier) == four scalar engines on the
    untiled batch: z and the PSNR trace, bit for bit."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    _force_path(monkeypatch, min_batch)
    T2, steps, ni = 3, 6, 2
    base = CsmriBatch.synthetic(ni, n, n, 0.3, 20.0, seed=21, dtype=dtype)
    eta, mb, sm = _trial_vectors(ni)
    variants = ('svrg',) if n == 256 else ('svrg', 'reference')
    for variant in variants:
        eng = SvrgEngine(base.tile(4), TVProx(sigma_modifier=sm), eta, T2, mb, variant=variant, seed=5, draw_id=np.tile(np.arange(ni), 4), **kw)
        if n == 256:
            assert eng.fused and (eng.outer_kernel_ok() or not eng.fold_outer)
        z, tr = _run_engine(eng, steps, T2, mode)
        for t, (ie, im, isg) in enumerate(_TRIALS):
            ref = SvrgEngine(base, TVProx(sigma_modifier=_SM[isg]), _ETA[ie], T2, _MB[im], variant=variant, seed=5, **kw)
            zr, trr = _run_engine(ref, steps, T2, mode)
            assert _same(z[t * ni:(t + 1) * ni], zr), (variant, t)
            assert _same(tr[:, t * ni:(t + 1) * ni], trr), (variant, t)
    assert not torch.equal(z[0], z[ni])


@pytest.mark.parametrize('algo', ['sgd', 'gd'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('multi', [True, False])
def test_sgd_gd_engines_tiled_trials(algo, dtype, multi, monkeypatch):
    from pnp_svrg_amd.engine import CsmriBatch, TVProx, make_engine
    _force_path(monkeypatch, 10 ** 6)
    n, ni, steps = 64, 2, 6
    base = CsmriBatch.synthetic(ni, n, n, 0.3, 20.0, seed=22, dtype=dtype)
    eta, mb, sm = _trial_vectors(ni)
    eng = make_engine(base.tile(4), TVProx(sigma_modifier=sm, multi=multi), eta * 1e-3 if algo == 'gd' else eta, 3, mb, lr_decay=0.9,
                      algorithm=algo, seed=5, draw_id=np.tile(np.arange(ni), 4))
    z, tr = _run_engine(eng, steps, 3, 'step')
    for t, (ie, im, isg) in enumerate(_TRIALS):
        ref = make_engine(base, TVProx(sigma_modifier=_SM[isg], multi=multi), _ETA[ie] * 1e-3 if algo == 'gd' else _ETA[ie], 3, _MB[im],
                          lr_decay=0.9, algorithm=algo, seed=5)
        zr, trr = _run_engine(ref, steps, 3, 'step')
        assert _same(z[t * ni:(t + 1) * ni], zr) and _same(tr[:, t * ni:(t + 1) * ni], trr), t


def test_svrg_engine_tiled_trials_dncnn(monkeypatch):
    """A prox without per-problem parameters passes through: DnCNN, 64 x 64, 2 items x 2 trials (eta, mb)."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, DnCNNProx
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    _force_path(monkeypatch, 10 ** 6)
    wts, ni, T2 = random_dncnn_weights(5, seed=1), 2, 3
    base = CsmriBatch.synthetic(ni, 64, 64, 0.3, 20.0, seed=23)
    eng = SvrgEngine(base.tile(2), DnCNNProx(wts, 15), np.repeat(_ETA, ni), T2, np.repeat(_MB, ni).astype(np.int32), seed=5,
                     draw_id=np.tile(np.arange(ni), 2))
    z, tr = _run_engine(eng, 6, T2, 'step')
    for t in range(2):
        zr, trr = _run_engine(SvrgEngine(base, DnCNNProx(wts, 15), _ETA[t], T2, _MB[t], seed=5), 6, T2, 'step')
        assert _same(z[t * ni:(t + 1) * ni], zr) and _same(tr[:, t * ni:(t + 1) * ni], trr)


def test_per_problem_minibatch_size_is_checked():
    from pnp_svrg_amd.engine import CsmriBatch, SgdEngine, TVProx
    b = CsmriBatch.synthetic(2, 64, 64, 0.3, 20.0, seed=1)
    for bad in ([100, 0], [100, int(b.M0[1]) + 1]):
        with pytest.raises(ValueError, match='problem 1'):
            SgdEngine(b, TVProx(), 1.0, np.array(bad, np.int32))


# ------------------------------------------------------------------------------------------------------------ 4. grid_search
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def _rows_key(rows):
    return [(r['id'], r['loss'], r['params'], r['psnr_init'], r['psnr_final']) for r in rows]


def test_grid_search_batched_equals_serial(monkeypatch):
    import functools
    from pnp_svrg_amd import ops, sweep
    _force_path(monkeypatch, 10 ** 6)
    imgs = _images(3, 64)
    items = [it for it in sweep.make_items(3, [0.3, 0.5], [20.0]) if it['id'] in (0, 3, 4)]
    mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'svrg', 'tv', n_inner=6, H=64, W=64, seeding='counter', max_batch=2)
    grid = {'eta': [500.0, 60.0], 'mini_batch_size': [150, 400], 'sigma_modifier': [1.0, 1.4], 'T2': [2, 3]}
    serial = sweep.grid_search(items, mk, grid)
    calls = []
    real = ops.CsmriPlan.generate
    monkeypatch.setattr(ops.CsmriPlan, 'generate', lambda self, *a, **k: (calls.append(self.B), real(self, *a, **k))[1])
    batched = sweep.grid_search(items, mk, grid, batch_trials=True)
    assert calls == [2, 1]                                             # once per chunk (3 items, max_batch 2), not per trial or group
    assert _rows_key(batched) == _rows_key(serial)
    small = sweep.grid_search(items, mk, grid, batch_trials=True, max_batch_trials=5)      # 2 trials (of 8 per group) per slab
    assert _rows_key(small) == _rows_key(serial)
    for algo in ('sgd', 'gd'):
        mk2 = functools.partial(sweep.make_runner, imgs, 'csmri', algo, 'tv', n_inner=4, T2=2, H=64, W=64, seeding='counter',
                                **({} if algo == 'sgd' else {'mini_batch_size': None}))
        g2 = {'eta': [1.0, 0.2] if algo == 'gd' else [500.0, 60.0], 'sigma_modifier': [1.0, 1.4]}
        if algo == 'sgd':
            g2['mini_batch_size'] = [150, 400]
        assert _rows_key(sweep.grid_search(items, mk2, g2, batch_trials=True)) == _rows_key(sweep.grid_search(items, mk2, g2))


@pytest.mark.parametrize('kw,word', [(dict(problem='deblur'), 'deblur'), (dict(algorithm='saga'), 'saga'), (dict(algorithm='sarah'), 'sarah'),
                                     (dict(denoiser='nlm'), 'nlm'), (dict(seeding='legacy'), 'legacy')])
def test_grid_search_batched_refuses(kw, word):
    from pnp_svrg_amd import sweep
    a = dict(problem='csmri', algorithm='svrg', denoiser='tv', seeding='counter')
    a.update(kw)
    items = sweep.make_items(1, [0.5], [20.0])

    def mk(eta):
        return sweep.make_runner(_images(1, 64), a['problem'], a['algorithm'], a['denoiser'], eta=eta, n_inner=2, mini_batch_size=50, T2=2,
                                 H=64, W=64, seeding=a['seeding'])
    with pytest.raises(ValueError, match=word):
        sweep.grid_search(items, mk, {'eta': [1.0, 2.0]}, batch_trials=True)


# ------------------------------------------------------------------------------------------------------------ 5. independence
def test_item_does_not_depend_on_the_batch(monkeypatch):
    """Item 0 of a 15 x 16 tiled batch (B = 240, 256 x 256, f32, TV, two outer iterations) == the same item and trial of a
    2 x 2 tiled run, with the one-kernel path forced on both sides."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    _force_path(monkeypatch, 1)
    T2, n = 3, 256
    big = CsmriBatch.synthetic(15, n, n, 0.3, 20.0, seed=31)
    small = CsmriBatch(big.xrec[:2].cpu().numpy(), big.mask_np[:2], np.swapaxes(big.YT[:2].cpu().numpy(), 1, 2),
                       big.xinit[:2].cpu().numpy().reshape(2, -1))
    etas, mbs_, sms = np.linspace(100, 600, 16), np.linspace(200, 2000, 16).astype(np.int32), np.linspace(0.8, 1.5, 16)
    e1 = SvrgEngine(big.tile(16), TVProx(sigma_modifier=np.repeat(sms, 15)), np.repeat(etas, 15), T2, np.repeat(mbs_, 15), seed=1,
                    draw_id=np.tile(np.arange(15), 16))
    e1.run_outer(2)
    pick = [0, 9]
    e2 = SvrgEngine(small.tile(2), TVProx(sigma_modifier=np.repeat(sms[pick], 2)), np.repeat(etas[pick], 2), T2, np.repeat(mbs_[pick], 2),
                    seed=1, draw_id=np.tile(np.arange(2), 2))
    e2.run_outer(2)
    torch.cuda.synchronize()
    t1, t2 = e1.psnr_trace(), e2.psnr_trace()
    for k, t in enumerate(pick):
        assert _same(e1.z[t * 15], e2.z[k * 2]) and _same(t1[:, t * 15], t2[:, k * 2])
        assert _same(e1.z[t * 15 + 1], e2.z[k * 2 + 1])
