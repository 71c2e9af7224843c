"""The one-kernel pnp_sarah inner iteration (pnp_csmri_sarah_step, csrc/csmri_fused.hip) and SarahEngine(fused=True):
the kernel against the gradient-only instantiation of the same transform code and against the streaming kernels, its aliasing and
per-problem forms, the engine against the streaming engine, scalar engines, its hipGraph form, the oracle loop, and the sweep.

Every case is 256 x 256 (the kernel has no other size) with B = 3.  The bounds are the ones tests/test_gpu_engine.py holds
pnp_csmri_svrg_step and SvrgEngine(fused=True) to: the operands have the same scale."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
B, MB, LR, SM = 3, 1000, 2e3, 1.3


def _f64(n):
    return torch.empty(n, dtype=torch.float64, device='cuda')


@pytest.fixture(scope='module')
def ops_():
    """Operands of one inner iteration (a = w_next, b = w_prev, c1 = v_prev, c2 = z), one drawn selector, and the all-distinct call."""
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.engine import CsmriBatch
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=41)
    p = batch.plan
    rng = np.random.default_rng(0)
    dev = lambda v: torch.from_numpy(v).float().cuda().contiguous()                  # noqa: E731
    z = batch.xinit.clone()
    w_next = dev(batch.xinit.cpu().numpy() + 0.05 * rng.standard_normal((B, 256, 256)))
    w_prev = dev(batch.xinit.cpu().numpy() + 0.05 * rng.standard_normal((B, 256, 256)))
    v_prev = dev(1e-4 * rng.standard_normal((B, 256, 256)))
    selbits = torch.empty((1, B, 256, 8), dtype=torch.int32, device='cuda')
    p.draw_thresholds(batch.bits, MB, seed=3, step0=7, nsteps=1, selbits=selbits)
    o = dict(batch=batch, p=p, a=w_next, b=w_prev, c1=v_prev, c2=z, sel=selbits[0])
    keep = {k: o[k].clone() for k in ('a', 'b', 'c1', 'c2')}
    nan = lambda: torch.full_like(z, float('nan'))                                   # noqa: E731
    v_out, out, out2 = nan(), nan(), nan()
    r = p.sarah_step(w_next, w_prev, selbits[0], alpha=1.0 / MB, beta=1.0, c1=v_prev, gamma=-LR, c2=z, v_out=v_out, out=out, out2=out2,
                     xrec=batch.xrec, sigma_modifier=SM, sse=_f64(B))
    torch.cuda.synchronize()
    o.update(keep=keep, v_out=v_out, out=out, out2=out2, sse=r[1], sig=r[2], ret=r)
    return o


def test_v_out_is_the_gradient_only_instantiation(ops_, monkeypatch):
    """v_out == the one-kernel gradient of the same operands, bit for bit (the gradient-only instantiation of the same transform
    code, reached on a plan made under PNP_CSMRI_FUSED_MIN_BATCH=1); against the streaming kernels 2e-6 * max(1, |ref|)."""
    from pnp_svrg_amd import ops
    o = ops_
    assert o['ret'][0] is o['out'] and o['ret'][3] is o['v_out']
    monkeypatch.setenv('PNP_CSMRI_FUSED_MIN_BATCH', '1')
    pf = ops.CsmriPlan(256, 256, B, torch.float32)
    monkeypatch.delenv('PNP_CSMRI_FUSED_MIN_BATCH')
    kw = dict(bits=o['sel'], b=o['b'], alpha=1.0 / MB, beta=1.0, c1=o['c1'])
    one = pf.grad(o['a'], **kw)
    assert one.abs().max().item() > 0 and torch.equal(o['v_out'], one)
    ref = o['p'].grad(o['a'], **kw)                              # B = 3: the three streaming kernels
    d, bound = (o['v_out'] - ref).abs().max().item(), 2e-6 * max(1.0, ref.abs().max().item())
    print(f'v_out vs streaming: {d:.3e} (bound {bound:.3e})')
    assert d <= bound


def test_denoise_off_stores_the_stepped_image(ops_):
    """denoise=0: out == c2 + gamma * v_out to one float32 ulp (reference formed in float64 from the returned v_out, rounded
    once); the noise estimate is the streaming one to 1e-6 relative."""
    from pnp_svrg_amd import ops
    o = ops_
    out, sse, sig, v = o['p'].sarah_step(o['a'], o['b'], o['sel'], alpha=1.0 / MB, beta=1.0, c1=o['c1'], gamma=-LR, c2=o['c2'],
                                         denoise=False)
    assert sse is None and torch.equal(v, o['v_out'])
    ref = (o['c2'].double() + (-LR) * v.double()).float()
    inf = torch.full_like(ref, float('inf'))
    ok = (out == ref) | (out == torch.nextafter(ref, inf)) | (out == torch.nextafter(ref, -inf))
    assert bool(ok.all()), (out - ref).abs().max().item()
    assert not torch.equal(out, o['c2'])
    want = ops.sigma_est(out)
    assert (sig - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    assert (o['sig'] - want).abs().max().item() <= 1e-6 * want.abs().max().item()      # ... and the same with the prox on


def test_whole_step_against_streaming_kernels(ops_):
    """pnp_csmri_grad_sel (streaming) + pnp_axpbypcz + pnp_prox_tv: |out - want| <= 2e-5, sse to rtol 1e-4, out2 == out."""
    from pnp_svrg_amd import ops
    o = ops_
    v = o['p'].grad(o['a'], bits=o['sel'], b=o['b'], alpha=1.0 / MB, beta=1.0, c1=o['c1'])
    stepped = ops.axpbypcz(1.0, o['c2'], -LR, v)
    want, want_sse, want_sig = ops.prox_tv(stepped, xrec=o['batch'].xrec, sigma_modifier=SM)
    assert not torch.equal(want, stepped)
    d = (o['out'] - want).abs().max().item()
    print(f'out vs streaming: {d:.3e} (bound 2e-5)')
    assert d <= 2e-5
    np.testing.assert_allclose(o['sse'].cpu().numpy(), want_sse.cpu().numpy(), rtol=1e-4)
    assert torch.equal(o['out2'], o['out'])
    assert (o['sig'] - want_sig).abs().max().item() <= 1e-6 * want_sig.abs().max().item()


def test_aliasing_the_engines_calling_form(ops_):
    """v_out = c1, out = c2, out2 = b (what SarahEngine passes) == the all-distinct call; the NaN sentinels of the all-distinct
    call are all overwritten and its inputs unchanged."""
    o = ops_
    for k in ('v_out', 'out', 'out2'):
        assert not torch.isnan(o[k]).any(), k
    for k, v in o['keep'].items():
        assert torch.equal(o[k], v), k
    a, b, c1, c2 = (o[k].clone() for k in ('a', 'b', 'c1', 'c2'))
    sse = _f64(B)
    o['p'].sarah_step(a, b, o['sel'], alpha=1.0 / MB, beta=1.0, c1=c1, gamma=-LR, c2=c2, v_out=c1, out=c2, out2=b,
                      xrec=o['batch'].xrec, sigma_modifier=SM, sse=sse)
    assert torch.equal(c1, o['v_out']) and torch.equal(c2, o['out']) and torch.equal(b, o['out2']) and torch.equal(a, o['a'])
    assert torch.equal(sse, o['sse'])


def test_per_problem_coefficients(ops_):
    """_pp: problem b == the plain call on a B = 1 plan with b's scalars, bit for bit (so a problem does not depend on its batch
    either); a _pp call with every array NULL == the plain call."""
    from pnp_svrg_amd import _native as N, ops
    o = ops_
    al, ga, sm = [1.0 / 900, 1.0 / 1000, 1.0 / 1300], [-1.5e3, -2e3, -2.75e3], [0.9, 1.3, 1.7]
    t = lambda v: torch.tensor(v, dtype=torch.float64, device='cuda')              # noqa: E731
    sse = _f64(B)
    out, _, sig, v = o['p'].sarah_step(o['a'], o['b'], o['sel'], alpha=t(al), beta=1.0, c1=o['c1'], gamma=t(ga), c2=o['c2'],
                                       xrec=o['batch'].xrec, sigma_modifier=t(sm), sse=sse)
    p1 = ops.CsmriPlan(256, 256, 1, torch.float32)
    for k in range(B):
        s = slice(k, k + 1)
        sse1 = _f64(1)
        out1, _, sig1, v1 = p1.sarah_step(o['a'][s], o['b'][s], o['sel'][s].contiguous(), alpha=al[k], beta=1.0, c1=o['c1'][s], gamma=ga[k],
                                          c2=o['c2'][s], xrec=o['batch'].xrec[s], sigma_modifier=sm[k], sse=sse1)
        assert torch.equal(v[s], v1) and torch.equal(out[s], out1) and torch.equal(sig[s], sig1) and torch.equal(sse[s], sse1), k
    assert not torch.equal(out[0], out[1])
    # every array NULL
    v2, out2, out22 = (torch.empty_like(o['out']) for _ in range(3))
    sse2, sig2 = _f64(B), torch.empty(B, device='cuda')
    P = ops._p
    N.call('pnp_csmri_sarah_step_pp', o['p']._h, P(o['a']), P(o['b']), P(o['sel']), 1.0 / MB, None, None, 1.0, P(o['c1']), -LR, None,
           P(o['c2']), P(v2), P(out2), P(out22), 1, SM, None, 0.0, P(o['batch'].xrec), P(sse2), P(sig2), ops._stream())
    assert torch.equal(v2, o['v_out']) and torch.equal(out2, o['out']) and torch.equal(out22, o['out2'])
    assert torch.equal(sse2, o['sse']) and torch.equal(sig2, o['sig'])


def test_argument_checks(ops_):
    """PNP_ERR_ARG from the library and ValueError from the front end, before any device work (nothing is launched)."""
    from pnp_svrg_amd import _native as N, ops
    o = ops_
    p, kw = o['p'], dict(alpha=1.0 / MB, beta=1.0, c1=o['c1'], gamma=-LR, c2=o['c2'])
    with pytest.raises(ValueError, match='out2 needs denoise'):
        p.sarah_step(o['a'], o['b'], o['sel'], out2=torch.empty_like(o['a']), denoise=False, **kw)
    with pytest.raises(ValueError, match='v_out may alias c1 only'):
        p.sarah_step(o['a'], o['b'], o['sel'], v_out=o['a'], **kw)
    small = torch.zeros((1, 128, 128), device='cuda')
    with pytest.raises(ValueError, match='256 x 256'):
        ops.CsmriPlan(128, 128, 1, torch.float32).sarah_step(small, small, torch.zeros((1, 128, 4), dtype=torch.int32, device='cuda'),
                                                             c1=small, c2=small)
    with pytest.raises(ValueError, match='float32'):
        ops.CsmriPlan(256, 256, 1, torch.float64).sarah_step(o['a'][:1].double(), o['b'][:1].double(), o['sel'][:1].contiguous(),
                                                             c1=o['c1'][:1].double(), c2=o['c2'][:1].double())
    # the library's own return codes: plan, a, b, bitsT, alpha, alpha_vec, beta, c1, gamma, c2, v_out, out, out2, denoise, ...
    h, P = N.lib(), ops._p
    spare = [torch.empty_like(o['a']) for _ in range(3)]
    ok = [p._h, P(o['a']), P(o['b']), P(o['sel']), 1.0 / MB, None, 1.0, P(o['c1']), -LR, P(o['c2']), P(spare[0]), P(spare[1]), P(spare[2]),
          1, 1.0, 0.0, None, None, None, None]
    p128, p64 = ops.CsmriPlan(128, 128, 1, torch.float32), ops.CsmriPlan(256, 256, 1, torch.float64)
    bad = {'out2 with denoise 0': {13: 0}, 'v_out is a': {10: P(o['a'])}, 'v_out is b': {10: P(o['b'])}, 'v_out is c2': {10: P(o['c2'])},
           'v_out is out': {10: P(spare[1])}, 'v_out is out2': {10: P(spare[2])}, '128 x 128 plan': {0: p128._h}, 'float64 plan': {0: p64._h},
           'null b': {2: None}, 'null c1': {7: None}, 'null c2': {9: None}, 'null v_out': {10: None}, 'null out': {11: None},
           'sse without xrec': {17: P(_f64(B))}}
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_csmri_sarah_step(*args) == 1, what
        assert h.pnp_last_error().decode(), what
        pp = args[:5] + [None] + args[5:9] + [None] + args[9:15] + [None] + args[15:]
        assert h.pnp_csmri_sarah_step_pp(*pp) == 1, what


def _mk_prox(kind):
    from pnp_svrg_amd.engine import TVProx, DnCNNProx
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    if kind == 'tv':
        return TVProx(sigma_modifier=1.1), 2e3
    return DnCNNProx(random_dncnn_weights(17, seed=1), 15), 1.0


@pytest.mark.parametrize('prox_kind', ['tv', 'dncnn'])
def test_fused_engine_equals_streaming_engine(prox_kind):
    """SarahEngine(fused=True) walks the trajectory of the streaming SarahEngine: device draws and host index lists, T2 = 4, 9 steps
    (12 log rows).  Bounds: those of test_fused_engine_equals_unfused."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine
    T2, steps = 4, 9
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=13)
    for host in ((False, True) if prox_kind == 'tv' else (False,)):
        (pf, eta), (pu, _) = _mk_prox(prox_kind), _mk_prox(prox_kind)
        ef = SarahEngine(batch, pf, eta, T2, MB, seed=4, fused=True)
        eu = SarahEngine(batch, pu, eta, T2, MB, seed=4)
        assert ef.fused and not eu.fused
        idx = batch.draw_minibatches(steps, MB, seed=2) if host else None
        for s in range(steps):
            ef.step(None if idx is None else idx[s])
            eu.step(None if idx is None else idx[s])
        dz, bound = (ef.z - eu.z).abs().max().item(), 5e-5 * max(1.0, eu.z.abs().max().item())
        tf, tu = ef.psnr_trace(), eu.psnr_trace()
        print(f'[{prox_kind}, host={host}] |z_f - z_u| = {dz:.3e} (bound {bound:.3e}), PSNR {np.abs(tf - tu).max():.4f} dB')
        assert tf.shape == tu.shape == (steps + 3, B)
        assert dz <= bound
        assert np.abs(tf - tu).max() <= 0.01 + 1e-9
        assert prox_kind != 'tv' or ef.prox.t == eu.prox.t == steps + 3
        assert torch.equal(ef.w_prev, ef.z)
        assert (ef.v_prev - eu.v_prev).abs().max().item() <= 5e-5 * max(1.0, eu.v_prev.abs().max().item())


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
def test_per_problem_values_equal_scalar_engines(lr_decay):
    """1 item x 3 trials on a tiled batch with per-problem eta, mini_batch_size and sigma_modifier under fused=True == three scalar
    fused engines, bit for bit on z and on every log row; with lr_decay the outer coefficient does not decay, the inner one does."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    T2, steps = 3, 7
    one = CsmriBatch.synthetic(1, 256, 256, 0.2, 20.0, seed=19)
    eta, mb, sm = np.array([1.5e3, 2e3, 2.5e3]), np.array([800, 1000, 1300], np.int32), np.array([0.9, 1.1, 1.4])
    e = SarahEngine(one.tile(3), TVProx(sigma_modifier=sm), eta, T2, mb, lr_decay=lr_decay, seed=6, draw_id=[0, 0, 0], fused=True)
    for _ in range(steps):
        e.step()
    rows = steps + 3
    assert e.n_prox == rows
    for k in range(3):
        r = SarahEngine(one, TVProx(sigma_modifier=float(sm[k])), float(eta[k]), T2, int(mb[k]), lr_decay=lr_decay, seed=6, fused=True)
        for _ in range(steps):
            r.step()
        assert torch.equal(e.z[k], r.z[0]) and torch.equal(e.v_prev[k], r.v_prev[0]) and torch.equal(e.w_next[k], r.w_next[0]), k
        assert torch.equal(e.sse_log[:rows, k], r.sse_log[:rows, 0]), k
    assert not torch.equal(e.z[0], e.z[1])


def test_hipgraph_form():
    """capture() + run_outer(2) == 2 * T2 eager fused steps, bit for bit; capture() leaves the state untouched; no graph for the
    streaming path or a decaying step size."""
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    T2 = 4
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=13)
    mk = lambda **kw: SarahEngine(batch, TVProx(sigma_modifier=1.1), 2e3, T2, MB, seed=4, **kw)      # noqa: E731
    g, e = mk(fused=True), mk(fused=True)
    assert g.graph_ok()
    g.step(), e.step()                                           # (state that is not the initial one: garbage would show)
    for _ in range(T2 - 1):
        g.step(), e.step()
    keep = [t.clone() for t in (g.z, g.w_prev, g.w_next, g.v_prev, g.sse_log)]
    g.capture()
    assert all(torch.equal(a, b) for a, b in zip(keep, (g.z, g.w_prev, g.w_next, g.v_prev, g.sse_log)))
    assert (g.s, g.n_prox, g.prox.t) == (T2, T2 + 1, T2 + 1)
    g.run_outer(2)
    for _ in range(2 * T2):
        e.step()
    assert (g.s, g.n_prox, g.prox.t) == (e.s, e.n_prox, e.prox.t) == (3 * T2, 3 * T2 + 3, 3 * T2 + 3)
    assert torch.equal(g.z, e.z) and torch.equal(g.v_prev, e.v_prev) and torch.equal(g.w_prev, e.w_prev)
    assert np.array_equal(g.psnr_trace(), e.psnr_trace())
    for bad in (mk(), mk(fused=True, lr_decay=0.9)):
        assert not bad.graph_ok()
        with pytest.raises(ValueError, match='hipGraph'):
            bad.capture()


def test_fused_engine_against_the_oracle_loop():
    """One problem, host-drawn minibatches, T2 = 3, two outer iterations, against oracle.loops.pnp_sarah fed the same minibatches:
    every PSNR within 0.01 dB, |z - z_ref| <= 1e-3 (the bounds of test_one_kernel_iteration_engine_vs_reference_trace)."""
    import problems as P
    from oracle import denoise as od, loops as ol, problems as op
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    img, T2, steps, eta = os.path.join(GOLDEN, 'synth256.png'), 3, 6, 2e3
    np.random.seed(0)
    p = P.CSMRI(img, H=256, W=256, sample_prob=0.2, snr=20., upload=False)
    np.random.seed(1)
    idx = np.stack([np.flatnonzero(p.select_mb(MB)) for _ in range(steps)]).astype(np.int32)
    eng = SarahEngine(CsmriBatch.from_problems([p]), TVProx(), eta, T2, MB, fused=True)
    idx_d = torch.from_numpy(idx[:, None, :]).cuda()
    for s in range(steps):
        eng.step(idx_d[s])
    tr = eng.psnr_trace()[:, 0]
    np.random.seed(0)
    po = op.CSMRI(img, H=256, W=256, sample_prob=0.2, snr=20.)
    masks = []
    for s in range(steps):
        m = np.zeros(256 * 256, int)
        m[idx[s]] = 1
        masks.append(m.reshape(256, 256))
    it = iter(masks)
    po.select_mb = lambda size: next(it)
    o, j = (steps - 1) // T2, (steps - 1) % T2
    ro = ol.pnp_sarah(po, od.TVDenoiser(), eta, 1 + o * (5 + 5 * T2) + 5 + 5 * j + 1, T2, MB, converge_check=False, clock=ol.CountingClock())
    ref = np.array(ro['psnr_per_iter'])
    assert len(ref) == len(tr) == steps + 2
    print(f'PSNR vs oracle: {np.abs(tr - ref).max():.4f} dB; |z - z_ref| = {np.abs(eng.z[0].double().cpu().numpy().ravel() - ro["z"]).max():.3e}')
    assert np.abs(tr - ref).max() <= 0.01 + 1e-9
    assert np.abs(eng.z[0].double().cpu().numpy().ravel() - ro['z']).max() <= 1e-3


def test_sweep_runner_option():
    """make_runner(sarah_fused=True, sarah_trials=True) on 2 items x 2 trials against the same runner without it: the same row keys,
    psnr_final within 0.01 dB -- through run(items) and through run_trials."""
    from pnp_svrg_amd import sweep
    rng = np.random.default_rng(3)
    imgs = [np.cumsum(np.cumsum(rng.standard_normal((256, 256)), 0), 1) for _ in range(2)]
    items = [{'id': 0, 'image': 0, 'alpha': 0.2, 'snr': 20.0, 'seed': 0}, {'id': 1, 'image': 1, 'alpha': 0.3, 'snr': 20.0, 'seed': 1}]
    trials = [{'eta': 1.5e3}, {'eta': 2e3, 'mini_batch_size': 800, 'sigma_modifier': 1.2}]
    res = {}
    for fused in (True, False):
        run = sweep.make_runner(imgs, problem='csmri', algorithm='sarah', denoiser='tv', eta=2e3, n_inner=8, mini_batch_size=MB, T2=4,
                                seeding='counter', sarah_trials=True, sarah_fused=fused)
        res[fused] = (run(items), run.run_trials(run.prepare_data(items), trials))
    for rf, ru in zip([res[True][0]] + res[True][1], [res[False][0]] + res[False][1]):
        assert len(rf) == len(ru) == 2
        for a, b in zip(rf, ru):
            assert a.keys() == b.keys() and a['id'] == b['id']
            assert abs(a['psnr_final'] - b['psnr_final']) <= 0.01 + 1e-9, (a['psnr_final'], b['psnr_final'])
