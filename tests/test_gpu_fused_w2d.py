"""The 2-D wavelet BayesShrink prox inside the one-kernel CSMRI iteration (`denoise = 2` of the step entry points,
pnp_csmri_svrg_outer_iteration_prox, TVProx(multi=False, in_kernel=True); csrc/csmri_fused_w2d.h).

Every case is 256 x 256 f32 (the kernel has no other shape) with B <= 3 and at most 10 steps.  The in-kernel prox computes the
coefficients of pnp_prox_wavelet2d bit for bit and differs from it only in the order of the 15 sub-band sums, so it is held to the
float64 restatement (tests/wavelet2d_ref.py) with that kernel's tolerance -- 2e-5 absolute, sse rtol 1e-4 -- to the stand-alone
kernel itself within that kernel's own distance from the restatement, and bit for bit where every sum is exact (a constant image).
Loops: the project's f32 loop tolerances, +-0.01 dB and 5e-4.  The one-launch and per-problem forms: bit for bit."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

import wavelet2d_ref as wr
from oracle import loops as ol
from test_gpu_kernel_edges import tol_img

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
IMG256 = os.path.join(GOLDEN, 'synth256.png')
B = 3


def _f64(n):
    return torch.zeros(n, dtype=torch.float64, device='cuda')


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope='module')
def env():
    """One synthetic batch of three problems and three noisy images of the wavelet fixture (its 256 x 256 image as it is and with
    white noise of two strengths), with the noise estimate of the denoise = 0 call and the float64 restatement fed that estimate."""
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.engine import CsmriBatch
    ops.require_gpu()
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=41)
    z0 = wr.load_fixture()['h256w256_z0']
    rng = np.random.default_rng(7)
    imgs = np.stack([z0, z0 + 0.03 * rng.standard_normal(z0.shape), z0 + 0.08 * rng.standard_normal(z0.shape)]).astype(np.float32)
    img = torch.from_numpy(imgs).cuda().contiguous()
    sig0 = torch.zeros(B, device='cuda')
    stepped = batch.plan.svrg_step(batch.xinit, batch.xrec, batch.bits, alpha=0.0, beta=1.0, c1=img, denoise=0, sigma_out=sig0)[0]
    assert torch.equal(stepped, img)                            # alpha = 0: the prox input is exactly c1
    s = sig0.cpu().numpy().astype(np.float64)
    assert (s > 0).all()
    return dict(ops=ops, batch=batch, p=batch.plan, img=img, imgs=imgs.astype(np.float64), sig0=sig0, s=s)


def _prox_only(e, img, **kw):
    b = e['batch']
    sse, sig = _f64(img.shape[0]), torch.zeros(img.shape[0], device='cuda')
    out = e['p'].svrg_step(b.xinit, b.xrec, b.bits, alpha=0.0, beta=1.0, c1=img, denoise=2, xrec=b.xrec, sse=sse, sigma_out=sig, **kw)[0]
    return out, sse, sig


# ------------------------------------------------------------------------------------------------------------ 1: the prox alone
@pytest.mark.parametrize('mod', [1.0, 1.7])
def test_prox_alone_through_the_step_kernel(env, mod):
    e = env
    out, sse, sig = _prox_only(e, e['img'], sigma_modifier=mod)
    assert torch.equal(sig, e['sig0'])                          # the noise estimate of the denoise = 0 call, bit for bit
    ref = np.stack([wr.prox(x, s, sigma_modifier=mod) for x, s in zip(e['imgs'], e['s'])])
    got = out.double().cpu().numpy()
    err = np.abs(got - ref).max()
    alone = e['ops'].prox_wavelet2d(e['img'], sigma_in=e['sig0'], sigma_modifier=mod)[0]
    d_alone = (out - alone).abs().max().item()
    own = np.abs(alone.double().cpu().numpy() - ref).max()
    print(f'mod {mod}: in-kernel vs float64 {err:.3e} (bound {tol_img(F32, ref):.1e}); vs pnp_prox_wavelet2d {d_alone:.3e}; '
          f'pnp_prox_wavelet2d vs float64 {own:.3e}')
    assert not torch.equal(out, e['img'])
    assert err <= tol_img(F32, ref)
    xr = e['batch'].xrec.double().cpu().numpy()
    np.testing.assert_allclose(sse.cpu().numpy(), ((xr - ref) ** 2).reshape(B, -1).sum(1), rtol=1e-4)
    assert d_alone <= own


# ------------------------------------------------------------------------------------------------------------ 2: exact zeros
def test_constant_images_equal_the_stand_alone_kernel_bit_for_bit(env):
    """Constant images: every band sum is exactly 0 in both kernels, so the thresholds and with them the results are the stand-alone
    kernel's bit for bit, NaN positions included.  The noise estimate of a constant image is no signal: NaN where every db2 detail
    coefficient is an exact zero (skimage masks zeros: the median of nothing), else the rounding residue of the filter, ~1e-8 -- not
    the exact 0 one might expect.  Where it is not > 0 the fallback strength holds, which is the sigma_in = 0 call."""
    e = env
    img = torch.empty((B, 256, 256), device='cuda')
    for k, v in enumerate((0.5, 0.0, -1.25)):
        img[k] = v
    for fb in (0.07, 1e-3):
        out, _, sig = _prox_only(e, img, fallback_sigma=fb)
        s = sig.cpu().numpy()
        print('constant images: noise estimates', s)
        assert not (s > 1e-6).any() and not (s > 0).all()
        want = e['ops'].prox_wavelet2d(img, sigma_in=sig, fallback_sigma=fb)[0]
        assert np.array_equal(out.cpu().numpy(), want.cpu().numpy(), equal_nan=True)
        zero = e['ops'].prox_wavelet2d(img, sigma_in=torch.zeros(B, device='cuda'), fallback_sigma=fb)[0]
        for k in np.flatnonzero(~(s > 0)):
            assert np.array_equal(out[k].cpu().numpy(), zero[k].cpu().numpy(), equal_nan=True), k


# ------------------------------------------------------------------------------------------------------------ 3: batch independence
def test_problem_of_a_batch_equals_the_problem_alone(env):
    """A whole step (alpha != 0) with the in-kernel prox: problem b of the B = 3 call == the B = 1 call on it, and run to run."""
    from pnp_svrg_amd import ops
    e = env
    b = e['batch']
    kw = dict(alpha=-2e3 / 1000, beta=1.0, gamma=-0.5, denoise=2, sigma_modifier=1.3)
    sse, sig = _f64(B), torch.zeros(B, device='cuda')
    out = e['p'].svrg_step(e['img'], b.xinit, b.bits, c1=e['img'], c2=b.xrec, xrec=b.xrec, sse=sse, sigma_out=sig, **kw)[0]
    sse2, sig2 = _f64(B), torch.zeros(B, device='cuda')
    again = e['p'].svrg_step(e['img'], b.xinit, b.bits, c1=e['img'], c2=b.xrec, xrec=b.xrec, sse=sse2, sigma_out=sig2, **kw)[0]
    assert torch.equal(out, again) and torch.equal(sse, sse2) and torch.equal(sig, sig2)
    p1 = ops.CsmriPlan(256, 256, 1)
    for k in range(B):
        one = lambda t: t[k:k + 1].contiguous()
        s1, g1 = _f64(1), torch.zeros(1, device='cuda')
        o1 = p1.svrg_step(one(e['img']), one(b.xinit), one(b.bits), c1=one(e['img']), c2=one(b.xrec), xrec=one(b.xrec), sse=s1,
                          sigma_out=g1, **kw)[0]
        assert torch.equal(o1[0], out[k]) and torch.equal(s1[0], sse[k]) and torch.equal(g1[0], sig[k]), k
    assert not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------------------ 4: SvrgEngine
def _csmri(dtype):
    import problems
    np.random.seed(0)
    return problems.CSMRI(IMG256, H=256, W=256, sample_prob=0.2, snr=20., dtype=dtype)


def _inner_rows(ps, T2):
    return np.array([v for i, v in enumerate(np.asarray(ps)[1:]) if i % (T2 + 1) != 0])


@pytest.fixture(scope='module')
def loop():
    """The set-up of test_fused_engine_runs_the_2d_prox_after_the_gradient_kernel: one problem twice, host-drawn minibatches."""
    from pnp_svrg_amd.engine import CsmriBatch
    T2, mb, eta, steps = 5, 1000, 2e3, 10
    p = _csmri(F32)
    np.random.seed(1)
    idx = np.stack([np.flatnonzero(p.select_mb(mb)) for _ in range(steps)]).astype(np.int32)
    idx_d = torch.from_numpy(np.repeat(idx[:, None, :], 2, axis=1)).cuda()
    return dict(T2=T2, mb=mb, eta=eta, steps=steps, idx=idx, idx_d=idx_d, batch=CsmriBatch.from_problems([p, p]))


def _close(a, b):
    assert np.abs(a[0] - b[0]).max() <= 0.01 + 1e-9, np.abs(a[0] - b[0]).max()
    assert np.abs(a[1] - b[1]).max() <= 5e-4, np.abs(a[1] - b[1]).max()


@pytest.mark.parametrize('kw', [dict(), dict(denoise_strength=0.05, decay=0.9, sigma_modifier=1.2)], ids=['plain', 'strength'])
def test_svrg_engine_in_kernel_against_the_other_forms(loop, kw):
    import algorithms as A
    import denoisers as D
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    L = loop
    T2, mb, eta, steps = L['T2'], L['mb'], L['eta'], L['steps']
    runs = {}
    for name, fused, pkw in (('in_kernel', True, dict(in_kernel=True)), ('two_launch', True, {}), ('streaming', False, {})):
        eng = SvrgEngine(L['batch'], TVProx(multi=False, **pkw, **kw), eta, T2, mb, variant='svrg', fused=fused)
        assert eng.fused == fused
        for s in range(steps):
            eng.step(L['idx_d'][s])
        assert eng.prox.t == steps
        runs[name] = (eng.psnr_trace(), eng.z.double().cpu().numpy())
    tr = runs['in_kernel'][0]
    assert np.array_equal(tr[:, 0], tr[:, 1]) and np.array_equal(runs['in_kernel'][1][0], runs['in_kernel'][1][1])
    _close(runs['in_kernel'], runs['two_launch'])
    _close(runs['in_kernel'], runs['streaming'])
    p64 = _csmri(F64)
    it = iter(L['idx'])

    def select_mb(size):
        m = np.zeros(256 * 256, int)
        m[next(it)] = 1
        return m.reshape(256, 256)
    p64.select_mb = select_mb
    r = A.pnp_svrg(p64, D.TVDenoiser(multi=False, dtype=F64, **kw), eta, 2 + 3 * 2 + 5 * steps - 1, T2, mb, verbose=False,
                   converge_check=False, clock=ol.CountingClock(), variant='svrg')
    inner = _inner_rows(r['psnr_per_iter'], T2)
    assert len(inner) == steps
    print('in-kernel vs float64 loop: psnr', np.abs(inner - tr[:, 0]).max(), 'z', np.abs(r['z'] - runs['in_kernel'][1][0].ravel()).max())
    assert np.abs(inner - tr[:, 0]).max() <= 0.01 + 1e-9
    assert np.abs(r['z'] - runs['in_kernel'][1][0].ravel()).max() <= 5e-4


# ------------------------------------------------------------------------------------------------------------ 5: one launch
def test_one_launch_outer_iteration_equals_eager_steps(loop):
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    L = loop
    T2 = L['T2']
    mk = lambda: SvrgEngine(L['batch'], TVProx(multi=False, in_kernel=True), L['eta'], T2, L['mb'], variant='svrg', fused=True, seed=3)
    e1 = mk()
    for _ in range(2 * T2):
        e1.step()
    e2 = mk()
    assert e2.outer_kernel_ok()
    e2.run_outer(2, one_launch=True)
    assert e2.s == e1.s == 2 * T2 and e2.prox.t == e1.prox.t == 2 * T2
    assert torch.equal(e1.z, e2.z) and np.array_equal(e1.psnr_trace(), e2.psnr_trace())
    assert torch.equal(e1.w, e2.w) and torch.equal(e1.mu, e2.mu)
    # not the per-column prox
    e3 = SvrgEngine(L['batch'], TVProx(), L['eta'], T2, L['mb'], variant='svrg', fused=True, seed=3)
    e3.run_outer(2, one_launch=True)
    assert not torch.equal(e3.z, e2.z)


def test_outer_iteration_prox_with_denoise_1_is_the_pp_entry_point(env):
    from pnp_svrg_amd import _native as N
    from pnp_svrg_amd.ops import _p, _stream
    e = env
    b, T2, lr, mb = e['batch'], 3, 2e3, 1000
    mbs = b.minibatches(T2)
    b.draw(mbs, mb, 11, 0, T2)
    sm = _dev([1.0, 1.3, 0.8])
    outs = []
    for name, tail in (('pnp_csmri_svrg_outer_iteration_pp', ()), ('pnp_csmri_svrg_outer_iteration_prox', (1,))):
        z, w, mu = b.xinit.clone(), torch.zeros_like(b.xinit), torch.zeros_like(b.xinit)
        log, sig = torch.zeros((4, B), dtype=torch.float64, device='cuda'), torch.zeros(B, device='cuda')
        N.call(name, b.plan._h, _p(z), _p(w), _p(mu), _p(b.bits), _p(b.yh_full), _p(b.inv_m0), _p(mbs.selbits), T2, lr, None, mb, None,
               1.0, _p(sm), 0.0, _p(b.xrec), _p(log), 1, 4, _p(sig), *tail, _stream())
        outs.append((z, w, mu, log, sig))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert not torch.equal(outs[0][0], b.xinit)


# ------------------------------------------------------------------------------------------------------------ 6: per problem
@pytest.mark.parametrize('mode', ['step', 'outer'])
def test_per_problem_eta_and_sigma_modifier(loop, mode):
    """Problem b of a batch with per-problem eta and sigma_modifier == the scalar run made with its values, bit for bit."""
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    L = loop
    T2 = L['T2']
    eta, sm = np.array([2e3, 1234.5]), np.array([1.0, 1.3])

    def run(eta_, sm_):
        eng = SvrgEngine(L['batch'], TVProx(multi=False, in_kernel=True, sigma_modifier=sm_), eta_, T2, L['mb'], variant='svrg', fused=True,
                         seed=5, draw_id=np.zeros(2, np.int64))
        if mode == 'outer':
            assert eng.outer_kernel_ok()
            eng.run_outer(1, one_launch=True)
        else:
            for _ in range(T2):
                eng.step()
        return eng.z.clone(), eng.psnr_trace()
    z, tr = run(eta, sm)
    for k in range(2):
        zr, trr = run(float(eta[k]), float(sm[k]))
        assert torch.equal(z[k], zr[k]) and np.array_equal(tr[:, k], trr[:, k]), k
    assert not torch.equal(z[0], z[1])


# ------------------------------------------------------------------------------------------------------------ 7: the other loops
@pytest.mark.parametrize('algo', ['gd', 'sgd', 'saga', 'sarah'])
def test_other_engines_step_with_one_kernel(loop, algo):
    from pnp_svrg_amd.engine import TVProx, make_engine
    L = loop
    eta = L['eta'] * (1e-3 if algo == 'gd' else 1.0)
    def mk(multi_true=False, **pkw):
        prox = TVProx() if multi_true else TVProx(multi=False, **pkw)
        return make_engine(L['batch'], prox, eta, 3, L['mb'], algorithm=algo, hist_size=4, fused=True, seed=3)
    e_in, e_two = mk(in_kernel=True), mk()
    if algo == 'sarah':                                         # (no span form; its one-launch outer iteration holds the 1-D prox only)
        assert not e_in.outer_kernel_ok() and mk(multi_true=True).outer_kernel_ok()
    else:
        assert not e_in.span_kernel_ok()
    for _ in range(6):
        e_in.step()
        e_two.step()
    _close((e_in.psnr_trace(), e_in.z.double().cpu().numpy()), (e_two.psnr_trace(), e_two.z.double().cpu().numpy()))
    assert e_in.prox.t == e_two.prox.t
    if algo != 'sarah':                                         # run_span(4) == four steps, bit for bit (eager: no span kernel holds it)
        e_a, e_b = mk(in_kernel=True), mk(in_kernel=True)
        e_a.run_span(4)
        for _ in range(4):
            e_b.step()
        assert e_a.s == e_b.s == 4 and torch.equal(e_a.z, e_b.z) and np.array_equal(e_a.psnr_trace(), e_b.psnr_trace())


def test_per_problem_t2_and_hist_size_with_the_in_kernel_prox(loop):
    """Per-problem T2 steps eagerly (pnp_csmri_svrg_span_pp holds the per-column prox only); a per-problem hist_size is refused with
    a message that names in_kernel."""
    from pnp_svrg_amd.engine import SagaEngine, SvrgEngine, TVProx
    L = loop
    t2 = np.array([2, 3], np.int32)
    mk = lambda: SvrgEngine(L['batch'], TVProx(multi=False, in_kernel=True), L['eta'], t2, L['mb'], variant='svrg', fused=True, seed=3)
    e1, e2 = mk(), mk()
    e1.run_span(6)
    for _ in range(6):
        e2.step()
    assert torch.equal(e1.z, e2.z) and np.array_equal(e1.psnr_trace(), e2.psnr_trace())
    ref = SvrgEngine(L['batch'], TVProx(multi=False), L['eta'], t2, L['mb'], variant='svrg', fused=True, seed=3)
    for _ in range(6):
        ref.step()
    _close((e1.psnr_trace(), e1.z.double().cpu().numpy()), (ref.psnr_trace(), ref.z.double().cpu().numpy()))
    with pytest.raises(ValueError, match='in_kernel'):
        SagaEngine(L['batch'], TVProx(multi=False, in_kernel=True), L['eta'], L['mb'], hist_size=np.array([3, 4]), fused=True)


# ------------------------------------------------------------------------------------------------------------ 8: refusals
def test_multi_step_entry_points_refuse_denoise_2(env):
    """Plain argument checks: every call returns PNP_ERR_ARG before any device work."""
    from pnp_svrg_amd import _native as N
    from pnp_svrg_amd.ops import _p, _stream
    e = env
    b = e['batch']
    z, tsum = b.xinit.clone(), torch.zeros_like(b.xinit)
    table = torch.zeros((2, B, 256, 256), device='cuda')
    rows, prev = torch.zeros((1, B), dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.int32, device='cuda')
    sel = torch.zeros((1, B, 256, 8), dtype=torch.int32, device='cuda')
    log, sig, ih = torch.zeros((2, B), dtype=torch.float64, device='cuda'), torch.zeros(B, device='cuda'), _dev([0.5] * B)
    h = b.plan._h
    calls = {
        'pnp_csmri_grad_span': lambda d: (h, _p(z), _p(b.bits), _p(b.yh_full), None, -1.0, None, _p(b.inv_m0), 1.0, d, 1.0, None, 0.0,
                                          _p(b.xrec), 1, _p(log), 0, 2, _p(sig), _stream()),
        'pnp_csmri_saga_span': lambda d: (h, _p(z), _p(sel), _p(b.YT), 1e-3, None, None, _p(table), _p(rows), _p(prev), _p(tsum), 1.0,
                                          None, 0.5, 2, d, 1.0, None, 0.0, _p(b.xrec), 1, _p(log), 0, 2, _p(sig), _stream()),
        'pnp_csmri_saga_span_hist': lambda d: (h, _p(z), _p(sel), _p(b.YT), 1e-3, None, None, _p(table), _p(rows), _p(prev), _p(tsum),
                                               1.0, None, 0.5, _p(ih), 2, d, 1.0, None, 0.0, _p(b.xrec), 1, _p(log), 0, 2, _p(sig),
                                               _stream()),
        'pnp_csmri_saga_step_hist_pp': lambda d: (h, _p(z), _p(sel[0]), _p(b.YT), 1e-3, None, None, _p(table), _p(prev), _p(prev),
                                                  _p(tsum), 1.0, None, 0.5, _p(ih), 2, _p(z), d, 1.0, None, 0.0, _p(b.xrec), _p(log[0]),
                                                  _p(sig), _stream()),
    }
    before = z.clone()
    for name, args in calls.items():
        status = getattr(N.lib(), name)(*args(2))
        assert status != 0 and b'denoise' in N.lib().pnp_last_error(), name
        with pytest.raises(N.NativeError, match='denoise'):
            N.call(name, *args(2))
    torch.cuda.synchronize()
    assert torch.equal(z, before)
    with pytest.raises(N.NativeError, match='denoise'):
        N.call('pnp_csmri_svrg_outer_iteration_prox', h, _p(z), _p(tsum), _p(table[0]), _p(b.bits), _p(b.yh_full), _p(b.inv_m0), None, 1,
               1.0, None, 100, None, 1.0, None, 0.0, _p(b.xrec), _p(log), 0, 2, _p(sig), 0, _stream())


def test_in_kernel_needs_the_2d_prox():
    from pnp_svrg_amd.engine import TVProx
    with pytest.raises(ValueError, match='multi=False'):
        TVProx(multi=True, in_kernel=True)
    with pytest.raises(ValueError):
        TVProx(in_kernel=True)
