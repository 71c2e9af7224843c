"""GPU parity of the 2-D wavelet BayesShrink prox, TVDenoiser(multi=False) -> pnp_prox_wavelet2d: the kernel against the
real library's outputs (tests/golden/wavelet2d*.npz) and against the NumPy restatement of tests/wavelet2d_ref.py (which
tests/test_cpu_wavelet2d.py holds to the same fixture bit for bit), then every layer above it: denoiser class, drop-in
loops (eager and hipGraph), engines, sweep runner.

The kernel has ONE dispatch form (a workgroup per image at every batch size); the batch sizes below are those of
pnp_prox_tv's split (1, 32, 33), whose kernels make the noise estimate the 2-D prox must reproduce bit for bit.

Tolerances are the project's: f64 <= 1e-12 * max(1, max|ref|), f32 <= 2e-5 absolute on O(1) images, sse rtol
1e-10 / 1e-4; loops: f64 identical rounded PSNR traces and |z - z_ref| <= 1e-9, f32 +-0.01 dB and 5e-4.
"""
import os
import numpy as np
import pytest
import torch
from conftest import GOLDEN

import wavelet2d_ref as wr
from oracle import loops as ol
from test_gpu_kernel_edges import SHAPES, images, assert_close_nan, tol_img, tol_sigma, dev, host

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
IMG256 = os.path.join(GOLDEN, 'synth256.png')
IMG64 = os.path.join(GOLDEN, 'synth64.png')
FIXTURE_SHAPES = ((16, 16), (16, 48), (128, 32), (32, 256), (64, 80), (256, 112), (256, 256))
BATCHES = (1, 32, 33)


@pytest.fixture(scope='module')
def ops():
    from pnp_svrg_amd import ops as o
    o.require_gpu()
    return o


@pytest.fixture(scope='module')
def g():
    return wr.load_fixture()


# ----------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('H,W', FIXTURE_SHAPES)
def test_kernel_vs_reference_fixture(ops, g, H, W, dtype):
    """All three branches (estimate, sigma_modifier, fixed strength) at B = 1, 32, 33, out of place and in place."""
    tag = f'h{H}w{W}'
    z0, s0 = g[f'{tag}_z0'], float(g[f'{tag}_sigma_est'])
    for B in BATCHES:
        zt = dev(np.broadcast_to(z0, (B, H, W)), dtype)
        zeros = torch.zeros(B, dtype=dtype, device='cuda')
        for key, kw in (('w2d', {}), ('w2d_mod', dict(sigma_modifier=1.7)),
                        ('w2d_strength', dict(sigma_in=zeros, fallback_sigma=0.07 * 0.9))):
            ref = g[f'{tag}_{key}']
            out, _, sig = ops.prox_wavelet2d(zt, **kw)
            err = np.abs(host(out) - ref).max()
            print(f'{tag} {dtype} B={B} {key}: max err {err:.3e}')
            assert err <= tol_img(dtype, ref), (B, key)
            if 'sigma_in' not in kw:
                np.testing.assert_allclose(host(sig), s0, rtol=tol_sigma(dtype))
            zz = zt.clone()
            ops.prox_wavelet2d(zz, out=zz, **kw)                          # in place
            assert torch.equal(zz, out), (B, key)
            assert torch.equal(out, out[:1].expand_as(out))               # the same image at every index of the batch


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('H,W', SHAPES)
def test_kernel_vs_restatement_and_batch_independence(ops, H, W, dtype):
    """Distinct images per batch entry, per-image sigma_in with zeros (fallback), sigma_modifier, xrec / sse, sigma_out
    == ops.sigma_est bit for bit; image b of B = 33 == image b run alone, bit for bit."""
    Bmax = 33
    z = images(Bmax, H, W, seed=H * 1000 + W + 7)
    xr = np.clip(z, 0, 1)
    mod, fb = 1.3, 0.0625
    zt_all, xr_all = dev(z, dtype), dev(xr, dtype)
    s_dev = ops.sigma_est(zt_all)
    s_ref = host(s_dev)                                       # pinned to skimage by the existing sigma tests
    assert (s_ref > 0).all()
    est_ref = np.stack([wr.prox(x, s, sigma_modifier=mod) for x, s in zip(z, s_ref)])
    sig_in = 0.02 + 0.001 * np.arange(Bmax)
    sig_in[::4] = 0.0                                         # the sigma_est <= 0 fallback
    sig_in = sig_in.astype(np.float32).astype(np.float64)
    given_ref = np.stack([wr.prox(x, s, sigma_modifier=mod, fallback_sigma=fb) for x, s in zip(z, sig_in)])
    sig_all = dev(sig_in, dtype)
    ssr = 1e-10 if dtype == F64 else 1e-4
    alone = {}
    for B in BATCHES:
        zt, xrt = zt_all[:B].contiguous(), xr_all[:B].contiguous()
        out, sse, sig = ops.prox_wavelet2d(zt, sigma_modifier=mod, xrec=xrt)
        assert torch.equal(sig, ops.sigma_est(zt)) and torch.equal(sig, s_dev[:B])
        err = np.abs(host(out) - est_ref[:B]).max()
        print(f'{H}x{W} {dtype} B={B}: estimate branch max err {err:.3e}')
        assert err <= tol_img(dtype, est_ref)
        np.testing.assert_allclose(sse.cpu().numpy(), ((xr[:B] - est_ref[:B]) ** 2).reshape(B, -1).sum(1), rtol=ssr)
        gv, gsse, gsig = ops.prox_wavelet2d(zt, sigma_in=sig_all[:B].contiguous(), sigma_modifier=mod, fallback_sigma=fb, xrec=xrt)
        err = np.abs(host(gv) - given_ref[:B]).max()
        print(f'{H}x{W} {dtype} B={B}: sigma_in branch max err {err:.3e}')
        assert err <= tol_img(dtype, given_ref)
        assert torch.equal(gsig, sig_all[:B])
        zz = zt.clone()
        _, sse2, _ = ops.prox_wavelet2d(zz, sigma_modifier=mod, xrec=xrt, out=zz)
        assert torch.equal(zz, out) and torch.equal(sse2, sse)
        if B == 1:
            alone[0] = (out, sig, sse, gv, gsse)
            o = ops.prox_wavelet2d(zt_all[32:].contiguous(), sigma_modifier=mod, xrec=xr_all[32:].contiguous())
            q = ops.prox_wavelet2d(zt_all[32:].contiguous(), sigma_in=sig_all[32:].contiguous(), sigma_modifier=mod,
                                   fallback_sigma=fb, xrec=xr_all[32:].contiguous())
            alone[32] = (o[0], o[2], o[1], q[0], q[1])
        if B == 33:
            for b, (o1, s1, e1, g1, ge1) in alone.items():
                assert torch.equal(out[b], o1[0]) and torch.equal(sig[b], s1[0]) and torch.equal(sse[b], e1[0])
                assert torch.equal(gv[b], g1[0]) and torch.equal(gsse[b], ge1[0])


@pytest.mark.parametrize('dtype', [F64, F32])
def test_nonfinite_pixels(ops, g, dtype):
    """A NaN, +inf or -inf pixel: NaN positions first, then infinities, then the finite values (fixture = real library)."""
    z, ref = g['nonfinite_z0'], g['nonfinite_w2d']
    for B in (3, 36):
        reps = B // 3
        zt = dev(np.tile(z, (reps, 1, 1)), dtype)
        out, _, sig = ops.prox_wavelet2d(zt, fallback_sigma=0.05)
        assert np.array_equal(host(sig), host(ops.sigma_est(zt)), equal_nan=True)
        assert np.array_equal(np.isnan(host(sig))[:3], np.isnan(g['nonfinite_sigma_est']))
        o = host(out)
        for k in range(B):
            assert_close_nan(o[k], ref[k % 3], tol_img(dtype, ref[np.isfinite(ref)]))


def test_multi_true_path_is_untouched(ops):
    import denoisers
    z = dev(images(3, 64, 64, seed=5), F32)
    s = ops.sigma_est(z)
    a, _, _ = denoisers.TVDenoiser(sigma_modifier=1.2).denoise_device(z, sigma_est=s)
    b, _, _ = ops.prox_tv(z, sigma_in=s, sigma_modifier=1.2)
    assert torch.equal(a, b)
    c, _, _ = denoisers.TVDenoiser(multi=False, sigma_modifier=1.2).denoise_device(z, sigma_est=s)
    assert torch.equal(c, ops.prox_wavelet2d(z, sigma_in=s, sigma_modifier=1.2)[0]) and not torch.equal(a, c)


def test_denoiser_class_vs_fixture(g):
    """The public class on NumPy input, as the reference is called: estimate branch, modifier, decaying fixed strength."""
    import denoisers
    for tag in ('h64w80', 'h256w112'):
        z0, s = g[f'{tag}_z0'], float(g[f'{tag}_sigma_est'])
        for key, kw, se in (('w2d', {}, s), ('w2d_mod', dict(sigma_modifier=1.7), s),
                            ('w2d_strength', dict(denoise_strength=0.07, decay=0.9), 0)):
            d = denoisers.TVDenoiser(multi=False, dtype=F64, **kw)
            out = d.denoise(noisy=z0, sigma_est=se)
            assert d.t == 1 and out.dtype == np.float64
            assert np.abs(out - g[f'{tag}_{key}']).max() <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- loops
def _csmri(n, dtype):
    import problems
    np.random.seed(0)
    return problems.CSMRI(IMG64 if n == 64 else IMG256, H=n, W=n, sample_prob=0.2, snr=20., dtype=dtype)


def _check(r, g, name, dtype):
    ps, ref = np.array(r['psnr_per_iter']), g[f'{name}_psnr']
    assert len(ps) == len(ref)
    print(name, dtype, 'max |psnr - ref|', np.abs(ps - ref).max(), 'max |z - ref|', np.abs(r['z'] - g[f'{name}_z']).max())
    if dtype == F64:
        assert list(ps) == list(ref)
        np.testing.assert_allclose(r['z'], g[f'{name}_z'], rtol=0, atol=1e-9)
    else:
        assert np.abs(ps - ref).max() <= 0.01 + 1e-9
        np.testing.assert_allclose(r['z'], g[f'{name}_z'], rtol=0, atol=5e-4)


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('name', ['svrg64', 'saga64'])
def test_dropin_loops_64(g, name, dtype):
    import algorithms as A
    import denoisers as D
    p = _csmri(64, dtype)
    d = D.TVDenoiser(multi=False, dtype=dtype)
    np.random.seed(1)
    if name == 'svrg64':
        r = A.pnp_svrg(p, d, 5e2, 60, 4, 200, verbose=False, converge_check=False, clock=ol.CountingClock())
    else:
        r = A.pnp_saga(p, d, 5e2, 53, 200, hist_size=5, verbose=False, converge_check=False, clock=ol.CountingClock())
    _check(r, g, name, dtype)


@pytest.mark.parametrize('graph', [None, False])
def test_dropin_svrg_256_f32_with_and_without_graph(g, graph):
    import algorithms as A
    import denoisers as D
    p = _csmri(256, F32)
    np.random.seed(1)
    r = A.pnp_svrg(p, D.TVDenoiser(multi=False), 2e3, 2 + 4 * 53, 10, 1000, verbose=False, converge_check=False,
                   clock=ol.CountingClock(), graph=graph)
    _check(r, g, 'svrg256', F32)


# ----------------------------------------------------------------------------------------------------------------- engines
def _inner_rows(ps, T2):
    """psnr_per_iter of pnp_svrg (1 initial entry, then per outer iteration 1 entry + up to T2 inner entries) -> the
    entries that follow a prox evaluation, i.e. the rows of SvrgEngine.psnr_trace()."""
    return np.array([v for i, v in enumerate(np.asarray(ps)[1:]) if i % (T2 + 1) != 0])


def test_svrg_engine_streaming_f64_vs_fixture(g):
    """SvrgEngine (reference semantics, streaming kernels, f64) with TVProx(multi=False) on the fixture's problem with the
    fixture's minibatches (legacy stream, seed 1): the reference's own rounded PSNR trace and iterate."""
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    T2, mb = 4, 200
    ref = _inner_rows(g['svrg64_psnr'], T2)
    p = _csmri(64, F64)
    np.random.seed(1)
    idx = np.stack([np.flatnonzero(p.select_mb(mb)) for _ in range(len(ref))]).astype(np.int32)
    batch = CsmriBatch.from_problems([p, p], dtype=F64)
    eng = SvrgEngine(batch, TVProx(multi=False), 5e2, T2, mb, variant='reference')
    idx_d = torch.from_numpy(np.repeat(idx[:, None, :], 2, axis=1)).cuda()
    for s in range(len(ref)):
        eng.step(idx_d[s])
    tr = eng.psnr_trace()
    assert np.array_equal(tr[:, 0], tr[:, 1]) and list(tr[:, 0]) == list(ref)
    z = eng.z.cpu().numpy().reshape(2, -1)
    assert np.array_equal(z[0], z[1]) and np.abs(z[0] - g['svrg64_z']).max() <= 1e-9


def test_saga_engine_f64_vs_fixture(g):
    """SagaEngine with TVProx(multi=False) fed the legacy stream's minibatches and replaced rows (algorithms/pnp_saga.py:
    one select_mb for the table, then select_mb + np.random.choice(hist_size, 1) per iteration): the fixture's trace."""
    from pnp_svrg_amd.engine import CsmriBatch, TVProx, make_engine
    mb, hist = 200, 5
    ref = g['saga64_psnr'][1:]
    p = _csmri(64, F64)
    np.random.seed(1)
    idx0 = np.flatnonzero(p.select_mb(mb)).astype(np.int32)
    idx, rs = [], []
    for _ in range(len(ref)):
        idx.append(np.flatnonzero(p.select_mb(mb)).astype(np.int32))
        rs.append(np.random.choice(hist, 1).item())
    batch = CsmriBatch.from_problems([p], dtype=F64)
    eng = make_engine(batch, TVProx(multi=False), 5e2, 4, mb, algorithm='saga', hist_size=hist,
                      idx0=torch.from_numpy(idx0[None]).cuda())
    for s in range(len(ref)):
        eng.step(torch.from_numpy(idx[s][None]).cuda(), r=rs[s])
    assert list(eng.psnr_trace()[:, 0]) == list(ref)
    assert np.abs(eng.z.cpu().numpy().ravel() - g['saga64_z']).max() <= 1e-9


def test_gd_engine_f64_vs_dropin_loop():
    import algorithms as A
    import denoisers as D
    from pnp_svrg_amd.engine import CsmriBatch, TVProx, make_engine
    steps = 8
    p = _csmri(64, F64)
    batch = CsmriBatch.from_problems([p], dtype=F64)
    eng = make_engine(batch, TVProx(multi=False), 5e2, 4, 200, algorithm='gd')
    for _ in range(steps):
        eng.step()
    r = A.pnp_gd(p, D.TVDenoiser(multi=False, dtype=F64), 5e2, 6 * steps - 3, verbose=False, converge_check=False,
                 clock=ol.CountingClock())
    got = np.array(r['psnr_per_iter'])[1:]
    assert len(got) == steps and list(got) == list(eng.psnr_trace()[:, 0])
    np.testing.assert_allclose(r['z'], eng.z.cpu().numpy().ravel(), rtol=0, atol=1e-10)


def test_fused_engine_runs_the_2d_prox_after_the_gradient_kernel():
    """One-kernel iteration (f32, 256 x 256): the gradient kernel makes step + noise estimate, the 2-D prox follows with
    sigma_in (the DnCNNProx pattern).  Against the streaming engine and the f64 drop-in loop on the same minibatches:
    +-0.01 dB on every PSNR; the decaying fixed strength advances once per prox evaluation in both; whole outer
    iterations cannot run as one launch, run_outer replays the captured graph instead, bit for bit the eager steps."""
    import algorithms as A
    import denoisers as D
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    T2, mb, eta, steps = 5, 1000, 2e3, 10
    p = _csmri(256, F32)
    np.random.seed(1)
    idx = np.stack([np.flatnonzero(p.select_mb(mb)) for _ in range(steps)]).astype(np.int32)
    idx_d = torch.from_numpy(np.repeat(idx[:, None, :], 2, axis=1)).cuda()
    batch = CsmriBatch.from_problems([p, p])
    for kw in (dict(), dict(denoise_strength=0.05, decay=0.9, sigma_modifier=1.2)):
        traces = []
        for fused in (True, False):
            eng = SvrgEngine(batch, TVProx(multi=False, **kw), eta, T2, mb, variant='svrg', fused=fused)
            assert eng.fused == fused and not eng.outer_kernel_ok()
            for s in range(steps):
                eng.step(idx_d[s])
            assert eng.prox.t == steps
            traces.append((eng.psnr_trace(), eng.z.double().cpu().numpy()))
        assert np.array_equal(traces[0][0][:, 0], traces[0][0][:, 1])
        assert np.abs(traces[0][0] - traces[1][0]).max() <= 0.01 + 1e-9
        assert np.abs(traces[0][1] - traces[1][1]).max() <= 5e-4
    p64 = _csmri(256, F64)
    it = iter(idx)

    def select_mb(size):
        m = np.zeros(256 * 256, int)
        m[next(it)] = 1
        return m.reshape(256, 256)
    p64.select_mb = select_mb
    r = A.pnp_svrg(p64, D.TVDenoiser(multi=False, denoise_strength=0.05, decay=0.9, sigma_modifier=1.2, dtype=F64), eta,
                   2 + 3 * 2 + 5 * steps - 1, T2, mb, verbose=False, converge_check=False, clock=ol.CountingClock(), variant='svrg')
    inner = _inner_rows(r['psnr_per_iter'], T2)
    assert len(inner) == steps
    assert np.abs(inner - traces[0][0][:, 0]).max() <= 0.01 + 1e-9
    assert np.abs(r['z'] - traces[0][1][0].ravel()).max() <= 5e-4
    # device-drawn minibatches: eager steps == replays of the captured outer iteration
    e1 = SvrgEngine(batch, TVProx(multi=False), eta, T2, mb, variant='svrg', fused=True, seed=3)
    for _ in range(2 * T2):
        e1.step()
    e2 = SvrgEngine(batch, TVProx(multi=False), eta, T2, mb, variant='svrg', fused=True, seed=3)
    assert not e2.outer_kernel_ok() and e2.graph_ok()
    e2.run_outer(2)
    assert e2.s == e1.s == 2 * T2 and e2.prox.t == e1.prox.t
    assert torch.equal(e1.z, e2.z) and np.array_equal(e1.psnr_trace(), e2.psnr_trace())


def test_graph_replay_equals_eager():
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    B, n, mb, T2 = 2, 64, 100, 5
    batch = CsmriBatch.synthetic(B, n, n, 0.2, 20.0, seed=5)
    e1 = SvrgEngine(batch, TVProx(multi=False), 5e2, T2, mb, seed=3)
    for _ in range(3 * T2):
        e1.step()
    e2 = SvrgEngine(batch, TVProx(multi=False), 5e2, T2, mb, seed=3)
    assert e2.graph_ok() and not e2.outer_kernel_ok()
    e2.capture()
    assert e2.s == 0 and torch.equal(e2.z, batch.xinit)
    e2.run_outer(3)
    assert e2.s == e1.s == 15
    assert torch.equal(e1.z, e2.z) and np.array_equal(e1.psnr_trace(), e2.psnr_trace())
    assert not SvrgEngine(batch, TVProx(multi=False, denoise_strength=0.1), 5e2, T2, mb).graph_ok()


# ----------------------------------------------------------------------------------------------------------------- sweep
def test_sweep_cell_vs_restatement_through_the_oracle_loop():
    """One cell of the sweep (CSMRI x svrg x 'tv' with multi=False, legacy seeding, 2 images x 2 ratios at 64 x 64, f64)
    against oracle.loops.pnp_svrg with the restatement as a foreign denoiser object: identical rounded traces."""
    from oracle import problems as op
    from pnp_svrg_amd import sweep
    rng = np.random.default_rng(0)
    imgs = []
    for _ in range(2):
        x = rng.random((64, 64))
        q = np.pad(x, 2, mode='wrap')
        imgs.append(sum(q[i:i + 64, j:j + 64] for i in range(5) for j in range(5)) / 25.0)
    T2, mb, n_inner, eta = 4, 150, 10, 5e2
    items = sweep.make_items(2, [0.2, 0.4], [20.0])
    runner = sweep.make_runner(imgs, 'csmri', 'svrg', denoiser='tv', denoiser_kwargs={'multi': False}, eta=eta, n_inner=n_inner,
                               mini_batch_size=mb, T2=T2, H=64, W=64, dtype=F64, seeding='legacy', keep_trace=True)
    res = sweep.run_sweep(items, runner)
    assert [r['id'] for r in res] == list(range(4))
    n_outer = -(-n_inner // T2)
    for r in res:
        it = r['item']
        np.random.seed(it['seed'])
        po = op.CSMRI(None, H=64, W=64, sample_prob=it['alpha'], snr=it['snr'], img=imgs[it['image']])
        assert po.M0 == r['M0']
        np.random.seed(1)
        ro = ol.pnp_svrg(po, wr.Wavelet2dDenoiser(), eta, 2 + 3 * n_outer + 5 * n_inner - 1, T2, mb, converge_check=False,
                         clock=ol.CountingClock(), variant='svrg')
        inner = _inner_rows(ro['psnr_per_iter'], T2)
        assert len(inner) == n_inner
        assert list(inner) == list(r['psnr_trace']), (it, inner, r['psnr_trace'])
        assert np.abs(r['z'].ravel() - ro['z']).max() <= 1e-9
