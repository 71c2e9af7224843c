"""GPU side of the device-side CSMRI problem generator: pnp_csmri_generate / CsmriPlan.generate / CsmriBatch.generate /
make_runner(seeding='device') against the NumPy restatement of the published stream (tests/csmri_generate_ref.py).

Tolerances are the project's: f64 <= 1e-12 * max(1, max|ref|); loops f64 |psnr diff| <= 0.01 + 1e-9 and |z diff| <= 1e-9,
f32 +-0.01 dB and 5e-4.  The f32 bound on Y and Xinit is measured against a yardstick: an independent complex64 pipeline
(torch.fft on the GPU) on the same f32 image, restated mask and restated noise; the kernels may err at most 4 x the
yardstick's maximum error per shape (a different radix factorisation and the Hermitian split are a few more roundings per
element)."""
import gc

import numpy as np
import pytest
import torch

import csmri_generate_ref as gr

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _free_plans():
    """Plans free their workspaces with hipFree when collected; collect here, so that none is left to be freed in the middle
    of a later test's hipGraph capture (which a free would invalidate)."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _images(n_img, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_img):
        x = rng.random((n, n))
        p = np.pad(x, 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def _items(n_img, alphas, snrs=(20.0,), seeds=(0,)):
    from pnp_svrg_amd import sweep
    return sweep.make_items(n_img, alphas, snrs, seeds)


def _ref(images, items, dtype=F64):
    """Restatement per item; for f32 the restatement sees the image as the device does (rounded to f32)."""
    out = []
    for it in items:
        x = gr.norm01(images[it['image']])
        if dtype == F32:
            x = x.astype(np.float32).astype(np.float64)
        out.append(dict(gr.generate(x, it), x=x))
    return out


def _gen(images, items, n, dtype):
    from pnp_svrg_amd.engine import CsmriBatch
    return CsmriBatch.generate(images, items, n, n, dtype)


def _Y(batch):
    return batch.YT.cpu().numpy().swapaxes(1, 2)


@pytest.mark.parametrize('dtype', [F64, F32])
@pytest.mark.parametrize('n', [64, 128, 256])
def test_mask_and_m0_exact(n, dtype):
    imgs = _images(2, n)
    items = _items(2, [0.1, 0.5, 1.0], seeds=(0, 2))
    b = _gen(imgs, items, n, dtype)
    masks = np.stack([gr.mask(it['seed'], it['id'], it['alpha'], n, n) for it in items])
    assert np.array_equal(b.M0, masks.reshape(len(items), -1).sum(1))
    assert np.array_equal(b.maskT.cpu().numpy(), masks.swapaxes(1, 2))
    assert np.array_equal(b.mask_np, masks) and b.mask_np.dtype == np.uint8            # lazily read back
    want_bits = b.plan.pack_mask(torch.from_numpy(np.ascontiguousarray(masks.swapaxes(1, 2))).cuda())
    assert torch.equal(b.bits, want_bits)
    assert items[4]['alpha'] == 1.0 and (masks[4] == 1).all() and b.M0[4] == n * n      # alpha = 1 samples every position
    inv = b.inv_m0.double().cpu().numpy()
    assert np.allclose(inv, 1.0 / b.M0, rtol=1e-6 if dtype == F32 else 1e-15)
    assert b.max_mb == b.M0.min()


@pytest.mark.parametrize('n', [64, 128, 256])
def test_f64_against_restatement(n):
    imgs = _images(2, n, seed=1)
    items = _items(2, [0.2, 0.5], snrs=(10.0, 30.0))
    b = _gen(imgs, items, n, F64)
    ref = _ref(imgs, items)
    Y, xi, sg, xr = _Y(b), b.xinit.cpu().numpy(), b.sigma.cpu().numpy(), b.xrec.cpu().numpy()
    for j, r in enumerate(ref):
        assert np.array_equal(xr[j], r['x'])
        tol = 1e-12 * max(1.0, np.abs(r['Y']).max())
        eY, eX, eS = np.abs(Y[j] - r['Y']).max(), np.abs(xi[j] - r['xinit']).max(), abs(sg[j] - r['sigma'])
        print(f'f64 n={n} item {j}: |Y| err {eY:.3e} (tol {tol:.3e}), Xinit err {eX:.3e}, sigma err {eS:.3e}')
        assert eY <= tol and eX <= 1e-12 and eS <= 1e-12 * max(1.0, r['sigma'])
        assert np.array_equal(Y[j][r['mask'] == 0], np.zeros((r['mask'] == 0).sum()))
    assert torch.equal(b.yh_full, b.plan.pack_y(b.YT, b.maskT))


@pytest.mark.parametrize('n', [64, 128, 256])
def test_f32_within_four_times_an_independent_f32_pipeline(n):
    imgs = _images(2, n, seed=2)
    items = _items(2, [0.2, 0.5])
    b = _gen(imgs, items, n, F32)
    ref = _ref(imgs, items, F32)
    Y, xi = _Y(b).astype(np.complex128), b.xinit.double().cpu().numpy()
    errY = errX = yardY = yardX = 0.0
    for j, r in enumerate(ref):
        # the yardstick: complex64 torch.fft on the same f32 image, the restated mask and the restated noise
        x32 = torch.from_numpy(r['x'].astype(np.float32)).cuda()
        mk = torch.from_numpy(r['mask'].astype(np.float32)).cuda()
        nz = torch.from_numpy((r['sigma'] * r['noise']).astype(np.float32)).cuda()
        Yy = mk * torch.fft.fft2(x32.to(torch.complex64)) + (mk * nz).to(torch.complex64)
        m = torch.fft.ifft2(Yy).abs()
        Xy = (m - m.min()) / (m.max() - m.min())
        yardY = max(yardY, np.abs(Yy.cpu().numpy().astype(np.complex128) - r['Y']).max())
        yardX = max(yardX, np.abs(Xy.double().cpu().numpy() - r['xinit']).max())
        errY = max(errY, np.abs(Y[j] - r['Y']).max())
        errX = max(errX, np.abs(xi[j] - r['xinit']).max())
        assert abs(b.sigma[j].item() - r['sigma']) <= 1e-6 * r['sigma']
    print(f'f32 n={n}: Y err {errY:.3e} (yardstick {yardY:.3e}), Xinit err {errX:.3e} (yardstick {yardX:.3e})')
    assert errY <= 4 * yardY and errX <= 4 * yardX
    assert torch.equal(b.yh_full, b.plan.pack_y(b.YT, b.maskT))


@pytest.mark.parametrize('dtype,n', [(F64, 64), (F32, 256), (F32, 128)])
def test_batch_independence(dtype, n):
    imgs = _images(3, n, seed=3)
    items = _items(3, [0.1, 0.3, 0.6, 0.9], snrs=(15.0, 25.0, 35.0))[:33]
    assert len(items) == 33
    dev = _gen(imgs, items[:1], n, dtype).xrec.device
    from pnp_svrg_amd.engine import CsmriBatch
    up = CsmriBatch.upload_images(imgs, n, n, dtype)
    assert up.device == dev
    full = _gen(up, items, n, dtype)
    rev = _gen(up, items[::-1], n, dtype)
    names = ('bits', 'YT', 'yh_full', 'xinit', 'sigma', 'maskT', 'xrec', 'inv_m0')
    for nm in names:
        assert torch.equal(getattr(full, nm), getattr(rev, nm).flip(0)), nm
    assert np.array_equal(full.M0, rev.M0[::-1])
    for j in (0, 7, 32):
        one = _gen(up, items[j:j + 1], n, dtype)
        for nm in names:
            assert torch.equal(getattr(one, nm)[0], getattr(full, nm)[j]), (nm, j)
        assert one.M0[0] == full.M0[j]


def _hand_built(imgs, items, n, dtype):
    from pnp_svrg_amd.engine import CsmriBatch
    ref = _ref(imgs, items)
    return CsmriBatch(np.stack([r['x'] for r in ref]), np.stack([r['mask'] for r in ref]), np.stack([r['Y'] for r in ref]),
                      np.stack([r['xinit'].ravel() for r in ref]), dtype=dtype)


def _run(eng, steps):
    for _ in range(steps):
        eng.step()
    return eng.psnr_trace(), eng.z.double().cpu().numpy()


@pytest.mark.parametrize('algo,dtype,n,fused', [('svrg', F64, 64, False), ('svrg', F32, 64, False), ('svrg', F32, 256, True),
                                                 ('saga', F64, 64, False), ('saga', F32, 64, False), ('gd', F64, 64, False),
                                                 ('gd', F32, 64, False)])
def test_engines_on_generated_and_hand_built_batches(algo, dtype, n, fused):
    from pnp_svrg_amd.engine import SvrgEngine, SagaEngine, GdEngine, TVProx
    imgs = _images(2, n, seed=4)
    items = _items(2, [0.3, 0.5])
    gen, hand = _gen(imgs, items, n, dtype), _hand_built(imgs, items, n, dtype)
    assert np.array_equal(gen.M0, hand.M0) and torch.equal(gen.bits, hand.bits)
    assert np.abs(gen.psnr_init() - hand.psnr_init()).max() <= 0.01 + 1e-9
    mb, eta, steps = (1000 if n == 256 else 150), 5e2, 8

    def make(b):
        if algo == 'svrg':
            return SvrgEngine(b, TVProx(), eta, 4, mb, seed=7, fused=fused)
        if algo == 'saga':
            return SagaEngine(b, TVProx(), eta, mb, hist_size=4, seed=7)
        return GdEngine(b, TVProx(), eta)
    (tg, zg), (th, zh) = _run(make(gen), steps), _run(make(hand), steps)
    dp, dz = np.abs(tg - th).max(), np.abs(zg - zh).max()
    print(f'{algo} {dtype} n={n} fused={fused}: |psnr diff| {dp:.3e}, |z diff| {dz:.3e}')
    assert np.isfinite(tg).all() and tg.shape == (steps, len(items))
    if dtype == F64:
        assert dp <= 0.01 + 1e-9 and dz <= 1e-9
    else:
        assert dp <= 0.01 + 1e-9 and dz <= 5e-4
    # set_host / draw_minibatches accept a generated batch: host-drawn index lists through the streaming engine
    if algo == 'svrg' and not fused:
        idx = gen.draw_minibatches(2, mb, seed=3)
        e = SvrgEngine(gen, TVProx(), eta, 4, mb)
        e.step(idx[0])
        e.step(idx[1])
        assert torch.isfinite(e.z).all()


def test_graph_replay_on_generated_batch_is_bit_identical():
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    imgs = _images(2, 64, seed=5)
    items = _items(2, [0.2, 0.4])
    a = SvrgEngine(_gen(imgs, items, 64, F32), TVProx(), 5e2, 4, 120, seed=3)
    b = SvrgEngine(_gen(imgs, items, 64, F32), TVProx(), 5e2, 4, 120, seed=3)
    a.run_outer(3)
    for _ in range(12):
        b.step()
    assert torch.equal(a.z, b.z) and np.array_equal(a.psnr_trace(), b.psnr_trace())


def _runner(imgs, seeding, dtype=F64, **kw):
    from pnp_svrg_amd import sweep
    return sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', eta=5e2, n_inner=8, mini_batch_size=150, T2=4, H=64, W=64, dtype=dtype,
                             seeding=seeding, keep_trace=True, **kw)


def test_sweep_device_seeding():
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    imgs = _images(2, 64, seed=6)
    items = _items(2, [0.2, 0.5])
    res = sweep.run_sweep(items, _runner(imgs, 'device'))
    assert [r['id'] for r in res] == [0, 1, 2, 3]
    for r, it in zip(res, items):
        assert r['M0'] == int(gr.mask(it['seed'], it['id'], it['alpha'], 64, 64).sum())
    eng = SvrgEngine(_gen(imgs, items, 64, F64), TVProx(), 5e2, 4, 150, seed=items[0]['id'] + 1)
    tr, z = _run(eng, 8)
    for j, r in enumerate(res):
        assert np.array_equal(r['z'], z[j]) and np.array_equal(r['psnr_trace'], tr[:, j])


def test_device_seeding_rejects_other_problems():
    from pnp_svrg_amd import sweep
    with pytest.raises(ValueError, match='csmri'):
        sweep.make_runner(_images(1, 64), 'deblur', 'saga', 'tv', eta=1.0, n_inner=4, mini_batch_size=100, H=64, W=64, seeding='device')


def test_generator_and_legacy_modes_unchanged():
    """The other two modes still equal CsmriBatch(...) built by hand from their own host arrays (a guard on the shared
    constructor); the device mode is a third stream, not theirs."""
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd import problems as P
    from pnp_svrg_amd.engine import CsmriBatch, SvrgEngine, TVProx
    imgs = _images(2, 64, seed=7)
    items = _items(2, [0.2, 0.5])
    gen = sweep.run_sweep(items, _runner(imgs, 'generator'))
    d = [sweep._csmri_item_generator(imgs[it['image']], it, 64, 64) for it in items]
    hb = CsmriBatch(np.stack([t[0] for t in d]), np.stack([t[1] for t in d]), np.stack([t[2] for t in d]),
                    np.stack([t[3] for t in d]).reshape(len(items), -1), dtype=F64)
    assert isinstance(hb.mask_np, np.ndarray) and np.array_equal(hb.mask_np, np.stack([t[1] for t in d]))
    _, z = _run(SvrgEngine(hb, TVProx(), 5e2, 4, 150, seed=items[0]['id'] + 1), 8)
    for j, r in enumerate(gen):
        assert np.array_equal(r['z'], z[j])
    leg = sweep.run_sweep(items, _runner(imgs, 'legacy'))
    probs, idx = [], []
    for it in items:
        np.random.seed(it['seed'])
        p = P.CSMRI(None, H=64, W=64, sample_prob=it['alpha'], snr=it['snr'], img=imgs[it['image']], upload=False)
        np.random.seed(1)
        idx.append(np.stack([np.flatnonzero(p.select_mb(150)) for _ in range(8)]).astype(np.int32))
        probs.append(p)
    lb = CsmriBatch(np.stack([p.Xrec for p in probs]), np.stack([p.mask for p in probs]), np.stack([p.Y for p in probs]),
                    np.stack([p.Xinit for p in probs]), dtype=F64)
    eng = SvrgEngine(lb, TVProx(), 5e2, 4, 150, seed=items[0]['id'] + 1)
    idx_d = torch.from_numpy(np.stack(idx, axis=1)).cuda()
    for s in range(8):
        eng.step(idx_d[s])
    zl = eng.z.cpu().numpy()
    for j, r in enumerate(leg):
        assert np.array_equal(r['z'], zl[j])
    dev = sweep.run_sweep(items, _runner(imgs, 'device'))
    assert [r['M0'] for r in dev] != [r['M0'] for r in gen]
    assert [r['M0'] for r in dev] == [int(gr.mask(it['seed'], it['id'], it['alpha'], 64, 64).sum()) for it in items]
