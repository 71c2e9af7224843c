"""GPU side of the device-side Deblur / phase-retrieval problem generators: DeblurBatch.generate, PrBatch.generate and
make_runner(seeding='counter') against the NumPy restatement of the published stream (tests/setup_generate_ref.py).

Tolerances: f64 A, Y, sigma <= 1e-12 * max(1, max|ref|); Deblur Xinit exact.  PR Xinit in f64: spec_iters equal to
the restatement's and the error <= 16 x the disagreement of two CPU evaluations of the restatement that sum the products in
different orders (not below the f64 bound) -- the device's tree is a third order and the error compounds over spec_iters steps.
f32: within 4 x the error of an independent plain-float32 torch pipeline on the same generated A and image, spec_iters equal to
the restatement fed the float32-rounded A, x, Y.  Loop tolerances as tests/test_gpu_csmri_generate.py.  The PR items are the
fixed ones of tests/test_cpu_setup_generate.py."""
import gc

import numpy as np
import pytest
import torch

import csmri_generate_ref as gr
import setup_generate_ref as sr
from test_cpu_setup_generate import PR_ITEMS_32, PR_ITERS_32, PR_IMAGES_32, PR_ITEM_128, PR_ITERS_128, pr_case_32, pr_case_128

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32

@pytest.fixture(autouse=True)
def _free_plans():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _items(n_img, alphas, snrs=(20.0,), seeds=(0,)):
    from pnp_svrg_amd import sweep
    return sweep.make_items(n_img, alphas, snrs, seeds)


def _pr_imgs():
    return sr.images(**PR_IMAGES_32)


def _pr_gen(items, dtype, **kw):
    from pnp_svrg_amd.engine import PrBatch
    return PrBatch.generate(_pr_imgs(), items, 32, 32, 5120, dtype, **kw)


def _tol(ref):
    return 1e-12 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize('n', [64, 256])
@pytest.mark.parametrize('sp', [100, 50])
def test_deblur_f64_against_restatement(n, sp):
    from pnp_svrg_amd.engine import DeblurBatch
    imgs = sr.images(2, n, seed=1)
    items = _items(2, [sp / 100.0], snrs=(10.0, 30.0))
    b = DeblurBatch.generate(imgs, items, n, n, F64, scale_percent=sp)
    assert b.M == (n * sp // 100) ** 2 and tuple(b.Y.shape) == (len(items), b.M)
    for j, it in enumerate(items):
        x = gr.norm01(imgs[it['image']])
        r = sr.deblur_generate(x, it, scale_percent=sp)
        eY, eS = np.abs(b.Y[j].cpu().numpy() - r['Y']).max(), abs(b.sigma[j].item() - r['sigma'])
        print(f'deblur f64 n={n} sp={sp} item {j}: Y err {eY:.3e} (tol {_tol(r["Y"]):.3e}), sigma err {eS:.3e}')
        assert np.array_equal(b.xrec[j].cpu().numpy(), x)
        assert eY <= _tol(r['Y']) and eS <= 1e-12 * max(1.0, r['sigma'])
        assert torch.equal(b.xinit[j].reshape(-1).cpu(), torch.from_numpy(r['xinit']))
    b32 = DeblurBatch.generate(imgs, items, n, n, F32, scale_percent=sp)
    for j, it in enumerate(items):
        x32 = sr.r32(gr.norm01(imgs[it['image']]))
        r = sr.deblur_generate(x32, it, scale_percent=sp)
        assert torch.equal(b32.xinit[j].reshape(-1).cpu(), torch.from_numpy(r['xinit']).float())      # the same rounding
        # yardstick: a plain float32 torch pipeline (complex64 FFT blur, float32 taps) on the same image and noise
        xt = torch.from_numpy(x32.ravel()).float().cuda()
        Bt = torch.from_numpy(sr.blur_kernel(n, n)).float().cuda()
        bl = (torch.fft.ifft(torch.fft.fft(xt.to(torch.complex64)) * torch.fft.fft(Bt.to(torch.complex64))).real * float(np.sqrt(n * n))).cpu().numpy().astype(np.float32)
        y0 = sr.bilinear(bl.astype(np.float64), n, n, sp).astype(np.float32)
        yard = np.abs((y0 + (r['sigma'] * r['noise']).astype(np.float32)).astype(np.float64) - r['Y']).max()
        err = np.abs(b32.Y[j].double().cpu().numpy() - r['Y']).max()
        print(f'deblur f32 n={n} sp={sp} item {j}: Y err {err:.3e} (yardstick {yard:.3e})')
        assert err <= 4 * yard and abs(b32.sigma[j].item() - r['sigma']) <= 1e-6 * r['sigma']


def _check_pr_f64(b, j, x, d, s, label):
    A, Y = b.A[j].cpu().numpy(), b.Y[j].cpu().numpy()
    eA, eY, eS = np.abs(A - d['A']).max(), np.abs(Y - d['Y']).max(), abs(b.sigma[j].item() - d['sigma'])
    other = sr.spec_init(d['A'], d['Y'], x, order='chunked', max_iters=1000)
    yard = np.abs(other['xinit'] - s['xinit']).max()
    eX = np.abs(b.xinit[j].reshape(-1).cpu().numpy() - s['xinit']).max()
    print(f'{label}: A err {eA:.3e}, Y err {eY:.3e} (tol {_tol(d["Y"]):.3e}), sigma err {eS:.3e}, spec_iters {b.spec_iters[j]} '
          f'(ref {s["iters"]}), Xinit err {eX:.3e} (two CPU orders disagree by {yard:.3e})')
    assert np.array_equal(b.xrec[j].cpu().numpy(), x)
    assert eA <= _tol(d['A']) and eY <= _tol(d['Y']) and eS <= 1e-12 * max(1.0, d['sigma'])
    assert b.spec_iters[j] == s['iters'] == other['iters']
    assert eX <= max(16 * yard, 1e-12)


def test_pr_f64_against_restatement():
    b = _pr_gen(PR_ITEMS_32[:3], F64)
    assert list(b.spec_iters) == PR_ITERS_32[:3]
    for j in range(3):
        x, d, s = pr_case_32(j)
        _check_pr_f64(b, j, x, d, s, f'pr f64 32x32 item {j}')


def test_pr_f64_one_item_at_128():
    from pnp_svrg_amd.engine import PrBatch
    imgs = sr.images(1, 128, seed=12)
    b = PrBatch.generate(imgs, [PR_ITEM_128], 128, 128, 8192, F64, max_iters=1000, check_every=8)
    x, d, s = pr_case_128()
    assert s['iters'] == PR_ITERS_128
    _check_pr_f64(b, 0, x, d, s, 'pr f64 128x128 M=8192')


def test_pr_f32_against_restatement_and_a_plain_f32_pipeline():
    b = _pr_gen(PR_ITEMS_32[:3], F32)
    for j in range(3):
        x, d, s = pr_case_32(j)
        A32 = b.A[j].double().cpu().numpy()
        dA = np.abs(A32 - sr.r32(d['A']))                                             # one rounding of the double stream: equal, but
        assert dA.max() <= 2.0 ** -21 and (dA != 0).mean() <= 1e-6                   # for doubles an ulp from a float32 tie
        x32 = sr.r32(x)
        Y32 = b.Y[j].double().cpu().numpy()
        s32 = sr.spec_init(A32, Y32, x32)                                              # the restatement fed the rounded A, x, Y
        assert b.spec_iters[j] == s32['iters'] == s['iters']
        # yardstick: plain float32 torch on the same generated A and image
        At, xt = b.A[j], b.xrec[j].reshape(-1)
        y0 = (At @ xt).abs()
        nz = torch.from_numpy(d['sigma'] * d['noise']).float().cuda()
        Yy = y0 + nz
        v, lead = torch.full_like(xt, 2.0), 1.0
        for _ in range(s['iters']):
            v = At.t() @ (Yy * (At @ v)) / 5120
            lead = v.max()
            v = v / lead
        x0 = torch.sqrt(lead) * v / torch.linalg.vector_norm(v) * torch.linalg.vector_norm(xt)
        Xy = (x0 - x0.min()) / (x0.max() - x0.min())
        yardY, yardX = np.abs(Yy.double().cpu().numpy() - d['Y']).max(), np.abs(Xy.double().cpu().numpy() - s['xinit']).max()
        errY, errX = np.abs(Y32 - d['Y']).max(), np.abs(b.xinit[j].reshape(-1).double().cpu().numpy() - s['xinit']).max()
        print(f'pr f32 item {j}: Y err {errY:.3e} (yardstick {yardY:.3e}), Xinit err {errX:.3e} (yardstick {yardX:.3e}), '
              f'spec_iters {b.spec_iters[j]}')
        assert errY <= 4 * yardY and errX <= 4 * yardX
        assert abs(b.sigma[j].item() - d['sigma']) <= 1e-6 * d['sigma']


@pytest.mark.parametrize('dtype', [F64, F32])
def test_pr_batch_independence(dtype):
    from pnp_svrg_amd.engine import PrBatch
    up = PrBatch.upload_images(_pr_imgs(), 32, 32, dtype)
    gen = lambda items: PrBatch.generate(up, items, 32, 32, 5120, dtype)
    full, rev = gen(PR_ITEMS_32), gen(PR_ITEMS_32[::-1])
    assert len(set(full.spec_iters.tolist())) == 5                                   # every item stops at another step: freezing
    names = ('A', 'Y', 'xrec', 'xinit', 'sigma')
    for nm in names:
        assert torch.equal(getattr(full, nm), getattr(rev, nm).flip(0)), nm
    assert np.array_equal(full.spec_iters, rev.spec_iters[::-1])
    for j in (0, 3):
        one = gen(PR_ITEMS_32[j:j + 1])
        for nm in names:
            assert torch.equal(getattr(one, nm)[0], getattr(full, nm)[j]), (nm, j)
        assert one.spec_iters[0] == full.spec_iters[j]


def test_deblur_batch_independence():
    from pnp_svrg_amd.engine import DeblurBatch
    imgs = sr.images(3, 64, seed=3)
    items = _items(3, [0.5], snrs=(15.0, 25.0, 35.0))[:7]
    up = DeblurBatch.upload_images(imgs, 64, 64, F32)
    gen = lambda its: DeblurBatch.generate(up, its, 64, 64, F32, scale_percent=50)
    full, rev, one = gen(items), gen(items[::-1]), gen(items[4:5])
    for nm in ('Y', 'xrec', 'xinit', 'sigma'):
        assert torch.equal(getattr(full, nm), getattr(rev, nm).flip(0)), nm
        assert torch.equal(getattr(one, nm)[0], getattr(full, nm)[4]), nm


def test_iteration_cap_names_the_item():
    with pytest.raises(ValueError, match=r'items \[50\]'):
        _pr_gen(PR_ITEMS_32[1:2], F64, max_iters=2, check_every=8)
    b = _pr_gen(PR_ITEMS_32[:1], F64, max_iters=28, check_every=7)                    # exactly enough
    assert b.spec_iters[0] == 28


def _run(eng, steps):
    for _ in range(steps):
        eng.step()
    return eng.psnr_trace(), eng.z.double().cpu().numpy()


@pytest.mark.parametrize('problem,algo,dtype', [('deblur', 'svrg', F64), ('deblur', 'saga', F32), ('pr', 'svrg', F32), ('pr', 'sarah', F64)])
def test_engines_on_generated_and_hand_built_batches(problem, algo, dtype):
    from pnp_svrg_amd.engine import DeblurBatch, PrBatch, SvrgEngine, SagaEngine, SarahEngine, TVProx
    from pnp_svrg_amd.problems import _deblur_taps
    if problem == 'deblur':
        imgs = sr.images(2, 64, seed=4)
        items = _items(2, [0.5])
        gen = DeblurBatch.generate(imgs, items, 64, 64, dtype, scale_percent=50)
        ref = [sr.deblur_generate(gr.norm01(imgs[it['image']]), it, scale_percent=50) for it in items]
        hand = DeblurBatch(np.stack([gr.norm01(imgs[it['image']]) for it in items]), sr.blur_kernel(64, 64), np.stack([r['Y'] for r in ref]),
                           np.stack([r['xinit'] for r in ref]), dtype=dtype, bilinear=_deblur_taps(64, 64, 50))
        eta, mb = 1e7, 300
    else:
        items = PR_ITEMS_32[:2]
        gen = _pr_gen(items, dtype)
        cases = [pr_case_32(j) for j in range(2)]
        hand = PrBatch(np.stack([c[0] for c in cases]), np.stack([c[1]['A'] for c in cases]), np.stack([c[1]['Y'] for c in cases]),
                       np.stack([c[2]['xinit'] for c in cases]), dtype=dtype)
        eta, mb = 0.05, 200
    assert gen.M == hand.M and gen.max_mb == hand.max_mb and type(gen) is type(hand)
    assert np.abs(gen.psnr_init() - hand.psnr_init()).max() <= 0.01 + 1e-9

    def make(b):
        if algo == 'svrg':
            return SvrgEngine(b, TVProx(), eta, 4, mb, seed=7)
        if algo == 'saga':
            return SagaEngine(b, TVProx(), eta, mb, hist_size=4, seed=7)
        return SarahEngine(b, TVProx(), eta, 4, mb, seed=7)
    (tg, zg), (th, zh) = _run(make(gen), 8), _run(make(hand), 8)
    dz = np.abs(zg - zh).max()
    print(f'{problem} {algo} {dtype}: |psnr diff| {np.abs(tg - th).max():.3e}, |z diff| {dz:.3e}')
    assert np.isfinite(tg).all() and np.array_equal(tg, th)                           # identical rounded PSNR traces
    assert dz <= (1e-9 if dtype == F64 else 5e-4)


def test_sweep_counter_seeding():
    from pnp_svrg_amd import sweep
    kw = dict(eta=1e7, n_inner=8, mini_batch_size=200, T2=4, H=64, W=64, dtype=F32, keep_trace=True)
    imgs = sr.images(2, 64, seed=6)
    items = _items(2, [0.5, 1.0])                                                     # alpha = 0.5: super-resolution
    res = sweep.run_sweep(items, sweep.make_runner(imgs, 'deblur', 'svrg', 'tv', seeding='counter', **kw))
    assert [r['id'] for r in res] == [0, 1, 2, 3] and all(np.isfinite(r['z']).all() and np.isfinite(r['psnr_final']) for r in res)
    pr = sweep.make_runner(_pr_imgs(), 'pr', 'svrg', 'tv', seeding='counter', **dict(kw, H=32, W=32, eta=0.05))
    res = sweep.run_sweep(PR_ITEMS_32[:2], pr)
    assert len(res) == 2 and all(np.isfinite(r['z']).all() for r in res)
    a, b = (sweep.run_sweep(items, sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', seeding=m, **dict(kw, eta=5e2))) for m in ('counter', 'device'))
    for ra, rb in zip(a, b):
        assert np.array_equal(ra['z'], rb['z']) and np.array_equal(ra['psnr_trace'], rb['psnr_trace']) and ra['M0'] == rb['M0']
