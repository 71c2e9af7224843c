"""The one-launch forms: a whole pnp_sarah outer iteration in one launch (pnp_csmri_sarah_outer_iteration, k_sarah_outer) and
n-step spans of the pnp_gd / pnp_sgd / pnp_saga inner iteration (pnp_csmri_grad_span, pnp_csmri_saga_span) against the eager
`fused=True` engines they replace -- the same kernel bodies run back to back by the workgroup that owns a problem, so every
comparison is torch.equal -- plus the refusals, one SARAH run against the oracle loop and the sweep runner's option.

Every case is 256 x 256 (the kernels have no other size) with B = 3 (masks of different M0) or B = 1."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, MB, ETA, SM, HIST = 3, 1000, 2e3, 1.1, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def batch():
    from pnp_svrg_amd.engine import CsmriBatch
    return CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=13)


@pytest.fixture(scope='module')
def one():
    from pnp_svrg_amd.engine import CsmriBatch
    return CsmriBatch.synthetic(1, 256, 256, 0.2, 20.0, seed=19)


def _tv(sm=SM):
    from pnp_svrg_amd.engine import TVProx
    return TVProx(sigma_modifier=sm)


def _sarah(batch, T2, **kw):
    from pnp_svrg_amd.engine import SarahEngine
    return SarahEngine(batch, _tv(), ETA, T2, MB, seed=4, fused=True, **kw)


def _same_sarah(a, b, rows=None):
    for n in ('z', 'w_prev', 'w_next', 'v_prev'):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    la, lb = (a.sse_log, b.sse_log) if rows is None else (a.sse_log[:rows], b.sse_log[:rows])
    assert torch.equal(la, lb) and torch.equal(a.prox.sig, b.prox.sig)
    assert (a.s, a.n_prox, a.prox.t) == (b.s, b.n_prox, b.prox.t)


# ---------------------------------------------------------------------------------------------------------------------- SARAH
def test_sarah_outer_iteration_in_one_launch_is_bit_identical(batch):
    """T2 = 4: run_outer(2, one_launch=True) == 8 eager fused steps on z, w_prev, w_next, v_prev, log rows 0..9 and the noise estimate;
    continued with eager steps (into the middle of an outer iteration) the two stay equal."""
    T2 = 4
    o, e = _sarah(batch, T2), _sarah(batch, T2)
    assert o.outer_kernel_ok()
    o.run_outer(2, one_launch=True)
    for _ in range(2 * T2):
        e.step()
    assert (o.s, o.n_prox, o.prox.t) == (8, 10, 10)
    _same_sarah(o, e, rows=10)
    assert not torch.equal(o.z, batch.xinit) and not torch.equal(o.sse_log[0], o.sse_log[9]) and torch.equal(o.w_prev, o.z)
    assert not o.sse_log[10:].any()
    for _ in range(T2 + 2):
        o.step(), e.step()
    assert (o.s, o.n_prox) == (14, 18)
    _same_sarah(o, e)
    # and back: a one-launch outer iteration behind eager ones
    for _ in range(T2 - 2):
        o.step(), e.step()
    o.run_outer(1, one_launch=True)
    for _ in range(T2):
        e.step()
    assert (o.s, o.n_prox) == (20, 25)
    _same_sarah(o, e)


@pytest.mark.parametrize('T2,n_log,n_outer', [(1, 4096, 3), (4, 7, 2)])
def test_sarah_edges(batch, T2, n_log, n_outer):
    """T2 = 1: slot 0 is the only slot of selbits and must be read (k_svrg_outer skips it); n_log = 7 with T2 = 4 over two outer
    iterations: the log ring wraps inside an outer iteration."""
    o, e = _sarah(batch, T2, n_log=n_log), _sarah(batch, T2, n_log=n_log)
    o.run_outer(n_outer, one_launch=True)
    for _ in range(n_outer * T2):
        e.step()
    _same_sarah(o, e)
    assert o.n_prox == n_outer * (T2 + 1) and np.array_equal(o.psnr_trace(), e.psnr_trace())
    if T2 == 1:                                                  # the inner iteration moved z: its minibatch gradient was not skipped
        assert not torch.equal(o.z, batch.xinit) and not torch.equal(o.v_prev, torch.zeros_like(o.v_prev))
    else:
        assert o.n_prox > n_log and o.sse_log.all()


@pytest.mark.parametrize('lr_decay', [1.0, 0.9])
def test_sarah_per_problem_values_equal_scalar_engines(one, lr_decay):
    """The _pp entry: one.tile(3) with per-problem eta, mini_batch_size and sigma_modifier, two outer iterations in two launches ==
    three scalar B = 1 engines stepping eagerly, bit for bit; with lr_decay the outer step does not decay (F6), the inner ones do."""
    from pnp_svrg_amd.engine import SarahEngine
    T2 = 3
    eta, mb, sm = np.array([1.5e3, 2e3, 2.5e3]), np.array([800, 1000, 1300], np.int32), np.array([0.9, 1.1, 1.4])
    e = SarahEngine(one.tile(3), _tv(sm), eta, T2, mb, lr_decay=lr_decay, seed=6, draw_id=[0, 0, 0], fused=True)
    e.run_outer(2, one_launch=True)
    rows = 2 * (T2 + 1)
    assert (e.s, e.n_prox) == (2 * T2, rows)
    for k in range(3):
        r = SarahEngine(one, _tv(float(sm[k])), float(eta[k]), T2, int(mb[k]), lr_decay=lr_decay, seed=6, fused=True)
        for _ in range(2 * T2):
            r.step()
        for n in ('z', 'w_prev', 'w_next', 'v_prev'):
            assert torch.equal(getattr(e, n)[k], getattr(r, n)[0]), (k, n)
        assert torch.equal(e.sse_log[:rows, k], r.sse_log[:rows, 0]) and torch.equal(e.prox.sig[k], r.prox.sig[0]), k
    assert not torch.equal(e.z[0], e.z[1])


# ---------------------------------------------------------------------------------------------------------------------- spans
def _same_steps(a, b):
    assert torch.equal(a.z, b.z) and torch.equal(a.sse_log, b.sse_log) and torch.equal(a.prox.sig, b.prox.sig)
    assert (a.s, a.n_prox, a.prox.t) == (b.s, b.n_prox, b.prox.t)


def test_gd_span(batch):
    """run_span(5) == 5 eager fused steps; then 20 more, across two launches."""
    from pnp_svrg_amd.engine import GdEngine
    o, e = GdEngine(batch, _tv(), ETA, fused=True), GdEngine(batch, _tv(), ETA, fused=True)
    assert o.span_kernel_ok()
    o.run_span(5)
    for _ in range(5):
        e.step()
    assert o.s == 5 and not torch.equal(o.z, batch.xinit)
    _same_steps(o, e)
    o.run_span(20)
    for _ in range(20):
        e.step()
    _same_steps(o, e)


def test_sgd_span_from_an_unaligned_step(batch):
    """run_span(18) from s = 3: crosses the AHEAD windows of the eager draws with an unaligned start; a later eager step redraws."""
    from pnp_svrg_amd.engine import SgdEngine
    o, e = (SgdEngine(batch, _tv(), ETA, MB, seed=4, fused=True) for _ in range(2))
    for _ in range(3):
        o.step(), e.step()
    o.run_span(18)
    for _ in range(18):
        e.step()
    assert o.s == 21
    _same_steps(o, e)
    o.step(), e.step()
    _same_steps(o, e)


def test_saga_span(batch):
    """hist_size = 4, run_span(9, r=...) with row == prev_row inside the span and at its start == step(r=...) on z, table, tsum, the
    log and r_prev; then r=None on two engines of the same seed: the trajectory stepping walks."""
    from pnp_svrg_amd.engine import SagaEngine
    rows = [2, 2, 0, 3, 3, 3, 1, 0, 0]
    o, e = (SagaEngine(batch, _tv(), ETA, MB, hist_size=HIST, seed=4, fused=True) for _ in range(2))
    o.step(r=2), e.step(r=2)                                     # the span starts on the row the step before replaced
    o.run_span(9, r=rows)
    for r in rows:
        e.step(r=r)

    def same():
        _same_steps(o, e)
        assert torch.equal(o.table, e.table) and torch.equal(o.tsum, e.tsum) and np.array_equal(o.r_prev, e.r_prev)
    same()
    assert o.r_prev == 0 and not torch.equal(o.table[1], o.table[2])
    o.run_span(20)                                               # r=None: two launches, the engine's own rows
    for _ in range(20):
        e.step()
    same()
    per = np.array([[0, 1, 2], [0, 3, 2], [1, 1, 1]])            # per-problem rows, some equal to the previous step's
    o.run_span(3, r=per)
    for r in per:
        e.step(r=r)
    same()
    o.step(), e.step()
    same()


@pytest.mark.parametrize('algo', ['gd', 'sgd', 'saga'])
def test_span_per_problem_values_equal_scalar_engines(one, algo):
    """one.tile(3) with per-problem eta, mini_batch_size and sigma_modifier (saga: per-problem rows as well) through run_span == three
    scalar B = 1 engines stepping eagerly, bit for bit."""
    from pnp_svrg_amd.engine import make_engine
    n = 5
    eta, mb, sm = np.array([1.5e3, 2e3, 2.5e3]), np.array([800, 1000, 1300], np.int32), np.array([0.9, 1.1, 1.4])
    rows = np.array([[0, 1, 2], [0, 1, 0], [2, 2, 1], [1, 0, 1], [1, 2, 2]])
    kw = dict(algorithm=algo, hist_size=3, seed=6, fused=True)
    e = make_engine(one.tile(3), _tv(sm), eta, None, None if algo == 'gd' else mb, draw_id=[0, 0, 0], **kw)
    assert e.span_kernel_ok()
    if algo == 'saga':
        e.run_span(n, r=rows)
    else:
        e.run_span(n)
    for k in range(3):
        r = make_engine(one, _tv(float(sm[k])), float(eta[k]), None, None if algo == 'gd' else int(mb[k]), **kw)
        for s in range(n):
            if algo == 'saga':
                r.step(r=int(rows[s, k]))
            else:
                r.step()
        assert torch.equal(e.z[k], r.z[0]) and torch.equal(e.sse_log[:n, k], r.sse_log[:n, 0]) and torch.equal(e.prox.sig[k], r.prox.sig[0]), k
        if algo == 'saga':
            assert torch.equal(e.table[:, k], r.table[:, 0]) and torch.equal(e.tsum[k], r.tsum[0]), k
    assert not torch.equal(e.z[0], e.z[1])


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_what_refuses_and_what_falls_back(batch):
    from pnp_svrg_amd.engine import DnCNNProx, SarahEngine, SgdEngine
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    T2 = 2
    e = SarahEngine(batch, DnCNNProx(random_dncnn_weights(17, seed=1), 15), 1.0, T2, MB, seed=4, fused=True)
    assert not e.outer_kernel_ok()
    with pytest.raises(ValueError, match=r'one_launch=True\) needs a prox that runs inside the kernel: TVProx \(got DnCNNProx\)'):
        e.run_outer(1, one_launch=True)
    e = _sarah(batch, T2)
    idx = batch.draw_minibatches(T2, MB, seed=2)
    for s in range(T2):
        e.step(idx[s])                                           # a host-fed outer iteration: its slots hold host selectors
    assert e.s % T2 == 0 and not e.outer_kernel_ok()
    with pytest.raises(ValueError, match='needs device-drawn minibatches'):
        e.run_outer(1, one_launch=True)
    e = _sarah(batch, T2)
    e.step()
    with pytest.raises(ValueError, match=r'needs a step count that is a multiple of T2 \(s = 1, T2 = 2\)'):
        e.run_outer(1, one_launch=True)
    assert e.s == 1
    # a decaying step size has no span form: run_span steps eagerly, and equals stepping
    o, r = (SgdEngine(batch, _tv(), ETA, MB, lr_decay=0.9, seed=4, fused=True) for _ in range(2))
    assert not o.span_kernel_ok()
    o.run_span(5)
    for _ in range(5):
        r.step()
    _same_steps(o, r)


# --------------------------------------------------------------------------------------------------------------------- oracle
def test_sarah_one_launch_against_the_oracle_loop():
    """One problem (tests/golden/synth256.png), T2 = 3, two outer iterations in two launches, against oracle.loops.pnp_sarah fed the
    minibatches the device drew (decoded from the selector bits): every PSNR within 0.01 dB, |z - z_oracle| <= 1e-3 (the project's
    float32 bounds, test_fused_engine_against_the_oracle_loop)."""
    import problems as P
    from oracle import denoise as od, loops as ol, problems as op
    from pnp_svrg_amd.engine import CsmriBatch, SarahEngine, TVProx
    img, T2, n_outer, eta = os.path.join(GOLDEN, 'synth256.png'), 3, 2, 2e3
    steps = n_outer * T2
    np.random.seed(0)
    p = P.CSMRI(img, H=256, W=256, sample_prob=0.2, snr=20., upload=False)
    eng = SarahEngine(CsmriBatch.from_problems([p]), TVProx(), eta, T2, MB, seed=5, fused=True)
    sel = []
    for _ in range(n_outer):
        eng.run_outer(1, one_launch=True)
        sel.append(eng.mbs.selbits.cpu().numpy().copy())        # [T2][1][kx][ky >> 5] words of this outer iteration
    tr = eng.psnr_trace()[:, 0]
    shifts = np.arange(32, dtype=np.uint32)
    masks = []
    for o in range(n_outer):
        for j in range(T2):
            w = sel[o][j][0].view(np.uint32)
            ind = ((w[:, :, None] >> shifts) & 1).reshape(256, 256).T.astype(int)    # [ky][kx] = the H x W indicator select_mb returns
            assert ind.sum() == MB and (ind <= p.mask).all()
            masks.append(ind)
    assert not np.array_equal(masks[0], masks[1])
    np.random.seed(0)
    po = op.CSMRI(img, H=256, W=256, sample_prob=0.2, snr=20.)
    it = iter(masks)
    po.select_mb = lambda size: next(it)
    o, j = (steps - 1) // T2, (steps - 1) % T2
    ro = ol.pnp_sarah(po, od.TVDenoiser(), eta, 1 + o * (5 + 5 * T2) + 5 + 5 * j + 1, T2, MB, converge_check=False, clock=ol.CountingClock())
    ref = np.array(ro['psnr_per_iter'])
    assert len(ref) == len(tr) == steps + n_outer
    dp, dz = np.abs(tr - ref).max(), np.abs(eng.z[0].double().cpu().numpy().ravel() - ro['z']).max()
    print(f'PSNR vs oracle: {dp:.4f} dB; |z - z_ref| = {dz:.3e}')
    assert dp <= 0.01 + 1e-9
    assert dz <= 1e-3


# --------------------------------------------------------------------------------------------------------------------- runner
@pytest.mark.parametrize('algo', ['sarah', 'saga'])
def test_runner_one_launch_cells(algo):
    """make_runner(one_launch=True) on two items == the same runner without the option: z bit for bit, the same rows."""
    from pnp_svrg_amd import sweep
    rng = np.random.default_rng(3)
    imgs = [np.cumsum(np.cumsum(rng.standard_normal((256, 256)), 0), 1) for _ in range(2)]
    items = [{'id': 0, 'image': 0, 'alpha': 0.2, 'snr': 20.0, 'seed': 0}, {'id': 1, 'image': 1, 'alpha': 0.3, 'snr': 20.0, 'seed': 1}]
    opt = dict(sarah_fused=True, sarah_trials=True) if algo == 'sarah' else dict(fused_steps=True)
    res = {}
    for on in (True, False):
        run = sweep.make_runner(imgs, problem='csmri', algorithm=algo, denoiser='tv', eta=2e3, n_inner=8, mini_batch_size=MB, T2=4,
                                hist_size=HIST, seeding='counter', keep_trace=True, one_launch=on, **opt)
        res[on] = run(items)
    for a, b in zip(res[True], res[False]):
        assert a.keys() == b.keys() and a['id'] == b['id']
        assert np.array_equal(a['z'], b['z']) and np.array_equal(a['psnr_trace'], b['psnr_trace']) and a['psnr_final'] == b['psnr_final']
    assert len(res[True][0]['psnr_trace']) == (10 if algo == 'sarah' else 8)
