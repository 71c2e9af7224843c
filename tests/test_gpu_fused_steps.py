"""The one-kernel inner iterations of pnp_gd, pnp_sgd and pnp_saga on CSMRI (pnp_csmri_grad_step, pnp_csmri_saga_step,
csrc/csmri_fused.hip) and GdEngine / SgdEngine / SagaEngine with fused=True: the minibatch data term inside the fused
column phase against the streaming column kernel, the whole steps against the streaming sequences, their aliased and per-problem
forms, the engines against the streaming engines and the oracle loops, and the sweep.

Every case is 256 x 256 (the kernels have no other size) with B = 3 (masks of different M0) or B = 1.  The bounds are the ones
tests/test_gpu_sarah_fused.py holds this file's kernels to: 2e-6 gradient against streaming, 2e-5 whole step, 5e-5 and 0.01 dB for an
engine after 9 steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, MB, LR, SM, HIST = 3, 1000, 2e3, 1.3, 4


def _f64(n):
    return torch.empty(n, dtype=torch.float64, device='cuda')


@pytest.fixture(scope='module')
def env():
    """One synthetic batch (Bernoulli masks: M0 differs from problem to problem), an iterate away from xinit, drawn selectors at
    mb = 1, MB and M0, and a hand-made selector with the edge cases of the column phase."""
    from pnp_svrg_amd.engine import CsmriBatch
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=41)
    p = batch.plan
    rng = np.random.default_rng(0)
    z = torch.from_numpy(batch.xinit.cpu().numpy() + 0.05 * rng.standard_normal((B, 256, 256))).float().cuda().contiguous()
    m0 = np.asarray(batch.M0, np.int32)
    assert len(set(m0.tolist())) == B
    sel = {}
    for name, mb in (('one', 1), ('mid', MB), ('all', torch.from_numpy(m0).cuda())):
        sb = torch.empty((1, B, 256, 8), dtype=torch.int32, device='cuda')
        p.draw_thresholds(batch.bits, mb, seed=3, step0=7, nsteps=1, selbits=sb)
        sel[name] = sb[0].contiguous()
    # selT[b, kx, ky]: points without their mirrors, points in the packed columns kx = 0 and kx = 128, at ky = 0 and ky = 128
    selT = torch.zeros((B, 256, 256), dtype=torch.uint8)
    for kx, ky in ((0, 0), (0, 128), (0, 5), (128, 0), (128, 128), (128, 7), (128, 249), (3, 9), (64, 0), (64, 128), (192, 128), (17, 0),
                   (255, 255), (1, 128), (127, 200), (129, 31), (129, 32)):
        selT[:, kx, ky] = 1
    assert selT[0, 0, 251] == 0 and selT[0, 253, 247] == 0 and selT[0, 128, 7] == 1 and selT[0, 192, 0] == 0
    extra = rng.random((B, 256, 256)) < 0.01
    selT |= torch.from_numpy(extra.astype(np.uint8))
    sel['hand'] = p.pack_mask(selT.cuda().contiguous())
    torch.cuda.synchronize()
    return dict(batch=batch, p=p, z=z, sel=sel, m0=m0)


# ------------------------------------------------------------------------------------------------------------------ data term
@pytest.mark.parametrize('which', ['one', 'mid', 'all', 'hand'])
def test_minibatch_data_term_against_streaming_columns(env, which):
    """grad_step(denoise=0, beta=0, YT, slot) == pnp_csmri_grad_sel(YT=..., the same slot) -- the streaming k_cols, whose YT branch
    the fused column phase mirrors -- to 2e-6 * max(1, |ref|)."""
    e = env
    bits, alpha = e['sel'][which], {'one': 1.0, 'mid': 1.0 / MB, 'all': 1.0 / 13000, 'hand': 1.0 / 700}[which]
    out, sse, _ = e['p'].grad_step(e['z'], bits, YT=e['batch'].YT, alpha=alpha, beta=0.0, c1=e['z'], denoise=False)
    ref = e['p'].grad(e['z'], bits=bits, YT=e['batch'].YT, alpha=alpha)            # YT != NULL: the three streaming kernels
    assert sse is None and ref.abs().max().item() > 0
    d, bound = (out - ref).abs().max().item(), 2e-6 * max(1.0, ref.abs().max().item())
    print(f'[{which}] fused data term vs streaming: {d:.3e} (bound {bound:.3e}, |ref| {ref.abs().max().item():.3e})')
    assert d <= bound


def test_yt_form_on_the_mask_equals_the_yh_form(env):
    """mb = M0 draws the whole mask; on it the data term built from YT equals the one packed by pnp_csmri_pack_y (2e-6)."""
    e = env
    b = e['batch']
    assert torch.equal(e['sel']['all'], b.bits)
    kw = dict(alpha=-LR, alpha_vec=b.inv_m0, beta=1.0, c1=e['z'], denoise=False)
    yt = e['p'].grad_step(e['z'], b.bits, YT=b.YT, **kw)[0]
    yh = e['p'].grad_step(e['z'], b.bits, yh=b.yh_full, **kw)[0]
    d, bound = (yt - yh).abs().max().item(), 2e-6 * max(1.0, yh.abs().max().item())
    print(f'YT form vs yh form on the mask: {d:.3e} (bound {bound:.3e})')
    assert d <= bound and not torch.equal(yh, e['z'])


# ----------------------------------------------------------------------------------------------------------------- whole step
def _grad_forms(e):
    b = e['batch']
    return {'gd': dict(bits=b.bits, yh=b.yh_full, alpha=-LR, alpha_vec=b.inv_m0),
            'sgd': dict(bits=e['sel']['mid'], YT=b.YT, alpha=-LR / MB)}


@pytest.mark.parametrize('form', ['gd', 'sgd'])
def test_grad_step_against_streaming_sequence(env, form):
    """pnp_csmri_grad_sel (streaming, B = 3) + pnp_prox_tv: |out - want| <= 2e-5, sse to rtol 1e-4, sigma to 1e-6 relative; the
    in-place form (out = a = c1, what the engines pass) equals the out-of-place one bit for bit."""
    from pnp_svrg_amd import ops
    e = env
    b, kw = e['batch'], dict(_grad_forms(e)[form])
    bits = kw.pop('bits')
    sse = _f64(B)
    out, _, sig = e['p'].grad_step(e['z'], bits, beta=1.0, c1=e['z'], xrec=b.xrec, sigma_modifier=SM, sse=sse, **kw)
    stepped = e['p'].grad(e['z'], bits=bits, beta=1.0, c1=e['z'], **kw)
    want, want_sse, want_sig = ops.prox_tv(stepped.clone(), xrec=b.xrec, sigma_modifier=SM)
    assert not torch.equal(want, stepped)
    d = (out - want).abs().max().item()
    print(f'[{form}] out vs streaming: {d:.3e} (bound 2e-5)')
    assert d <= 2e-5
    np.testing.assert_allclose(sse.cpu().numpy(), want_sse.cpu().numpy(), rtol=1e-4)
    assert (sig - want_sig).abs().max().item() <= 1e-6 * want_sig.abs().max().item()
    zz, sse2 = e['z'].clone(), _f64(B)
    e['p'].grad_step(zz, bits, beta=1.0, c1=zz, out=zz, xrec=b.xrec, sigma_modifier=SM, sse=sse2, **kw)
    assert torch.equal(zz, out) and torch.equal(sse2, sse)
    # denoise == 0 stores the stepped image
    raw = e['p'].grad_step(e['z'], bits, beta=1.0, c1=e['z'], denoise=False, **kw)[0]
    assert (raw - stepped).abs().max().item() <= 2e-6 * max(1.0, stepped.abs().max().item())


def _saga_state(e, hist, seed=5):
    rng = np.random.default_rng(seed)
    table = torch.from_numpy(1e-4 * rng.standard_normal((hist, B, 256, 256))).float().cuda().contiguous()
    return table, table.sum(0).contiguous()


def _rows(v):
    return torch.tensor(v, dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('hist,row,prev', [(HIST, [2, 2, 2], [1, 1, 1]), (HIST, [0, 3, 1], [3, 3, 0]), (HIST, [1, 2, 3], [1, 2, 3]),
                                          (1, [0, 0, 0], [0, 0, 0])])
def test_saga_step_against_streaming_sequence(env, hist, row, prev):
    """pnp_csmri_grad_sel(YT) + pnp_saga_table_update_pp + pnp_prox_tv: out to 2e-5, sse to rtol 1e-4, sigma to 1e-6; the replaced
    row and the sum to 2e-6 * max(1, |ref|), every other row of the table bit-unchanged.  One row for the batch, per-problem rows,
    row == prev_row, hist_size = 1."""
    from pnp_svrg_amd import ops
    e = env
    b, bits = e['batch'], e['sel']['mid']
    table, tsum = _saga_state(e, hist)
    t0 = table.clone()
    t_ref, s_ref, z_ref = table.clone(), tsum.clone(), e['z'].clone()
    g = e['p'].grad(e['z'], bits=bits, YT=b.YT, alpha=1.0 / MB)
    ops.saga_table_update_pp(z_ref, g, t_ref, _rows(row), _rows(prev), s_ref, LR, 1.0 / hist)
    want, want_sse, want_sig = ops.prox_tv(z_ref, xrec=b.xrec, sigma_modifier=SM)
    sse = _f64(B)
    out, _, sig = e['p'].saga_step(e['z'], bits, b.YT, table, _rows(row), _rows(prev), tsum, LR, 1.0 / hist, alpha=1.0 / MB,
                                   xrec=b.xrec, sigma_modifier=SM, sse=sse)
    d = (out - want).abs().max().item()
    print(f'[hist {hist}, rows {row}/{prev}] out vs streaming: {d:.3e} (bound 2e-5)')
    assert d <= 2e-5
    np.testing.assert_allclose(sse.cpu().numpy(), want_sse.cpu().numpy(), rtol=1e-4)
    assert (sig - want_sig).abs().max().item() <= 1e-6 * want_sig.abs().max().item()
    assert (tsum - s_ref).abs().max().item() <= 2e-6 * max(1.0, s_ref.abs().max().item())
    for k in range(B):
        for r in range(hist):
            if r == row[k]:
                assert (table[r, k] - g[k]).abs().max().item() <= 2e-6 * max(1.0, g.abs().max().item()), (r, k)
                assert torch.equal(t_ref[r, k], g[k])
            else:
                assert torch.equal(table[r, k], t0[r, k]), (r, k)
    # in place (out = z, the engines' form) == out of place, bit for bit; denoise == 0 stores the stepped image
    table2, tsum2 = _saga_state(e, hist)
    zz, sse2 = e['z'].clone(), _f64(B)
    e['p'].saga_step(zz, bits, b.YT, table2, _rows(row), _rows(prev), tsum2, LR, 1.0 / hist, alpha=1.0 / MB, out=zz, xrec=b.xrec,
                     sigma_modifier=SM, sse=sse2)
    assert torch.equal(zz, out) and torch.equal(sse2, sse) and torch.equal(table2, table) and torch.equal(tsum2, tsum)
    table3, tsum3 = _saga_state(e, hist)
    raw = e['p'].saga_step(e['z'], bits, b.YT, table3, _rows(row), _rows(prev), tsum3, LR, 1.0 / hist, alpha=1.0 / MB, denoise=False)[0]
    z_step = e['z'].clone()
    ops.saga_table_update_pp(z_step, g, t0.clone(), _rows(row), _rows(prev), _saga_state(e, hist)[1], LR, 1.0 / hist)
    assert (raw - z_step).abs().max().item() <= 2e-6 * max(1.0, z_step.abs().max().item())
    assert torch.equal(table3, table)


# --------------------------------------------------------------------------------------------------------------- bit-identity
def test_per_problem_forms_and_batch_independence(env):
    """_pp: problem b == the plain call on a B = 1 plan with b's scalars, bit for bit (so a problem depends neither on the batch size
    nor on its position); a _pp call with every array NULL == the plain call."""
    from pnp_svrg_amd import _native as N, ops
    e = env
    b, bits = e['batch'], e['sel']['mid']
    al, lr, sm = [-LR / 900, -LR / 1000, -LR / 1300], [1.5e3, 2e3, 2.75e3], [0.9, 1.3, 1.7]
    row, prev = [0, 3, 1], [3, 3, 0]
    t = lambda v: torch.tensor(v, dtype=torch.float64, device='cuda')              # noqa: E731
    p1 = ops.CsmriPlan(256, 256, 1, torch.float32)
    one = lambda x, k: x[k:k + 1].contiguous()                                     # noqa: E731
    # grad_step, both forms
    for form in ('gd', 'sgd'):
        kw = dict(_grad_forms(e)[form])
        fbits = kw.pop('bits')
        kw.pop('alpha')
        sse = _f64(B)
        out, _, sig = e['p'].grad_step(e['z'], fbits, alpha=t(al), beta=1.0, c1=e['z'], xrec=b.xrec, sigma_modifier=t(sm), sse=sse, **kw)
        for k in range(B):
            kw1 = {n: one(v, k) for n, v in kw.items()}
            sse1 = _f64(1)
            out1, _, sig1 = p1.grad_step(one(e['z'], k), one(fbits, k), alpha=al[k], beta=1.0, c1=one(e['z'], k), xrec=one(b.xrec, k),
                                         sigma_modifier=sm[k], sse=sse1, **kw1)
            assert torch.equal(out[k:k + 1], out1) and torch.equal(sig[k:k + 1], sig1) and torch.equal(sse[k:k + 1], sse1), (form, k)
        assert not torch.equal(out[0], out[1])
    # saga_step
    table, tsum = _saga_state(e, HIST)
    t0, s0 = table.clone(), tsum.clone()
    sse = _f64(B)
    out, _, sig = e['p'].saga_step(e['z'], bits, b.YT, table, _rows(row), _rows(prev), tsum, t(lr), 1.0 / HIST, alpha=t([1 / 900, 1e-3, 1 / 1300]),
                                   xrec=b.xrec, sigma_modifier=t(sm), sse=sse)
    for k in range(B):
        tk, sk, sse1 = t0[:, k:k + 1].contiguous(), one(s0, k), _f64(1)
        out1, _, sig1 = p1.saga_step(one(e['z'], k), one(bits, k), one(b.YT, k), tk, _rows(row[k:k + 1]), _rows(prev[k:k + 1]), sk, lr[k],
                                     1.0 / HIST, alpha=[1 / 900, 1e-3, 1 / 1300][k], xrec=one(b.xrec, k), sigma_modifier=sm[k], sse=sse1)
        assert torch.equal(out[k:k + 1], out1) and torch.equal(sig[k:k + 1], sig1) and torch.equal(sse[k:k + 1], sse1), k
        assert torch.equal(table[:, k:k + 1], tk) and torch.equal(tsum[k:k + 1], sk), k
    # every array NULL
    P = ops._p
    ref_sse = _f64(B)
    ref, _, ref_sig = e['p'].grad_step(e['z'], bits, YT=b.YT, alpha=-LR / MB, beta=1.0, c1=e['z'], xrec=b.xrec, sigma_modifier=SM, sse=ref_sse)
    out2, sse2, sig2 = torch.empty_like(ref), _f64(B), torch.empty(B, device='cuda')
    N.call('pnp_csmri_grad_step_pp', e['p']._h, P(e['z']), P(bits), None, P(b.YT), -LR / MB, None, None, 1.0, P(e['z']), P(out2), 1, SM, None,
           0.0, P(b.xrec), P(sse2), P(sig2), ops._stream())
    assert torch.equal(out2, ref) and torch.equal(sse2, ref_sse) and torch.equal(sig2, ref_sig)
    ta, sa, rv, pv = t0.clone(), s0.clone(), _rows(row), _rows(prev)               # (the row vectors outlive the raw call below)
    ref = e['p'].saga_step(e['z'], bits, b.YT, ta, rv, pv, sa, LR, 1.0 / HIST, alpha=1.0 / MB, xrec=b.xrec, sigma_modifier=SM)[0]
    tb, sb_, out3 = t0.clone(), s0.clone(), torch.empty_like(ref)
    N.call('pnp_csmri_saga_step_pp', e['p']._h, P(e['z']), P(bits), P(b.YT), 1.0 / MB, None, None, P(tb), P(rv), P(pv), P(sb_),
           LR, None, 1.0 / HIST, HIST, P(out3), 1, SM, None, 0.0, P(b.xrec), None, P(sig2), ops._stream())
    assert torch.equal(out3, ref) and torch.equal(tb, ta) and torch.equal(sb_, sa)


def test_argument_checks_on_the_device(env):
    """ValueError from the front end and PNP_ERR_ARG from the library on real plans of the wrong size or type, and on table / sum
    that overlap the images; nothing is launched."""
    from pnp_svrg_amd import _native as N, ops
    e = env
    b, bits = e['batch'], e['sel']['mid']
    with pytest.raises(ValueError, match='exactly one'):
        e['p'].grad_step(e['z'], bits, c1=e['z'])
    with pytest.raises(ValueError, match='exactly one'):
        e['p'].grad_step(e['z'], bits, yh=b.yh_full, YT=b.YT, c1=e['z'])
    small = torch.zeros((1, 128, 128), device='cuda')
    with pytest.raises(ValueError, match='256 x 256'):
        ops.CsmriPlan(128, 128, 1, torch.float32).grad_step(small, torch.zeros((1, 128, 4), dtype=torch.int32, device='cuda'), c1=small)
    h, P = N.lib(), ops._p
    table, tsum = _saga_state(e, HIST)
    p128, p64 = ops.CsmriPlan(128, 128, 1, torch.float32), ops.CsmriPlan(256, 256, 1, torch.float64)
    out = torch.empty_like(e['z'])
    ok = [e['p']._h, P(e['z']), P(bits), P(b.YT), 1e-3, None, P(table), P(_rows([0, 1, 2])), P(_rows([0, 0, 0])), P(tsum), LR, 0.25, HIST,
          P(out), 1, 1.0, 0.0, P(b.xrec), None, None, None]
    inside = torch.empty((HIST + 1, B, 256, 256), device='cuda')
    bad = {'128 plan': {0: p128._h}, 'f64 plan': {0: p64._h}, 'table is z': {6: P(e['z'])}, 'sum is out': {9: P(out)},
           'sum is xrec': {9: P(b.xrec)}, 'sum inside table': {6: P(inside), 9: P(inside[HIST - 1])}, 'z inside table': {6: P(inside), 1: P(inside[1])},
           'hist 0': {12: 0}}
    for what, change in bad.items():
        args = list(ok)
        for pos, val in change.items():
            args[pos] = val
        assert h.pnp_csmri_saga_step(*args) == 1, what
        assert h.pnp_last_error().decode(), what
    assert h.pnp_csmri_grad_step(p128._h, P(e['z']), P(bits), None, P(b.YT), 1.0, None, 1.0, P(e['z']), P(out), 1, 1.0, 0.0, None, None, None,
                                 None) == 1


# -------------------------------------------------------------------------------------------------------------------- engines
def _mk_prox(kind):
    from pnp_svrg_amd.engine import TVProx, DnCNNProx
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    if kind == 'tv':
        return TVProx(sigma_modifier=1.1), 2e3
    return DnCNNProx(random_dncnn_weights(17, seed=1), 15), 1.0


@pytest.mark.parametrize('algo,prox_kind', [('gd', 'tv'), ('sgd', 'tv'), ('saga', 'tv'), ('sgd', 'dncnn')])
def test_fused_engine_equals_streaming_engine(algo, prox_kind):
    """fused=True walks the trajectory of the streaming engine: device draws and host index lists (per-problem SAGA rows with the
    lists), 9 steps; |z_f - z_u| <= 5e-5 * max(1, |z|), every PSNR within 0.01 dB.  The DnCNN case goes through denoise == 0."""
    from pnp_svrg_amd.engine import CsmriBatch, make_engine
    steps = 9
    batch = CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=13)
    rs = np.random.default_rng(8).integers(0, HIST, size=(steps, B))
    for host in ((False, True) if (prox_kind == 'tv' and algo != 'gd') else (False,)):
        (pf, eta), (pu, _) = _mk_prox(prox_kind), _mk_prox(prox_kind)
        kw = dict(algorithm=algo, hist_size=HIST, seed=4)
        ef = make_engine(batch, pf, eta, None, MB, fused=True, **kw)
        eu = make_engine(batch, pu, eta, None, MB, **kw)
        assert ef.fused and not eu.fused
        idx = batch.draw_minibatches(steps, MB, seed=2) if host else None
        for s in range(steps):
            for eng in (ef, eu):
                if algo == 'gd':
                    eng.step()
                elif algo == 'saga':
                    eng.step(None if idx is None else idx[s], r=rs[s] if host else int(rs[s, 0]))
                else:
                    eng.step(None if idx is None else idx[s])
        dz, bound = (ef.z - eu.z).abs().max().item(), 5e-5 * max(1.0, eu.z.abs().max().item())
        tf, tu = ef.psnr_trace(), eu.psnr_trace()
        print(f'[{algo}, {prox_kind}, host={host}] |z_f - z_u| = {dz:.3e} (bound {bound:.3e}), PSNR {np.abs(tf - tu).max():.4f} dB')
        assert tf.shape == tu.shape == (steps, B) and (ef.s, ef.n_prox) == (eu.s, eu.n_prox) == (steps, steps)
        assert dz <= bound
        assert np.abs(tf - tu).max() <= 0.01 + 1e-9
        assert prox_kind != 'tv' or ef.prox.t == eu.prox.t == steps
        if algo == 'saga':
            assert (ef.tsum - eu.tsum).abs().max().item() <= 5e-5 * max(1.0, eu.tsum.abs().max().item())
            assert (ef.table - eu.table).abs().max().item() <= 5e-5 * max(1.0, eu.table.abs().max().item())


def test_per_problem_values_equal_scalar_engines():
    """1 item x 3 trials on a tiled batch with per-problem eta, mini_batch_size and sigma_modifier under fused=True == three scalar
    fused engines, bit for bit on z and on every log row (sgd and saga, lr_decay != 1)."""
    from pnp_svrg_amd.engine import CsmriBatch, TVProx, make_engine
    steps = 4
    one = CsmriBatch.synthetic(1, 256, 256, 0.2, 20.0, seed=19)
    eta, mb, sm = np.array([1.5e3, 2e3, 2.5e3]), np.array([800, 1000, 1300], np.int32), np.array([0.9, 1.1, 1.4])
    for algo in ('sgd', 'saga'):
        kw = dict(algorithm=algo, hist_size=3, lr_decay=0.9, seed=6, fused=True)
        e = make_engine(one.tile(3), TVProx(sigma_modifier=sm), eta, None, mb, draw_id=[0, 0, 0], **kw)
        step = (lambda en, s: en.step(r=s % 3)) if algo == 'saga' else (lambda en, s: en.step())
        for s in range(steps):
            step(e, s)
        for k in range(3):
            r = make_engine(one, TVProx(sigma_modifier=float(sm[k])), float(eta[k]), None, int(mb[k]), **kw)
            for s in range(steps):
                step(r, s)
            assert torch.equal(e.z[k], r.z[0]) and torch.equal(e.sse_log[:steps, k], r.sse_log[:steps, 0]), (algo, k)
        assert not torch.equal(e.z[0], e.z[1])


@pytest.mark.parametrize('algo', ['gd', 'sgd', 'saga'])
def test_fused_runner_against_the_oracle_loops(algo):
    """Two legacy-seeded items (sampling ratios 0.2 and 0.3) through make_runner(fused_steps=True), each against oracle.loops.pnp_gd /
    pnp_sgd / pnp_saga on the same seeds: every PSNR within 0.01 dB, |z - z_ref| <= 1e-3 (the bounds of
    test_fused_engine_against_the_oracle_loop in test_gpu_sarah_fused.py)."""
    from pnp_svrg_amd import sweep
    from oracle import denoise as od, loops as ol, problems as op
    n_it, eta = 5, 2e3
    rng = np.random.default_rng(3)
    imgs = [np.cumsum(np.cumsum(rng.standard_normal((256, 256)), 0), 1) for _ in range(2)]
    items = [{'id': 0, 'image': 0, 'alpha': 0.2, 'snr': 20.0, 'seed': 0}, {'id': 1, 'image': 1, 'alpha': 0.3, 'snr': 20.0, 'seed': 5}]
    run = sweep.make_runner(imgs, 'csmri', algo, 'tv', eta=eta, n_inner=n_it, mini_batch_size=MB, hist_size=HIST, seeding='legacy',
                            keep_trace=True, fused_steps=True)
    res = sweep.run_sweep(items, run)
    for it, r in zip(items, res):
        np.random.seed(it['seed'])
        p = op.CSMRI(None, H=256, W=256, sample_prob=it['alpha'], snr=it['snr'], img=imgs[it['image']])
        np.random.seed(1)
        kw = dict(converge_check=False, clock=ol.CountingClock())
        if algo == 'gd':
            ro = ol.pnp_gd(p, od.TVDenoiser(), eta, 6 * n_it - 3, **kw)
        elif algo == 'sgd':
            ro = ol.pnp_sgd(p, od.TVDenoiser(), eta, 5 * n_it - 2, MB, **kw)
        else:
            ro = ol.pnp_saga(p, od.TVDenoiser(), eta, 5 * n_it - 1, MB, hist_size=HIST, **kw)
        ref = np.array(ro['psnr_per_iter'])
        assert len(ref) == n_it + 1
        dp, dz = np.abs(np.asarray(r['psnr_trace']) - ref[1:]).max(), np.abs(np.asarray(r['z']).ravel() - ro['z']).max()
        print(f'[{algo}, item {it["id"]}] PSNR vs oracle: {dp:.4f} dB; |z - z_ref| = {dz:.3e}')
        assert dp <= 0.01 + 1e-9 and dz <= 1e-3


def test_trial_batched_saga_grid():
    """make_runner(fused_steps=True, wide_trials=True), algorithm='saga': 2 items x 2 trials as one tiled batch against the per-trial
    runs of the same runner -- item i walks in every trial the trajectory the per-trial runner gives it (psnr_final within 0.01 dB) --
    and against the streaming runner."""
    from pnp_svrg_amd import sweep
    rng = np.random.default_rng(3)
    imgs = [np.cumsum(np.cumsum(rng.standard_normal((256, 256)), 0), 1) for _ in range(2)]
    items = [{'id': 0, 'image': 0, 'alpha': 0.2, 'snr': 20.0, 'seed': 0}, {'id': 1, 'image': 1, 'alpha': 0.3, 'snr': 20.0, 'seed': 1}]
    trials = [{'eta': 1.5e3}, {'eta': 2e3, 'mini_batch_size': 800, 'sigma_modifier': 1.2}]
    mk = lambda fused, **kw: sweep.make_runner(imgs, problem='csmri', algorithm='saga', denoiser='tv', n_inner=6, hist_size=HIST,   # noqa: E731
                                               seeding='counter', wide_trials=True, fused_steps=fused,
                                               **{'eta': 2e3, 'mini_batch_size': MB, **kw})
    grid = {f: mk(f).run_trials(mk(f).prepare_data(items), trials) for f in (True, False)}
    for t, tr in enumerate(trials):
        per_trial = mk(True, **tr)(items)
        for a, b, c in zip(grid[True][t], per_trial, grid[False][t]):
            assert a.keys() == c.keys() and a['id'] == b['id'] == c['id']
            assert abs(a['psnr_final'] - b['psnr_final']) <= 0.01 + 1e-9, (t, a['psnr_final'], b['psnr_final'])
            assert abs(a['psnr_final'] - c['psnr_final']) <= 0.01 + 1e-9, (t, a['psnr_final'], c['psnr_final'])
