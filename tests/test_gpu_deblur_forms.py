"""Every form of the Deblur / super-resolution operator family (csrc/deblur.hip, csrc/deblur_mixed.hip, ops.DeblurPlan and
DeblurPlan.mixed) against the float64 reference of tests/deblur_ref.py, piece by piece: the forward blur, the adjoint blur
(conjugated spectrum), the 4-tap down-sampler and its CSR adjoint behind an identity blur, the whole gradient with its three
selector forms and both scale forms, the selector's edges, non-square images, the adjoint identity, a mixed-scale plan, and the
table checks of pnp_deblur_plan_create.  Plans are built directly on synthetic data (deblur_ref.images / problem): a sparse
asymmetric kernel whose taps cross both digits of the four-step index, a dense one, unit impulses, and the plane waves at the
edges of the line transform's <RA, LA> split.  Batches of 1 to 3 (5 in the mixed plan), one launch each, nothing iterates.

Bounds, in the metric of deblur_ref (max|o - ref| / S, S the largest magnitude the last blur can produce): float64 1e-11;
float32 4 * e32, e32 being the float32 error of the reference operation itself, measured on the CPU for the size, scale and
kernel of the case (tests/test_cpu_deblur_ref.py holds it below 2e-4 / 4).  A float32 case feeds the reference the float32
roundings of its inputs.  Non-square images run at scale_percent 100 only (tests/test_cpu_deblur_ref.py, module docstring).
Every figure is printed before it is asserted."""
import gc

import numpy as np
import pytest
import torch

import deblur_ref as dr

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
DTYPES = pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
SIDES = pytest.mark.parametrize('n', [64, 128, 256])
SCALE, SCALE_PP = 0.37, [0.37, -1.5, 2.25e-3]


@pytest.fixture(autouse=True)
def _free_plans():
    yield
    gc.collect()
    torch.cuda.synchronize()


def _bound(dtype, H, W, scale, kname):
    return dr.F64_BOUND if dtype == F64 else dr.f32_bound(H, W, scale, kname)


def _rounded(a, dtype):
    """The values the kernels see, as float64."""
    return np.asarray(a, NP[dtype]).astype(np.float64)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, NP[dtype])).cuda()


def _host(t):
    return t.double().cpu().numpy()


def _plan(H, W, B, dtype, kname, scale):
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.problems import _deblur_taps
    return ops.DeblurPlan(H, W, B, dtype, dr.kernel(kname, H * W).Bk, bilinear=_deblur_taps(H, W, scale))


def _check(what, got, ref, S, bound):
    assert np.isfinite(got).all(), what
    e = dr.err(got, ref, S)
    print(f'{what}: err {e:.3e} (bound {bound:.3e})')
    assert e <= bound, (what, e, bound)


def _in_threes(fn, x, dtype):
    """fn over the rows of x, three to a launch -> stacked host result."""
    out = [fn(_dev(x[i:i + 3], dtype)).reshape(3, -1).clone() for i in range(0, x.shape[0], 3)]
    return _host(torch.cat(out))


# ------------------------------------------------------------------------------------------------------------ 1, 2: the blurs
@pytest.mark.parametrize('kname', ['edge', 'dense'])
@DTYPES
@SIDES
def test_forward_blur_alone(n, dtype, kname):
    N = n * n
    kern, x = dr.kernel(kname, N), _rounded(dr.images(N), dtype)
    plan = _plan(n, n, 3, dtype, kname, 100)
    got = _in_threes(plan.forward, x, dtype)
    _check(f'forward {n} {kname}', got, kern.fwd(x), kern.span(x), _bound(dtype, n, n, 100, kname))


@pytest.mark.parametrize('kname', ['edge', 'dense'])
@DTYPES
@SIDES
def test_adjoint_blur_alone(n, dtype, kname):
    """grad(z = 0, Y = -r, scale = 1) at scale 100 is B^T r: the conjugated-spectrum path with nothing before it."""
    N = n * n
    kern, r = dr.kernel(kname, N), _rounded(dr.images(N), dtype)
    plan = _plan(n, n, 3, dtype, kname, 100)
    zero = torch.zeros((3, N), dtype=dtype, device='cuda')
    got = _in_threes(lambda y: plan.grad(zero, -y, scale=1.0), r, dtype)
    _check(f'adjoint {n} {kname}', got, kern.adj(r), kern.span(r), _bound(dtype, n, n, 100, kname))


# ------------------------------------------------------------------------------------------------------------ 3: the down-sampler
@pytest.mark.parametrize('n,scale', [(n, s) for n in (64, 128, 256) for s in (50, 75)] + [(64, 2)])
@DTYPES
def test_down_sampler_alone(n, scale, dtype):
    """Behind the identity blur: forward is k_gather4 alone, grad(z = 0, Y = -r) is k_csr alone."""
    N = n * n
    p = dr.problem(n, n, scale, 'identity')
    kern, pts, M = p['kern'], p['pts'], p['M']
    assert M == {50: N // 4, 75: (3 * n // 4) ** 2, 2: 1}[scale]
    bound = _bound(dtype, n, n, scale, 'identity')
    plan = _plan(n, n, 3, dtype, 'identity', scale)
    assert plan.M == M
    x = _rounded(dr.images(N)[:9], dtype)
    got = _in_threes(plan.forward, x, dtype)
    assert got.shape == (9, M)
    _check(f'down {n} {scale}', got, dr.down(x, pts, n, n), kern.span(x), bound)
    r = _rounded(p['r'], dtype)
    got = _host(plan.grad(torch.zeros((3, N), dtype=dtype, device='cuda'), _dev(-r, dtype), scale=1.0))
    ref = dr.up(r, pts, n, n)
    _check(f'up {n} {scale}', got, ref, kern.span(ref), bound)


# ------------------------------------------------------------------------------------------------------------ 4: the whole gradient
def _gradient_case(H, W, scale, dtype, kname, what):
    from pnp_svrg_amd import ops
    p = dr.problem(H, W, scale, kname)
    kern, pts, M, N = p['kern'], p['pts'], p['M'], p['N']
    z, Y = _rounded(p['z'], dtype), _rounded(p['Y'], dtype)
    bound = _bound(dtype, H, W, scale, kname)
    plan = _plan(H, W, 3, dtype, kname, scale)
    zd, Yd = _dev(z, dtype), _dev(Y, dtype)
    _check(f'{what} forward', _host(plan.forward(zd)).reshape(3, M), dr.forward(z, kern, pts, H, W), kern.span(z), bound)
    mbd = ops.draw_thresholds(M, 3, max(M // 4, 1), 11, 2)[0].contiguous()
    sel = ops.indicator_from_thresholds(M, mbd)
    sel_np = sel.cpu().numpy()
    assert (sel_np.sum(axis=1) == max(M // 4, 1)).all()
    for sc, sc_dev in ((SCALE, SCALE), (SCALE_PP, torch.tensor(SCALE_PP, dtype=F64, device='cuda'))):
        form = 'scalar' if sc is SCALE else 'per-problem'
        ref_all, S_all = dr.grad(z, Y, None, sc, kern, pts, H, W, parts=True)
        ref_sel, S_sel = dr.grad(z, Y, sel_np, sc, kern, pts, H, W, parts=True)
        _check(f'{what} grad all {form}', _host(plan.grad(zd, Yd, scale=sc_dev)).reshape(3, N), ref_all, S_all, bound)
        _check(f'{what} grad sel {form}', _host(plan.grad(zd, Yd, sel=sel, scale=sc_dev)).reshape(3, N), ref_sel, S_sel, bound)
        _check(f'{what} grad mbd {form}', _host(plan.grad(zd, Yd, mbd=mbd, scale=sc_dev)).reshape(3, N), ref_sel, S_sel, bound)


@pytest.mark.parametrize('kname', ['edge', 'dense'])
@pytest.mark.parametrize('scale', [100, 50])
@DTYPES
@SIDES
def test_whole_gradient(n, dtype, scale, kname):
    """No selector, `sel` and `mbd` on the same subset; a scalar scale and a [B] scale of three values; B = 3, so blockIdx.y > 0
    is read everywhere."""
    _gradient_case(n, n, scale, dtype, kname, f'{n} {scale} {kname}')


# ------------------------------------------------------------------------------------------------------------ 5: selector edges
@pytest.mark.parametrize('scale', [100, 50])
@DTYPES
def test_selector_edges(dtype, scale):
    H = W = 64
    p = dr.problem(H, W, scale, 'edge')
    kern, pts, M, N = p['kern'], p['pts'], p['M'], p['N']
    z, Y = _rounded(p['z'], dtype), _rounded(p['Y'], dtype)
    bound = _bound(dtype, H, W, scale, 'edge')
    plan = _plan(H, W, 3, dtype, 'edge', scale)
    zd, Yd = _dev(z, dtype), _dev(Y, dtype)
    none = torch.zeros((3, M), dtype=torch.uint8, device='cuda')
    g = plan.grad(zd, Yd, sel=none, scale=SCALE)
    assert torch.count_nonzero(g) == 0                           # nothing selected: exactly 0
    last = none.clone()
    last[:, M - 1] = 1
    last[1, 0] = 1                                                # (problem 1: the first and the last measurement)
    ref, S = dr.grad(z, Y, last.cpu().numpy(), SCALE, kern, pts, H, W, parts=True)
    assert (S > 0).all()
    _check(f'only M-1, scale {scale}', _host(plan.grad(zd, Yd, sel=last, scale=SCALE)).reshape(3, N), ref, S, bound)
    # non-finite Y at deselected measurements: the epilogues assign 0, they do not multiply
    sel = torch.from_numpy(dr.selection(M, 3)).cuda()
    sel[:, M - 1] = 0
    sel[:, 0] = 0
    clean = plan.grad(zd, Yd, sel=sel, scale=SCALE).clone()
    dirty = Yd.clone()
    off = (sel == 0)
    dirty[off] = float('nan')
    dirty[:, M - 1] = float('inf')
    dirty[:, 0] = float('-inf')
    g = plan.grad(zd, dirty, sel=sel, scale=SCALE)
    assert torch.isfinite(g).all() and torch.equal(g, clean)
    _check(f'non-finite Y, scale {scale}', _host(g).reshape(3, N), *dr.grad(z, Y, sel.cpu().numpy(), SCALE, kern, pts, H, W, parts=True),
           bound)


# ------------------------------------------------------------------------------------------------------------ 6: non-square
@pytest.mark.parametrize('H,W', [(32, 128), (128, 32), (64, 256)])
@DTYPES
def test_non_square(H, W, dtype):
    """H != W with H*W a supported length, scale 100 (the reference's grid leaves a non-square image below 100)."""
    _gradient_case(H, W, 100, dtype, 'edge', f'{H} x {W}')


# ------------------------------------------------------------------------------------------------------------ 7: adjoint identity
@pytest.mark.parametrize('scale', [100, 50])
@DTYPES
@SIDES
def test_adjoint_dot(n, dtype, scale):
    """<S B x, S B x> == <x, grad(x, Y = 0)>.  float64: rel 1e-11.  float32: every element of S B x is within e * S_f and every
    element of the gradient within e * S_g of the exact one (e the bound of the module docstring), so the two inner products,
    summed in float64 on the host, differ by at most e * (2 ||S B x||_1 S_f + ||x||_1 S_g), the square of the error aside."""
    N = n * n
    p = dr.problem(n, n, scale, 'edge')
    kern, pts, M = p['kern'], p['pts'], p['M']
    plan = _plan(n, n, 1, dtype, 'edge', scale)
    x = _rounded(p['z'][:1], dtype)
    xd = _dev(x, dtype)
    y = _host(plan.forward(xd)).ravel()
    g = _host(plan.grad(xd, torch.zeros((1, M), dtype=dtype, device='cuda'), scale=1.0)).ravel()
    lhs, rhs = float(np.dot(y, y)), float(np.dot(x.ravel(), g))
    if dtype == F64:
        print(f'dot {n} {scale}: {lhs!r} {rhs!r} rel {abs(lhs - rhs) / abs(lhs):.3e}')
        assert lhs == pytest.approx(rhs, rel=1e-11)
    else:
        e = _bound(dtype, n, n, scale, 'edge')
        S_f = kern.span(x)[0]
        S_g = kern.span(dr.up(dr.forward(x, kern, pts, n, n), pts, n, n))[0]
        tol = e * (2 * np.abs(y).sum() * S_f + np.abs(x).sum() * S_g)
        print(f'dot {n} {scale}: {lhs!r} {rhs!r} diff {abs(lhs - rhs):.3e} (bound {tol:.3e})')
        assert abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------------------ 8: mixed plan
MIXED_SCALES = [100, 50, 2, 75, 50]


@DTYPES
def test_mixed_plan(dtype):
    """One batch of scales [100, 50, 2, 75, 50] at 64 x 64 (M_b = 4096, 1024, 1, 2304, 1024; Mmax = 4096), Y with NaN in its
    padding m >= M_b throughout: forward (padding exactly 0), the gradient without a selector, with `sel` and with `mbd`
    (the _mpp draws, M_b = mb_b = 1 among them), and the objective, each member against the reference of its scale."""
    from pnp_svrg_amd import ops
    from pnp_svrg_amd.problems import deblur_operator_sets
    H = W = 64
    N, B = H * W, len(MIXED_SCALES)
    kern = dr.kernel('edge', N)
    sets, set_of, M_vec = deblur_operator_sets(H, W, MIXED_SCALES)
    assert M_vec.tolist() == [dr.n_meas(H, W, s) for s in MIXED_SCALES] == [4096, 1024, 1, 2304, 1024]
    plan = ops.DeblurPlan.mixed(H, W, dtype, kern.Bk, sets, set_of, M_vec)
    Mmax = plan.M
    rng = np.random.default_rng(8)
    z = _rounded(rng.normal(size=(B, N)), dtype)
    pts = [dr.bilinear_points(H, W, s) for s in MIXED_SCALES]
    Y = np.full((B, Mmax), np.nan)
    for b in range(B):
        Y[b, :M_vec[b]] = _rounded(dr.forward(rng.normal(size=N), kern, pts[b], H, W) + 0.1 * rng.normal(size=M_vec[b]), dtype)
    zd, Yd = _dev(z, dtype), _dev(Y, dtype)
    bounds = [_bound(dtype, H, W, s, 'edge') for s in MIXED_SCALES]

    fwd = _host(plan.forward(zd)).reshape(B, Mmax)
    for b in range(B):
        assert np.count_nonzero(fwd[b, M_vec[b]:]) == 0, b
        _check(f'mixed forward {b}', fwd[b, :M_vec[b]], dr.forward(z[b], kern, pts[b], H, W), kern.span(z[b]), bounds[b])

    mb = torch.tensor([1000, 300, 1, 500, 1], dtype=torch.int32, device='cuda')
    mbd = ops.draw_thresholds_mpp(plan.M_dev, mb, 21, 4)[0].contiguous()
    sel = ops.indicator_from_thresholds_m(plan.M_dev, Mmax, mbd)
    sel_np = sel.cpu().numpy()
    assert sel_np.sum(axis=1).tolist() == mb.tolist() and all(sel_np[b, M_vec[b]:].sum() == 0 for b in range(B))
    sc = torch.tensor([0.37, -1.5, 2.25e-3, 1.0, 0.5], dtype=F64, device='cuda')
    got = {'all': plan.grad(zd, Yd, scale=sc), 'sel': plan.grad(zd, Yd, sel=sel, scale=sc), 'mbd': plan.grad(zd, Yd, mbd=mbd, scale=sc),
           'all scalar': plan.grad(zd, Yd, scale=SCALE)}
    got = {k: _host(v).reshape(B, N) for k, v in got.items()}
    sc = sc.cpu().numpy()
    for b in range(B):
        Yb, Mb = Y[b:b + 1, :M_vec[b]], M_vec[b]
        for form, s_np, scale in (('all', None, sc[b]), ('sel', sel_np[b:b + 1, :Mb], sc[b]), ('mbd', sel_np[b:b + 1, :Mb], sc[b]),
                                  ('all scalar', None, SCALE)):
            ref, S = dr.grad(z[b:b + 1], Yb, s_np, scale, kern, pts[b], H, W, parts=True)
            _check(f'mixed grad {form} {b}', got[form][b:b + 1], ref, S, bounds[b])

    f = plan.objective(zd, Yd, 0.5).cpu().numpy()
    assert np.isfinite(f).all()
    for b in range(B):
        d = dr.forward(z[b], kern, pts[b], H, W) - Y[b, :M_vec[b]]
        ref = dr.objective(z[b], Y[b, :M_vec[b]], 0.5 / M_vec[b], kern, pts[b], H, W)
        delta = bounds[b] * kern.span(z[b])[0]                     # every (S B z)[m] is within delta of the exact one
        tol = 0.5 / M_vec[b] * (2 * np.abs(d).sum() * delta + M_vec[b] * delta ** 2) + 4096 * 2.0 ** -53 * ref
        print(f'mixed objective {b}: {f[b]!r} ref {ref!r} diff {abs(f[b] - ref):.3e} (bound {tol:.3e})')
        assert abs(f[b] - ref) <= tol, b


# ------------------------------------------------------------------------------------------------------------ host table checks
def test_plan_create_refuses_corrupted_tables():
    """One corrupted entry of g_idx, a_rowptr or a_col: PNP_ERR_ARG / NativeError before any allocation or launch; the tables as
    they come build a plan."""
    from pnp_svrg_amd import ops, _native
    from pnp_svrg_amd.problems import _deblur_taps
    taps = _deblur_taps(64, 64, 50)
    Bk = dr.kernel('edge', 4096).Bk
    for what, bad, msg in dr.corrupted_tables(taps, 4096):
        with pytest.raises(_native.NativeError, match=r'pnp_deblur_plan_create failed \(status 1\).*' + msg):
            ops.DeblurPlan(64, 64, 1, F64, Bk, bilinear=bad)
    assert ops.DeblurPlan(64, 64, 1, F64, Bk, bilinear=taps).M == 1024
