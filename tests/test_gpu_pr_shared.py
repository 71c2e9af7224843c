"""pnp_pr_grad_shared (csrc/pr_shared.hip): G trials of `items` phase-retrieval problems on the items' shared matrices, against
the per-problem kernel of pr.hip on materialised copies of A, and the layers above it (PrBatch.tile, the engines, the grid).

Inputs: Gaussian A, Y = |A x| + a little noise, W and W2 near x.  The amplitude weight ((|t| - y) / |t|) t jumps where t = A w
crosses zero, so rows that come within 1e-3 of the median |t| for ANY vector of the case are redrawn from the same stream when the
inputs are built (with 10^5 products per case no seed avoids them all), and every case asserts the condition on what it uses."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 12, 77), (7, 15, 40), (16, 16, 320), (32, 32, 2048)]
GMAX = 17
NPDT = {torch.float32: np.float32, torch.float64: np.float64}


@functools.lru_cache(maxsize=None)
def _inputs(H, W, M, items):
    """float64 NumPy: A [items, M, N], x [items, N], Y [items, M], W, W2 [GMAX * items, N] (problem b = t * items + i)."""
    N = H * W
    rng = np.random.default_rng(1000 * M + 10 * N + items)
    x = rng.random((items, N))
    B = GMAX * items
    Wz = x[np.arange(B) % items] * (1 + 0.03 * rng.standard_normal((B, N)))
    Ww = x[np.arange(B) % items] * (1 + 0.03 * rng.standard_normal((B, N)))
    A = rng.standard_normal((items, M, N))
    for i in range(items):
        V = np.concatenate([Wz[i::items], Ww[i::items], x[i:i + 1]])          # every vector that meets A[i]
        for _ in range(100):
            t = np.abs(A[i] @ V.T)
            bad = np.flatnonzero(t.min(1) < 4e-3 * np.median(t))
            if bad.size == 0:
                break
            A[i, bad] = rng.standard_normal((bad.size, N))
    Y = np.abs(np.einsum('imn,in->im', A, x)) * (1 + 0.01 * rng.standard_normal((items, M)))
    for a in (A, Y, Wz, Ww):
        a.setflags(write=False)
    return A, Y, Wz, Ww


def _case(shape, items, G, dtype):
    """The first G trials of the case in `dtype` on the device + the same values (as rounded to dtype) in float64 NumPy."""
    A, Y, Wz, Ww = _inputs(*shape, items)
    B = G * items
    host = [np.ascontiguousarray(a.astype(NPDT[dtype])) for a in (A, Y, Wz[:B], Ww[:B])]
    dev = [torch.from_numpy(a).cuda() for a in host]
    h64 = [a.astype(np.float64) for a in host]
    t = np.abs(np.concatenate([h64[0][i] @ np.concatenate([h64[2][i::items], h64[3][i::items]]).T for i in range(items)]))
    assert t.min() >= 1e-3 * np.median(t), 'input condition: a product A w too close to zero'
    return dev, h64


def _np_grad(A, Y, Wv, sel, items):
    """float64: g_b(W[b]) over the rows sel[b] (bool [B, M]) for every problem."""
    out = np.empty_like(Wv)
    for b in range(Wv.shape[0]):
        Ai, y = A[b % items][sel[b]], Y[b % items][sel[b]]
        t = Ai @ Wv[b]
        out[b] = Ai.T @ (((np.abs(t) - y) / np.abs(t)) * t)
    return out


def _existing(A, Y, Wv, rows_of, items):
    """pnp_pr_grad_batch on a materialised copy of A per problem.  rows_of: None (all rows), or [(problem indices, rows)] groups."""
    from pnp_svrg_amd import ops
    B = Wv.shape[0]
    idx = torch.arange(B, device=A.device) % items
    Ar, Yr = A[idx].contiguous(), Y[idx].contiguous()
    if rows_of is None:
        return ops.pr_grad_batch(Ar, Wv, Yr)
    out = torch.empty_like(Wv)
    for pick, rows in rows_of:
        out[pick] = ops.pr_grad_batch(Ar[pick].contiguous(), Wv[pick].contiguous(), Yr[pick].contiguous(), rows=rows)
    return out


def _draw(M, B, mb, seed=7, step=3):
    """One step's descriptors for B problems (mb: an int or [B] ints), the indicator, and the row-list groups of `_existing`."""
    from pnp_svrg_amd import ops
    if np.ndim(mb) == 0:
        mbd = ops.draw_thresholds(M, B, int(mb), seed, step)[0]
        groups = [(torch.arange(B, device='cuda'), ops.rows_from_thresholds(M, int(mb), mbd))]
    else:
        mbv = np.asarray(mb, np.int32)
        mbd = ops.draw_thresholds(M, B, torch.from_numpy(mbv).cuda(), seed, step)[0]
        groups = []
        for v in np.unique(mbv):
            pick = torch.from_numpy(np.flatnonzero(mbv == v)).cuda()
            groups.append((pick, ops.rows_from_thresholds(M, int(v), mbd[pick].contiguous())))
    return mbd, ops.indicator_from_thresholds(M, mbd), groups


def _bound(got, yard, ref64, dtype, what):
    """f64: within 1e-12 max(1, max|ref|) of the existing kernel.  f32: the error against the float64 evaluation is at most 4 x the
    existing f32 kernel's error against it."""
    got, yard = got.double().cpu().numpy(), yard.double().cpu().numpy()
    e_new, e_old = np.abs(got - ref64).max(), np.abs(yard - ref64).max()
    print(f'{what} {str(dtype)[6:]}: shared-kernel error {e_new:.3e}, existing kernel {e_old:.3e}, max|ref| {np.abs(ref64).max():.3e}')
    if dtype == torch.float64:
        assert np.abs(got - yard).max() <= 1e-12 * max(1.0, np.abs(yard).max()), what
    else:
        assert e_new <= 4 * e_old, (what, e_new, e_old)


# ------------------------------------------------------------------------------------------- 1. against the existing kernel
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('items', [1, 2])
@pytest.mark.parametrize('G', [1, 3, 16, 17])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_against_the_existing_kernel(shape, G, items, dtype):
    from pnp_svrg_amd import ops
    (A, Y, Wz, Ww), (A64, Y64, Wz64, Ww64) = _case(shape, items, G, dtype)
    M, B = shape[2], G * items
    full = np.ones((B, M), bool)
    # grad_full: all rows, 1 / M
    got = ops.pr_grad_shared(A, Y, Wz, alpha_div=M)
    _bound(got, _existing(A, Y, Wz, None, items) / M, _np_grad(A64, Y64, Wz64, full, items) / M, dtype, 'full')
    # device draws: a scalar mb, then per-problem mb; one vector and the difference of two
    mbs = [max(1, M // 3), (np.arange(B) % 3 + 1) * max(1, M // 4)]
    for k, mb in enumerate(mbs):
        mbd, ind, groups = _draw(M, B, mb)
        sel = ind.cpu().numpy().astype(bool)
        assert (sel.sum(1) == np.broadcast_to(mb, (B,))).all()
        gz, gw = _existing(A, Y, Wz, groups, items), _existing(A, Y, Ww, groups, items)
        rz, rw = _np_grad(A64, Y64, Wz64, sel, items), _np_grad(A64, Y64, Ww64, sel, items)
        _bound(ops.pr_grad_shared(A, Y, Wz, mbd=mbd), gz, rz, dtype, f'stoch{k}')
        _bound(ops.pr_grad_shared(A, Y, Wz, Ww, mbd=mbd), gz - gw, rz - rw, dtype, f'diff{k}')


# ------------------------------------------------------------------------------------------- 2. mbd path == ind path
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape,G,items', [(SHAPES[0], 17, 2), (SHAPES[1], 3, 1), (SHAPES[2], 16, 2), (SHAPES[3], 17, 1)])
def test_descriptors_equal_indicator(shape, G, items, dtype):
    from pnp_svrg_amd import ops
    (A, Y, Wz, Ww), _ = _case(shape, items, G, dtype)
    M, B = shape[2], G * items
    mbd, ind, _ = _draw(M, B, (np.arange(B) % 4 + 1) * max(1, M // 5))
    assert torch.equal(ops.pr_grad_shared(A, Y, Wz, Ww, mbd=mbd), ops.pr_grad_shared(A, Y, Wz, Ww, ind=ind))
    assert torch.equal(ops.pr_grad_shared(A, Y, Wz, mbd=mbd), ops.pr_grad_shared(A, Y, Wz, ind=ind))
    with pytest.raises(Exception, match='both selections'):
        ops.pr_grad_shared(A, Y, Wz, mbd=mbd, ind=ind)


# ------------------------------------------------------------------------------------------- 3. composition invariance
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_problem_does_not_depend_on_the_batch(shape, dtype):
    from pnp_svrg_amd import ops
    items, M = 2, shape[2]
    (A, Y, Wz, Ww), _ = _case(shape, items, GMAX, dtype)
    mbd, ind, _ = _draw(M, GMAX * items, (np.arange(GMAX * items) % 4 + 1) * max(1, M // 5))
    for t, i in [(0, 0), (2, 1), (16, 0)]:
        b = t * items + i
        pick = lambda v, bs: v[bs].contiguous()
        # alone: G = 1 on the one matrix it uses
        one = ops.pr_grad_shared(A[i:i + 1].contiguous(), Y[i:i + 1].contiguous(), Wz[b:b + 1], Ww[b:b + 1], ind=ind[b:b + 1])
        # in G = 17 where it is; in G = 3 at trial 1 among other problems; with the others' selections changed
        g17 = ops.pr_grad_shared(A, Y, Wz, Ww, mbd=mbd)
        assert torch.equal(g17[b], one[0]), (t, i)
        bs = [6, 7, 8, 9, 10, 11]
        bs[2 + i] = b                                                     # trial 1, item i
        g3 = ops.pr_grad_shared(A, Y, pick(Wz, bs), pick(Ww, bs), ind=pick(ind, bs))
        assert torch.equal(g3[2 + i], one[0]), (t, i)
        other, rest = ind.clone(), torch.arange(GMAX * items, device='cuda') != b
        other[rest] = 1 - other[rest]
        assert torch.equal(ops.pr_grad_shared(A, Y, Wz, Ww, ind=other)[b], one[0]), (t, i)
        # a non-selected row may hold anything finite: its weight is written as 0
        row = int(np.flatnonzero(ind[b].cpu().numpy() == 0)[0])
        A2 = A.clone()
        A2[i, row] = 1e6
        assert torch.equal(ops.pr_grad_shared(A2, Y, Wz, Ww, ind=ind)[b], one[0]), (t, i)
        assert torch.equal(ops.pr_grad_shared(A2, Y, Wz, Ww, mbd=mbd)[b], one[0]), (t, i)
    assert not torch.equal(g17[0], g17[items])


# ------------------------------------------------------------------------------------------- 4. epilogue
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape,G,items', [(SHAPES[1], 3, 2), (SHAPES[3], 16, 1)])
def test_epilogue(shape, G, items, dtype):
    from pnp_svrg_amd import ops
    (A, Y, Wz, Ww), (A64, Y64, Wz64, Ww64) = _case(shape, items, G, dtype)
    M, B = shape[2], G * items
    mbd, ind, groups = _draw(M, B, max(1, M // 3))
    sel = ind.cpu().numpy().astype(bool)
    rng = np.random.default_rng(5)
    c1, c2 = (torch.from_numpy(rng.random(Wz.shape).astype(NPDT[dtype])).cuda() for _ in range(2))     # (iterates: in [0, 1))
    alpha_v, gamma_v = -1.0 / (1 + np.arange(B) % 3), 0.25 * (1 + np.arange(B) % 3)
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    g = (_existing(A, Y, Wz, groups, items) - _existing(A, Y, Ww, groups, items)).double()       # the un-fused result
    r = _np_grad(A64, Y64, Wz64, sel, items) - _np_grad(A64, Y64, Ww64, sel, items)
    c164, c264 = c1.double().cpu().numpy(), c2.double().cpu().numpy()
    for name, al, ga in [('scalar', -0.8, 0.7), ('per-problem', alpha_v, gamma_v)]:
        a_d, g_d = (dv(al), dv(ga)) if np.ndim(al) else (al, ga)
        col = lambda v: np.reshape(v, (-1, 1)) if np.ndim(v) else v
        tcol = lambda v: dv(v).reshape(-1, 1) if np.ndim(v) else v
        yard = tcol(al) * g + 1.0 * c1.double() + tcol(ga) * c2.double()
        ref = col(al) * r + 1.0 * c164 + col(ga) * c264
        got = ops.pr_grad_shared(A, Y, Wz, Ww, mbd=mbd, alpha=a_d, beta=1.0, c1=c1, gamma=g_d, c2=c2)
        _bound(got, yard, ref, dtype, 'epilogue ' + name)
    # the engines' out=z, c1=z: W is read before anything is stored
    z = Wz.clone()
    ops.pr_grad_shared(A, Y, z, Ww, mbd=mbd, alpha=dv(alpha_v), beta=1.0, c1=z, gamma=0.7, c2=c2, out=z)
    assert torch.equal(z, ops.pr_grad_shared(A, Y, Wz, Ww, mbd=mbd, alpha=dv(alpha_v), beta=1.0, c1=Wz, gamma=0.7, c2=c2))
    # grad_full's 1 / M: the quotient of the per-problem value equals the scalar's
    assert torch.equal(ops.pr_grad_shared(A, Y, Wz, alpha=dv(np.full(B, -0.3)), alpha_div=M), ops.pr_grad_shared(A, Y, Wz, alpha=-0.3, alpha_div=M))


# ------------------------------------------------------------------------------------------- 5. engines on a tiled batch
def _pr_batch(dtype, items=2, shape=SHAPES[3]):
    from pnp_svrg_amd.engine import PrBatch
    H, W, M = shape
    A, Y, _, _ = _inputs(H, W, M, items)
    x = np.random.default_rng(1000 * M + 10 * H * W + items).random((items, H * W))      # (the x of `_inputs`: its stream's first draw)
    xinit = np.clip(x * (1 + 0.2 * np.random.default_rng(3).standard_normal(x.shape)), 0, 1)
    return PrBatch(x.reshape(items, H, W), A, Y, xinit, dtype=dtype)


_ETA, _MB = np.array([0.3, 0.15, 0.05]), np.array([512, 1024, 256], np.int32)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('algo', ['gd', 'sgd', 'svrg'])
def test_engines_on_a_tiled_batch(algo, dtype):
    from pnp_svrg_amd.engine import make_engine, TVProx
    base, ni, steps = _pr_batch(dtype), 2, 8
    tiled = base.tile(3)
    assert tiled.A.data_ptr() == base.A.data_ptr() and tiled.B == 6 and tiled.per_problem and not base.per_problem
    eng = make_engine(tiled, TVProx(), np.repeat(_ETA, ni), 4, np.repeat(_MB, ni), algorithm=algo, seed=5, draw_id=np.tile(np.arange(ni), 3))
    for _ in range(steps):
        eng.step()
    z, tr = eng.z.clone(), eng.psnr_trace()
    for t in range(3):
        ref = make_engine(base, TVProx(), float(_ETA[t]), 4, int(_MB[t]), algorithm=algo, seed=5)
        for _ in range(steps):
            ref.step()
        zr, trr = ref.z, ref.psnr_trace()
        print(algo, dtype, t, 'max |dz|', float((z[t * ni:(t + 1) * ni] - zr).abs().max()), 'max |dPSNR|', np.abs(tr[:, t * ni:(t + 1) * ni] - trr).max())
        if dtype == torch.float64:
            assert np.array_equal(tr[:, t * ni:(t + 1) * ni], trr), (algo, t)
            assert float((z[t * ni:(t + 1) * ni] - zr).abs().max()) <= 1e-10 * float(zr.abs().max()), (algo, t)
        else:
            assert np.abs(tr[:, t * ni:(t + 1) * ni] - trr).max() <= 0.01 + 1e-9, (algo, t)
    assert not torch.equal(z[0], z[ni])


def test_untiled_and_deblur_batches_still_refuse_per_problem_values():
    from pnp_svrg_amd.engine import GdEngine, SgdEngine, TVProx
    base = _pr_batch(torch.float32)
    with pytest.raises(ValueError, match="on a CsmriBatch.*'pr'"):
        GdEngine(base, TVProx(), np.array([0.1, 0.2]))
    with pytest.raises(ValueError, match="need a CsmriBatch.*'pr'"):
        SgdEngine(base, TVProx(), 0.1, np.array([5, 6], np.int32))


# ------------------------------------------------------------------------------------------- 6. grid
def _images(k, n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
def test_grid_search_on_shared_matrices(dtype, monkeypatch):
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import PrBatch
    imgs = _images(2, 16)
    items = sweep.make_items(2, [4.0], [30.0])
    mk = functools.partial(sweep.make_runner, imgs, 'pr', 'svrg', 'tv', n_inner=8, H=16, W=16, dtype=dtype, seeding='counter',
                           shared_matrix=True)
    grid = {'eta': [0.4, 0.05], 'mini_batch_size': [256, 700], 'T2': [2, 4]}
    serial = sweep.grid_search(items, mk, grid)
    seen, real = [], PrBatch.tile
    monkeypatch.setattr(PrBatch, 'tile', lambda self, n: (lambda t: (seen.append((n, t.A.data_ptr() == self.A.data_ptr())), t)[1])(real(self, n)))
    batched = sweep.grid_search(items, mk, grid, batch_trials=True, max_batch_trials=6)       # 3 of a group's 4 trials per slab
    assert seen and all(same for _, same in seen) and {n for n, _ in seen} == {3, 1}
    assert [(r['id'], r['params']) for r in batched] == [(r['id'], r['params']) for r in serial]
    for rb, rs in zip(batched, serial):
        print(dtype, rb['id'], rb['params'], rb['loss'], rs['loss'])
        if dtype == torch.float64:
            assert rb['loss'] == rs['loss'] and rb['psnr_final'] == rs['psnr_final']
        else:
            assert abs(rb['loss'] - rs['loss']) <= 0.01 + 1e-9
    with pytest.raises(ValueError, match='shared_matrix=True'):
        sweep.grid_search(items, functools.partial(sweep.make_runner, imgs, 'pr', 'svrg', 'tv', n_inner=8, H=16, W=16, seeding='counter'),
                          grid, batch_trials=True)


# ------------------------------------------------------------------------------------------- 7. graph capture
def test_graph_replay_equals_eager_steps():
    from pnp_svrg_amd.engine import SvrgEngine, TVProx
    tiled, ni = _pr_batch(torch.float32).tile(3), 2
    mk = lambda: SvrgEngine(tiled, TVProx(), np.repeat(_ETA, ni), 4, np.repeat(_MB, ni), seed=5, draw_id=np.tile(np.arange(ni), 3))
    eager, graph = mk(), mk()
    assert graph.graph_ok()
    for _ in range(8):
        eager.step()
    graph.run_outer(2, one_launch=False)
    torch.cuda.synchronize()
    assert torch.equal(graph.z, eager.z) and np.array_equal(graph.psnr_trace(), eager.psnr_trace())
