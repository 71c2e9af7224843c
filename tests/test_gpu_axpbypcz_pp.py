"""pnp_axpbypcz_pp against the plain call: problem p of a batch == pnp_axpbypcz on p's views with float(coef[p]), bit patterns
compared (NaNs count).  Nothing here has a tolerance: the kernel's statements are the scalar kernel's."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SHAPES = [(1, 1), (3, 5), (7, 1027), (2, 4096), (5, 64 * 64), (3, 256 * 256)]
LONG = (2, 2048 * 256 * 4 + 3)                                  # more than the capped grid covers in one stride
ARRAYS = [m for m in itertools.product((False, True), repeat=3) if any(m)]     # which of a, b, c are per problem: 7 combinations
SCALARS = (1.25, -0.3, 0.7)


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def _operand(rng, B, L, dtype, special=True):
    """[B, L] values of mixed magnitude with NaN, +-inf, -0.0 and denormals sprinkled in."""
    v = rng.standard_normal((B, L)) * 10.0 ** rng.integers(-3, 4, (B, L))
    if special:
        tiny = np.finfo(np.float32 if dtype == torch.float32 else np.float64).tiny
        flat = v.reshape(-1)
        for val in (np.nan, np.inf, -np.inf, -0.0, 0.0, tiny / 8, -tiny / 1024, tiny):
            flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = val
    return torch.from_numpy(v).to('cuda', dtype)


def _coefs(rng, B, mask):
    """a, b, c as ops.axpbypcz takes them (a float, or a float64 [B] device tensor) and their host values [3][B]."""
    dev, host = [], []
    for k, per in enumerate(mask):
        if per:
            h = rng.standard_normal(B) * 3.0 + 0.1 * np.pi       # (doubles that are no float32 values: the cast is exercised)
            dev.append(torch.from_numpy(h).cuda())
        else:
            h = np.full(B, SCALARS[k])
            dev.append(SCALARS[k])
        host.append(h)
    return dev, host


def _plain_per_problem(ops, host, x, y, w, out):
    """The reference: one plain call per problem on that problem's views."""
    for p in range(x.shape[0]):
        ops.axpbypcz(float(host[0][p]), x[p], float(host[1][p]), None if y is None else y[p], float(host[2][p]),
                     None if w is None else w[p], out=out[p])
    return out


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('B,L', SHAPES)
def test_equals_the_plain_call_per_problem(dtype, B, L):
    """Every y / w presence x every combination of array coefficients; the all-scalar `_pp` call against ONE plain call."""
    from pnp_svrg_amd import _native as N, ops
    rng = np.random.default_rng(B * 1000003 + L)
    x, y, w = (_operand(rng, B, L, dtype) for _ in range(3))
    for has_y, has_w in itertools.product((False, True), repeat=2):
        yy, ww = (y if has_y else None), (w if has_w else None)
        for mask in ARRAYS:
            dev, host = _coefs(rng, B, mask)
            want = _plain_per_problem(ops, host, x, yy, ww, torch.empty_like(x))
            got = ops.axpbypcz(dev[0], x, dev[1], yy, dev[2], ww, out=torch.full_like(x, 7.0))
            assert _same(got, want), (has_y, has_w, mask)
        # all three arrays NULL: legal, and the plain whole-batch call
        want = ops.axpbypcz(*[v for pair in zip(SCALARS, (x, yy, ww)) for v in pair], out=torch.empty_like(x))
        got = torch.full_like(x, 7.0)
        N.call('pnp_axpbypcz_pp', SCALARS[0], None, ops._p(x), SCALARS[1], None, ops._p(yy), SCALARS[2], None, ops._p(ww), ops._p(got),
               x.numel(), B, ops._DT[dtype], ops._stream())
        assert _same(got, want), (has_y, has_w, 'scalars')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_a_problem_longer_than_one_grid_stride(dtype):
    from pnp_svrg_amd import ops
    B, L = LONG
    rng = np.random.default_rng(11)
    x, y, w = (_operand(rng, B, L, dtype) for _ in range(3))
    dev, host = _coefs(rng, B, (True, True, True))
    assert _same(ops.axpbypcz(dev[0], x, dev[1], y, dev[2], w), _plain_per_problem(ops, host, x, y, w, torch.empty_like(x)))
    # the 16-byte path at a length past one stride too: the same problems without their last three elements
    L4 = L - 3
    xs, ys, ws = (t[:, :L4].contiguous() for t in (x, y, w))
    assert _same(ops.axpbypcz(dev[0], xs, dev[1], ys, dev[2], ws), _plain_per_problem(ops, host, xs, ys, ws, torch.empty_like(xs)))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('B,L', [(3, 5), (7, 1027), (5, 64 * 64)])
def test_out_may_alias_each_operand(dtype, B, L):
    from pnp_svrg_amd import ops
    rng = np.random.default_rng(L)
    src = [_operand(rng, B, L, dtype) for _ in range(3)]
    dev, host = _coefs(rng, B, (True, False, True))
    want = _plain_per_problem(ops, host, *src, torch.empty_like(src[0]))
    for k in range(3):
        x, y, w = (t.clone() for t in src)
        out = (x, y, w)[k]
        assert ops.axpbypcz(dev[0], x, dev[1], y, dev[2], w, out=out) is out
        assert _same(out, want), 'xyw'[k]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('B,L', [(3, 5), (2, 4096), (5, 64 * 64)])
def test_views_offset_by_one_element(dtype, B, L):
    """Every operand a contiguous view that starts one element into its allocation: the element-by-element path, and nothing
    outside the view is written."""
    from pnp_svrg_amd import ops
    rng = np.random.default_rng(L + 1)
    dev, host = _coefs(rng, B, (False, True, True))
    big = [_operand(rng, 1, B * L + 2, dtype).reshape(-1) for _ in range(3)]
    x, y, w = (t[1:1 + B * L].view(B, L) for t in big)
    assert all(t.data_ptr() % 16 != 0 and t.is_contiguous() for t in (x, y, w))
    buf = torch.full((B * L + 2,), 7.0, dtype=dtype, device='cuda')
    out = buf[1:1 + B * L].view(B, L)
    ops.axpbypcz(dev[0], x, dev[1], y, dev[2], w, out=out)
    want = _plain_per_problem(ops, host, x.contiguous(), y.contiguous(), w.contiguous(), torch.empty((B, L), dtype=dtype, device='cuda'))
    assert _same(out, want)
    assert buf[0].item() == 7.0 and buf[-1].item() == 7.0
    # mixed: an aligned x with an offset out takes the same path
    xa = x.clone()
    buf.fill_(7.0)
    ops.axpbypcz(dev[0], xa, dev[1], y, dev[2], w, out=out)
    assert _same(out, want) and buf[0].item() == 7.0 and buf[-1].item() == 7.0


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('B,L', [(7, 1027), (5, 64 * 64)])
def test_a_problem_does_not_depend_on_its_batch(dtype, B, L):
    from pnp_svrg_amd import ops
    rng = np.random.default_rng(L + 2)
    x, y, w = (_operand(rng, B, L, dtype) for _ in range(3))
    dev, _ = _coefs(rng, B, (True, True, True))
    whole = ops.axpbypcz(dev[0], x, dev[1], y, dev[2], w)
    for p in (0, B // 2, B - 1):
        alone = ops.axpbypcz(dev[0][p:p + 1].clone(), x[p:p + 1].clone(), dev[1][p:p + 1].clone(), y[p:p + 1].clone(),
                             dev[2][p:p + 1].clone(), w[p:p + 1].clone())
        assert _same(alone[0], whole[p]), p


@pytest.mark.parametrize('L', [3, 4])
def test_more_problems_than_a_grid_has_rows(L):
    """batch > 65535 (the y limit of a grid): the kernel strides over problems, on either path (L = 4 floats: 16 bytes).  Two
    coefficient values, so the reference is two plain whole-batch calls selected per problem."""
    from pnp_svrg_amd import ops
    B = 65535 + 1500
    rng = np.random.default_rng(3)
    x, y = (_operand(rng, B, L, torch.float32, special=False) for _ in range(2))
    pick = rng.random(B) < 0.5
    vals = (0.1 * np.pi, -2.0 / 3.0)
    b = torch.from_numpy(np.where(pick, vals[0], vals[1])).cuda()
    got = ops.axpbypcz(1.0, x, b, y)
    ref = [ops.axpbypcz(1.0, x, v, y) for v in vals]
    want = torch.where(torch.from_numpy(pick).cuda()[:, None], ref[0], ref[1])
    assert _same(got, want)
