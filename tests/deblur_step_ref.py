"""What tests/test_cpu_deblur_step.py and tests/test_gpu_deblur_step.py share: the cases, inputs, float64 reference, metric and bound
of the one-pass Deblur step (pnp_deblur_grad_step)
    out = beta*c1 + gamma_b*c2 + scale_b * B^T S^T (sel o (S B (a - b) - Y))
on top of tests/deblur_ref.py.  No GPU; imports neither the package under test nor the oracle.

Reference: the `dtype` roundings of a, b, Y, c1, c2, beta and gamma, everything else in float64.
Metric   : deblur_ref.err of  got - (beta*c1 + gamma*c2)  against the gradient term, per problem, S from the reference's intermediate
           of a - b (deblur_ref.grad(..., parts=True)).
Bound    : deblur_ref.F64_BOUND (float64) or deblur_ref.f32_bound (float32: F32_MARGIN * e32, capped)
           + 4 eps(dtype): one rounding of a - b carried through two blurs of gain <= S each in the metric, two roundings of the addend sums
           + 2 eps(dtype) * max|beta*c1 + gamma*c2| / S: the addends' own roundings.
A problem whose selector row is all zeros has S = 0 and no metric: its result must be the addends exactly (the tests compare bits)."""
import functools

import numpy as np

import deblur_ref as dr

# (n, scale_percent, kernel): <8,8>, the asymmetric <8,16> and <16,16>; the fused middle pass (100) and the gather/CSR middle (50);
# a down-sampler whose M is no multiple of a block (75: 48 x 48) and the single measurement (2: M = 1)
CASES = [(n, s, k) for n in (64, 128, 256) for k in ('edge', 'dense') for s in (100, 50)] + [(64, 75, 'edge'), (64, 2, 'edge')]
SCALE, SCALE_PP = 0.37, [0.37, -1.5, 2.25e-3]
BETA = -0.6
GAMMA, GAMMA_PP = 1.3, [1.3, -2.5e-2, 40.0]


@functools.lru_cache(maxsize=None)
def inputs(n, scale, kname):
    """deblur_ref.problem(n, n, scale, kname, B=3) (a = its z, Y) and a second normal image set for b, c1 and c2, all float64 and
    read-only."""
    p = dr.problem(n, n, scale, kname, B=3)
    rng = np.random.default_rng([17, n, scale])
    more = {k: rng.normal(size=(3, p['N'])) for k in ('b', 'c1', 'c2')}
    for v in more.values():
        v.setflags(write=False)
    return dict(a=p['z'], Y=p['Y'], kern=p['kern'], pts=p['pts'], N=p['N'], M=p['M'], **more)


def rounded(x, npdt):
    """The values the kernels see, as float64 (None stays None)."""
    return None if x is None else np.asarray(x, npdt).astype(np.float64)


def edge_selection(M):
    """uint8 [3, M]: a single one at measurement 0, a single one at M - 1, all zeros."""
    sel = np.zeros((3, M), np.uint8)
    sel[0, 0] = 1
    sel[1, M - 1] = 1
    return sel


def gradient_term(inp, n, a, b, Y, sel, scale):
    """(scale_b * B^T S^T (sel o (S B (a - b) - Y)), S [B]) in float64 from rounded inputs (b, Y, sel: None = absent)."""
    d = a if b is None else a - b
    Y0 = np.zeros((d.shape[0], inp['M'])) if Y is None else Y
    return dr.grad(d, Y0, sel, scale, inp['kern'], inp['pts'], n, n, parts=True)


def addends(beta, c1, gamma, c2, npdt, shape):
    """beta*c1 + gamma_b*c2 in float64 from rounded c1, c2 (None = absent) and the `dtype` roundings of beta and gamma."""
    out = np.zeros(shape)
    if c1 is not None:
        out = out + float(npdt(beta)) * c1
    if c2 is not None:
        g = np.asarray(gamma, npdt).astype(np.float64)
        out = out + (g[:, None] if g.ndim else g) * c2
    return out


def base_bound(npdt, n, scale, kname, margin=dr.F32_MARGIN):
    if npdt == np.float64:
        return dr.F64_BOUND
    return min(margin * dr.e32(n, n, scale, kname), dr.F32_CAP)


def check(what, got, add, ref, S, base, npdt):
    """Print, then assert, the metric of every problem with S > 0 against its bound; -> the errors."""
    eps = float(np.finfo(npdt).eps)
    got, add, ref = (np.asarray(x, np.float64).reshape(len(S), -1) for x in (got, add, ref))
    assert np.isfinite(got).all(), what
    errs = []
    for b, Sb in enumerate(S):
        if Sb == 0:
            continue
        e = float(np.abs(got[b] - add[b] - ref[b]).max() / Sb)
        bound = base + 4 * eps + 2 * eps * float(np.abs(add[b]).max()) / Sb
        print(f'{what} [problem {b}]: err {e:.3e} (bound {bound:.3e})')
        errs.append((e, bound))
    for e, bound in errs:
        assert e <= bound, (what, e, bound)
    return errs


@functools.lru_cache(maxsize=None)
def unit_term(n, scale, kname, dtname, with_b, with_Y, selname):
    """`gradient_term` at scale 1 of the case's inputs rounded to dtype `dtname`, computed once and shared: the term is linear in
    the scale, so (scale_b * g, |scale_b| * S) is the reference of any scale.  selname: 'all', 'selection' or 'edges'."""
    npdt = np.dtype(dtname).type
    inp = inputs(n, scale, kname)
    sel = {'all': None, 'selection': dr.selection(inp['M'], 3), 'edges': edge_selection(inp['M'])}[selname]
    g, S = gradient_term(inp, n, rounded(inp['a'], npdt), rounded(inp['b'], npdt) if with_b else None,
                         rounded(inp['Y'], npdt) if with_Y else None, sel, 1.0)
    g.setflags(write=False)
    S.setflags(write=False)
    return g, S, sel


def scaled(g, S, scale):
    sc = np.broadcast_to(np.asarray(scale, np.float64), S.shape)
    return sc[:, None] * g, np.abs(sc) * S
