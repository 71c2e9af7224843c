"""Float64 NumPy reference of the Deblur / super-resolution operator family for the operator-form tests: every piece of
    grad = scale * B^T S^T (sel o (S B z - Y))
on its own -- the blur as a direct circular convolution of the ravelled vector with a sparse kernel (no FFT), its adjoint, the
bilinear down-sampler from the textbook formula and its adjoint -- the compositions, the inputs that tests/test_cpu_deblur_ref.py
(the reference against oracle.problems.Deblur) and tests/test_gpu_deblur_forms.py (the kernels against the reference) share, and
`e32`: the float32 error of the reference operation itself, from which the float32 bound of the GPU tests is made.  No GPU; this
module imports neither the package under test nor the oracle.

Error metric of a blur or gradient output o (`err`): max|o - ref| / S with S = sqrt(N) * sum|B_t| * max|input of the last blur|,
the largest magnitude that blur can produce, taken from the reference's intermediate (times |scale| where the output is scaled).
F64_BOUND is what the project's 256 x 256 float64 Deblur test already holds; a float32 result is held to F32_MARGIN * e32, and
never to more than F32_CAP, the bound of the natural-image tests."""
import functools

import numpy as np

F64_BOUND = 1e-11
F32_MARGIN = 4.0                     # the device FFT is another factorisation with float32 twiddle tables; both are O(eps log N)
F32_CAP = 2e-4
LINE_SPLIT = {64: (8, 8), 128: (8, 16), 256: (16, 16)}      # n -> <RA, LA> of the kernels' line transform


# ------------------------------------------------------------------------------------------------------------ the blur
def blur(a, taps, N):
    """out[i] = sqrt(N) * sum_t v_t * a[(i - p_t) mod N] over the last axis: fft_blur(a, B) for B = sum_t v_t e_{p_t}."""
    a = np.asarray(a, np.float64)
    pos, val = taps
    out = np.zeros_like(a)
    i = np.arange(N)
    for p, v in zip(pos, val):
        out += v * a[..., (i - int(p)) % N]
    return out * np.sqrt(N)


def blur_adj(a, taps, N):
    """out[i] = sqrt(N) * sum_t v_t * a[(i + p_t) mod N]: fft_blur(a, roll(flip(B), 1)), the transpose of `blur`."""
    a = np.asarray(a, np.float64)
    pos, val = taps
    out = np.zeros_like(a)
    i = np.arange(N)
    for p, v in zip(pos, val):
        out += v * a[..., (i + int(p)) % N]
    return out * np.sqrt(N)


def blur_dense(a, B):
    """fft_blur(a, B) with np.fft in float64: for kernels too dense for `blur`."""
    a = np.asarray(a, np.float64)
    return np.real(np.fft.ifft(np.fft.fft(a, axis=-1) * np.fft.fft(np.asarray(B, np.float64)))) * np.sqrt(a.shape[-1])


def adjoint_kernel(B):
    """roll(flip(B), 1): the kernel whose blur is the transpose of B's."""
    return np.roll(np.flip(np.asarray(B, np.float64)), 1)


def kernel_vector(taps, N):
    B = np.zeros(N)
    np.add.at(B, np.asarray(taps[0]), np.asarray(taps[1], np.float64))
    return B


class Kernel:
    """A blur kernel: the raw vector `Bk` a plan takes (nothing further is divided by N), `l1` = sum|B_t|, and its two blurs."""

    def __init__(self, name, N, taps=None, Bk=None):
        self.name, self.N, self.taps = name, N, taps
        self.Bk = kernel_vector(taps, N) if taps is not None else np.asarray(Bk, np.float64)
        self.l1 = float(np.abs(self.Bk).sum())

    def fwd(self, a):
        return blur(a, self.taps, self.N) if self.taps is not None else blur_dense(a, self.Bk)

    def adj(self, a):
        return blur_adj(a, self.taps, self.N) if self.taps is not None else blur_dense(a, adjoint_kernel(self.Bk))

    def span(self, a):
        """S of the metric for a blur of `a` by this kernel, per leading index."""
        a = np.asarray(a, np.float64)
        return np.sqrt(self.N) * self.l1 * np.abs(a).reshape(-1, a.shape[-1]).max(axis=1)


def edge_taps(N):
    """Sparse and asymmetric: 6 taps of unequal weights and both signs at 0, 1, n-1, n, N/2 + n/3, N-1 (n = sqrt(N)).  The
    positions cross both digits of the four-step index a*n + b; no position is the mirror of another but 1 and N-1, whose weights
    differ, so a missing or doubled conjugate shows."""
    n = int(round(np.sqrt(N)))
    assert n * n == N
    pos = np.array([0, 1, n - 1, n, N // 2 + n // 3, N - 1])
    val = np.array([0.5, -0.25, 0.125, 0.3125, -0.1875, 0.0625]) / np.sqrt(N)
    return pos, val


@functools.lru_cache(maxsize=None)
def kernel(name, N):
    """'edge' (edge_taps), 'dense' (default_rng normal / N), or 'identity' (the unit impulse at 0 times 1/sqrt(N): fft_blur is
    the identity)."""
    if name == 'edge':
        return Kernel(name, N, taps=edge_taps(N))
    if name == 'identity':
        return Kernel(name, N, taps=(np.array([0]), np.array([1.0 / np.sqrt(N)])))
    if name == 'dense':
        return Kernel(name, N, Bk=np.random.default_rng(1234 + N).normal(size=N) / N)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------------------ the down-sampler
def bilinear_points(H, W, scale_percent, eps=1e-10):
    """The reference's sampling grid (problems/DeblurSR.py:95-108) -> (rows, cols), each [M], or None for scale_percent == 100.
    The two outputs of its `meshgrid` are bound in swapped order -- rows come from the points over W, columns from those over H --
    which is harmless on square images and is kept as it is."""
    if scale_percent == 100:
        return None
    lrH, lrW = int(H * scale_percent / 100), int(W * scale_percent / 100)
    ptsH = np.linspace(eps, H - (1 + eps), lrH)
    ptsW = np.linspace(eps, W - (1 + eps), lrW)
    meshW, meshH = np.meshgrid(ptsH, ptsW)
    return meshH.ravel(), meshW.ravel()


def n_meas(H, W, scale_percent):
    return int(H * scale_percent / 100) * int(W * scale_percent / 100)


def _cells(pts):
    r0 = np.floor(pts[0]).astype(np.int64)
    c0 = np.floor(pts[1]).astype(np.int64)
    return r0, c0, pts[0] - r0, pts[1] - c0


def down(x, pts, H, W):
    """Bilinear interpolation of the H x W image(s) x [..., H*W] at pts -> [..., M]; the identity for pts None."""
    x = np.asarray(x, np.float64)
    if pts is None:
        return x.copy()
    im = x.reshape(x.shape[:-1] + (H, W))
    r0, c0, fr, fc = _cells(pts)
    return ((1 - fr) * (1 - fc) * im[..., r0, c0] + fr * (1 - fc) * im[..., r0 + 1, c0]
            + (1 - fr) * fc * im[..., r0, c0 + 1] + fr * fc * im[..., r0 + 1, c0 + 1])


def up(y, pts, H, W):
    """The transpose of `down`: y [..., M] -> [..., H*W]."""
    y = np.asarray(y, np.float64)
    if pts is None:
        return y.copy()
    r0, c0, fr, fc = _cells(pts)
    flat = y.reshape(-1, y.shape[-1])
    out = np.zeros((flat.shape[0], H, W))
    for b in range(flat.shape[0]):
        np.add.at(out[b], (r0, c0), (1 - fr) * (1 - fc) * flat[b])
        np.add.at(out[b], (r0 + 1, c0), fr * (1 - fc) * flat[b])
        np.add.at(out[b], (r0, c0 + 1), (1 - fr) * fc * flat[b])
        np.add.at(out[b], (r0 + 1, c0 + 1), fr * fc * flat[b])
    return out.reshape(y.shape[:-1] + (H * W,))


def down_matrix(pts, H, W):
    """`down` as a dense M x N matrix (small images only)."""
    return down(np.eye(H * W), pts, H, W).T


# ------------------------------------------------------------------------------------------------------------ compositions
def forward(x, kern, pts, H, W):
    return down(kern.fwd(x), pts, H, W)


def residual(z, Y, sel, kern, pts, H, W):
    """sel o (S B z - Y): assigned 0 where sel is 0, whatever Y holds there."""
    res = forward(z, kern, pts, H, W) - np.asarray(Y, np.float64)
    if sel is not None:
        res = np.where(np.asarray(sel) != 0, res, 0.0)
    return res


def grad(z, Y, sel, scale, kern, pts, H, W, parts=False):
    """scale * B^T S^T (sel o (S B z - Y)) for z [B, N], Y [B, M]; scale a scalar or [B].  parts=True -> (grad, S) with S [B] the
    metric's magnitude of the last blur times |scale|."""
    lifted = up(residual(z, Y, sel, kern, pts, H, W), pts, H, W)
    sc = np.broadcast_to(np.asarray(scale, np.float64), lifted.shape[:-1])
    g = sc[..., None] * kern.adj(lifted)
    return (g, kern.span(lifted) * np.abs(sc).reshape(-1)) if parts else g


def objective(z, Y, scale, kern, pts, H, W):
    """scale * sum_m (S B z - Y)^2 per problem."""
    d = forward(z, kern, pts, H, W) - np.asarray(Y, np.float64)
    return scale * np.sum(d * d, axis=-1)


def err(got, ref, S):
    """max_b max_i |got - ref| / S_b."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref).reshape(-1, ref.shape[-1]).max(axis=1)
    return float((d / np.broadcast_to(np.asarray(S, np.float64), d.shape)).max())


# ------------------------------------------------------------------------------------------------------------ inputs
def plane_wave_orders(N):
    """k = k1 + n*k2 with k1, k2 from {0, 1, RA-1, RA, n/2, n-1} of that size's <RA, LA> split."""
    n = int(round(np.sqrt(N)))
    RA = LINE_SPLIT[n][0]
    digits = [0, 1, RA - 1, RA, n // 2, n - 1]
    return [k1 + n * k2 for k2 in digits for k1 in digits]


@functools.lru_cache(maxsize=None)
def images(N):
    """[42, N]: two default_rng normal images, the unit impulses at 0, n-1, n, N-1, and the 36 real plane waves
    cos(2 pi k i / N) of `plane_wave_orders` -- 14 batches of three."""
    n = int(round(np.sqrt(N)))
    rng = np.random.default_rng(99 + N)
    rows = [rng.normal(size=N), rng.normal(size=N)]
    for p in (0, n - 1, n, N - 1):
        e = np.zeros(N)
        e[p] = 1.0
        rows.append(e)
    i = np.arange(N)
    for k in plane_wave_orders(N):
        rows.append(np.cos(2 * np.pi * ((k * i) % N) / N))
    out = np.stack(rows)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def problem(H, W, scale_percent, kname, B=3, seed=0):
    """Synthetic data of a gradient case: z [B, N] normal, Y = S B z' + noise for another normal z', r [B, M] normal."""
    N, M = H * W, n_meas(H, W, scale_percent)
    rng = np.random.default_rng([seed, H, W, scale_percent])
    kern, pts = kernel(kname, N), bilinear_points(H, W, scale_percent)
    z = rng.normal(size=(B, N))
    Y = forward(rng.normal(size=(B, N)), kern, pts, H, W) + 0.1 * rng.normal(size=(B, M))
    r = rng.normal(size=(B, M))
    for a in (z, Y, r):
        a.setflags(write=False)
    return dict(z=z, Y=Y, r=r, kern=kern, pts=pts, N=N, M=M)


def selection(M, B, seed=3):
    """A uint8 [B, M] indicator of about a quarter of the measurements (at least one per row)."""
    rng = np.random.default_rng([seed, M, B])
    sel = (rng.random((B, M)) < 0.25).astype(np.uint8)
    sel[:, rng.integers(M)] = 1
    return sel


def corrupted_tables(taps, N):
    """(what, the five tables (g_idx, g_w, a_rowptr, a_col, a_val) with ONE entry of one table changed, the message of the
    refusal) for every table check of pnp_deblur_plan_create."""
    M = taps[0].shape[0]
    out = []
    for what, k, at, value, msg in (('g_idx high', 0, (M - 1, 3), N, 'g_idx outside'), ('g_idx negative', 0, (0, 0), -1, 'g_idx outside'),
                                    ('rowptr start', 2, 0, 1, 'a_rowptr must run'), ('rowptr end', 2, N, 4 * M - 1, 'a_rowptr must run'),
                                    ('rowptr order', 2, N // 2, 4 * M + 1, 'must not decrease'),
                                    ('a_col high', 3, 4 * M - 1, M, 'a_col outside'), ('a_col negative', 3, 0, -1, 'a_col outside')):
        bad = [np.array(t) for t in taps]
        bad[k][at] = value
        out.append((what, tuple(bad), msg))
    return out


# (H, W, scale_percent, kernel) of every float32 GPU case
E32_CASES = ([(n, n, s, k) for n in (64, 128, 256) for k in ('edge', 'dense') for s in (100, 50)]
             + [(n, n, s, 'identity') for n in (64, 128, 256) for s in (50, 75)] + [(64, 64, 2, 'identity')]
             + [(64, 64, 75, 'edge'), (64, 64, 2, 'edge')] + [(32, 128, 100, 'edge'), (128, 32, 100, 'edge'), (64, 256, 100, 'edge')])
E32_SCALE = 0.37                     # the scalar scale of e32's gradient (so that the final multiply rounds)


# ------------------------------------------------------------------------------------------------------------ e32
def _render32(H, W, scale_percent, kname):
    """The reference operation in float32: torch.fft on complex64 (fft, product, ifft), taps and their transpose in float32."""
    import torch
    N = H * W
    kern, pts = kernel(kname, N), bilinear_points(H, W, scale_percent)
    f32 = np.float32
    sq = f32(np.sqrt(N))

    def blur32(a, B):
        fa = torch.fft.fft(torch.from_numpy(np.ascontiguousarray(a, f32)).to(torch.complex64), dim=-1)
        fb = torch.fft.fft(torch.from_numpy(np.ascontiguousarray(B, f32)).to(torch.complex64))
        return torch.fft.ifft(fa * fb, dim=-1).real.numpy().astype(f32) * sq

    if pts is not None:
        r0, c0, fr, fc = _cells(pts)
        idx = np.stack([r0 * W + c0, (r0 + 1) * W + c0, r0 * W + c0 + 1, (r0 + 1) * W + c0 + 1], axis=1)
        wts = np.stack([(1 - fr) * (1 - fc), fr * (1 - fc), (1 - fr) * fc, fr * fc], axis=1).astype(f32)

    def down32(x):
        if pts is None:
            return x
        o = np.zeros(x.shape[:-1] + (idx.shape[0],), f32)
        for t in range(4):
            o += wts[:, t] * x[..., idx[:, t]]
        return o

    def up32(y):
        if pts is None:
            return y
        o = np.zeros((y.shape[0], N), f32)
        for b in range(y.shape[0]):
            for t in range(4):
                np.add.at(o[b], idx[:, t], wts[:, t] * y[b])
        return o

    Bk32 = kern.Bk.astype(f32)
    Ba32 = adjoint_kernel(Bk32)
    return dict(fwd=lambda x: down32(blur32(x, Bk32)), adj=lambda r: blur32(up32(np.ascontiguousarray(r, f32)), Ba32),
                grad=lambda z, Y, sel, sc: f32(sc) * blur32(up32(np.where(sel != 0, down32(blur32(z, Bk32)) - Y.astype(f32), f32(0))),
                                                            Ba32))


@functools.lru_cache(maxsize=None)
def e32(H, W, scale_percent, kname='edge'):
    """The reference's own float32 error in the metric of the module docstring: the largest, over the forward pass of `images`,
    the adjoint of `problem`'s r and the gradient of `problem` (all measurements and `selection`), of max|float32 rendering -
    float64 reference| / S.  The float32 renderings take the float32 roundings of the float64 inputs, as the kernels do."""
    N = H * W
    p = problem(H, W, scale_percent, kname)
    kern, pts = p['kern'], p['pts']
    r32 = _render32(H, W, scale_percent, kname)
    f32 = np.float32
    x = images(N).astype(f32)
    worst = err(r32['fwd'](x), forward(x, kern, pts, H, W), kern.span(x))
    r = p['r'].astype(f32)
    lifted = up(r, pts, H, W)
    worst = max(worst, err(r32['adj'](r), kern.adj(lifted), kern.span(lifted)))
    z, Y = p['z'].astype(f32), p['Y'].astype(f32)
    for sel in (np.ones((3, p['M']), np.uint8), selection(p['M'], 3)):
        ref, S = grad(z, Y, sel, E32_SCALE, kern, pts, H, W, parts=True)
        worst = max(worst, err(r32['grad'](z, Y, sel, E32_SCALE), ref, S))
    return worst


def f32_bound(H, W, scale_percent, kname='edge'):
    """The float32 bound of a device result in the metric: F32_MARGIN * e32, never above F32_CAP."""
    return min(F32_MARGIN * e32(H, W, scale_percent, kname), F32_CAP)
