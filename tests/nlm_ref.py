"""Float64 NumPy reference of the NLM prox for the kernel-form tests: `oracle.denoise.nl_means_2d` restated operation for
operation (the image it returns equals the oracle's bit for bit, tests/test_cpu_nlm_ref.py) with two extra results that say
where a float32 kernel may legitimately differ, and the images, cases and cached references that tests/test_cpu_nlm_ref.py
(the conditions on the inputs) and tests/test_gpu_nlm_forms.py (the kernels) share.  No GPU."""
import functools

import numpy as np

from oracle import denoise as od

# |running distance - 5| <= TAU at one of the per-row tests marks the pixel: float32 rounding of the running sum is about
# 2 S^2 2^-24 sum|terms| ~ 1e-4 for S = 7 and sums around 20; 1e-3 leaves a factor of ten above that
TAU = 1e-3
CUT = 5.0
NEAR_CUT_CAP = 0.02                  # largest share of marked pixels a float32 case may have
LIVE_DIST_CAP = 700.0                # beyond ~709 Schraudolph's integer wraps and the reference's weights are garbage
FAST_EXP_RANGE = 2.0 ** 31 / 1512775.3951951856938          # ~1419.6: (int)(2^20/ln2 * -dist) leaves int32 beyond it


def side_of(patch_size):
    return patch_size + 1 if patch_size % 2 == 0 else patch_size


def nlm_ref(img, h, sigma, patch_size=4, patch_distance=5):
    """-> (image, near_cut, max_live_dist).  image: od.nl_means_2d(img, h, sigma, patch_size, patch_distance), the same
    operations in the same order.  near_cut [H, W] bool: for some candidate inside the image and not yet cut, the running
    distance lay within TAU of 5 at one of the tests in front of a patch row -- there `dist > 5` can fall on the other side
    in float32, and one flipped candidate moves the output by up to exp(-5) of a pixel difference.  max_live_dist: the
    largest final distance of a candidate that was not cut."""
    x = np.asarray(img, dtype=np.float64)
    s = side_of(patch_size)
    d = patch_distance
    off = s // 2
    H, W = x.shape
    pad = np.pad(x, off, mode='reflect')
    A = (s - 1.0) / 4.0
    g = np.arange(-off, off + 1)
    gr, gc = np.meshgrid(g, g, indexing='ij')
    w = np.exp(-(gr * gr + gc * gc) / (2 * A * A))
    w = w * (1.0 / (1 * np.sum(w) * h * h))
    var = 2.0 * sigma * sigma
    rows = np.arange(H)[:, None]
    cols = np.arange(W)[None, :]
    wsum = np.zeros((H, W))
    acc = np.zeros((H, W))
    near_cut = np.zeros((H, W), dtype=bool)
    max_live = -np.inf
    for di in range(-d, d + 1):
        for dj in range(-d, d + 1):
            valid = ((rows + di >= 0) & (rows + di < H) &
                     (cols + dj >= 0) & (cols + dj < W))
            ri = np.clip(rows + di, 0, H - 1)
            cj = np.clip(cols + dj, 0, W - 1)
            dist = np.zeros((H, W))
            dead = np.zeros((H, W), dtype=bool)
            for pi in range(s):
                near_cut |= valid & ~dead & (np.abs(dist - CUT) <= TAU)
                dead |= dist > CUT
                for pj in range(s):
                    diff = pad[rows + pi, cols + pj] - pad[ri + pi, cj + pj]
                    dist = dist + w[pi, pj] * (diff * diff - var)
            live = valid & ~dead
            if live.any():
                max_live = max(max_live, float(dist[live].max()))
            weight = od.fast_exp(-np.maximum(0.0, dist))
            weight = np.where(dead, 0.0, weight)
            weight = np.where(valid, weight, 0.0)
            wsum = wsum + weight
            acc = acc + weight * pad[ri + off, cj + off]
    with np.errstate(all='ignore'):
        return acc / wsum, near_cut, max_live


# --------------------------------------------------------------------------
# images
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def images(H, W, n=6, seed=None):
    """[n, H, W] float64 in [0, 1] on the 2^-16 grid (exact in float32): uniform noise, wrapped 3 x 3 box blur, plus
    0.05 * standard normal; one generator seeded with 100 H + W draws the n images in turn.  Read only."""
    rng = np.random.default_rng(100 * H + W if seed is None else seed)
    out = np.empty((n, H, W))
    for b in range(n):
        u = rng.random((H, W))
        box = sum(np.roll(np.roll(u, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) / 9.0
        z = box + 0.05 * rng.standard_normal((H, W))
        out[b] = np.clip(np.round(z * 65536.0) / 65536.0, 0.0, 1.0)
    out.setflags(write=False)
    return out


def overflow_image():
    """16 x 16, for patch side 5, radius 1 and h = sigma = 0.005: every row is constant except row 10, which alternates 0, 1.
    For the pixels of row 8 the horizontal neighbours' patches agree exactly in their first four rows (so they are never
    cut: the distance is tested only in front of a row) and differ by 1 in every element of the last: the final distance
    is in the thousands, beyond FAST_EXP_RANGE, and fast_exp's (int) conversion is out of range."""
    z = np.empty((16, 16))
    z[:] = (np.arange(16)[:, None] * 37 % 16) / 16.0
    z[10] = np.arange(16) % 2
    return z


OVERFLOW = dict(patch_size=5, patch_distance=1, h=0.005)


# --------------------------------------------------------------------------
# cases: (H, W, patch side, radius)
# --------------------------------------------------------------------------
PAIRS = [(s, d) for s in (3, 5, 7) for d in (1, 5, 8)]
CORNERS = [(5, 5), (7, 8), (3, 1)]
CASES = ([(17, 33, s, d) for s, d in PAIRS]                       # one-pixel ragged tiles both ways
         + [(16, 16, s, d) for s, d in CORNERS]                   # exactly one tile
         + [(5, 40, s, d) for s, d in CORNERS]                    # H below the radius and the tile
         + [(4, 4, s, d) for s, d in CORNERS]                     # the smallest image side 7 takes; the window is the image
         + [(33, 16, 5, 5), (33, 16, 7, 8)]                       # three tile rows, one tile column
         + [(40, 56, 7, 3), (40, 56, 3, 8)])
H_F64 = (0.05, 0.1)
H_F32 = (0.1, 0.2)
FIXED_H_CASES = [(17, 33, 5, 5), (17, 33, 3, 8)]                  # strip form, LDS form
FIXED_H = 0.2
PP_PAIRS = [(s, d) for s in (3, 5, 7) for d in (5, 3)]
PP_SHAPE = (17, 33)
PP_SIGMA = (0.1, 0.08, 0.25)
PP_MODIFIER = (1.0, 1.5, 0.8)                                     # h = 0.1, 0.12, 0.2


def f32(v):
    return float(np.float32(v))


def h_of(h, f32_case):
    """The h the kernel computes with: a float32 kernel holds it as a float32."""
    return f32(h) if f32_case else float(h)


def pp_h(b, f32_case):
    """h of image b of the per-problem cases: (T)((double)sigma_in[b] * modifier[b])."""
    if f32_case:
        return f32(f32(PP_SIGMA[b]) * PP_MODIFIER[b])
    return PP_SIGMA[b] * PP_MODIFIER[b]


@functools.lru_cache(maxsize=None)
def _reference(H, W, b, s, d, h, sigma):
    out = nlm_ref(images(H, W)[b], h, sigma, s, d)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def reference(H, W, s, d, h, b=0, fixed=False):
    """nlm_ref of image b of images(H, W), computed once per process; h as `h_of` / `pp_h` give it; fixed: the fixed_h path
    (sigma = 0, so var = 0)."""
    return _reference(H, W, b, s, d, float(h), 0.0 if fixed else float(h))


def f32_reference_cases():
    """Every reference a float32 test compares with, as (id, arguments of `reference`): tests/test_cpu_nlm_ref.py asserts the
    two conditions on each."""
    out = []
    for (H, W, s, d) in CASES:
        for h in H_F32:
            out.append((f'{H}x{W}-s{s}-d{d}-h{h}', dict(H=H, W=W, s=s, d=d, h=h_of(h, True))))
    for (H, W, s, d) in FIXED_H_CASES:
        out.append((f'fixed-{H}x{W}-s{s}-d{d}', dict(H=H, W=W, s=s, d=d, h=h_of(FIXED_H, True), fixed=True)))
    for (s, d) in PP_PAIRS:
        for b in range(3):
            out.append((f'pp-s{s}-d{d}-b{b}', dict(H=PP_SHAPE[0], W=PP_SHAPE[1], s=s, d=d, h=pp_h(b, True), b=b)))
    return out
