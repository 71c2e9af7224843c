"""float64 NumPy restatement of the device-side CSMRI problem generator (pnp_csmri_generate), from the stream
published in include/pnp_hip.h -- not from the kernels:

    state_k = mix64(mix64(mix64(seed) + id) + k)          key_k(i) = mb_key(state_k, i),  i = ky*W + kx
    mask    : (uint64)key_0(i) < T,  T = floor(alpha * 2^32) clipped to [0, 2^32]
    data    : Y0 = mask o fft2(x);  sigma = sqrt(||Y0||_2 / 10^(snr/10) / H / W)
    noise   : u1 = (key_1 + 1) 2^-32, u2 = key_2 2^-32, n = sqrt(-2 ln u1) cos(2 pi u2);  Y = Y0 + mask * sigma * n  (real part)
    init    : Xinit = minmax(|ifft2(Y)|)

tests/test_cpu_csmri_generate.py holds the keys to literals computed with plain Python integers."""
import numpy as np

_U64 = np.uint64


def mix64(x):
    with np.errstate(over='ignore'):
        x = _U64(x) + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
        return x ^ (x >> _U64(31))


def state(seed, item_id, k):
    with np.errstate(over='ignore'):
        return mix64(mix64(mix64(_U64(int(seed) & (2 ** 64 - 1))) + _U64(int(item_id) & (2 ** 64 - 1))) + _U64(k))


def keys(seed, item_id, k, pos):
    """key_k(i) for the positions `pos` (any integer array) as uint32."""
    st = int(state(seed, item_id, k))
    with np.errstate(over='ignore'):
        x = (np.uint32(st & 0xFFFFFFFF) ^ np.asarray(pos).astype(np.uint32)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
        x ^= x >> np.uint32(15)
        x = (x * np.uint32(0x846ca68b)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        return (x ^ np.uint32(st >> 32)).astype(np.uint32)


def threshold(alpha):
    return min(max(int(np.floor(np.float64(alpha) * 2.0 ** 32)), 0), 2 ** 32)


def mask(seed, item_id, alpha, H, W):
    """[H, W] uint8 Bernoulli(alpha) mask of the item."""
    k0 = keys(seed, item_id, 0, np.arange(H * W)).astype(np.uint64)
    return (k0 < np.uint64(threshold(alpha))).astype(np.uint8).reshape(H, W) if threshold(alpha) < 2 ** 32 \
        else np.ones((H, W), np.uint8)


def noise(seed, item_id, H, W):
    """[H, W] standard normal draws n(i) of the item (every position; the generator uses those on the mask)."""
    pos = np.arange(H * W)
    u1 = (keys(seed, item_id, 1, pos).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = keys(seed, item_id, 2, pos).astype(np.float64) * 2.0 ** -32
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(H, W)


def norm01(img):
    x = np.asarray(img, np.float64)
    return (x - x.min()) / (x.max() - x.min())


def generate(x, item):
    """One item (dict with id, alpha, snr, seed) on the normalised H x W image x -> dict(mask, M0, sigma, noise, Y, xinit)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    mk = mask(item['seed'], item['id'], item['alpha'], H, W)
    Y0 = mk * np.fft.fft2(x)
    sigma = np.sqrt(np.linalg.norm(Y0.ravel()) / 10 ** (item['snr'] / 10) / H / W)
    n = noise(item['seed'], item['id'], H, W)
    Y = Y0 + mk * (sigma * n)
    xi = np.absolute(np.fft.ifft2(Y))
    with np.errstate(invalid='ignore', divide='ignore'):
        xinit = (xi - xi.min()) / (xi.max() - xi.min())
    return dict(mask=mk, M0=int(mk.sum()), sigma=float(sigma), noise=n, Y=Y, xinit=xinit)
