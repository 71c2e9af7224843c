"""Every DnCNN conv form (conv modes 0, 1, 5, 6) against float64 across its launch geometries.

The middle-layer kernels split the batch into regions (8 x 32 tiles for modes 0 and 1, 8 x 64 or 4 x 64 regions for modes 5 and
6) and walk them with persistent workgroups (`csrc/tilewalk.h`); mode 5 also picks between a full-wave 8 x 64 launch and a 4 x 64
tail launch (`wino44_layer`).  Which branch runs depends on the batch and on the number of CUs, so the table below is derived at run
time from the device's CU count C, and `_branch` restates the dispatch arithmetic and asserts that each row reaches the branch it
is named for.  Every check is against a float64 restatement (oracle.denoise.conv_layer64 / dncnn_forward64), never against another
GPU kernel.

Per-element bound of one layer:  |y - y64| <= kappa_form * 2^-24 * ((|X| (*) |W|) + |b|), (*) = the 3x3 conv, right side in
float64.  kappa was calibrated on one MI355X (C = 256): about 4x the largest ratio seen over all rows, both layers and both
activations:
    form                 largest ratio   kappa
    0 direct                  5.86         24
    1 F(2,3)                  3.24         13
    5 F(4x4,3x3)             52.3         210
    6 F(4x4,3x3) bf16 x 3    47.3         190
    5 fused last layer        0.44        1.8   (bound: |W_last| (*) ((|X| (*) |W|) + |b|))
The Winograd forms sit far above the direct one: their transform entries run from 1/24 to 8."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import denoise as od

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
KAPPA = {0: 24.0, 1: 13.0, 5: 210.0, 6: 190.0}
KAPPA_FUSED = 1.8
GUARD = 1 << 18                     # floats (1 MiB) of NaN on each side of a buffer
SLOPE = 0.1


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _walk(ntiles, grid):
    """tile_walk (csrc/tilewalk.h): XCD-aware when the grid is a multiple of 8 and divides the tile count."""
    return 'xcd' if grid % 8 == 0 and ntiles % grid == 0 else 'plain'


def _launches(mode, H, W, B, C, rows=0):
    """The middle-layer launches of a form as (region rows, regions, grid, walk): wino44_layer for mode 5, one launch of
    8 x 64 regions for mode 6, one of 8 x 32 tiles for modes 0 and 1."""
    if mode in (0, 1):
        n = B * (H // 8) * (W // 32)
        return [(8, n, min(n, C), _walk(n, min(n, C)))]
    units = B * (H // 8) * (W // 64)
    if mode == 6:
        return [(8, units, min(units, C), _walk(units, min(units, C)))]
    full = 0 if rows == 1 else units if rows == 2 else (units // C) * C
    if rows == 0 and 2 * (units - full) > C:
        full = units
    out = []
    if full > 0:
        out.append((8, full, min(full, C), _walk(full, min(full, C))))
    if full < units:
        n1 = 2 * (units - full)
        out.append((4, n1, min(n1, C), _walk(n1, min(n1, C))))
    return out


def _branch(mode, H, W, B, C, rows=0):
    """The dispatch branch a layer of this geometry takes (the names of the table)."""
    L = _launches(mode, H, W, B, C, rows)
    if mode in (0, 1):
        _, n, g, walk = L[0]
        if n == 1:
            return 'one tile'
        if n < C:
            return 'tiles < C'
        if walk == 'xcd':
            return 'xcd walk'
        return 'plain walk, several per wg' if n > g and n % g else 'plain walk'
    if len(L) == 2:
        return 'whole waves + 4x64 tail'
    r, n, g, walk = L[0]
    if r == 4:
        return 'tail only'
    if n < C:
        return 'one partial wave, ' + walk
    if n % C == 0:
        return 'whole waves'
    return 'partial last wave'


# (id, H, W, B(C), forced rows, branch, branch of mode 6).  Mode 6 runs the mode 5 rows without forced rows, in one launch of
# 8 x 64 regions.  8 x 64 / 8 x 32 images are one region wide and high: every region touches all four image edges.
W44_ROWS = [
    ('tail-8x64', 8, 64, lambda C: 1, 0, 'tail only', 'one partial wave, plain'),
    ('tail-72x128', 72, 128, lambda C: 3, 0, 'tail only', 'one partial wave, plain'),
    ('b-plain-8x64', 8, 64, lambda C: C // 2 + 3, 0, 'one partial wave, plain', 'one partial wave, plain'),
    ('b-xcd-64x64', 64, 64, lambda C: (5 * C // 8) // 8, 0, 'one partial wave, xcd', 'one partial wave, xcd'),
    ('whole-64x64', 64, 64, lambda C: C // 8, 0, 'whole waves', 'whole waves'),
    ('wt-8x64', 8, 64, lambda C: C + 5, 0, 'whole waves + 4x64 tail', 'partial last wave'),
    ('wt-64x64', 64, 64, lambda C: C // 8 + 1, 0, 'whole waves + 4x64 tail', 'partial last wave'),
    ('e-8x64', 8, 64, lambda C: C + C // 2 + 7, 0, 'partial last wave', 'partial last wave'),
    ('e-128x128', 128, 128, lambda C: (3 * C // 2) // 32 + 1, 0, 'partial last wave', 'partial last wave'),
    ('rows1-e-128x128', 128, 128, lambda C: (3 * C // 2) // 32 + 1, 1, 'tail only', None),
    ('rows2-wt-8x64', 8, 64, lambda C: C + 5, 2, 'partial last wave', None),
]
DIRECT_ROWS = [
    ('one-8x32', 8, 32, lambda C: 1, 0, 'one tile', None),
    ('lt-256x32', 256, 32, lambda C: 1, 0, 'tiles < C', None),
    ('eq-64x64', 64, 64, lambda C: C // 16, 0, 'xcd walk', None),
    ('plain-8x32', 8, 32, lambda C: C + 44, 0, 'plain walk, several per wg', None),
    ('plain-64x64', 64, 64, lambda C: C // 16 + 1, 0, 'plain walk, several per wg', None),
    ('w96-40x96', 40, 96, lambda C: 2, 0, 'tiles < C', None),
    ('w160-24x160', 24, 160, lambda C: 3, 0, 'tiles < C', None),
]
CASES = ([(5, r) for r in W44_ROWS] + [(6, r) for r in W44_ROWS if r[6]] +
         [(m, r) for m in (0, 1) for r in DIRECT_ROWS])
ROW = {r[0]: r for r in W44_ROWS + DIRECT_ROWS}


def _geometry(mode, row):
    """(H, W, B, rows) of a row on this device, after checking that it reaches its branch."""
    name, H, W, fB, rows, branch, branch6 = row
    branch = branch6 if mode == 6 else branch
    C = _cu()
    B = fB(C)
    got = _branch(mode, H, W, B, C, rows)
    assert got == branch, (mode, name, C, B, got, _launches(mode, H, W, B, C, rows))
    return H, W, B, rows


def test_geometry_table_reaches_every_branch():
    """The table covers each dispatch branch of every form on this device, and the (b) / (e) rows have the shape the branch
    name promises: (b) one launch of fewer 8 x 64 regions than CUs, (e) workgroups with unequal region counts."""
    C = _cu()
    seen = {}
    for mode, row in CASES:
        H, W, B, rows = _geometry(mode, row)
        seen.setdefault(mode, set()).add(_branch(mode, H, W, B, C, rows))
    assert seen[5] >= {'tail only', 'one partial wave, plain', 'one partial wave, xcd', 'whole waves', 'whole waves + 4x64 tail',
                       'partial last wave'}
    assert seen[0] == seen[1] == {'one tile', 'tiles < C', 'xcd walk', 'plain walk, several per wg'}
    for name in ('e-8x64', 'e-128x128'):
        _, H, W, fB = ROW[name][:4]
        [(r, n, g, walk)] = _launches(5, H, W, fB(C), C)
        assert r == 8 and walk == 'plain' and n > g and n % g != 0, name
    # 8 x 64 at B = C / 2 + 3 runs without the 4 x 64 form; one region more than half a wave tips the choice
    assert _launches(5, 8, 64, C // 2, C)[0][0] == 4 and _launches(5, 8, 64, C // 2 + 1, C)[0][0] == 8
    print('geometry table built for C = %d CUs' % C)


# ------------------------------------------------------------------------------------------------------------- helpers
def _weights(slope=0.0, n_layers=5, seed=31):
    """n_layers - 2 middle layers, each with its own weights and nonzero bias; no BatchNorm (the plan uploads them as given)."""
    rng = np.random.default_rng(seed)
    w = {'n_layers': np.int64(n_layers)}
    for i in range(n_layers):
        cin, cout = (1 if i == 0 else 64), (1 if i == n_layers - 1 else 64)
        w[f'conv{i}.weight'] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        if 0 < i < n_layers - 1:
            w[f'conv{i}.bias'] = (0.1 * rng.standard_normal(64)).astype(np.float32)
    if slope:
        w['negative_slope'] = np.float32(slope)
    return w


def _plan(monkeypatch, w, H, W, B, mode, fusion=True):
    from pnp_svrg_amd import ops
    monkeypatch.setenv('PNP_DNCNN_EDGE_FUSION', '1' if fusion else '0')
    return ops.DncnnPlan(w, H, W, B, winograd=mode)


def _distinct(B):
    return min(B, 4)


def _banded(n, fill):
    t = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    if fill is not None:
        t[GUARD:GUARD + n] = fill
    return t


def _bands_intact(t, n):
    return bool(torch.isnan(t[:GUARD]).all()) and bool(torch.isnan(t[GUARD + n:]).all())


_X = {}
_REF = {}


def _layer_input(H, W):
    """4 distinct activations [4, 64, H, W] (float32 values), offset so that every halo value matters."""
    if (H, W) not in _X:
        rng = np.random.default_rng(H * 1000 + W)
        _X[(H, W)] = (rng.standard_normal((4, 64, H, W)) + 0.5).astype(np.float32)
    return _X[(H, W)]


def _layer_ref(w, H, W, layer):
    """float64 pre-activation of middle layer `layer` on the distinct inputs and the magnitude (|X| (*) |W|) + |b|."""
    key = (H, W, layer)
    if key not in _REF:
        x = torch.from_numpy(_layer_input(H, W)).double()
        wl, bl = w[f'conv{layer + 1}.weight'], w[f'conv{layer + 1}.bias']
        pre = od.conv_layer64(x, wl, bl)
        mag = od.conv_layer64(x.abs(), np.abs(wl), np.abs(bl))
        _REF[key] = (pre, mag)
    return _REF[key]


def _ratio(y, ref, mag, K):
    """max over the batch of |y - y64| / (2^-24 mag); image b of the batch is distinct image b % K."""
    B = y.shape[0]
    idx = torch.arange(B, device=y.device) % K
    r = (y.double() - ref[idx]).abs() / (ULP * mag[idx])
    return r.max().item()


# ------------------------------------------------------------------------------------------------------- one layer
@pytest.mark.parametrize('act', ['relu', 'leaky'])
@pytest.mark.parametrize('mode,row', CASES, ids=[f'{m}-{r[0]}' for m, r in CASES])
def test_mid_layer_vs_float64(monkeypatch, mode, row, act):
    """One middle layer (indices 0 and 2 of three, each with its own weights and bias) through `debug_mid_layer` on a
    NaN-banded input, into an output that is NaN everywhere beforehand: the bands stay intact, every output element is
    written and finite, and each element is within the per-element float64 bound of its form."""
    H, W, B, rows = _geometry(mode, row)
    slope = SLOPE if act == 'leaky' else 0.0
    w = _weights(slope)
    plan = _plan(monkeypatch, w, H, W, B, mode)
    K = _distinct(B)
    n = B * 64 * H * W
    x = torch.from_numpy(_layer_input(H, W)[:K]).cuda()
    xb = x.repeat((B + K - 1) // K, 1, 1, 1)[:B].reshape(-1)
    xin = _banded(n, xb)
    worst = 0.0
    for layer in (0, 2):
        yout = _banded(n, None)                                     # NaN inside too: an unwritten region cannot pass
        vin, vout = xin[GUARD:GUARD + n].view(B, 64, H, W), yout[GUARD:GUARD + n].view(B, 64, H, W)
        plan.debug_mid_layer(layer, vin, vout, rows=rows)
        torch.cuda.synchronize()
        assert _bands_intact(xin, n) and _bands_intact(yout, n), (mode, row[0], layer)
        assert torch.equal(xin[GUARD:GUARD + n], xb)
        assert torch.isfinite(vout).all(), (mode, row[0], layer, 'unwritten or non-finite output')
        pre, mag = _layer_ref(w, H, W, layer)
        ref = F.leaky_relu(pre, slope) if slope else F.relu(pre)
        rt = _ratio(vout, ref[:K].cuda(), mag[:K].cuda(), K)
        print(f'KAPPA form={mode} row={row[0]} act={act} layer={layer} ratio={rt:.3f}')
        worst = max(worst, rt)
    assert worst <= KAPPA[mode], (mode, row[0], act, worst)


@pytest.mark.parametrize('row', [r for r in W44_ROWS], ids=[r[0] for r in W44_ROWS])
def test_fused_last_vs_float64(monkeypatch, row):
    """The last middle layer with the 64 -> 1 output conv fused in (`debug_fused_last`, mode 5, ReLU): the 6 x 6 patches,
    added up, against the float64 output conv of the float64 layer computed from the layer's INPUT; NaN bands around input and
    patch buffer intact, the patch buffer (NaN beforehand) fully written."""
    H, W, B, rows = _geometry(5, row)
    w = _weights()
    plan = _plan(monkeypatch, w, H, W, B, 5)
    K = _distinct(B)
    n, npart = B * 64 * H * W, B * (H // 4) * (W // 4) * 36
    x = torch.from_numpy(_layer_input(H, W)[:K]).cuda()
    xb = x.repeat((B + K - 1) // K, 1, 1, 1)[:B].reshape(-1)
    xin, pb = _banded(n, xb), _banded(npart, None)
    vin, vpart = xin[GUARD:GUARD + n].view(B, 64, H, W), pb[GUARD:GUARD + npart]
    plan.debug_fused_last(vin, vpart, rows=rows)
    torch.cuda.synchronize()
    assert _bands_intact(xin, n) and _bands_intact(pb, npart)
    assert torch.equal(xin[GUARD:GUARD + n], xb)
    assert torch.isfinite(vpart).all()
    # patch (py, px) of block (by, bx) is pixel (4 by + py - 1, 4 bx + px - 1): fold onto the image padded by one
    cols = vpart.view(B, (H // 4) * (W // 4), 36).permute(0, 2, 1).double()
    r = F.fold(cols, output_size=(H + 2, W + 2), kernel_size=6, stride=4)[:, :, 1:H + 1, 1:W + 1]
    pre, mag = _layer_ref(w, H, W, 2)
    wl = w['conv4.weight']
    ref = od.conv_layer64(F.relu(pre), wl)
    bmag = od.conv_layer64(mag, np.abs(wl))
    rt = _ratio(r, ref[:K].cuda(), bmag[:K].cuda(), K)
    print(f'KAPPA form=fused row={row[0]} ratio={rt:.3f}')
    assert rt <= KAPPA_FUSED, (row[0], rt)


# ------------------------------------------------------------------------------------------------------ whole prox
PROX_ROWS = {5: ['tail-8x64', 'b-plain-8x64', 'wt-8x64', 'e-8x64', 'e-128x128'], 6: ['b-plain-8x64', 'e-8x64'],
             0: ['one-8x32', 'plain-8x32', 'w96-40x96'], 1: ['one-8x32', 'plain-8x32', 'w96-40x96']}
PROX_CASES = [(m, name) for m in (5, 6, 0, 1) for name in PROX_ROWS[m]]


def _images(H, W, B, seed):
    """B images built from 4 distinct ones in [0, 1) plus noise (numpy float64 [K, H, W], tiled [B, H, W])."""
    K = _distinct(B)
    rng = np.random.default_rng(seed + H + W)
    base = rng.random((K, H, W)) * 0.8 + 0.1 + 0.05 * rng.standard_normal((K, H, W))
    return base, np.concatenate([base] * ((B + K - 1) // K))[:B]


@pytest.mark.parametrize('mode,name', PROX_CASES, ids=[f'{m}-{n}' for m, n in PROX_CASES])
def test_prox_vs_float64(monkeypatch, mode, name):
    """The whole prox at dispatch-edge geometries against oracle.dncnn_forward64 (5-layer net with BatchNorm, folded by the
    plan and applied unfolded by the oracle): `forward` with edge fusion on and off, `denoise` with float32 and float64 storage
    and `xrec` (image and per-item squared error), and `mmo_denoise` on a net with biases, LeakyReLU and transposed taps."""
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    H, W, B, _ = _geometry(mode, ROW[name])
    K = _distinct(B)
    idx = np.arange(B) % K
    w = random_dncnn_weights(5, seed=17)
    base, z = _images(H, W, B, 3)
    # forward: the raw residual
    x32 = base.astype(np.float32)
    ref = od.dncnn_forward64(w, x32)
    scale = max(1.0, np.abs(ref).max())
    xb = torch.from_numpy(x32[idx]).cuda()
    for fusion in (True, False):
        r = _plan(monkeypatch, w, H, W, B, mode, fusion).forward(xb).cpu().numpy().astype(np.float64)
        err = np.abs(r - ref[idx]).max()
        assert err <= 2e-5 * scale, (mode, name, fusion, err)
    # denoise: the RealSN_DnCNN wrapper arithmetic around the net (oracle.DnCNNDenoiser, sigma_net = 15)
    lo, hi = base.min(axis=(1, 2), keepdims=True), base.max(axis=(1, 2), keepdims=True)
    srange = 1.0 + 15 / 255.0 / 2.0
    sshift = (1.0 - srange) / 2.0
    xt = (base - lo) / (hi - lo) * srange + sshift
    den = ((xt - od.dncnn_forward64(w, xt.astype(np.float32)) - sshift) / srange) * (hi - lo) + lo
    xrec = np.clip(base, 0, 1)
    sse_ref = ((xrec - den) ** 2).sum(axis=(1, 2))
    plan = _plan(monkeypatch, w, H, W, B, mode)
    for dt in (torch.float32, torch.float64):
        zt = torch.from_numpy(z).to('cuda', dt)
        xr = torch.from_numpy(xrec[idx]).to('cuda', dt)
        out, sse = plan.denoise(zt, 15, xrec=xr)
        o = out.cpu().numpy().astype(np.float64)
        err = np.abs(o - den[idx]).max()
        assert err <= 2e-5, (mode, name, dt, err)
        s = sse.cpu().numpy()
        np.testing.assert_allclose(s, ((xr.cpu().numpy().astype(np.float64) - o) ** 2).sum(axis=(1, 2)), rtol=1e-10)
        np.testing.assert_allclose(s, sse_ref[idx], rtol=1e-4)
    # mmo_denoise: clip(xc + net(xc), 0, 1), xc = clip(z, 0, 1) in float32
    wm = _weights(0.01, seed=5)
    for i in (0, 4):
        wm[f'conv{i}.bias'] = (0.05 * np.random.default_rng(i).standard_normal(wm[f'conv{i}.weight'].shape[0])).astype(np.float32)
    wm['transpose_taps'] = True
    zc = np.clip(base, 0, 1).astype(np.float32).astype(np.float64)
    mref = np.clip(zc + od.dncnn_forward64(wm, zc), 0, 1)
    plan = _plan(monkeypatch, wm, H, W, B, mode)
    for dt in (torch.float32, torch.float64):
        zt = torch.from_numpy(z).to('cuda', dt)
        xr = torch.from_numpy(xrec[idx]).to('cuda', dt)
        out, sse = plan.mmo_denoise(zt, xrec=xr)
        o = out.cpu().numpy().astype(np.float64)
        err = np.abs(o - mref[idx]).max()
        assert err <= 2e-5, (mode, name, dt, err)
        np.testing.assert_allclose(sse.cpu().numpy(), ((xr.cpu().numpy().astype(np.float64) - o) ** 2).sum(axis=(1, 2)),
                                   rtol=1e-10)
