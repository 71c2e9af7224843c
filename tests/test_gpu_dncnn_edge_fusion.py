"""The DnCNN's 64 -> 1 output conv fused into the last F(4x4,3x3) middle layer (conv mode 5, ReLU, float32): every 4 x 4
block of that layer writes the 6 x 6 patch of output partials its activations feed, and a small kernel adds the patches
that cover a pixel.  PNP_DNCNN_EDGE_FUSION=0 (read when a plan is created) selects the separate last-layer kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _plan(monkeypatch, w, H, W, B, fused, **kw):
    from pnp_svrg_amd import ops
    monkeypatch.setenv('PNP_DNCNN_EDGE_FUSION', '1' if fused else '0')
    return ops.DncnnPlan(w, H, W, B, **kw)


@pytest.mark.parametrize('B', [1, 3, 5, 120])
def test_fused_last_layer_matches_unfused(monkeypatch, B):
    """Fusion on vs off: the network residual, the denoised iterate and the squared error agree to 1e-6 relative (the last
    layer's sums change order); B = 1 runs the 4 x 64 region form only, 3 and 5 both forms, 120 full waves of 8 x 64."""
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    w = random_dncnn_weights(17, seed=3)
    rng = np.random.default_rng(B)
    x = torch.from_numpy(rng.random((B, 256, 256), dtype=np.float32)).cuda()
    xrec = torch.from_numpy(rng.random((B, 256, 256), dtype=np.float32)).cuda()
    on, off = _plan(monkeypatch, w, 256, 256, B, True), _plan(monkeypatch, w, 256, 256, B, False)
    r_on, r_off = on.forward(x), off.forward(x)
    z_on, sse_on = on.denoise(x, 15.0, xrec=xrec)
    z_off, sse_off = off.denoise(x, 15.0, xrec=xrec)
    torch.cuda.synchronize()
    assert torch.isfinite(r_on).all() and torch.isfinite(z_on).all()
    assert not torch.equal(r_on, r_off)                                        # really the other path
    dr = (r_on - r_off).abs().max().item() / r_off.abs().max().item()
    dz = (z_on - z_off).abs().max().item() / z_off.abs().max().item()
    ds = ((sse_on - sse_off).abs() / sse_off.abs()).max().item()
    print('B=%d  rel. max |dr| %.2e  |dz| %.2e  |dsse| %.2e' % (B, dr, dz, ds))
    assert dr <= 1e-6 and dz <= 1e-6 and ds <= 1e-6


def test_fused_last_layer_batch_invariant(monkeypatch):
    """An item's fused result does not depend on the batch it runs in nor on the region form: B = 1 (4 x 64 regions
    only) equals every item of a B = 5 batch (items 0-3 in 8 x 64 regions, item 4 in the 4 x 64 tail launch), bit for bit;
    and the fused path is run-to-run identical."""
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    w = random_dncnn_weights(17, seed=4)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.random((5, 256, 256), dtype=np.float32)).cuda()
    p5 = _plan(monkeypatch, w, 256, 256, 5, True)
    p1 = _plan(monkeypatch, w, 256, 256, 1, True)
    r5 = p5.forward(x).cpu().numpy()
    assert np.array_equal(r5, p5.forward(x).cpu().numpy())
    for i in range(5):
        r1 = p1.forward(x[i:i + 1].contiguous()).cpu().numpy()
        assert np.array_equal(r1[0], r5[i]), i


def test_fused_last_layer_guard_bands(monkeypatch):
    """The fused layer on caller-provided buffers with NaN guard bands around its input and its patch buffer (both region
    forms, the tail path, shapes whose regions all touch an edge): (a) every canary intact -- nothing written outside the
    patch buffer; (b) the patches, added up, equal the float64 3x3 conv of the same layer's activations."""
    import torch.nn.functional as F
    from pnp_svrg_amd.denoisers import random_dncnn_weights
    w = random_dncnn_weights(4, seed=9)
    wl = torch.from_numpy(np.asarray(w['conv3.weight'], np.float64).reshape(1, 64, 3, 3)).cuda()
    rng = np.random.default_rng(21)
    GUARD = 1 << 18
    cases = [(72, 128, 3, 0), (256, 256, 5, 0), (256, 256, 5, 1), (256, 256, 5, 2), (8, 64, 1, 0), (64, 192, 2, 0)]
    for (H, Wd, B, rows) in cases:
        plan = _plan(monkeypatch, w, H, Wd, B, True, winograd=5)
        n, npart = B * 64 * H * Wd, B * (H // 4) * (Wd // 4) * 36
        x = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()

        def banded(nfloats, fill):
            t = torch.full((nfloats + 2 * GUARD,), float('nan'), dtype=torch.float32, device='cuda')
            t[GUARD:GUARD + nfloats] = fill
            return t
        xin, pb = banded(n, x), banded(npart, 0.0)
        vin, vpart = xin[GUARD:GUARD + n].view(B, 64, H, Wd), pb[GUARD:GUARD + npart]
        plan.debug_fused_last(vin, vpart, rows=rows)
        act = torch.empty((B, 64, H, Wd), dtype=torch.float32, device='cuda')
        plan.debug_mid_layer(plan.n_mid - 1, x.view(B, 64, H, Wd), act, rows=rows)
        torch.cuda.synchronize()
        for t, nn in ((xin, n), (pb, npart)):
            assert torch.isnan(t[:GUARD]).all() and torch.isnan(t[GUARD + nn:]).all(), (H, Wd, B, rows)
        assert torch.equal(xin[GUARD:GUARD + n], x)
        assert torch.isfinite(vpart).all()
        # patch (py, px) of block (by, bx) is pixel (4 by + py - 1, 4 bx + px - 1): fold onto the image padded by one
        cols = vpart.view(B, (H // 4) * (Wd // 4), 36).permute(0, 2, 1).double()
        r = F.fold(cols, output_size=(H + 2, Wd + 2), kernel_size=6, stride=4)[:, 0, 1:H + 1, 1:Wd + 1]
        ref = F.conv2d(act.double(), wl, padding=1)[:, 0]
        err = (r - ref).abs().max().item()
        assert err <= 1e-5 * max(1.0, ref.abs().max().item()), (H, Wd, B, rows, err)
