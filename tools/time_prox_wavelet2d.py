"""Timing of pnp_prox_wavelet2d next to pnp_prox_tv (sigma_in given, xrec / sse on, in place), f32 256 x 256, alternating
the two in one process: hipEvents around N calls after warm-up, best of ROUNDS rounds.  Bytes per image are counted from
shapes: both read z and xrec and write z once (3 * H * W * 4); the 2-D prox reads z a second time (pass 2), a re-read
the caches may or may not absorb -- the HBM fraction is given for both counts.

    python tools/time_prox_wavelet2d.py [out.json]
"""
import json
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_svrg_amd import ops

HBM_PEAK = 8.0e12                                   # bytes / s, MI355X HBM3E
N, ROUNDS, H, W = 200, 5, 256, 256


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3            # us per call


rows = []
for B in (1, 32, 120, 1024):
    z0 = torch.rand(B, H, W, device='cuda')
    z = z0.clone()
    xrec = torch.rand_like(z)
    sig = torch.full((B,), 0.05, device='cuda')
    sse = torch.empty(B, dtype=torch.float64, device='cuda')
    so = torch.empty(B, device='cuda')
    fns = {'prox_tv': lambda: ops.prox_tv(z, sigma_in=sig, xrec=xrec, out=z, sse=sse, sigma_out=so),
           'prox_wavelet2d': lambda: ops.prox_wavelet2d(z, sigma_in=sig, xrec=xrec, out=z, sse=sse, sigma_out=so)}
    best = {k: float('inf') for k in fns}
    for k, fn in fns.items():                       # warm-up
        for _ in range(20):
            fn()
    for _ in range(ROUNDS):
        for k, fn in fns.items():                   # alternate
            z.copy_(z0)
            torch.cuda.synchronize()
            best[k] = min(best[k], timeit(fn))
    once, twice = 3 * H * W * 4, 4 * H * W * 4
    row = dict(B=B, dtype='float32', H=H, W=W, us_prox_tv=best['prox_tv'], us_prox_wavelet2d=best['prox_wavelet2d'],
               ratio=best['prox_wavelet2d'] / best['prox_tv'], bytes_per_image_prox_tv=once, bytes_per_image_prox_wavelet2d=twice,
               hbm_fraction_prox_tv=once * B / (best['prox_tv'] * 1e-6) / HBM_PEAK,
               hbm_fraction_prox_wavelet2d=twice * B / (best['prox_wavelet2d'] * 1e-6) / HBM_PEAK)
    rows.append(row)
    print(json.dumps(row))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(rows, f, indent=1)
