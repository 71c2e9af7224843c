"""Setup time of a CSMRI sweep batch, host-built against device-generated: wall clock of `runner.prepare(items)` for
make_runner(seeding='generator') (per-item NumPy + upload) and seeding='device' (pnp_csmri_generate), 256 x 256, f32, TV
prox, B = 15, 120, 1024; the two modes alternate in one process, every measurement bracketed by torch.cuda.synchronize, best
of 5 after one warm-up of each.  Also the bare `plan.generate` launch sequence timed by hipEvents (best of 5 x 20 calls).
Bytes per item are counted from shapes.

    python tools/time_csmri_generate.py [out.json]
"""
import json
import os
import sys
import time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_svrg_amd import sweep
from pnp_svrg_amd.engine import CsmriBatch

H = W = 256
ROUNDS, CALLS = 5, 20


def images(n):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(n):
        x = rng.random((H, W))
        p = np.pad(x, 2, mode='wrap')
        out.append(sum(p[i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del keep
    return dt


imgs = images(12)
rows = []
for B in (15, 120, 1024):
    items = sweep.make_items(12, [0.1 * k for k in range(1, 11)], [20.0], seeds=range(-(-B // 120)))[:B]
    assert len(items) == B
    runners = {m: sweep.make_runner(imgs, 'csmri', 'svrg', 'tv', eta=5e2, n_inner=10, mini_batch_size=1000, T2=10, H=H, W=W,
                                    max_batch=B, seeding=m) for m in ('generator', 'device')}
    best = {m: float('inf') for m in runners}
    for m, r in runners.items():                                  # warm-up: code objects, allocator, the image upload
        wall(lambda: r.prepare(items))
    for _ in range(ROUNDS):
        for m, r in runners.items():                              # alternate
            best[m] = min(best[m], wall(lambda: r.prepare(items)))
    up = CsmriBatch.upload_images(imgs, H, W)
    b = CsmriBatch.generate(up, items, H, W)
    par = [torch.zeros(B, dtype=torch.int32, device='cuda'), torch.full((B,), 2 ** 31, dtype=torch.int64, device='cuda'),
           torch.full((B,), 0.01, dtype=torch.float64, device='cuda'), torch.zeros(B, dtype=torch.int64, device='cuda'),
           torch.arange(B, dtype=torch.int64, device='cuda')]
    ev = float('inf')
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            b.plan.generate(up, *par)
        e1.record()
        torch.cuda.synchronize()
        ev = min(ev, e0.elapsed_time(e1) / CALLS)
    row = dict(B=B, H=H, W=W, dtype='float32', prepare_generator_s=best['generator'], prepare_device_s=best['device'],
               ratio=best['generator'] / best['device'], generate_launches_ms=ev,
               note='generate_launches_ms includes the output allocations of ops.CsmriPlan.generate')
    rows.append(row)
    print(json.dumps(row))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(rows, f, indent=1)
