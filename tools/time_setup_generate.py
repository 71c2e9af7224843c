"""Setup time of Deblur and phase-retrieval sweep batches, host-built against device-generated: wall clock of
`runner.prepare(items)` for make_runner(seeding='generator') (per-item NumPy + upload; unchanged, so it stands for the code
before seeding='counter' existed) and seeding='counter' (pnp_deblur_generate / pnp_pr_generate + pnp_pr_spectral_init_batch).
Shapes: Deblur 256 x 256 (B = 64), PR 32 x 32 x 5120 at B = 64, PR 128 x 128 x 8192 at B = 4; f32, TV prox; the two modes alternate
in one process, every measurement bracketed by torch.cuda.synchronize, best of 5 after one warm-up of each.  Also, by hipEvents:
the A generation alone (bytes written / time against the HBM peak of 8 TB/s) and the batched spectral initialisation (time per
step against the two-pass byte count 2 M N sizeof).

    python tools/time_setup_generate.py [out.json] [--host-128]

Without --host-128 the host mode is not timed at 128 x 128 x 8192 (134 M normals, a 1 GiB float64 matrix and several hundred
host GEMV pairs per item: minutes per item).
"""
import json
import os
import sys
import time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnp_svrg_amd import ops, sweep
from pnp_svrg_amd.engine import PrBatch

ROUNDS = 5
HBM_PEAK = 8.0e12


def images(n_img, n):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(n_img):
        x = rng.random((n, n))
        p = np.pad(x, 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del keep
    return dt


def events(fn, calls):
    best = float('inf')
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls)
    return best * 1e-3


rows = []
for problem, n, alpha, B in (('deblur', 256, 1.0, 64), ('pr', 32, 5.0, 64), ('pr', 128, 0.5, 4)):
    imgs = images(4, n)
    items = sweep.make_items(4, [alpha], [20.0], seeds=range(-(-B // 4)))[:B]
    kw = dict(eta=1e7 if problem == 'deblur' else 0.05, n_inner=10, mini_batch_size=200, T2=10, H=n, W=n, max_batch=B)
    big = (problem, n) == ('pr', 128)
    modes = ('counter',) if big and '--host-128' not in sys.argv else ('generator', 'counter')   # (host mode: minutes per item there)
    runners = {m: sweep.make_runner(imgs, problem, 'svrg', 'tv', seeding=m, **kw) for m in modes}
    best = {m: float('inf') for m in runners}
    for m, r in runners.items():                                        # warm-up: code objects, allocator, the image upload
        if not (big and m == 'generator'):
            wall(lambda: r.prepare(items))
    for _ in range(1 if big else ROUNDS):
        for m, r in runners.items():                                    # alternate
            best[m] = min(best[m], wall(lambda: r.prepare(items)))
    row = dict(problem=problem, H=n, W=n, B=B, dtype='float32', prepare_generator_s=best.get('generator'), prepare_counter_s=best['counter'],
               ratio=best['generator'] / best['counter'] if 'generator' in best else None)
    if problem == 'pr':
        M = sweep.pr_num_meas(alpha, n, n)
        up = PrBatch.upload_images(imgs, n, n)
        b = PrBatch.generate(up, items, n, n, M)
        par = [torch.zeros(B, dtype=torch.int32, device='cuda'), torch.full((B,), 0.01, dtype=torch.float64, device='cuda'),
               torch.zeros(B, dtype=torch.int64, device='cuda'), torch.arange(B, dtype=torch.int64, device='cuda')]
        t_gen = events(lambda: ops.pr_generate(up, *par, M), 3)
        a_bytes = B * M * n * n * 4
        iters = int(b.spec_iters.max())
        t_si = events(lambda: ops.pr_spectral_init_batch(b.A, b.Y, b.xrec, 10 ** 6, 8), 1)
        steps = -(-iters // 8) * 8
        row.update(M=M, pr_generate_s=t_gen, A_bytes=a_bytes, A_write_fraction_of_hbm_peak=a_bytes / t_gen / HBM_PEAK,
                   note='pr_generate_s covers A, the gather, |A x|, sigma and the noise, output allocations included',
                   spec_iters_max=iters, spec_iters_mean=float(b.spec_iters.mean()), spectral_init_s=t_si, steps_launched=steps,
                   s_per_step=t_si / steps, two_pass_bytes_per_step=2 * B * M * n * n * 4,
                   step_fraction_of_hbm_peak=2 * B * M * n * n * 4 / (t_si / steps) / HBM_PEAK,
                   host_syncs_per_item_before=3 * iters, host_syncs_per_batch_after=-(-iters // 8))
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1 and not sys.argv[1].startswith('--'):
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(rows, f, indent=1)
