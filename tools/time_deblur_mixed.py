"""Time a Deblur sampling-ratio sweep run as one batch per alpha (the default, grouped runner) against ONE mixed-scale batch
(`make_runner(mixed_scales=True)`).

    python tools/time_deblur_mixed.py [--reps 3] [--n-inner 20] [--sizes 120 15] [-o profiles/deblur_mixed_timing.json]

12 images x alpha 0.1 .. 1.0 = 120 items at 256 x 256, f32, seeding='counter', with pnp_svrg + the TV prox and with pnp_saga + NLM;
the same at 15 items (rank 0's share of the 120 on 8 GPUs: `sweep.shard`).  Arm A is today's runner (10 groups; at 15 items one or
two items per group), arm B the mixed runner (one batch).  A timed pass is a whole `run(items)` -- plans, generation, engines, graph
capture, iterations, read-back -- between torch.cuda.synchronize() calls; one process, one warm-up pass of each arm, then the arms
alternate and the best of `reps` passes counts.  The rows of the two arms are compared (alpha != 1.0: equal; alpha == 1.0: within
0.01 dB) and the ratio A / B is written down as it comes out, below 1 where the mixed batch is slower."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = {'svrg-tv': dict(algorithm='svrg', denoiser='tv', T2=10),
         'saga-nlm': dict(algorithm='saga', denoiser='nlm', hist_size=10)}


def images(k, n=256, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n-inner', type=int, default=20)
    ap.add_argument('--mb', type=int, default=500)              # (scale 10 % of 256 x 256 has 625 measurements)
    ap.add_argument('--sizes', type=int, nargs='+', default=[120, 15])
    ap.add_argument('--cells', nargs='+', default=list(CELLS), choices=list(CELLS))
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'deblur_mixed_timing.json'))
    a = ap.parse_args()
    from pnp_svrg_amd import sweep
    imgs = images(12)
    all_items = sweep.make_items(12, [k / 10 for k in range(1, 11)], [20.0])
    results = []
    for cell in a.cells:
        for size in a.sizes:
            items = all_items if size >= len(all_items) else sweep.shard(all_items, 0, len(all_items) // size)
            kw = dict(problem='deblur', eta=1.0, n_inner=a.n_inner, mini_batch_size=a.mb, seeding='counter', keep_trace=True,
                      max_batch=128, **CELLS[cell])
            runs = {'A': sweep.make_runner(imgs, **kw), 'B': sweep.make_runner(imgs, mixed_scales=True, **kw)}

            def timed(arm):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = runs[arm](items)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, rows
            warm = {arm: timed(arm)[1] for arm in ('A', 'B')}
            t = {'A': [], 'B': []}
            for _ in range(a.reps):
                for arm in ('A', 'B'):
                    t[arm].append(timed(arm)[0])
            equal = all(np.array_equal(x['psnr_trace'], y['psnr_trace']) and np.array_equal(x['z'], y['z'])
                        for x, y in zip(warm['A'], warm['B']) if x['item']['alpha'] != 1.0)
            ident = max([float(np.abs(x['psnr_trace'] - y['psnr_trace']).max())
                         for x, y in zip(warm['A'], warm['B']) if x['item']['alpha'] == 1.0] or [0.0])
            row = {'cell': cell, 'items': len(items), 'n_inner': a.n_inner, 'mini_batch_size': a.mb, 'reps': a.reps,
                   'grouped_s': min(t['A']), 'grouped_all_s': t['A'], 'mixed_s': min(t['B']), 'mixed_all_s': t['B'],
                   'ratio_grouped_over_mixed': min(t['A']) / min(t['B']), 'rows_equal_alpha_below_1': bool(equal),
                   'max_db_difference_alpha_1': ident}
            print(json.dumps(row), flush=True)
            results.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'cells': CELLS, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
