"""Time `sweep.grid_search` with the trials of a grid run one after the other against `batch_trials=True`.

    python tools/time_grid_batched.py [--items 15 120] [--reps 5] [-o profiles/grid_batched_timing.json]

Per item count: 256 x 256, f32, TV prox, pnp_svrg, T2 = 10, two outer iterations, 16 trials (4 eta x 2 mini_batch_size x
2 sigma_modifier), seeding='counter'; both arms in one process, alternating, best of `reps` after one warm-up pass of each,
wall clock between torch.cuda.synchronize() calls.  The per-trial arm is the code as it stands without the option."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def images(k, n=256, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def main():
    from pnp_svrg_amd import sweep
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--items', type=int, nargs='+', default=[15, 120])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'grid_batched_timing.json'))
    a = ap.parse_args()
    grid = {'eta': [100.0, 250.0, 500.0, 1000.0], 'mini_batch_size': [1000, 4000], 'sigma_modifier': [1.0, 1.3]}
    imgs = images(12)
    tables = []
    for n_items in a.items:
        alphas = np.linspace(0.1, 1.0, 10)[:-(-n_items // 12)]
        items = sweep.make_items(12, alphas, [20.0])[:n_items]
        for i, it in enumerate(items):
            it['id'] = i
        mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'svrg', 'tv', n_inner=20, T2=10, seeding='counter', max_batch=128)

        def timed(batch_trials):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = sweep.grid_search(items, mk, grid, batch_trials=batch_trials)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, rows
        (_, r0), (_, r1) = timed(False), timed(True)                  # warm-up; the two arms must agree
        same = [(x['id'], x['loss'], x['params']) for x in r0] == [(x['id'], x['loss'], x['params']) for x in r1]
        t = {False: [], True: []}
        for _ in range(a.reps):
            for arm in (False, True):
                t[arm].append(timed(arm)[0])
        row = {'items': n_items, 'trials': len(sweep.grid_points(grid)), 'per_trial_s': min(t[False]), 'batched_s': min(t[True]),
               'ratio': min(t[False]) / min(t[True]), 'rows_equal': same, 'per_trial_all_s': t[False], 'batched_all_s': t[True]}
        print(json.dumps(row))
        tables.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'grid': grid, 'tables': tables}, f, indent=1)


if __name__ == '__main__':
    main()
