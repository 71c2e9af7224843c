"""Time a pnp_sarah grid that varies T2, grouped by T2 (`batch_trials=True`: one batch per T2 value) against one batch for the whole
grid (`batch_T2=True` on a `sarah_t2_trials` runner).

    python tools/time_sarah_t2_grid.py [--items 15 120] [--reps 5] [--paths fused streaming] [-o profiles/sarah_t2_grid_timing.json]

CSMRI 256 x 256, f32, TV prox, pnp_sarah, a grid of 4 eta x 4 T2 (T2 in 8, 10, 12, 16), n_inner = 48, seeding='counter', 15 and 120
items.  Arm A (`grouped_by_T2`): `grid_search(batch_trials=True)` -- four batches of 4 x items problems on scalar-T2 engines.  Arm B
(`one_batch`): the same with `batch_T2=True` -- one batch of 16 x items problems (in slabs of at most 1024) on a
SarahEngine(T2=[B], split_log=True), advanced by `run_span`.  Two paths, each timed with both arms:
  fused      runners made with sarah_fused=True: arm A replays hipGraphs of whole outer iterations where n_inner is a multiple of T2
             (eager one-kernel steps for T2 = 10), arm B runs launches of pnp_csmri_sarah_span_pp;
  streaming  the streaming kernels: arm A steps eagerly, arm B steps eagerly as well and pays the whole-batch outer step (full
             gradient + prox) at every step that is a multiple of any T2 of the slab.
One process, arms alternating, best of `--reps` after one warm-up pass of each, wall clock between torch.cuda.synchronize() calls;
the rows of both arms must be equal."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {'eta': [5e2, 1e3, 2e3, 4e3], 'T2': [8, 10, 12, 16]}
N_INNER = 48


def images(k, n=256, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def best_of(arms, reps):
    """arms: name -> thunk.  One warm-up pass of each, then `reps` rounds with the arms alternating -> name -> [seconds]."""
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for fn in arms.values():
        timed(fn)
    t = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            t[name].append(timed(fn))
    return t


def time_grid(sweep, n_items, reps, path):
    imgs = images(min(n_items, 15))
    items = sweep.make_items(len(imgs), [0.2], [20.0], seeds=range(-(-n_items // len(imgs))))[:n_items]
    mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'sarah', 'tv', n_inner=N_INNER, mini_batch_size=1000, seeding='counter',
                           max_batch=128, sarah_trials=True, sarah_t2_trials=True, sarah_fused=path == 'fused')
    rows = {}

    def run(name):
        rows[name] = [(r['id'], r['loss'], r['params']) for r in
                      sweep.grid_search(items, mk, GRID, batch_trials=True, batch_T2=name == 'one_batch')]
    t = best_of({name: functools.partial(run, name) for name in ('grouped_by_T2', 'one_batch')}, reps)
    row = {'path': path, 'items': n_items, 'trials': len(sweep.grid_points(GRID)), 'n_inner': N_INNER}
    for name, ts in t.items():
        row.update({name + '_s': min(ts), name + '_all_s': ts})
    row.update(ratio=row['grouped_by_T2_s'] / row['one_batch_s'], rows_equal=rows['grouped_by_T2'] == rows['one_batch'])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--items', type=int, nargs='+', default=[15, 120])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--paths', nargs='+', default=['fused', 'streaming'], choices=['fused', 'streaming'])
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'sarah_t2_grid_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import sweep
    res = {'device': torch.cuda.get_device_name(0), 'grid': GRID, 'reps': a.reps, 'grid_search': []}
    for path in a.paths:
        for n in a.items:
            row = time_grid(sweep, n, a.reps, path)
            res['grid_search'].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
