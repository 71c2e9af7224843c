"""Time a pnp_saga grid that varies hist_size, grouped by hist_size (`batch_trials=True`: one batch per value) against one batch for
the whole grid (`batch_hist=True` on a `hist_trials` runner).

    python tools/time_hist_grid.py [--items 15 120] [--reps 5] [--n-inner 48] [--nlm-items 15] [--nlm-inner 8] [--nlm-reps 1]
                                   [-o profiles/hist_grid_timing.json]

CSMRI 256 x 256, f32, TV prox, pnp_saga, a grid of 4 eta x 4 hist_size (5, 8, 12, 15), seeding='counter', 15 and 120 items.  Arm A:
`grid_search(batch_trials=True)` -- four batches of 4 x items problems, each with a table of its own hist_size.  Arm B: the same with
`batch_hist=True` -- one batch of 16 x items problems whose table is dense over 15 rows (in slabs capped by max_table_bytes).  One
process, arms alternating, best of `--reps` after one warm-up pass of each, wall clock between torch.cuda.synchronize() calls; the
rows of both arms must be equal.  Then the same pair on the Deblur + NLM cell (config 4's, where pnp_saga_table_update_hist_pp is the
path): `--nlm-items` items, `--nlm-inner` iterations, `--nlm-reps` timed passes (0 skips the cell)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {'eta': [5e2, 1e3, 2e3, 4e3], 'hist_size': [5, 8, 12, 15]}
NLM_ETA = [3e3, 6e3, 1e4, 2e4]


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


def time_grid(sweep, cell, n_items, n_inner, reps):
    imgs = images(min(n_items, 15))
    if cell == 'csmri-tv':
        items = sweep.make_items(len(imgs), [0.2], [20.0], seeds=range(-(-n_items // len(imgs))))[:n_items]
        mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'saga', 'tv', n_inner=n_inner, mini_batch_size=1000, seeding='counter',
                               max_batch=128, wide_trials=True, hist_trials=True)
        grid = GRID
    else:
        items = sweep.make_items(len(imgs), [1.0], [20.0], seeds=range(-(-n_items // len(imgs))))[:n_items]
        mk = functools.partial(sweep.make_runner, imgs, 'deblur', 'saga', 'nlm', n_inner=n_inner, mini_batch_size=1000, seeding='counter',
                               max_batch=128, wide_trials=True, hist_trials=True)
        grid = dict(GRID, eta=NLM_ETA)
    rows, slabs = {}, {}

    def run(name):
        rows[name] = [(r['id'], r['loss'], r['params']) for r in
                      sweep.grid_search(items, mk, grid, batch_trials=True, batch_hist=name == 'one_batch')]
    t = best_of({name: functools.partial(run, name) for name in ('grouped_by_hist', 'one_batch')}, reps)
    itemsize, n = 4, min(n_items, 128)
    for name, h in (('grouped_by_hist', None), ('one_batch', max(grid['hist_size']))):         # the slabs the table cap allows
        per = [sweep.table_trial_cap(n, hh, 256 * 256, itemsize) for hh in ([h] if h else grid['hist_size'])]
        slabs[name] = [len(sweep.trial_slabs(16 if h else 4, n, 1024, cap)) for cap in per]
    row = {'cell': cell, 'items': n_items, 'trials': len(sweep.grid_points(grid)), 'n_inner': n_inner, 'slabs_per_chunk': slabs}
    for name, ts in t.items():
        row.update({name + '_s': min(ts), name + '_all_s': ts})
    row.update(ratio=row['grouped_by_hist_s'] / row['one_batch_s'], rows_equal=rows['grouped_by_hist'] == rows['one_batch'])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--items', type=int, nargs='*', default=[15, 120])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-inner', type=int, default=48)
    ap.add_argument('--nlm-items', type=int, default=15)
    ap.add_argument('--nlm-inner', type=int, default=8)
    ap.add_argument('--nlm-reps', type=int, default=1)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'hist_grid_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import sweep
    res = {'device': torch.cuda.get_device_name(0), 'grid': GRID, 'nlm_eta': NLM_ETA, 'reps': a.reps, 'nlm_reps': a.nlm_reps, 'grid_search': []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    for n in a.items:
        row = time_grid(sweep, 'csmri-tv', n, a.n_inner, a.reps)
        res['grid_search'].append(row)
        print(json.dumps(row), flush=True)
        save()
    if a.nlm_reps > 0:
        row = time_grid(sweep, 'deblur-nlm', a.nlm_items, a.nlm_inner, a.nlm_reps)
        res['grid_search'].append(row)
        print(json.dumps(row), flush=True)
    save()


if __name__ == '__main__':
    main()
