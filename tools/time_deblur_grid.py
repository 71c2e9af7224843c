"""Time a Deblur + NLM + pnp_saga grid run one trial after the other against `batch_trials=True` on a `wide_trials` runner
(DESIGN 9.2).

    python tools/time_deblur_grid.py [--items 4] [--reps 2] [--arm both|serial|batched] [--pkg-root DIR] [-o profiles/deblur_grid_timing.json]

The cell of config 4: Deblur "Minimal", NLM prox, pnp_saga, 256 x 256, f32, seeding='counter'; `--n-inner` inner iterations,
hist_size `--hist`, a grid of eta x mini_batch_size x sigma_modifier (3 x 2 x 2 = 12 trials).  Wall clock of
`sweep.grid_search` between torch.cuda.synchronize() calls, best of `reps` after one warm-up pass of each arm; with both arms in
one process they alternate and their rows are compared.  `--pkg-root DIR` imports `pnp_svrg_amd` from DIR instead of this tree
(the serial arm of another commit: `--arm serial`, which passes no `wide_trials`)."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def images(k, n=256, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--items', type=int, default=4)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--n-inner', type=int, default=20)
    ap.add_argument('--hist', type=int, default=50)
    ap.add_argument('--arm', default='both', choices=['both', 'serial', 'batched'])
    ap.add_argument('--pkg-root', default=ROOT)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'deblur_grid_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    from pnp_svrg_amd import sweep
    grid = {'eta': [1e6, 2.5e6, 5e6], 'mini_batch_size': [1000, 3000], 'sigma_modifier': [1.0, 1.3]}
    imgs = images(a.items)
    items = sweep.make_items(a.items, [1.0], [20.0])
    kw = dict(n_inner=a.n_inner, hist_size=a.hist, seeding='counter', max_batch=128)
    if a.arm != 'serial':
        kw['wide_trials'] = True
    mk = functools.partial(sweep.make_runner, imgs, 'deblur', 'saga', 'nlm', **kw)

    def timed(batch_trials):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = sweep.grid_search(items, mk, grid, batch_trials=batch_trials)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rows
    arms = {'both': (False, True), 'serial': (False,), 'batched': (True,)}[a.arm]
    key = lambda rows: [(x['id'], x['loss'], x['params']) for x in rows]
    warm = {arm: key(timed(arm)[1]) for arm in arms}                  # warm-up; two arms must agree
    t = {arm: [] for arm in arms}
    for _ in range(a.reps):
        for arm in arms:
            t[arm].append(timed(arm)[0])
    row = {'items': a.items, 'trials': len(sweep.grid_points(grid)), 'n_inner': a.n_inner, 'hist_size': a.hist,
           'pkg_root': os.path.abspath(a.pkg_root), 'rows': warm[arms[0]]}
    if False in t:
        row.update(per_trial_s=min(t[False]), per_trial_all_s=t[False])
    if True in t:
        row.update(batched_s=min(t[True]), batched_all_s=t[True])
    if len(arms) == 2:
        row.update(ratio=min(t[False]) / min(t[True]), rows_equal=warm[False] == warm[True])
    print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'grid': grid, 'result': row}, f, indent=1)


if __name__ == '__main__':
    main()
