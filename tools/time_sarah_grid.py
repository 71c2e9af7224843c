"""Time (a) the per-problem combine `pnp_axpbypcz_pp` against what it replaces and (b) a 16-trial pnp_sarah grid run one trial after
the other against `batch_trials=True` on a `sarah_trials` runner.

    python tools/time_sarah_grid.py [--arm both|serial|batched|combine] [--pkg-root DIR] [--serial-json FILE] [-o profiles/sarah_grid_timing.json]

(a) the combine out = x + b_p * y alone, f32, B = 240 problems of 64 x 64 and of 256 x 256, three arms: ONE `pnp_axpbypcz_pp` launch
    with a [B] coefficient; B plain `pnp_axpbypcz` launches on the problems' views (what the commit before this one executes); ONE
    plain whole-batch launch with a scalar (the same bytes: the yardstick).  `--calls` calls per timed region, reported per call.
(b) CSMRI 256 x 256, TV prox, pnp_sarah, T2 = 10, two outer iterations, 15 items, seeding='counter', a grid of 4 eta x 2
    mini_batch_size x 2 sigma_modifier.  Wall clock of `sweep.grid_search`.
One process, arms alternating, best of `--reps` (5) after one warm-up pass of each arm, wall clock between torch.cuda.synchronize()
calls.  `--pkg-root DIR` imports `pnp_svrg_amd` from DIR instead of this tree: the serial arm of the commit before this one is
`--arm serial --pkg-root <that tree> -o FILE` (it passes no `sarah_trials` and skips (a)); `--arm batched --serial-json FILE` then
records both and their ratio."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {'eta': [5e2, 1e3, 2e3, 4e3], 'mini_batch_size': [500, 1000], 'sigma_modifier': [1.0, 1.3]}


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


def time_combine(ops, B, n, reps, calls):
    x, y = (torch.rand((B, n, n), dtype=torch.float32, device='cuda') for _ in range(2))
    out = torch.empty_like(x)
    coef = np.linspace(-2.0, -0.5, B)
    vec = torch.from_numpy(coef).cuda()
    host = [float(v) for v in coef]

    def pp():
        for _ in range(calls):
            ops.axpbypcz(1.0, x, vec, y, out=out)

    def per_problem():
        for _ in range(calls):
            for p in range(B):
                ops.axpbypcz(1.0, x[p], host[p], y[p], out=out[p])

    def whole():
        for _ in range(calls):
            ops.axpbypcz(1.0, x, -1.25, y, out=out)
    t = best_of({'pp_one_launch': pp, 'plain_per_problem': per_problem, 'plain_whole_batch': whole}, reps)
    row = {'B': B, 'n': n, 'calls_per_region': calls, 'bytes_per_call': 3 * x.numel() * 4}
    for name, ts in t.items():
        row[name + '_us'] = min(ts) / calls * 1e6
        row[name + '_all_us'] = [v / calls * 1e6 for v in ts]
    row['pp_over_whole'] = row['pp_one_launch_us'] / row['plain_whole_batch_us']
    row['per_problem_over_pp'] = row['plain_per_problem_us'] / row['pp_one_launch_us']
    return row


def time_grid(sweep, arm, n_items, reps):
    imgs = images(n_items)
    items = sweep.make_items(n_items, [0.2], [20.0])
    kw = dict(n_inner=20, T2=10, seeding='counter', max_batch=128)
    if arm != 'serial':
        kw['sarah_trials'] = True
    mk = functools.partial(sweep.make_runner, imgs, 'csmri', 'sarah', 'tv', **kw)
    names = {'both': ('per_trial', 'batched'), 'serial': ('per_trial',), 'batched': ('batched',)}[arm]
    rows = {}

    def run(name):
        rows[name] = [(r['id'], r['loss'], r['params']) for r in sweep.grid_search(items, mk, GRID, batch_trials=name == 'batched')]
    t = best_of({name: functools.partial(run, name) for name in names}, reps)
    row = {'items': n_items, 'trials': len(sweep.grid_points(GRID)), 'n_inner': 20, 'T2': 10, 'rows': rows[names[0]]}
    for name, ts in t.items():
        row.update({name + '_s': min(ts), name + '_all_s': ts})
    if len(names) == 2:
        row.update(ratio=row['per_trial_s'] / row['batched_s'], rows_equal=rows['per_trial'] == rows['batched'])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--items', type=int, default=15)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--arm', default='both', choices=['both', 'serial', 'batched', 'combine'])
    ap.add_argument('--pkg-root', default=ROOT)
    ap.add_argument('--serial-json', default=None)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'sarah_grid_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    from pnp_svrg_amd import ops, sweep
    res = {'device': torch.cuda.get_device_name(0), 'grid': GRID, 'reps': a.reps}
    if a.arm != 'serial':
        res['combine'] = [time_combine(ops, 240, n, a.reps, a.calls) for n in (64, 256)]
        for row in res['combine']:
            print(json.dumps(row))
    if a.arm != 'combine':
        row = time_grid(sweep, a.arm, a.items, a.reps)
        if a.serial_json:
            with open(a.serial_json) as f:
                ser = json.load(f)['grid_search']
            row.update(per_trial_s=ser['per_trial_s'], per_trial_all_s=ser['per_trial_all_s'], per_trial_from='the serial arm file',
                       ratio=ser['per_trial_s'] / row['batched_s'], rows_equal=ser['rows'] == json.loads(json.dumps(row['rows'])))
        res['grid_search'] = row
        print(json.dumps({k: v for k, v in row.items() if k != 'rows'}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
