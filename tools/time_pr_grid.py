"""Time phase-retrieval trial batches on ONE shared matrix (csrc/pr_shared.hip) against the per-problem kernel.

    python tools/time_pr_grid.py [--G 16] [--reps 5] [--skip-grid] [-o profiles/pr_shared_timing.json]

128 x 128, M = 8192, one item, f32, G trials; both arms in one process, alternating, best of `reps` after one warm-up pass of each,
wall clock between torch.cuda.synchronize() calls.
(a) grad_full and grad_stoch_diff (mb = 1000) of `PrBatch.tile(G)` against the same G problems through pnp_pr_grad_batch on a
    materialised [G][M][N] copy of A (8 GiB at G = 16);
(b) a G-trial pnp_svrg grid (TV prox, T2 = 10, 20 inner iterations) with batch_trials=True against False.  The per-trial arm is the
    code as it stands without the option."""
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

H = W = 128
M = 8192


def image(seed=0):
    p = np.pad(np.random.default_rng(seed).random((H, W)), 2, mode='wrap')
    return sum(p[i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0


def best_of(arms, reps, inner):
    """arms: {name: callable}; every callable runs `inner` times per sample -> {name: best seconds per call}."""
    t = {k: [] for k in arms}
    for r in range(reps + 1):                                           # (pass 0: warm-up)
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                f()
            torch.cuda.synchronize()
            if r:
                t[k].append((time.perf_counter() - t0) / inner)
    return {k: min(v) for k, v in t.items()}


def main():
    from pnp_svrg_amd import sweep
    from pnp_svrg_amd.engine import PrBatch
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--G', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-grid', action='store_true')
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'pr_shared_timing.json'))
    a = ap.parse_args()
    G, imgs = a.G, [image()]
    items = sweep.make_items(1, [M / (H * W)], [20.0])
    base = PrBatch.generate(imgs, items, H, W, M)
    tiled = base.tile(G)
    rep = lambda v: v.repeat((G,) + (1,) * (v.dim() - 1)).contiguous()
    copies = PrBatch._of(xrec=rep(base.xrec), xinit=rep(base.xinit), A=rep(base.A), Y=rep(base.Y))
    z = tiled.xinit.clone()
    w = (z * 0.98).contiguous()
    out, c2 = torch.empty_like(z), torch.rand_like(z)
    res = {'H': H, 'W': W, 'M': M, 'G': G, 'dtype': 'float32', 'reps': a.reps, 'A_bytes': base.A.numel() * 4}
    slots = {}
    for name, b in (('shared', tiled), ('copies', copies)):
        slots[name] = b.minibatches(1)
        b.draw(slots[name], 1000, 3, 0, 1)
    t = best_of({'shared': lambda: tiled.grad_full(z, out), 'copies': lambda: copies.grad_full(z, out)}, a.reps, 5)
    res['grad_full'] = {'shared_ms': t['shared'] * 1e3, 'copies_ms': t['copies'] * 1e3, 'speedup': t['copies'] / t['shared'],
                        'shared_TBps_of_2_streams': 2 * res['A_bytes'] / t['shared'] / 1e12,
                        'copies_TBps_of_2G_streams': 2 * G * res['A_bytes'] / t['copies'] / 1e12}
    d = lambda b, s: b.grad_stoch_diff(z, w, s, 0, out, alpha=-1e-3, beta=1.0, c1=z, gamma=-1.0, c2=c2)
    t = best_of({'shared': lambda: d(tiled, slots['shared']), 'copies': lambda: d(copies, slots['copies'])}, a.reps, 5)
    res['grad_stoch_diff_mb1000'] = {'shared_ms': t['shared'] * 1e3, 'copies_ms': t['copies'] * 1e3, 'speedup': t['copies'] / t['shared']}
    del copies
    torch.cuda.empty_cache()
    if not a.skip_grid:
        mk = functools.partial(sweep.make_runner, imgs, 'pr', 'svrg', 'tv', n_inner=20, T2=10, H=H, W=W, seeding='counter',
                               shared_matrix=True)
        etas = np.geomspace(0.02, 0.5, max(1, G // 2)).tolist()
        grid = {'eta': etas, 'mini_batch_size': [1000, 4000][:max(1, G // len(etas))]}
        rows = {}

        def run(arm):
            rows[arm] = sweep.grid_search(items, mk, grid, batch_trials=arm)
        t = best_of({False: lambda: run(False), True: lambda: run(True)}, a.reps, 1)
        res['svrg_grid'] = {'trials': len(sweep.grid_points(grid)), 'per_trial_s': t[False], 'batched_s': t[True],
                            'speedup': t[False] / t[True], 'same_best_params': rows[False][0]['params'] == rows[True][0]['params'],
                            'loss_per_trial': rows[False][0]['loss'], 'loss_batched': rows[True][0]['loss']}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
