"""Time the pnp_svrg inner iteration on CSMRI 256 x 256 f32 with the 2-D wavelet prox, TVProx(multi=False), in the one-kernel iteration
(DESIGN 9.10): (a) the two-launch form -- gradient kernel + pnp_prox_wavelet2d -- as replays of the captured outer iteration, its faster
form, and (a_eager) the same stepped eagerly; (b) TVProx(multi=False, in_kernel=True) stepped eagerly, ONE kernel per iteration; (c) the
same with run_outer(one_launch=True), ONE kernel per outer iteration; (d) the per-column prox, multi=True, one launch per outer
iteration, for context.

    python tools/time_fused_w2d.py [--batches 32 120 1024] [--steps 200] [--reps 5] [--T2 10] [-o profiles/fused_w2d_timing.json]

Device-drawn minibatches, mini_batch_size 1000.  A timed region is `--steps` inner iterations of an engine made (and, for (a),
captured) outside the clock.  One process, arms alternating, best of `--reps` after one warm-up pass of each arm, wall clock between
torch.cuda.synchronize() calls -- the method of tools/time_fused_steps.py.  Reported per arm: microseconds per inner iteration (best
and every repetition), the spread of (a)'s repetitions, and the ratios the gate of DESIGN 9.10 reads: a/c, a_eager/b, c/d."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB, ETA = 1000, 2e3
ARMS = ('a_two_launch_graph', 'a_two_launch_eager', 'b_in_kernel_eager', 'c_in_kernel_one_launch', 'd_per_column_one_launch')


def time_cell(E, batch, T2, steps, reps):
    n_outer = steps // T2

    def region(arm):
        """-> (seconds, engine): the engine is built (and captured) outside the clock, the iterations run inside it"""
        prox = {'a': lambda: E.TVProx(multi=False), 'b': lambda: E.TVProx(multi=False, in_kernel=True),
                'c': lambda: E.TVProx(multi=False, in_kernel=True), 'd': lambda: E.TVProx()}[arm[0]]()
        e = E.SvrgEngine(batch, prox, ETA, T2, MB, variant='svrg', fused=True, seed=4)
        if arm == 'a_two_launch_graph':
            e.capture()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if arm.endswith('eager'):
            for _ in range(n_outer * T2):
                e.step()
        elif arm == 'a_two_launch_graph':
            e.run_outer(n_outer, one_launch=False)
        else:
            e.run_outer(n_outer, one_launch=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e
    for arm in ARMS:
        region(arm)                                             # warm-up pass of each arm
    t, last = {arm: [] for arm in ARMS}, {}
    for _ in range(reps):
        for arm in ARMS:
            dt, last[arm] = region(arm)
            t[arm].append(dt)
    n = n_outer * T2
    row = {'B': batch.B, 'T2': T2, 'inner_iterations_per_region': n, 'psnr_init_mean': float(batch.psnr_init().mean())}
    for arm in ARMS:
        row[arm + '_us_per_inner'] = min(t[arm]) / n * 1e6
        row[arm + '_all_us'] = [v / n * 1e6 for v in t[arm]]
        row[arm + '_psnr_final_mean'] = float(last[arm].psnr_trace()[-1].mean())
    a = row['a_two_launch_graph_all_us']
    row['a_spread_us'] = max(a) - min(a)
    row['a_minus_c_us'] = row['a_two_launch_graph_us_per_inner'] - row['c_in_kernel_one_launch_us_per_inner']
    row['a_over_c'] = row['a_two_launch_graph_us_per_inner'] / row['c_in_kernel_one_launch_us_per_inner']
    row['a_eager_over_b'] = row['a_two_launch_eager_us_per_inner'] / row['b_in_kernel_eager_us_per_inner']
    row['c_over_d'] = row['c_in_kernel_one_launch_us_per_inner'] / row['d_per_column_one_launch_us_per_inner']
    row['max_abs_z_a_minus_c'] = (last['a_two_launch_graph'].z - last['c_in_kernel_one_launch'].z).abs().max().item()
    row['z_b_equals_z_c'] = bool(torch.equal(last['b_in_kernel_eager'].z, last['c_in_kernel_one_launch'].z))
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 120, 1024])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--T2', type=int, default=10)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'fused_w2d_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import engine as E
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'mini_batch_size': MB, 'eta': ETA, 'rows': []}
    for B in a.batches:
        batch = E.CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=7)
        row = time_cell(E, batch, a.T2, a.steps, a.reps)
        res['rows'].append(row)
        print(json.dumps(row), flush=True)
        del batch
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
