"""Time the pnp_sarah inner iteration on CSMRI 256 x 256 f32 with the TV prox: (A) the streaming SarahEngine, (B)
SarahEngine(fused=True) stepped eagerly, (C) SarahEngine(fused=True) through `run_outer` (one hipGraph replay per outer iteration).

    python tools/time_sarah_fused.py [--batches 192 1024] [--outer 4] [--reps 5] [--eta 5e2] [-o profiles/sarah_fused_timing.json]

T2 = 10, device-drawn minibatches, mini_batch_size 1000.  A timed region is `--outer` outer iterations (T2 inner iterations and one
outer step each) from xinit (the engines are reset outside the clock).  One process, arms alternating, best of `--reps` after one warm-up pass of each arm,
wall clock between torch.cuda.synchronize() calls -- the method of tools/time_sarah_grid.py.  Reported: microseconds per inner
iteration (the outer step's share included) per arm and the ratios A/B and A/C."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T2, MB = 10, 1000


def best_of(arms, reps):
    """arms: name -> (prepare, run).  One warm-up pass of each, then `reps` rounds with the arms alternating -> name -> [seconds];
    `prepare` runs outside the clock."""
    def timed(prep, fn):
        prep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for arm in arms.values():
        timed(*arm)
    t = {name: [] for name in arms}
    for _ in range(reps):
        for name, arm in arms.items():
            t[name].append(timed(*arm))
    return t


def time_batch(E, B, n_outer, reps, eta):
    batch = E.CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=7)
    mk = lambda **kw: E.SarahEngine(batch, E.TVProx(sigma_modifier=1.1), eta, T2, MB, seed=4, **kw)       # noqa: E731
    a, b, c = mk(), mk(fused=True), mk(fused=True)
    c.capture()

    def eager(e):
        def run():
            for _ in range(n_outer * T2):
                e.step()
        return run
    # every region runs the same n_outer outer iterations from xinit (reset outside the clock): the iterate stays the one of a real run
    t = best_of({'A_streaming': (a.reset, eager(a)), 'B_fused_eager': (b.reset, eager(b)),
                 'C_fused_graph': (c.reset, lambda: c.run_outer(n_outer))}, reps)
    steps = n_outer * T2
    row = {'B': B, 'T2': T2, 'eta': eta, 'inner_iterations_per_region': steps, 'z_equal_B_C': bool(torch.equal(b.z, c.z)),
           'trace_equal_B_C': bool((b.psnr_trace() == c.psnr_trace()).all()), 'max_abs_z_A': a.z.abs().max().item(),
           'max_abs_z_A_minus_B': (a.z - b.z).abs().max().item(), 'psnr_final_mean_A': float(a.psnr_trace()[-1].mean()),
           'psnr_final_mean_B': float(b.psnr_trace()[-1].mean()), 'psnr_init_mean': float(batch.psnr_init().mean())}
    for name, ts in t.items():
        row[name + '_us_per_inner'] = min(ts) / steps * 1e6
        row[name + '_all_us'] = [v / steps * 1e6 for v in ts]
    row['A_over_B'] = row['A_streaming_us_per_inner'] / row['B_fused_eager_us_per_inner']
    row['A_over_C'] = row['A_streaming_us_per_inner'] / row['C_fused_graph_us_per_inner']
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[192, 1024])
    ap.add_argument('--outer', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eta', type=float, default=5e2)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'sarah_fused_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import engine as E
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'outer_iterations_per_region': a.outer, 'mini_batch_size': MB, 'rows': []}
    for B in a.batches:
        row = time_batch(E, B, a.outer, a.reps, a.eta)
        res['rows'].append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
