"""Time the one-launch forms against the eager one-kernel iterations they replace, on CSMRI 256 x 256 f32 with the TV prox:
per algorithm (A) the engine with fused=True stepped eagerly -- one launch per inner iteration -- and (B) the one-launch form:
SarahEngine.run_outer(one_launch=True) (one launch per outer iteration, T2 = 10) or run_span of GdEngine / SgdEngine / SagaEngine
(16-step spans).  For pnp_sarah the hipGraph form (run_outer's default) is a third arm (C).

    python tools/time_outer_forms.py [--batches 192 1024] [--algorithms sarah gd sgd saga] [--steps 40] [--reps 5] [--eta 5e2]
                                     [-o profiles/outer_forms_timing.json]

Device-drawn minibatches, mini_batch_size 1000, hist_size 8.  A timed region is `--steps` inner iterations (rounded to whole outer
iterations for pnp_sarah) from xinit -- the engines are reset outside the clock; SagaEngine has no reset and goes on from where it is,
both arms alike.  One process, arms alternating, best of `--reps` after one warm-up pass of each arm, wall clock between
torch.cuda.synchronize() calls -- the method of tools/time_sarah_fused.py.  Reported: microseconds per inner iteration per arm (for
pnp_sarah the outer step's share included), the ratio A/B (above 1: the one-launch form is faster), and whether the arms ended on the
same bits."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T2, MB, HIST = 10, 1000, 8


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


def time_cell(E, batch, algo, steps, reps, eta):
    kw = dict(algorithm=algo, hist_size=HIST, seed=4, fused=True)
    mk = lambda: E.make_engine(batch, E.TVProx(sigma_modifier=1.1), eta, T2, MB, **kw)        # noqa: E731
    a, b = mk(), mk()

    def eager(e):
        def run():
            for _ in range(steps):
                e.step()
        return run
    if algo == 'sarah':
        steps -= steps % T2
        c = mk()
        c.capture()
        arms = {'A_eager': (a.reset, eager(a)), 'B_one_launch': (b.reset, lambda: b.run_outer(steps // T2, one_launch=True)),
                'C_graph': (c.reset, lambda: c.run_outer(steps // T2))}
        assert b.outer_kernel_ok()
    elif algo == 'saga':
        nothing = lambda: None                                                             # noqa: E731
        arms = {'A_eager': (nothing, eager(a)), 'B_one_launch': (nothing, lambda: b.run_span(steps))}
        assert b.span_kernel_ok()
    else:
        arms = {'A_eager': (a.reset, eager(a)), 'B_one_launch': (b.reset, lambda: b.run_span(steps))}
        assert b.span_kernel_ok()
    t = best_of(arms, reps)
    row = {'algorithm': algo, 'B': batch.B, 'inner_iterations_per_region': steps, 'steps_per_launch': T2 if algo == 'sarah' else b.AHEAD,
           'z_equal_A_B': bool(torch.equal(a.z, b.z)), 'trace_equal_A_B': bool((a.psnr_trace() == b.psnr_trace()).all()),
           'psnr_final_mean': float(b.psnr_trace()[-1].mean()), 'psnr_init_mean': float(batch.psnr_init().mean())}
    for name, ts in t.items():
        row[name + '_us_per_inner'] = min(ts) / steps * 1e6
        row[name + '_all_us'] = [v / steps * 1e6 for v in ts]
    row['A_over_B'] = row['A_eager_us_per_inner'] / row['B_one_launch_us_per_inner']
    if algo == 'sarah':
        row['A_over_C'] = row['A_eager_us_per_inner'] / row['C_graph_us_per_inner']
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[192, 1024])
    ap.add_argument('--algorithms', nargs='+', default=['sarah', 'gd', 'sgd', 'saga'])
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eta', type=float, default=5e2)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'outer_forms_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import engine as E
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'T2': T2, 'mini_batch_size': MB, 'hist_size': HIST, 'eta': a.eta,
           'rows': []}
    for B in a.batches:
        batch = E.CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=7)
        for algo in a.algorithms:
            row = time_cell(E, batch, algo, a.steps, a.reps, a.eta)
            res['rows'].append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        del batch
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
