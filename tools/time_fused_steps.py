"""Time the pnp_gd, pnp_sgd and pnp_saga inner iterations on CSMRI 256 x 256 f32 with the TV prox: (A) the streaming
engine, (B) the same engine with fused=True (ONE pnp_csmri_grad_step / pnp_csmri_saga_step per iteration).

    python tools/time_fused_steps.py [--batches 192 1024] [--steps 20] [--reps 5] [--eta 5e2] [-o profiles/fused_steps_timing.json]

Device-drawn minibatches, mini_batch_size 1000, hist_size 4 (saga; one row for the batch per step, the same rows in both arms).  A timed
region is `--steps` inner iterations of an engine made outside the clock (SagaEngine has no reset: its table initialisation is part
of the constructor).  One process, arms alternating, best of `--reps` after one warm-up pass of each arm, wall clock between
torch.cuda.synchronize() calls -- the method of tools/time_sarah_fused.py.  Reported: microseconds per inner iteration per arm and the
ratio A/B."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB, HIST = 1000, 4


def time_cell(E, batch, algo, steps, reps, eta):
    def region(fused):
        """-> (seconds, engine): the engine is built outside the clock, the steps run inside it"""
        kw = dict(fused=True) if fused else {}
        e = E.make_engine(batch, E.TVProx(sigma_modifier=1.1), eta, None, MB, algorithm=algo, hist_size=HIST, seed=4, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            if algo == 'saga':
                e.step(r=s % HIST)
            else:
                e.step()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e
    arms = {'A_streaming': False, 'B_fused': True}
    for f in arms.values():
        region(f)                                               # warm-up pass of each arm
    t, last = {name: [] for name in arms}, {}
    for _ in range(reps):
        for name, f in arms.items():
            dt, last[name] = region(f)
            t[name].append(dt)
    a, b = last['A_streaming'], last['B_fused']
    row = {'algorithm': algo, 'B': batch.B, 'eta': eta, 'inner_iterations_per_region': steps, 'max_abs_z_A': a.z.abs().max().item(),
           'max_abs_z_A_minus_B': (a.z - b.z).abs().max().item(), 'psnr_final_mean_A': float(a.psnr_trace()[-1].mean()),
           'psnr_final_mean_B': float(b.psnr_trace()[-1].mean()), 'psnr_init_mean': float(batch.psnr_init().mean())}
    for name, ts in t.items():
        row[name + '_us_per_inner'] = min(ts) / steps * 1e6
        row[name + '_all_us'] = [v / steps * 1e6 for v in ts]
    row['A_over_B'] = row['A_streaming_us_per_inner'] / row['B_fused_us_per_inner']
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, nargs='+', default=[192, 1024])
    ap.add_argument('--algorithms', nargs='+', default=['gd', 'sgd', 'saga'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eta', type=float, default=5e2)
    ap.add_argument('-o', dest='out', default=os.path.join(ROOT, 'profiles', 'fused_steps_timing.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import engine as E
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'mini_batch_size': MB, 'hist_size': HIST, 'rows': []}
    for B in a.batches:
        batch = E.CsmriBatch.synthetic(B, 256, 256, 0.2, 20.0, seed=7)
        for algo in a.algorithms:
            row = time_cell(E, batch, algo, a.steps, a.reps, a.eta)
            res['rows'].append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
