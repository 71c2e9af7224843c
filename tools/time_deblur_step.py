"""Time the one-pass Deblur step (`pnp_deblur_grad_step`) against what it replaces, f32, 256 x 256, B = 64 (config 4's
batch).

    python tools/time_deblur_step.py [--batch 64] [--reps 7] [--calls 50] [--steps 40] [-o profiles/deblur_step_timing.json]

(a) the SVRG correction and step alone, z <- z - lr/mb (gs(z) - gs(w)) - lr mu on a device-drawn minibatch: `grad_stoch_diff` + combine
    (today's path: two gradients, two elementwise launches, one allocation) against ONE `grad_step` (`one_pass=True`), at
    scale_percent 100 (the fused middle pass) and 50 (the gather / CSR middle).  `--calls` calls per timed region, reported per call.
(b) one `SvrgEngine` inner iteration with `TVProx` at scale_percent 100, default against `one_pass=True`: `--steps` steps per timed
    region (a multiple of T2 = 10, so both arms make the same refreshes), reported per step.
One process, the two forms alternating, best and median of `--reps` after one warm-up pass of each, wall clock between
torch.cuda.synchronize() calls.  Prints both times and their ratio and writes them to the JSON file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T2, MB, ETA = 10, 1500, 1e3


def images(k, n=256, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        p = np.pad(rng.random((n, n)), 2, mode='wrap')
        out.append(sum(p[i:i + n, j:j + n] for i in range(5) for j in range(5)) / 25.0)
    return out


def alternating(arms, reps):
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


def report(what, t, per, names=('default', 'one_pass')):
    a, b = (np.array(t[k]) / per for k in names)
    row = {'what': what, f'{names[0]}_us_best': a.min() * 1e6, f'{names[0]}_us_median': float(np.median(a)) * 1e6,
           f'{names[1]}_us_best': b.min() * 1e6, f'{names[1]}_us_median': float(np.median(b)) * 1e6,
           'ratio_best': a.min() / b.min(), 'ratio_median': float(np.median(a) / np.median(b))}
    print(f"{what}: {names[0]} {row[names[0] + '_us_best']:.1f} us (median {row[names[0] + '_us_median']:.1f}), "
          f"{names[1]} {row[names[1] + '_us_best']:.1f} us (median {row[names[1] + '_us_median']:.1f}), "
          f"ratio {row['ratio_best']:.2f}x (median {row['ratio_median']:.2f}x)", flush=True)
    return row


def make_batch(E, B, scale_percent):
    from pnp_svrg_amd import sweep
    items = sweep.make_items(B, [scale_percent / 100.0], [20.0])
    return E.DeblurBatch.generate(images(4), [dict(it, image=it['image'] % 4) for it in items], 256, 256, torch.float32, 'Minimal',
                                  scale_percent)


def time_correction(E, B, scale_percent, reps, calls):
    batch = make_batch(E, B, scale_percent)
    z0, w, mu = batch.xinit.clone(), batch.xinit.clone().mul_(0.9), torch.rand_like(batch.xinit)
    mbs = batch.minibatches(1)
    batch.draw(mbs, MB, 1, 0)
    z = z0.clone()

    def arm(**kw):
        def run():
            z.copy_(z0)
            for _ in range(calls):
                batch.grad_stoch_diff(z, w, mbs, 0, out=z, alpha=-ETA / MB * 1e-3, beta=1.0, c1=z, gamma=-1e-3, c2=mu, **kw)
        return run
    t = alternating({'default': arm(), 'one_pass': arm(one_pass=True)}, reps)
    return report(f'correction + step, scale {scale_percent}, B = {B}', t, calls)


def time_engine(E, B, reps, steps):
    batch = make_batch(E, B, 100)
    engs = {'default': E.SvrgEngine(batch, E.TVProx(), ETA, T2, MB, seed=3),
            'one_pass': E.SvrgEngine(batch, E.TVProx(), ETA, T2, MB, seed=3, one_pass=True)}

    def arm(eng):
        def run():
            for _ in range(steps):
                eng.step()
        return run
    t = alternating({k: arm(e) for k, e in engs.items()}, reps)
    row = report(f'SvrgEngine inner iteration (TVProx, T2 = {T2}, refreshes included), scale 100, B = {B}', t, steps)
    tr = {k: e.psnr_trace()[-1] for k, e in engs.items()}
    row['final_psnr_max_abs_diff'] = float(np.abs(tr['default'] - tr['one_pass']).max())
    print(f"  final PSNR of the two arms differs by at most {row['final_psnr_max_abs_diff']:.3f} dB")
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('-o', '--out', default=os.path.join(ROOT, 'profiles', 'deblur_step_timing.json'))
    args = ap.parse_args()
    if args.steps % T2:
        ap.error(f'--steps must be a multiple of T2 = {T2}')
    sys.path.insert(0, ROOT)
    from pnp_svrg_amd import engine as E, ops
    ops.require_gpu()
    rows = [time_correction(E, args.batch, 100, args.reps, args.calls), time_correction(E, args.batch, 50, args.reps, args.calls),
            time_engine(E, args.batch, args.reps, args.steps)]
    out = {'device': torch.cuda.get_device_name(0), 'dtype': 'float32', 'H': 256, 'W': 256, 'batch': args.batch, 'reps': args.reps,
           'calls': args.calls, 'steps': args.steps, 'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
