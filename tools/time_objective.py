"""Timing of `batch.objective(z)` next to `batch.grad_full(z, out)` on the same batch, alternating the two in one process:
hipEvents around N calls after a warm-up, best of ROUNDS rounds.  f32; CSMRI and Deblur at 256 x 256 with B = 32, 120, 1024,
phase retrieval at 128 x 128 with M = N / 2 and B = 8 (each problem its own 512 MiB matrix).  Bytes per problem are counted from
shapes; the objective does a subset of the gradient's passes -- the forward ones -- so it is expected to cost less.
Nothing here asserts that: the numbers are reported as measured.

    python tools/time_objective.py [out.json]        (default: profiles/objective_timing.json)
"""
import json
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pnp_svrg_amd import sweep
from pnp_svrg_amd.engine import CsmriBatch, DeblurBatch, PrBatch

HBM_PEAK = 8.0e12                                   # bytes / s, MI355X HBM3E
N_CALLS, ROUNDS = 50, 5


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N_CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N_CALLS * 1e3      # us per call


def measure(batch):
    z = batch.xinit
    g, f = torch.empty_like(z), torch.empty(batch.B, dtype=torch.float64, device=z.device)
    fns = {'objective': lambda: batch.objective(z, out=f), 'grad_full': lambda: batch.grad_full(z, g)}
    for fn in fns.values():                         # warm-up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    best = {k: float('inf') for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():                   # alternate
            best[k] = min(best[k], timeit(fn))
    return best


def row(kind, batch, shape, bytes_obj, bytes_grad, note):
    best = measure(batch)
    r = dict(problem=kind, B=batch.B, dtype='float32', shape=shape, us_objective=best['objective'], us_grad_full=best['grad_full'],
             ratio=best['objective'] / best['grad_full'], bytes_per_problem_objective=bytes_obj, bytes_per_problem_grad_full=bytes_grad,
             hbm_fraction_objective=bytes_obj * batch.B / (best['objective'] * 1e-6) / HBM_PEAK,
             hbm_fraction_grad_full=bytes_grad * batch.B / (best['grad_full'] * 1e-6) / HBM_PEAK, grad_full_path=note)
    print(json.dumps(r), flush=True)
    return r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'objective_timing.json')
    H = W = 256
    N = H * W
    rng = np.random.default_rng(0)
    images = [rng.random((H, W))]
    rows = []
    for B in (32, 120, 1024):
        items = sweep.make_items(1, [0.2], [20.0], seeds=range(B))
        b = CsmriBatch.generate(images, items, H, W)
        # objective: rows read z (4N) write the half spectrum (4N); columns read it (4N), YT (8N) and the mask bits (N/8)
        # grad_full, three streaming kernels: + yh (4N) in place of YT, the columns' write-back (4N), rows-inverse read + write (8N);
        #            the one-kernel form (B >= 192): z, yh, bits in, the image out
        fused = B >= 192
        rows.append(row('csmri', b, [H, W], 20 * N + N // 8, (12 * N if fused else 28 * N) + N // 8,
                        'one kernel (csmri_fused.hip)' if fused else 'rows, columns, rows-inverse'))
        del b
        b = DeblurBatch.generate(images, items, H, W)
        # one blur = column pass (4N in, 8N out), row pass (8N in, 8N out), column pass (8N in, 4N out) = 40N
        # objective: one blur + the reduction's reads of the forward image and Y (8N); grad_full: two blurs + Y (4N)
        rows.append(row('deblur', b, [H, W], 48 * N, 84 * N, 'two blurs'))
        del b
    n, B = 128, 8
    Nn, M = n * n, n * n // 2
    A = torch.randn((B, M, Nn), device='cuda')
    x = torch.rand((B, n, n), device='cuda')
    Y = torch.einsum('bmn,bn->bm', A, x.reshape(B, Nn)).abs()
    b = PrBatch._of(xrec=x, xinit=torch.rand_like(x), A=A, Y=Y)
    # objective: A once; grad_full: A twice (rows, then columns)
    rows.append(row('pr', b, [n, n, M], 4 * M * Nn, 8 * M * Nn, 'A streamed twice'))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
