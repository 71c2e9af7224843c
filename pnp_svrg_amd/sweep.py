"""Sharding of independent reconstructions over the GPUs of one node (BASELINE config 5).

Mirrors the work decomposition of reference script_diff_sampratio_set12.py:113-146 /
script_diff_snr_set12.py (one work item = image x sampling ratio x SNR x seed, all independent;
the reference maps them over a multiprocessing.Pool): items are dealt round-robin to ranks, one
process per GPU, every rank batches ITS items through the engine, and the only collective is the
final gather of the (small) results -- RCCL over xGMI when the group is NCCL, gloo in CPU tests.
There is no data-path collective to overlap: a 256x256 reconstruction is never split across GPUs.
"""
import csv
import os

import numpy as np
import torch
import torch.distributed as dist


def make_items(n_images, alphas, snrs, seeds=(0,)):
    """Canonical work-item list (same nesting order as the reference's loops: image, alpha, snr)."""
    items = []
    for img in range(n_images):
        for a in alphas:
            for s in snrs:
                for sd in seeds:
                    items.append({'id': len(items), 'image': img, 'alpha': float(a), 'snr': float(s), 'seed': int(sd)})
    return items


def shard(items, rank, world):
    """Static round-robin: item i -> rank i % world (items of equal cost; no exchange afterwards).  A rank's items
    are batched TOGETHER whatever their sampling ratio (per-problem 1/M0 and minibatch thresholds in the engine), so
    120 items on 8 ranks are 8 batches of 15, not 40 batches of 3."""
    return [it for it in items if it['id'] % world == rank]


def gather_results(local, dst=0, group=None):
    """Final gather of per-item results (list of dicts with an 'id').  Returns the full list sorted by
    id on rank `dst`, None elsewhere.  Single-process: returns the sorted local list."""
    if not (dist.is_available() and dist.is_initialized()):
        return sorted(local, key=lambda r: r['id'])
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    out = [None] * world if rank == dst else None
    dist.gather_object(local, out, dst=dst, group=group)
    if rank != dst:
        return None
    return sorted((r for part in out for r in part), key=lambda r: r['id'])


def gather_device(z_local, meta_local, n_items, dst=0, group=None):
    """The final gather as two tensor collectives (RCCL over xGMI when the group is NCCL): the reconstructions
    z_local [n_local, H, W] (device tensor, any float dtype) and one small float64 row per item meta_local [n_local, K] whose
    first column is the item id.  Ranks hold different numbers of items (round-robin shards), so rows are padded to
    ceil(n_items / world).  Returns (z [n_items, H, W], meta [n_items, K]) in id order on rank `dst` (CPU tensors), None
    elsewhere.  Single-process: the local data, sorted."""
    meta_local = torch.as_tensor(meta_local, dtype=torch.float64).reshape(z_local.shape[0], -1)
    if not (dist.is_available() and dist.is_initialized()):
        meta_local = meta_local.cpu()
        order = torch.argsort(meta_local[:, 0])
        return z_local.detach().cpu()[order], meta_local[order]
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    on_dev = dist.get_backend(group) == 'nccl'
    dev = z_local.device if on_dev else torch.device('cpu')
    cap = -(-n_items // world)
    zp = torch.zeros((cap,) + tuple(z_local.shape[1:]), dtype=z_local.dtype, device=dev)
    mp = torch.full((cap, meta_local.shape[1]), -1.0, dtype=torch.float64, device=dev)
    n = z_local.shape[0]
    zp[:n] = z_local.to(dev)
    mp[:n] = meta_local.to(dev)
    zs = [torch.empty_like(zp) for _ in range(world)] if rank == dst else None
    ms = [torch.empty_like(mp) for _ in range(world)] if rank == dst else None
    dist.gather(zp, zs, dst=dst, group=group)
    dist.gather(mp, ms, dst=dst, group=group)
    if rank != dst:
        return None
    z, m = torch.cat(zs).cpu(), torch.cat(ms).cpu()
    keep = m[:, 0] >= 0
    z, m = z[keep], m[keep]
    order = torch.argsort(m[:, 0])
    assert order.numel() == n_items, 'every item exactly once'
    return z[order], m[order]


def run_sweep(items, runner, group=None):
    """Run `runner(my_items) -> [result dict per item]` on this rank's shard and gather on rank 0."""
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    mine = shard(items, rank, world)
    res = runner(mine) if mine else []
    assert [r['id'] for r in res] == [it['id'] for it in mine], 'runner must return one result per item, in order'
    return gather_results(res, 0, group)


def _norm01(img):
    x = np.asarray(img, np.float64)
    return (x - x.min()) / (x.max() - x.min())


def _csmri_item_generator(img, it, H, W):
    """One work item's data from a Generator stream keyed by the item (fast path of the sweeps): Bernoulli mask like
    the reference (problems/CSMRI.py:43-45), masked spectrum + real noise on the support (:29-33), |ifft2| init."""
    rng = np.random.default_rng(1000003 * it['seed'] + it['id'])
    x = _norm01(img)
    mk = (rng.random((H, W)) < it['alpha']).astype(np.uint8)
    Y0 = mk * np.fft.fft2(x)
    sig = np.sqrt(np.linalg.norm(Y0.ravel()) / 10 ** (it['snr'] / 10) / H / W)
    Y = Y0 + mk * rng.normal(0, sig, (H, W))
    xi = np.absolute(np.fft.ifft2(Y))
    return x, mk, Y, ((xi - xi.min()) / (xi.max() - xi.min())).ravel()


def _minimal_kernel(H, W, kernel):
    """The reference's "Minimal" / "Identity" blur vectors (problems/DeblurSR.py:80-93), already divided by N."""
    Bk = np.zeros((H, W))
    Bk[0, 0] = 1
    if kernel == 'Minimal':
        Bk[H // 2, H // 2] = Bk[H // 2, H // 3] = Bk[H // 2, H // 4] = 1
        Bk /= 4
    elif kernel != 'Identity':
        raise ValueError(f'kernel {kernel!r}: "Minimal" or "Identity" (generator seeding; legacy seeding takes what problems.Deblur takes)')
    return Bk.ravel() / (H * W)


PROBLEMS = ('csmri', 'deblur', 'pr')
ALGORITHMS = ('gd', 'sgd', 'svrg', 'saga', 'sarah')
_REF_NAMES = {'csmri': 'CSMRI', 'deblur': 'DeblurSR', 'pr': 'PR', 'tv': 'TV', 'nlm': 'NLM', 'dncnn': 'CNN'}


def deblur_scale_percent(alpha):
    """item alpha (fraction of the full-resolution measurements, 0.1 .. 1.0) -> Deblur's scale_percent, as the reference's
    get_problem does with its alpha in 1 .. 10 (script_diff_sampratio_set12.py:45-46: int(alpha * 10))."""
    return int(round(alpha * 100))


def pr_num_meas(alpha, H, W):
    """item alpha (measurements per pixel) -> PhaseRetrieval's num_meas (script_diff_sampratio_set12.py:47-48)."""
    return int(alpha * H * W)


def make_prox(denoiser, **kw):
    """'tv' | 'nlm' -> a fresh engine prox (denoisers/TV.py, NLM.py semantics); a callable is called (e.g. a DnCNNProx factory)."""
    from .engine import TVProx, NLMProx
    if callable(denoiser):
        return denoiser()
    if denoiser == 'tv':
        return TVProx(**kw)
    if denoiser == 'nlm':
        return NLMProx(**kw)
    raise ValueError(f'unknown denoiser {denoiser!r}: "tv", "nlm" or a factory')


def make_runner(images, problem='csmri', algorithm='svrg', denoiser='tv', *, eta, n_inner, mini_batch_size=None, T2=None,
                hist_size=50, H=256, W=256, dtype=torch.float32, max_batch=128, seeding='generator', variant='svrg', run_seed=1,
                keep_trace=False, graph=True, kernel='Minimal', lr_decay=1.0, denoiser_kwargs=None, sigma_modifier=None,
                shared_matrix=False, wide_trials=False, sarah_trials=False, t2_trials=False, objective=False, sarah_fused=False,
                fused_steps=False, one_launch=False, hist_trials=False, mixed_scales=False, sarah_t2_trials=False, one_pass_diff=False):
    """Runner for `run_sweep` / `grid_search` over any cell of the reference's sweep (script_diff_sampratio_set12.py:23-25,
    41-51, 64-131): problem in {'csmri', 'deblur', 'pr'} x algorithm in {'gd', 'sgd', 'svrg', 'saga', 'sarah'} x denoiser in
    {'tv', 'nlm', factory}; `n_inner` inner iterations (prox evaluations of the stepped iterate) per item, hyper-parameters
    eta, mini_batch_size, T2 (svrg, sarah), hist_size (saga) -- the keys a search grid varies.

    A rank's items run as batches on the engines of `engine.py`: CSMRI items of ANY mix of sampling ratios together (per-problem
    1/M0 and minibatch thresholds); Deblur / PR items are grouped by alpha, which fixes the operator's shape (scale_percent =
    100 alpha; num_meas = alpha H W).
    seeding='generator': per-item data from a Generator stream keyed by the item, built on the host, minibatches drawn on the device;
    seeding='counter'  : per-item data generated ON THE DEVICE from the counter-based stream of include/pnp_hip.h, for all three
                         problems (engine.CsmriBatch.generate / DeblurBatch.generate / PrBatch.generate; the normalised image set
                         is uploaded once per runner): Deblur items with scale_percent = deblur_scale_percent(alpha), values other
                         than 100 (super-resolution) included; PR items with A generated in HBM and the spectral initialisation
                         batched on the device.  Minibatches drawn on the device and graph replay as with 'generator'; a third
                         stream: not the data of the other two modes;
    seeding='device'   : the older, CSMRI-only spelling of 'counter' (the same code path and the same data, bit for bit); any other
                         problem raises ValueError;
    seeding='legacy'   : per item exactly the reference's RNG use -- np.random.seed(item seed), the problem constructor's draws
                         in its order, np.random.seed(run_seed), then the loop's draws in ITS order (one select_mb per inner
                         iteration; pnp_saga: one select_mb for the table, then select_mb + np.random.choice(hist_size, 1) per
                         iteration, algorithms/pnp_saga.py:25-29,43-47) -- so an item's trajectory equals the reference loop's
                         (and the oracle's) on the same seeds.
    sigma_modifier: shorthand for denoiser_kwargs={'sigma_modifier': ...}, so that a search grid can name it as a key.
    shared_matrix: problem='pr' only (ValueError otherwise): a trial-batched grid runs its trials on `PrBatch.tile`, every trial of
    an item on that item's ONE matrix A (nothing of A is copied; csrc/pr_shared.hip streams it twice per gradient whatever the
    number of trials).  Without it `check_trials` refuses 'pr'.  `run(items)` itself is unchanged by it.
    wide_trials: opt in to the wider ground of a trial-batched grid: problem='deblur' (on `DeblurBatch.tile`, seeding
    'counter' or 'generator'), algorithm='saga' on csmri or deblur (one pnp_saga_table_update_pp launch per step; `run_trials` caps a
    slab so that its gradient table stays within max_table_bytes) and denoiser='nlm' with sigma_modifier as a per-problem key.
    Without it `check_trials` answers as it always has.  `run(items)` itself is unchanged by it.
    sarah_trials: opt in to algorithm='sarah' in a trial-batched grid (SarahEngine with per-problem eta, mini_batch_size and
    draw_id, its elementwise steps one pnp_axpbypcz_pp launch each) on 'csmri', on 'deblur' with wide_trials=True and on 'pr' with
    shared_matrix=True; per-problem keys eta, mini_batch_size, sigma_modifier (T2 stays structural).  Without it `check_trials`
    refuses 'sarah' as it always has.  `run(items)` itself is unchanged by it.
    t2_trials: opt in to 'T2' as a per-problem trial key of a trial-batched grid, algorithm='svrg' only (ValueError for
    another algorithm once a trial names 'T2'), on the batches batch_trials already takes for svrg: a slab whose trials name 'T2'
    runs on an SvrgEngine with a [B] T2 and advances by `run_span`.  Without it `check_trials` refuses the key as it always has.
    `run(items)` itself is unchanged by it.
    objective: True makes every engine log the data-fidelity objective f(z) beside the squared errors (engine `log_objective`,
    DESIGN 10; such engines step eagerly): result rows gain 'f_final' (f of the last logged iterate) and, with keep_trace=True,
    'f_trace' (one value per 'psnr_trace' entry); trial-batched runs carry it through.  False (default): rows, engines and launches
    are exactly what they were.  Anything but a bool is a ValueError.
    sarah_fused: opt in to the one-kernel forms of pnp_sarah (SarahEngine(fused=True)): problem='csmri', algorithm='sarah',
    float32 256 x 256 and the 'tv' denoiser or a DnCNN prox factory -- anything else is a ValueError that names the offender.  Goes
    together with sarah_trials=True; batches with device-drawn minibatches replay whole outer iterations as hipGraphs.  False
    (default): engines, launches, rows and messages are exactly what they were.
    fused_steps: opt in to the one-kernel inner iterations of pnp_gd, pnp_sgd and pnp_saga (GdEngine / SgdEngine / SagaEngine with
    fused=True): problem='csmri', algorithm in {'gd', 'sgd', 'saga'}, float32 256 x 256 and the 'tv' denoiser or a
    DnCNN prox factory -- anything else is a ValueError that names the offender.  Rides through `run(items)` and through
    trial-batched grids (wide_trials=True for 'saga').  False (default): engines, launches, rows and messages are exactly what they
    were.
    one_launch: opt in to the one-launch forms of those engines; needs sarah_fused=True or fused_steps=True (ValueError
    otherwise).  With sarah_fused, batches with device-drawn minibatches run whole outer iterations as ONE
    pnp_csmri_sarah_outer_iteration each (`run_outer(n, one_launch=True)`, where the engine's `outer_kernel_ok()` holds and the step
    counts are multiples of T2); with fused_steps they advance by `run_span(n)`.  The same bits as without it.  False (default):
    engines, launches, rows and messages are exactly what they were.
    hist_trials: opt in to 'hist_size' as a per-problem trial key of a trial-batched grid, algorithm='saga' only (ValueError
    for another algorithm once a trial names 'hist_size'), on the batches batch_trials already takes for saga: a slab whose trials name
    'hist_size' runs on a SagaEngine with a [B] hist_size, its table dense over the largest value.  Without it `check_trials` refuses
    the key as it always has.  `run(items)` itself is unchanged by it.
    mixed_scales: problem='deblur' only (a ValueError that names any other problem): a rank's Deblur items of ANY mix of alpha run as
    one batch, or slabs of max_batch, on a mixed-scale DeblurBatch instead of one batch per alpha -- under
    seeding='counter' through `DeblurBatch.generate(scale_percent=[...])`, under 'legacy' through `from_problems`; 'generator' keeps
    its scale-100 rule.  Every item keeps the minibatch stream (seed and id) and, for pnp_saga, the table rows of the group the
    default runner would have run it in, so its row equals the default runner's (items with alpha == 1.0: to rounding).  Rows come
    back in item order; `prepare_data` / `run_trials` (wide_trials=True) run on the tiled mixed batch.  False (default): grouping,
    engines, launches, rows and messages are exactly what they were.
    sarah_t2_trials: opt in to 'T2' as a per-problem trial key for algorithm='sarah' (DESIGN 9.11); needs sarah_trials=True and
    algorithm='sarah' (ValueError otherwise).  On the batches sarah_trials admits, a slab whose trials name 'T2' runs on a
    SarahEngine(T2=[B] ints, split_log=True) and advances by `run_span`; its rows ('psnr_trace' included: `psnr_trace_of`) are those of
    the per-trial runner.  Without it `check_trials` refuses the key, with or without t2_trials, in the words it always used.
    `run(items)` itself is unchanged by it.
    one_pass_diff: opt in to the one-pass correction and step of Deblur (SvrgEngine / SarahEngine with one_pass=True):
    problem='deblur', algorithm in {'svrg', 'sarah'}, without mixed_scales -- anything else is a ValueError that names the offender.
    An inner iteration's two minibatch gradients and their combination become ONE pnp_deblur_grad_step; rows agree with the default's
    to rounding, not bit for bit.  Rides through `run(items)` and through trial-batched grids.  False (default): engines, launches,
    rows and messages are exactly what they were.
    Beside `run(items)` the runner offers the pieces of a trial-batched grid (`grid_search(batch_trials=True)`):
    `run.prepare_data(items)` builds a rank's batches WITHOUT engines, `run.run_trials(data, trials, max_batch_trials)` runs a list
    of trials ({'eta', 'mini_batch_size', 'sigma_modifier'} overrides) on them as tiled batches, `run.data_key` says which runners
    may share prepared data."""
    from . import engine as E
    from . import problems as P
    if problem not in PROBLEMS or algorithm not in ALGORITHMS:
        raise ValueError(f'problem in {PROBLEMS}, algorithm in {ALGORITHMS}')
    if algorithm != 'gd' and mini_batch_size is None:
        raise ValueError('mini_batch_size is required')
    if algorithm in ('svrg', 'sarah') and T2 is None:
        raise ValueError('T2 is required')
    if seeding == 'device' and problem != 'csmri':
        raise ValueError(f"seeding='device' is supported for problem='csmri' only (got {problem!r}); use 'generator' or 'legacy'")
    if not isinstance(objective, (bool, np.bool_)):
        raise ValueError(f'objective: True or False, got {objective!r}')
    if not isinstance(sarah_fused, (bool, np.bool_)):
        raise ValueError(f'sarah_fused: True or False, got {sarah_fused!r}')
    if sarah_fused:
        if problem != 'csmri':
            raise ValueError(f"sarah_fused=True is for problem='csmri' (got {problem!r}): the one-kernel iteration is a CSMRI kernel")
        if algorithm != 'sarah':
            raise ValueError(f"sarah_fused=True is for algorithm='sarah' (got {algorithm!r})")
        if dtype != torch.float32 or (H, W) != (256, 256):
            raise ValueError(f'sarah_fused=True needs float32 images of 256 x 256 (got {dtype}, H = {H}, W = {W})')
        if not (denoiser == 'tv' or callable(denoiser)):
            raise ValueError(f"sarah_fused=True needs the 'tv' denoiser or a DnCNN prox factory (got {denoiser!r})")
        if objective:
            raise ValueError('sarah_fused=True needs objective=False (the one-kernel forms do not log the objective)')
    if not isinstance(fused_steps, (bool, np.bool_)):
        raise ValueError(f'fused_steps: True or False, got {fused_steps!r}')
    if fused_steps:
        if problem != 'csmri':
            raise ValueError(f"fused_steps=True is for problem='csmri' (got {problem!r}): the one-kernel iteration is a CSMRI kernel")
        if algorithm not in ('gd', 'sgd', 'saga'):
            raise ValueError(f"fused_steps=True is for algorithm in ('gd', 'sgd', 'saga') (got {algorithm!r})")
        if dtype != torch.float32 or (H, W) != (256, 256):
            raise ValueError(f'fused_steps=True needs float32 images of 256 x 256 (got {dtype}, H = {H}, W = {W})')
        if not (denoiser == 'tv' or callable(denoiser)):
            raise ValueError(f"fused_steps=True needs the 'tv' denoiser or a DnCNN prox factory (got {denoiser!r})")
        if objective:
            raise ValueError('fused_steps=True needs objective=False (the one-kernel forms do not log the objective)')
    if not isinstance(one_launch, (bool, np.bool_)):
        raise ValueError(f'one_launch: True or False, got {one_launch!r}')
    if one_launch and not (sarah_fused or fused_steps):
        raise ValueError('one_launch=True needs sarah_fused=True or fused_steps=True (the one-launch forms are those of the one-kernel '
                         'iterations)')
    eng_kw = {'log_objective': True} if objective else {}       # (off: the engines are made with the arguments they always got)
    if sarah_fused or fused_steps:
        eng_kw = dict(eng_kw, fused=True)                       # (rides with the other opt-in engine keyword)
    if not isinstance(mixed_scales, (bool, np.bool_)):
        raise ValueError(f'mixed_scales: True or False, got {mixed_scales!r}')
    if mixed_scales and problem != 'deblur':
        raise ValueError(f"mixed_scales=True is for problem='deblur' (got {problem!r}): CSMRI items of any mix of ratios already share a "
                         'batch, and the matrices of phase-retrieval items of different num_meas have different shapes')
    if not isinstance(sarah_t2_trials, (bool, np.bool_)):
        raise ValueError(f'sarah_t2_trials: True or False, got {sarah_t2_trials!r}')
    if sarah_t2_trials and not (sarah_trials and algorithm == 'sarah'):
        raise ValueError(f"sarah_t2_trials=True needs sarah_trials=True and algorithm='sarah' (got sarah_trials={bool(sarah_trials)!r}, "
                         f'algorithm {algorithm!r}): it makes T2 a per-problem key of the trial-batched pnp_sarah grid')
    if not isinstance(one_pass_diff, (bool, np.bool_)):
        raise ValueError(f'one_pass_diff: True or False, got {one_pass_diff!r}')
    if one_pass_diff:
        if problem != 'deblur':
            raise ValueError(f"one_pass_diff=True is for problem='deblur' (got {problem!r}): the one-pass step is a Deblur kernel")
        if algorithm not in ('svrg', 'sarah'):
            raise ValueError(f"one_pass_diff=True is for algorithm in ('svrg', 'sarah') (got {algorithm!r}): the others take no "
                             'difference of minibatch gradients')
        if mixed_scales:
            raise ValueError('one_pass_diff=True needs mixed_scales=False (a mixed-scale batch has no one-pass step)')
        eng_kw = dict(eng_kw, one_pass=True)                    # (rides with the other opt-in engine keywords)
    if shared_matrix and problem != 'pr':
        raise ValueError(f"shared_matrix=True is for problem='pr' (got {problem!r}): only its problems have a matrix to share")
    mb, dkw = mini_batch_size, dict(denoiser_kwargs or {})
    if sigma_modifier is not None:
        dkw['sigma_modifier'] = sigma_modifier
    dev_images = []                                              # seeding='counter' / 'device': the image set in HBM, uploaded on first use

    def group_key(it):
        return None if problem == 'csmri' else it['alpha']

    def build_generator(chunk):
        a = chunk[0]['alpha']
        if problem == 'csmri':
            d = [_csmri_item_generator(images[it['image']], it, H, W) for it in chunk]
            return E.CsmriBatch(np.stack([t[0] for t in d]), np.stack([t[1] for t in d]), np.stack([t[2] for t in d]),
                                np.stack([t[3] for t in d]).reshape(len(chunk), -1), dtype=dtype)
        if problem == 'deblur':
            if any(deblur_scale_percent(it['alpha']) != 100 for it in chunk):
                raise ValueError('generator seeding builds scale_percent == 100 Deblur items; use seeding="legacy" for the bilinear operator')
            Bk = _minimal_kernel(H, W, kernel)
            FB = np.fft.fft(Bk)
            xs, Ys, xi = [], [], []
            for it in chunk:
                rng = np.random.default_rng(1000003 * it['seed'] + it['id'])
                x = _norm01(images[it['image']])
                Y0 = np.real(np.fft.ifft(np.fft.fft(x.ravel()) * FB)) * np.sqrt(H * W)        # DeblurSR.py:119-120
                sig = np.sqrt(np.linalg.norm(Y0) / 10 ** (it['snr'] / 10) / H / W)
                xs.append(x); Ys.append(Y0 + rng.normal(0, sig, H * W)); xi.append(rng.uniform(0.0, 1.0, H * W))
            return E.DeblurBatch(np.stack(xs), Bk, np.stack(Ys), np.stack(xi), dtype=dtype)
        M = pr_num_meas(a, H, W)
        xs, As, Ys, xi = [], [], [], []
        for it in chunk:
            rng = np.random.default_rng(1000003 * it['seed'] + it['id'])
            x = _norm01(images[it['image']])
            A = rng.standard_normal((M, H * W))
            Y0 = np.absolute(A @ x.ravel())
            sig = np.sqrt(np.linalg.norm(Y0) / 10 ** (it['snr'] / 10) / H / W)
            Y = Y0 + rng.normal(0, sig, M)
            v, lead, lead_old, prev = np.full(H * W, 2.0), 1.0, 2.0, np.ones(H * W)          # PR.py:50-63 (host: small N)
            while abs(lead - lead_old) > 1e-5 and np.linalg.norm(v - prev) > 1e-5:
                lead_old, prev = lead, v
                v = A.T @ (Y * (A @ prev)) / M
                lead = v.max()
                v = v / lead
            x0 = np.sqrt(lead) * v / np.linalg.norm(v) * np.linalg.norm(x.ravel())
            xs.append(x); As.append(A); Ys.append(Y); xi.append((x0 - x0.min()) / (x0.max() - x0.min()))
        return E.PrBatch(np.stack(xs), np.stack(As), np.stack(Ys), np.stack(xi), dtype=dtype)

    def build_counter(dev_imgs, chunk):
        a = chunk[0]['alpha']
        if problem == 'csmri':
            return E.CsmriBatch.generate(dev_imgs, chunk, H, W, dtype)
        if problem == 'deblur' and mixed_scales:
            return E.DeblurBatch.generate(dev_imgs, chunk, H, W, dtype, kernel=kernel,
                                          scale_percent=[deblur_scale_percent(it['alpha']) for it in chunk])
        if problem == 'deblur':
            return E.DeblurBatch.generate(dev_imgs, chunk, H, W, dtype, kernel=kernel, scale_percent=deblur_scale_percent(a))
        return E.PrBatch.generate(dev_imgs, chunk, H, W, pr_num_meas(a, H, W), dtype)

    def build_legacy(chunk):
        """-> (batch, draws): per item the reference's constructor on its seed, then the loop's RNG draws on run_seed."""
        probs, draws = [], []
        n_mb = 0 if algorithm == 'gd' else n_inner + (1 if algorithm == 'saga' else 0)
        for it in chunk:
            np.random.seed(it['seed'])
            img = images[it['image']]
            if problem == 'csmri':
                p = P.CSMRI(None, H=H, W=W, sample_prob=it['alpha'], snr=it['snr'], img=img, upload=False)
            elif problem == 'deblur':
                p = P.Deblur(None, H=H, W=W, kernel=kernel, scale_percent=deblur_scale_percent(it['alpha']), snr=it['snr'], img=img,
                             dtype=dtype)
            else:
                p = P.PhaseRetrieval(None, H=H, W=W, num_meas=pr_num_meas(it['alpha'], H, W), snr=it['snr'], img=img, dtype=dtype)
            np.random.seed(run_seed)
            idx, rs = np.empty((n_mb, mb if n_mb else 0), np.int32), np.zeros(n_inner, np.int64)
            for s in range(n_mb):
                idx[s] = np.flatnonzero(p.select_mb(mb))
                if algorithm == 'saga' and s > 0:
                    rs[s - 1] = np.random.choice(hist_size, 1).item()
            probs.append(p)
            draws.append((idx, rs))
        cls = {'csmri': E.CsmriBatch, 'deblur': E.DeblurBatch, 'pr': E.PrBatch}[problem]
        return cls.from_problems(probs, dtype=dtype), draws

    class _Chunk:
        """One batch of a rank's items on its engine: built (data in HBM) by `prepare`, advanced by `advance`."""

        def __init__(self, chunk, with_engine=True):
            self.items = chunk
            if seeding == 'legacy':
                self.batch, draws = build_legacy(chunk)
                self.idx_d = torch.from_numpy(np.stack([d[0] for d in draws], axis=1)).to(self.batch.device) if algorithm != 'gd' else None
                self.rs = np.stack([d[1] for d in draws], axis=1)                  # [n_inner][B]
            elif seeding in ('device', 'counter'):
                if not dev_images:
                    dev_images.append(E.CsmriBatch.upload_images(images, H, W, dtype))
                self.batch, self.idx_d, self.rs = build_counter(dev_images[0], chunk), None, None
            else:
                self.batch, self.idx_d, self.rs = build_generator(chunk), None, None
            self.done = 0
            self.streams = None
            if mixed_scales and getattr(self.batch, 'M_vec', None) is not None:
                # every item keeps the minibatch stream of the group the default runner runs it in: that group's seed, its place there
                self.streams = [item_stream[it['id']] for it in chunk]
                self.batch.draw_seeds = torch.from_numpy(np.array([s for s, _ in self.streams], np.int64)).to(self.batch.device)
            if not with_engine:                                 # data only: trial slabs put their engines on tiles of it
                self.tiles = {}
                return
            kw = dict(seed=chunk[0]['id'] + 1)
            if self.streams is not None and algorithm != 'gd':
                kw['draw_id'] = [k for _, k in self.streams]
            self._row_rngs()
            if algorithm == 'saga' and self.idx_d is not None:
                kw['idx0'] = self.idx_d[0]
            self.eng = E.make_engine(self.batch, make_prox(denoiser, **dkw), eta, T2, mb, lr_decay=lr_decay, variant=variant,
                                     algorithm=algorithm, hist_size=hist_size, **kw, **eng_kw)
            self.done = 0

        def _row_rngs(self):
            """mixed_scales, pnp_saga with device draws: the row streams of the default groups' engines (engine.saga_row_rng)."""
            self.row_rng = None
            if self.streams is not None and algorithm == 'saga' and self.idx_d is None:
                self.row_rng = {s: E.saga_row_rng(s) for s, _ in self.streams}

        def _rows(self):
            draws = {s: int(g.integers(hist_size)) for s, g in self.row_rng.items()}
            return np.array([draws[s] for s, _ in self.streams], np.int64)

        def advance(self, n):
            eng, idx_d = self.eng, self.idx_d
            if np.ndim(getattr(eng, 'T2', 0)) != 0:             # per-problem T2: no common outer iteration, the engine's own spans
                eng.run_span(n)
                self.done += n
                return
            if one_launch and idx_d is None:                    # the one-launch forms (device-drawn minibatches only)
                if fused_steps:
                    eng.run_span(n)
                    self.done += n
                    return
                if n % T2 == 0 and eng.s % T2 == 0 and eng.outer_kernel_ok():
                    eng.run_outer(n // T2, one_launch=True)
                    self.done += n
                    return
            # device-drawn minibatches: whole outer iterations replay as hipGraphs (bit-identical to stepping; a rank's share
            # of a sweep is a small batch, where the ~25 launches of an inner iteration are a tenth of its time) -- when the
            # engine can be captured at all (an NLM prox ping-pongs between buffers and cannot: eager steps)
            if (graph and idx_d is None and hasattr(eng, 'run_outer') and n % T2 == 0 and eng.s % T2 == 0
                    and (n > T2 or eng.graph is not None) and eng.graph_ok()):
                eng.run_outer(n // T2)                          # (captures first when that has not happened yet: `warm`)
            else:
                for s in range(self.done, self.done + n):
                    if idx_d is None and self.row_rng is not None:
                        eng.step(r=self._rows())
                    elif idx_d is None:
                        eng.step()
                    elif algorithm == 'saga':
                        eng.step(idx_d[s + 1], r=self.rs[s])
                    else:
                        eng.step(idx_d[s])
            self.done += n

        def results(self):
            tr = self.eng.psnr_trace()                          # (a SarahEngine with a T2 vector: the inner rows, so tr[-1] is the last iterate's)
            split = getattr(self.eng, 'outer_log', None) is not None
            psnr0 = self.batch.psnr_init()
            z = self.eng.z.cpu().numpy()
            fl = self.eng.objective_log() if objective else None
            out = []
            for j, it in enumerate(self.items):
                r = {'id': it['id'], 'item': it, 'psnr_init': float(psnr0[j]), 'psnr_final': float(tr[-1, j]),
                     'loss': float(psnr0[j] - tr[-1, j]), 'z': z[j]}
                if problem == 'csmri':
                    r['M0'] = int(self.batch.M0[j])
                if keep_trace:
                    r['psnr_trace'] = self.eng.psnr_trace_of(j) if split else tr[:, j].copy()
                if objective:
                    r['f_final'] = float(fl[-1, j])
                    if keep_trace:
                        r['f_trace'] = fl[:, j].copy()
                out.append(r)
            return out

    class _TrialSlab(_Chunk):
        """Some trials of a grid on ONE engine: the data of a prepared chunk tiled once per trial (problem t * n + i = trial t
        of item i), per-problem eta / mini_batch_size / sigma_modifier, and the chunk's own seed and item-keyed minibatch
        streams (draw_id = i) -- so item i walks in every trial the trajectory the per-trial runner gives it."""

        def __init__(self, base, trials):
            n, nt = len(base.items), len(trials)
            self.items, self.idx_d, self.rs, self.done = base.items * nt, None, None, 0
            if nt not in base.tiles:
                base.tiles = {nt: base.batch.tile(nt)}           # (one tiled copy at a time: slabs of one size reuse it)
            self.batch = base.tiles[nt]
            self.streams = None if base.streams is None else base.streams * nt
            self._row_rngs()
            per_t2 = (sarah_t2_trials if algorithm == 'sarah' else t2_trials) and any('T2' in tr for tr in trials)
            per_hist = hist_trials and any('hist_size' in tr for tr in trials)
            lay = trial_layout(n, trials, {'eta': eta, 'mini_batch_size': mb, 'sigma_modifier': dkw.get('sigma_modifier', 1.0), 'T2': T2,
                                           'hist_size': hist_size},
                               keys=PER_PROBLEM_KEYS + (('T2',) if per_t2 else ()) + (('hist_size',) if per_hist else ()))
            pkw = dict(dkw)
            if any('sigma_modifier' in tr for tr in trials):
                pkw['sigma_modifier'] = lay['sigma_modifier']
            self.eng = E.make_engine(self.batch, make_prox(denoiser, **pkw), lay['eta'], lay['T2'] if per_t2 else T2,
                                     None if algorithm == 'gd' else lay['mini_batch_size'], lr_decay=lr_decay, variant=variant,
                                     algorithm=algorithm, hist_size=lay['hist_size'] if per_hist else hist_size,
                                     seed=base.items[0]['id'] + 1,
                                     draw_id=lay['draw_id'] if self.streams is None else [k for _, k in self.streams], **eng_kw,
                                     **(dict(split_log=True) if per_t2 and algorithm == 'sarah' else {}))

    item_stream = {}                                            # mixed_scales: item id -> (seed, place) of its minibatch stream

    def _group_chunks(items):
        groups = {}
        for it in items:
            groups.setdefault(group_key(it), []).append(it)
        chunks = [g[s0:s0 + max_batch] for g in groups.values() for s0 in range(0, len(g), max_batch)]
        if not mixed_scales:
            return chunks
        item_stream.clear()                                     # (the chunks made below copy what they need)
        for c in chunks:                                        # the default runner's batches: seed = first id + 1, id = place
            for k, it in enumerate(c):
                item_stream[it['id']] = (c[0]['id'] + 1, k)
        items = list(items)
        return [items[s0:s0 + max_batch] for s0 in range(0, len(items), max_batch)]

    def prepare(items):
        """Build this rank's batches (problem data resident in HBM, engines constructed): everything before the iterations."""
        return [_Chunk(c) for c in _group_chunks(items)]

    def check_trials(trials):
        """What a trial-batched run supports, each refusal naming the offender."""
        keys = PER_PROBLEM_KEYS
        if sarah_t2_trials and any('T2' in tr for tr in trials):     # (make_runner: sarah_trials=True, algorithm 'sarah')
            keys = PER_PROBLEM_KEYS + ('T2',)
        elif t2_trials and any('T2' in tr for tr in trials):
            if algorithm != 'svrg':
                raise ValueError(f"batch_trials: trial key 'T2' has no per-problem form for algorithm {algorithm!r} (t2_trials: 'svrg' "
                                 'only; SarahEngine logs its outer prox in a row of its own, the others have no T2)')
            keys = PER_PROBLEM_KEYS + ('T2',)
        if hist_trials and any('hist_size' in tr for tr in trials):
            if algorithm != 'saga':
                raise ValueError(f"batch_trials: trial key 'hist_size' has no per-problem form for algorithm {algorithm!r} (hist_trials: "
                                 "'saga' only; the others keep no gradient table)")
            keys = keys + ('hist_size',)
        if problem == 'pr' and not shared_matrix:
            raise ValueError(f"batch_trials: problem {problem!r} is not supported (only 'csmri') unless its trials share the "
                             'matrix: pass shared_matrix=True to make_runner')
        if wide_trials:                                         # + deblur, saga (csmri, deblur), nlm
            if (algorithm == 'sarah' and not sarah_trials) or (algorithm == 'saga' and problem == 'pr'):
                raise ValueError(f"batch_trials: algorithm {algorithm!r} is not supported on problem {problem!r} (wide_trials: 'gd', "
                                 "'sgd', 'svrg', and 'saga' on 'csmri' or 'deblur'; SarahEngine has no per-problem form)")
        else:
            if problem not in ('csmri', 'pr'):
                raise ValueError(f"batch_trials: problem {problem!r} is not supported (only 'csmri', and 'pr' with shared_matrix=True)")
            if algorithm not in ('gd', 'sgd', 'svrg') and not (sarah_trials and algorithm == 'sarah'):
                raise ValueError(f"batch_trials: algorithm {algorithm!r} is not supported (only 'gd', 'sgd', 'svrg')")
            if denoiser == 'nlm':
                raise ValueError("batch_trials: denoiser 'nlm' is not supported (NLMProx has no per-problem form)")
        if seeding == 'legacy':
            raise ValueError("batch_trials: seeding 'legacy' is not supported (host index lists; use 'counter' or 'generator')")
        for tr in trials:
            bad = [k for k in tr if k not in keys]
            if bad or (callable(denoiser) and 'sigma_modifier' in tr):
                raise ValueError(f'batch_trials: trial key {(bad or ["sigma_modifier"])[0]!r} has no per-problem form here '
                                 f'(per-problem keys: {keys}; a prox factory takes no sigma_modifier)')

    def prepare_data(items):
        """This rank's batches as `prepare` chunks them (the same groups, order and max_batch), data only."""
        return [_Chunk(c, with_engine=False) for c in _group_chunks(items)]

    def run_trials(data, trials, max_batch_trials=1024, max_table_bytes=MAX_TABLE_BYTES):
        """trials: dicts of per-problem overrides -> [results of run(items) per trial], on `data` = prepare_data(items): every
        chunk runs its trials in slabs of at most max_batch_trials problems (at least one trial); a pnp_saga slab also keeps its
        gradient table (hist_size * problems * H * W elements) within max_table_bytes, again with at least one trial; with
        hist_trials the table of a slab is dense over its largest hist_size, so the cap takes the largest value the trials name."""
        check_trials(trials)
        out = [[] for _ in trials]
        for base in data:
            n = len(base.items)
            cap = None
            if algorithm == 'saga':
                h_max = max([int(tr.get('hist_size', hist_size)) for tr in trials]) if hist_trials else hist_size
                cap = table_trial_cap(n, h_max, H * W, torch.empty((), dtype=dtype).element_size(), max_table_bytes)
            for t0, t1 in trial_slabs(len(trials), n, max_batch_trials, cap):
                slab = _TrialSlab(base, trials[t0:t1])
                slab.advance(n_inner)
                for j, r in enumerate(slab.results()):
                    out[t0 + j // n].append(r)
        return [sorted(rs, key=lambda r: r['id']) for rs in out]

    def advance(state, n):
        for c in state:
            c.advance(n)

    def warm(state):
        """Capture the hipGraphs of the batches that will replay them (a timed run then starts with replays, not with the
        capture's own warm-up pass); state and results are unchanged."""
        for c in state:
            eng = c.eng
            if (graph and c.idx_d is None and hasattr(eng, 'run_outer') and eng.s % T2 == 0 and eng.graph is None and eng.graph_ok()):
                eng.capture()

    def collect(state):
        return sorted((r for c in state for r in c.results()), key=lambda r: r['id'])

    def run(items):
        state = prepare(items)
        advance(state, n_inner)
        return collect(state)

    run.prepare, run.advance, run.collect, run.warm = prepare, advance, collect, warm
    run.prepare_data, run.run_trials, run.check_trials = prepare_data, run_trials, check_trials
    run.data_key = (id(images), problem, seeding, H, W, dtype, max_batch, kernel, bool(mixed_scales))
    run.objective = bool(objective)
    run.names = (_REF_NAMES[problem], 'CNN' if callable(denoiser) else _REF_NAMES.get(denoiser, str(denoiser)), 'pnp_' + algorithm)
    return run


def csmri_svrg_runner(images, denoiser_factory, eta, T2, mini_batch_size, n_inner, H=256, W=256, dtype=torch.float32,
                      max_batch=128, seeding='generator', algorithm='svrg', variant='svrg', run_seed=1, keep_trace=False, graph=True):
    """The config-5 runner (CSMRI + pnp_svrg, true SVRG direction): `make_runner(problem='csmri')` with a prox factory."""
    return make_runner(images, 'csmri', algorithm, denoiser_factory, eta=eta, n_inner=n_inner, mini_batch_size=mini_batch_size, T2=T2,
                       H=H, W=W, dtype=dtype, max_batch=max_batch, seeding=seeding, variant=variant, run_seed=run_seed,
                       keep_trace=keep_trace, graph=graph)


def write_csv(path, results, problem='csmri', denoiser='', algorithm='pnp_svrg', params=''):
    """CSV in the reference's schema (script_diff_sampratio_set12.py:131-136, :153-160):
    Problem,Denoiser,Algorithm,Alpha,SNR,Loss,PARAMETERS"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['Problem', 'Denoiser', 'Algorithm', 'Alpha', 'SNR', 'Loss', 'PARAMETERS'])
        for r in results:
            w.writerow([problem, denoiser, algorithm, r['item']['alpha'], r['item']['snr'], r['loss'], params])


# ---------------------------------------------------------------------------------------------- hyper-parameter search
def grid_points(grid):
    """Deterministic trial list from {'eta': [...], 'mini_batch_size': [...], 'T2': [...]}: the cartesian product in
    the key order given (the reference draws trials with hyperopt TPE, script_diff_sampratio_set12.py:116-123; a fixed
    grid is the reproducible replacement -- every item sees the same trials, so trials batch over items)."""
    import itertools
    keys = list(grid)
    return [dict(zip(keys, vals)) for vals in itertools.product(*(grid[k] for k in keys))]


SCORES = ('psnr', 'objective')


def _check_score(score):
    if score not in SCORES:
        raise ValueError(f'score: one of {SCORES}, got {score!r}')


def best_over_trials(per_trial, score='psnr'):
    """per_trial: list of (params, [result dict per item]) -> one row per item with the minimum loss (ties: first trial,
    like hyperopt's best_trial on equal losses) and the parameters that achieved it.  NaN losses never win.
    score='objective': the trial with the smallest 'f_final' wins instead (same ties, NaN never wins), and the row carries it; the
    results must hold 'f_final' (runners made with objective=True) -- ValueError otherwise."""
    _check_score(score)
    key = 'loss' if score == 'psnr' else 'f_final'
    if score == 'objective':
        for _, results in per_trial:
            if any('f_final' not in r for r in results):
                raise ValueError("score='objective' needs result rows with 'f_final': make the runners with objective=True")
    best = {}
    for params, results in per_trial:
        for r in results:
            cur = best.get(r['id'])
            val = r[key]
            if cur is None or (not np.isnan(val) and (np.isnan(cur[key]) or val < cur[key])):
                best[r['id']] = {'id': r['id'], 'item': r['item'], 'loss': r['loss'], 'params': dict(params),
                                 'psnr_init': r.get('psnr_init'), 'psnr_final': r.get('psnr_final')}
                if score == 'objective':
                    best[r['id']]['f_final'] = val
    return [best[k] for k in sorted(best)]


PER_PROBLEM_KEYS = ('eta', 'mini_batch_size', 'sigma_modifier')


def group_trials(trials, per_problem_keys=PER_PROBLEM_KEYS):
    """Trials (dicts, grid order) -> [(structural params, [trial indices])]: trials that agree in every key that is not per
    problem (by default T2 and hist_size included: they change the schedule and the table; `per_problem_keys` with 'T2' or 'hist_size'
    among them groups across it) form a group, groups and members in order of first appearance."""
    groups = {}
    for t, tr in enumerate(trials):
        key = tuple((k, tr[k]) for k in tr if k not in per_problem_keys)
        groups.setdefault(key, []).append(t)
    return [(dict(key), idx) for key, idx in groups.items()]


MAX_TABLE_BYTES = 8 * 2 ** 30                                   # default bound on the SAGA gradient table of one trial slab


def table_trial_cap(n_items, hist_size, n_elems, itemsize, max_table_bytes=MAX_TABLE_BYTES):
    """Trials per slab that keep a SAGA gradient table -- hist_size * (trials * n_items) * n_elems elements of itemsize bytes --
    within max_table_bytes; never below one trial (a single trial's table is what the per-trial runner allocates anyway)."""
    per_trial = int(hist_size) * max(1, int(n_items)) * int(n_elems) * int(itemsize)
    return max(1, int(max_table_bytes) // per_trial)


def trial_slabs(n_trials, n_items, max_batch_trials, max_trials=None):
    """[t0, t1) trial ranges of the slabs: as many whole trials as fit into max_batch_trials problems -- and, when given, at most
    max_trials of them (table_trial_cap) -- at least one."""
    per = max(1, int(max_batch_trials) // max(1, int(n_items)))
    if max_trials is not None:
        per = max(1, min(per, int(max_trials)))
    return [(t0, min(t0 + per, n_trials)) for t0 in range(0, n_trials, per)]


def trial_layout(n_items, trials, defaults, keys=PER_PROBLEM_KEYS):
    """Per-problem vectors of a slab of len(trials) trials over n_items items: problem b = t * n_items + i carries trial t's
    value of every per-problem key (`defaults` where the trial names none) and draw_id[b] = i.  keys: the per-problem keys to lay
    out; with 'T2' or 'hist_size' among them the layout holds an int32 vector of that name as well."""
    nt = len(trials)
    lay = {'draw_id': np.tile(np.arange(n_items, dtype=np.int64), nt)}
    for k in keys:
        if defaults.get(k) is None and not any(k in tr for tr in trials):
            lay[k] = None
            continue
        vals = np.repeat(np.array([tr.get(k, defaults.get(k)) for tr in trials]), n_items)
        lay[k] = vals.astype(np.int32 if k in ('mini_batch_size', 'T2', 'hist_size') else np.float64)
    return lay


def grid_search(items, make_runner, grid, group=None, *, batch_trials=False, max_batch_trials=1024, max_table_bytes=MAX_TABLE_BYTES,
                batch_T2=False, score='psnr', batch_hist=False):
    """The sweep the reference scripts run (process_img, script_diff_sampratio_set12.py:103-131): for every work item
    search the hyper-parameters and keep the best trial.  `make_runner(**params)` returns a runner as `run_sweep`
    takes; each rank runs every trial on ITS shard of the items (one batched engine per trial), the reduction over
    trials is local and the single gather at the end carries one small row per item.
    batch_trials=True (CSMRI, or PR from runners made with shared_matrix=True: every trial of an item then works on the item's one
    matrix, which is never copied; gd, sgd, svrg; not NLM; not legacy seeding -- ValueError otherwise): the trials of a rank run as
    ONE batch per chunk instead of one after the other.  Keys 'eta', 'mini_batch_size', 'sigma_modifier' become
    per-problem vectors; trials are grouped by every other key (T2 included), the problem data of a chunk is prepared once and
    shared by all groups, and a group runs on the chunk tiled once per trial in slabs of at most max_batch_trials problems.
    Runners made with wide_trials=True also take Deblur, pnp_saga (csmri, deblur) and the NLM prox; a pnp_saga slab is
    capped so that its gradient table stays within max_table_bytes (never below one trial).  Runners made with sarah_trials=True
    also take pnp_sarah on csmri, on deblur with wide_trials=True and on pr with shared_matrix=True.
    batch_T2=True (with batch_trials=True; runners made with t2_trials=True, pnp_svrg only -- ValueError otherwise): 'T2' is a
    per-problem key too, so trials that differ in T2 share a batch instead of splitting the grid.  Off by default.
    Runners made with sarah_trials=True, sarah_t2_trials=True take it for pnp_sarah as well.
    batch_hist=True (with batch_trials=True; runners made with hist_trials=True, pnp_saga only -- ValueError otherwise): 'hist_size' is
    a per-problem key too, so trials that differ in hist_size share a batch whose gradient table is dense over the largest of them
    (DESIGN 9.8).  Off by default.
    The rows returned are those of batch_trials=False.
    score: 'psnr' (default) keeps the trial with the smallest PSNR loss, as always; 'objective' keeps the trial with the smallest
    'f_final' -- the selection for measured data, where there is no ground truth -- and needs runners made with objective=True
    (ValueError before anything runs otherwise); its rows also carry 'f_final'."""
    _check_score(score)

    def check_runner(run):
        if score == 'objective' and not getattr(run, 'objective', True):       # (a runner that does not say is judged by its rows)
            raise ValueError("score='objective' needs runners made with objective=True (their rows carry 'f_final')")
        return run
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    mine = shard(items, rank, world)
    trials = grid_points(grid)
    per_trial = []
    if batch_T2 and not batch_trials:
        raise ValueError('batch_T2 groups the trials of a trial-batched grid: it needs batch_trials=True')
    if batch_hist and not batch_trials:
        raise ValueError('batch_hist groups the trials of a trial-batched grid: it needs batch_trials=True')
    if batch_trials:
        per_trial, data = [None] * len(trials), {}
        keys = PER_PROBLEM_KEYS + (('T2',) if batch_T2 else ()) + (('hist_size',) if batch_hist else ())
        for _, idx in group_trials(trials, keys):
            run = check_runner(make_runner(**trials[idx[0]]))
            if not hasattr(run, 'run_trials'):
                raise ValueError('batch_trials needs runners of sweep.make_runner (run.prepare_data / run.run_trials)')
            sub = [{k: v for k, v in trials[t].items() if k in keys} for t in idx]
            run.check_trials(sub)
            if run.data_key not in data:
                data[run.data_key] = run.prepare_data(mine)
            for t, res in zip(idx, run.run_trials(data[run.data_key], sub, max_batch_trials, max_table_bytes)):
                per_trial[t] = (trials[t], [{k: v for k, v in r.items() if k != 'z'} for r in res])
    else:
        for params in trials:
            res = check_runner(make_runner(**params))(mine) if mine else []
            per_trial.append((params, [{k: v for k, v in r.items() if k != 'z'} for r in res]))
    return gather_results(best_over_trials(per_trial, score), 0, group)


def write_tuning_csv(path, rows, problem='csmri', denoiser='', algorithm='pnp_svrg'):
    """The reference's result file, row for row (script_diff_sampratio_set12.py:131-136,153-160): a 'Results:' line,
    then Problem,Denoiser,Algorithm,Alpha,SNR,Loss,'PARAMETERS:',key,value,key,value,..."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w', newline='') as f:
        w = csv.writer(f, delimiter=',')
        w.writerow(['Results:'])
        for r in rows:
            row = [problem, denoiser, algorithm, r['item']['alpha'], r['item']['snr'], r['loss'], 'PARAMETERS:']
            for k, v in r['params'].items():
                row += [k, v]
            w.writerow(row)
