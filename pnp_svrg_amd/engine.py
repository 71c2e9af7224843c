"""Batched, sync-free PnP engines: B independent reconstructions advance together, one inner iteration per
`step()`, entirely in HBM.

These are the throughput forms of the reference loops -- algorithms/pnp_svrg.py:26-95, pnp_sgd.py:24-70,
pnp_gd.py:24-70, pnp_sarah.py:28-104, pnp_saga.py:25-72 -- for the sweep-style workloads of script_diff_*_set12.py,
where many reconstructions (image x sampling ratio x SNR x trial) are independent.  Nothing is read back per
iteration: squared errors (for PSNR) accumulate in a device log.  The drop-in loops of `algorithms.py` (golden-pinned)
are the specification: every engine is tested to walk the same trajectory as B drop-in loops fed the same minibatches.

The batch problems (CsmriBatch, DeblurBatch, PrBatch: the data of B problems and their gradients) are in `batches.py`, the prox
adapters (TVProx, DnCNNProx, NLMProx) in `prox.py`; both are re-exported here.

What each engine accepts.  Every option is opt-in: without it an engine makes exactly the calls it made before the option existed, and
with a per-problem value problem b walks, bit for bit, the trajectory a scalar engine with b's value walks.

Every engine: `eta` as a scalar or a [B] array on a batch with `per_problem` set (a CsmriBatch, `PrBatch.tile(n)`,
`DeblurBatch.tile(n)`).  A scalar stays the Python float of the plain calls; an array goes to the `_pp` entry points as a float64
device vector made on the host (`_c`: remade only when lr_decay changes it).  `log_objective=True`: a second ring `obj_log`,
row for row beside `sse_log`, of f(iterate) per logged prox (`objective_log()`); such an engine steps eagerly.
SgdEngine, SvrgEngine, SarahEngine, SagaEngine: `mini_batch_size` as a scalar or [B] int array, `draw_id` ([B] ints that replace the
batch index in the minibatch stream), host index lists per step (`step(idx_s)`).
GdEngine, SgdEngine, SagaEngine: `fused=True`, a step as ONE `pnp_csmri_grad_step` / `pnp_csmri_saga_step` on a float32
256 x 256 CsmriBatch; `run_span(n)`, launches of at most AHEAD steps of `pnp_csmri_grad_span` / `pnp_csmri_saga_span`.
SvrgEngine: `variant`, `fused` (None: by batch size) with `fold_outer`, `capture()` / `run_outer(n)` as a hipGraph or as one launch
per outer iteration; `T2` as a [B] int array with `span` and `run_span(n)` (`pnp_refresh_pp`, `pnp_csmri_svrg_span_pp`).
SarahEngine: per-problem values through `pnp_axpbypcz_pp`; `fused=True` with `capture()` / `run_outer(n)`,
`run_outer(n, one_launch=True)`; `T2` as a [B] int array with `split_log=True`: the outer rows in a ring
of their own, `span` and `run_span(n)` (`pnp_refresh_pp`, `pnp_select_pp`, `pnp_csmri_sarah_span_pp`).
SagaEngine: rows per step for the batch or per problem (one `pnp_saga_table_update_pp` launch); `hist_size` as a [B] int
array.
The one-kernel forms hold the per-column TV prox, the single-step kernels and SvrgEngine's one-launch outer iteration also the 2-D
wavelet prox of TVProx(in_kernel=True); any other prox with `fused_args` follows the kernel (`after_fused`).
"""
import numpy as np
import torch

from . import ops
from .batches import Minibatches, _BatchBase, CsmriBatch, DeblurBatch, PrBatch  # noqa: F401  (re-exported)
from .prox import TVProx, DnCNNProx, NLMProx  # noqa: F401  (re-exported)


class LoopEngine:
    """State and log machinery shared by the engines: the iterate z [B, H, W], a device log ring of the squared errors
    of every prox evaluation (-> rounded PSNR traces like the reference's psnr_per_iter), the step counter."""

    def __init__(self, batch, prox, eta, lr_decay=1.0, n_log=4096, seed=0, log_objective=False):
        self.b, self.prox, self.eta, self.lr_decay, self.seed = batch, prox, eta, lr_decay, seed
        self.log_objective = bool(log_objective)
        if np.ndim(eta) != 0:                                   # per-problem step sizes
            self.eta = np.ascontiguousarray(eta, np.float64)
            if self.eta.shape != (batch.B,) or not batch.per_problem:
                raise ValueError(f'per-problem eta: {batch.B} values on a CsmriBatch, got shape {self.eta.shape} on {batch.kind!r}')
        self._coef = {}
        dev = batch.xrec.device
        self.z = batch.xinit.clone()
        self.sse_log = torch.zeros((n_log, batch.B), dtype=torch.float64, device=dev)
        self.n_log = n_log
        # log_objective: a second ring, row for row beside sse_log, of f(iterate the logged prox returned) (batch.objective)
        self.obj_log = torch.zeros((n_log, batch.B), dtype=torch.float64, device=dev) if self.log_objective else None
        prox.bind(batch)
        self.s = 0                                              # inner iterations done
        self.n_prox = 0                                         # prox evaluations logged
        self.graph = None

    def reset(self):
        self.z.copy_(self.b.xinit)
        self.s = self.n_prox = 0
        if hasattr(self.prox, 't'):
            self.prox.t = 0

    def _c(self, name, k, v):
        """A coefficient as the kernels take it: a scalar stays the Python float of the plain calls; a per-problem array (float64,
        made on the host) is uploaded -- once when lr_decay == 1, else whenever the decay exponent k changes."""
        if np.ndim(v) == 0:
            return v
        key = (k if np.ndim(k) == 0 else tuple(k)) if self.lr_decay != 1.0 else 0       # (per-problem T2: one exponent per problem)
        hit = self._coef.get(name)
        if hit is None or hit[0] != key:
            hit = self._coef[name] = (key, torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(self.z.device))
        return hit[1]

    def _prox(self, z):
        out = self.prox(z, self.b.xrec, self.sse_log[self.n_prox % self.n_log])
        if self.log_objective:
            self._log_obj(self.n_prox % self.n_log, out)
        self.n_prox += 1
        return out

    def _log_obj(self, row, z):
        """log_objective: f(z) per problem into the row of obj_log that the SSE of this prox went to."""
        self.b.objective(z, out=self.obj_log[row])

    def _ring(self, log):
        """The rows of a log ring in chronological order: when more than n_log evaluations were logged, the last n_log of them."""
        if self.n_prox > self.n_log:
            return torch.roll(log, -(self.n_prox % self.n_log), 0)             # oldest surviving row first
        return log[:self.n_prox]

    def _psnr(self, log):
        """The rows of a ring of squared errors as PSNR, rounded to 0.01 dB like problems/problem.py:33-35, read back once (NaN stays
        NaN: the split log of SarahEngine)."""
        sse = self._ring(log).cpu().numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.around(10 * np.log10(1.0 / (sse / self.b.N)), 2)

    def objective_log(self):
        """[prox evaluations][B] float64: f of the iterate every logged prox returned, in chronological order, read back once; the
        rows are those of `psnr_trace` (when more than n_log evaluations were logged, the last n_log of them).  Needs an engine made
        with log_objective=True."""
        if not self.log_objective:
            raise ValueError('objective_log() needs an engine made with log_objective=True')
        return self._ring(self.obj_log).cpu().numpy()

    def _launched(self, steps, rows):
        """The counters after a launch (or a graph replay) that ran `steps` inner iterations and logged `rows` prox evaluations."""
        self.s += steps
        self.n_prox += rows
        if hasattr(self.prox, 't'):                             # (DnCNNProx keeps no call count)
            self.prox.t += rows

    def _run_steps(self, n):
        """`run_span(n)` where no span kernel applies: n eager steps."""
        for _ in range(n):
            self.step()

    def _fused_call(self, call, args, out, sse_out, **kw):
        """The envelope of every one-kernel call: plan method `call` on `args`, its result in `out`.  A prox inside the kernel
        writes its squared errors straight to the log row `sse_out`; one that is not (DnCNN, the 2-D wavelet prox) follows the
        kernel through `after_fused`."""
        b, px = self.b, self.prox
        call(*args, out=out, denoise=_fused_kind(px), xrec=b.xrec, sse=sse_out if px.fused_denoise else None, **kw, **px.fused_args())
        px.after_fused(out, b.xrec, sse_out)

    def _capture_graph(self, body, state):
        """`body` (the launches of one outer iteration) captured into a hipGraph (torch.cuda.CUDAGraph on ROCm): a warm-up pass on a
        side stream, then the capture.  `state` (the tensors `body` writes) and the prox's call counter are restored, also when the
        capture fails.  The one capture site of the engines."""
        keep = [t.clone() for t in state]
        t_keep = getattr(self.prox, 't', None)
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body()                                          # warm-up outside capture (lazy module loads)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with ops.collector_held(), torch.cuda.graph(g):     # (no plan may be destroyed, hipFree, while the stream captures)
                body()
            torch.cuda.synchronize()
        finally:
            for dst, src in zip(state, keep):
                dst.copy_(src)
            if t_keep is not None:
                self.prox.t = t_keep
        return g

    def psnr_trace(self):
        """[prox evaluations][B] PSNR (rounded to 0.01 dB like problems/problem.py:33-35) in chronological order,
        read back once; when more than n_log evaluations were logged, the last n_log of them."""
        return self._psnr(self.sse_log)


def _fused_missing(batch, prox, log_objective):
    """What the one-kernel forms need and this batch, prox or log does not give: every missing piece, named."""
    missing = []
    if getattr(batch, 'kind', None) != 'csmri':
        missing.append(f'a CsmriBatch (got {getattr(batch, "kind", type(batch).__name__)!r})')
    else:
        if batch.dtype != torch.float32:
            missing.append(f'float32 (got {batch.dtype})')
        if (batch.H, batch.W) != (256, 256):
            missing.append(f'256 x 256 images (got {batch.H} x {batch.W})')
    if not hasattr(prox, 'fused_args'):
        missing.append(f'a prox with fused_args: TVProx or DnCNNProx (got {type(prox).__name__})')
    if log_objective:
        missing.append('log_objective=False')
    return missing


def _check_fused(name, batch, prox, log_objective):
    """`fused=True` of GdEngine, SgdEngine, SagaEngine and SarahEngine: refused with everything that is missing."""
    missing = _fused_missing(batch, prox, log_objective)
    if missing:
        raise ValueError(f'{name}(fused=True) needs ' + ', '.join(missing))


def _check_one_pass(name, batch, fused):
    """`one_pass=True` of SvrgEngine and SarahEngine: the correction and the step of the streaming path as ONE
    pnp_deblur_grad_step."""
    if getattr(batch, 'kind', None) != 'deblur' or getattr(batch, 'M_vec', None) is not None:
        raise ValueError(f'{name}(one_pass=True) needs a uniform DeblurBatch (got {type(batch).__name__}'
                         f'{" of mixed scales" if getattr(batch, "M_vec", None) is not None else ""}): the one-pass step is a Deblur kernel')
    if fused:
        raise ValueError(f'{name}(one_pass=True) goes with the streaming path, not with fused=True (the one-kernel CSMRI iteration)')


class _FusedStep:
    """The one-kernel inner iteration of GdEngine, SgdEngine and SagaEngine (fused=True) and their span kernels."""

    def span_kernel_ok(self):
        """Whether `run_span` can run its steps as launches of a span kernel (pnp_csmri_grad_span / pnp_csmri_saga_span): the
        one-kernel iteration with the prox inside it (TV, no host-side per-call state), device-drawn minibatches, no objective log
        and a constant step size (the coefficients of a launch are those of its first step)."""
        mbs = getattr(self, 'mbs', None)
        return (self.fused and getattr(self.prox, 'fused_denoise', False) and not _in_kernel_2d(self.prox)
                and getattr(self.prox, 'denoise_strength', 0.0) == 0.0 and (mbs is None or all(h is None for h in mbs.host)) and not self.log_objective and self.lr_decay == 1.0)

    def _one_kernel(self, call, *args, **kw):
        self._fused_call(call, args, self.z, self.sse_log[self.n_prox % self.n_log], **kw)
        self.n_prox += 1


def _fused_kind(px):
    """`denoise` of a one-kernel step for prox px: 0 = the kernel stores the stepped image (the prox follows it), 1 = the per-column
    TV prox inside it, 2 = the 2-D wavelet prox inside it (TVProx(multi=False, in_kernel=True))."""
    return int(getattr(px, 'fused_kind', 1)) if px.fused_denoise else 0


def _in_kernel_2d(px):
    """Whether px is the 2-D wavelet prox held inside the one-kernel iteration: the single-step kernels and SvrgEngine's one-launch
    outer iteration hold it, the span kernels and the SARAH outer kernel do not."""
    return bool(getattr(px, 'fused_denoise', False)) and getattr(px, 'fused_kind', 1) == 2


class GdEngine(_FusedStep, LoopEngine):
    """pnp_gd over a batch (algorithms/pnp_gd.py:24-70): z <- prox(z - eta * decay^i * grad_full(z)).
    fused=True (opt-in): a step is ONE pnp_csmri_grad_step on the mask and its packed data term."""

    AHEAD = 16                                                  # steps per span launch (the draw window of the stochastic engines)

    def __init__(self, batch, prox, eta, lr_decay=1.0, n_log=4096, seed=0, log_objective=False, *, fused=False):
        self.fused = bool(fused)
        if self.fused:
            _check_fused('GdEngine', batch, prox, log_objective)
        super().__init__(batch, prox, eta, lr_decay, n_log, seed, log_objective=log_objective)

    def step(self):
        lr = self.eta * self.lr_decay ** self.s
        if self.fused:
            b = self.b
            self._one_kernel(b.plan.grad_step, self.z, b.bits, yh=b.yh_full, alpha=self._c('-lr', self.s, -lr), alpha_vec=b.inv_m0,
                             beta=1.0, c1=self.z)
            self.s += 1
            return
        self.b.grad_full(self.z, out=self.z, alpha=self._c('-lr', self.s, -lr), beta=1.0, c1=self.z)
        self.z = self._prox(self.z)
        self.s += 1

    def run_span(self, n):
        """n inner iterations.  Where `span_kernel_ok()` holds they run in launches of at most AHEAD steps, ONE pnp_csmri_grad_span
        each, in which the workgroup that owns a problem runs its steps back to back -- the same bits as stepping; otherwise n
        eager steps."""
        if not self.span_kernel_ok():
            return self._run_steps(n)
        b, px = self.b, self.prox
        while n > 0:
            m = min(n, self.AHEAD)
            lr = self.eta * self.lr_decay ** self.s             # (span_kernel_ok: lr_decay == 1)
            b.plan.grad_span(self.z, b.bits, m, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig, yh=b.yh_full,
                             alpha=self._c('-lr', self.s, -lr), alpha_vec=b.inv_m0, beta=1.0, sigma_modifier=px.sigma_modifier)
            self._launched(m, m)
            n -= m


def _int_vector(batch, name, values):
    """A per-problem integer hyper-parameter (`T2`, `hist_size`) checked on the host (the kernels cannot): -> the [B] int64 vector.
    Every refusal names the offender."""
    v = np.asarray(values)
    if not batch.per_problem:
        raise ValueError(f'per-problem {name} needs a batch that takes per-problem values (got {batch.kind!r})')
    if v.shape != (batch.B,) or not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f'per-problem {name}: {batch.B} integers, got shape {v.shape} of {v.dtype}')
    bad = np.flatnonzero((v < 1) | (v > np.iinfo(np.int32).max))
    if bad.size:
        raise ValueError(f'per-problem {name}: entries must be >= 1 (problem {int(bad[0])}: {name} {int(v[bad[0]])})')
    return np.ascontiguousarray(v, np.int64)


class _StochEngine(LoopEngine):
    # Engines that draw one minibatch per step (sgd, saga, sarah) draw AHEAD steps per launch: the draw kernel is
    # latency-bound (a 32-step radix select per problem, ~50 us whatever the grid), and a step's descriptor depends on
    # (seed, step, problem) only, so a window of steps drawn together holds the very same selections.
    AHEAD = 16

    def __init__(self, batch, prox, eta, mini_batch_size, lr_decay=1.0, n_log=4096, seed=0, n_slots=None, draw_id=None,
                 log_objective=False):
        super().__init__(batch, prox, eta, lr_decay, n_log, seed, log_objective=log_objective)
        batch._check_mb(mini_batch_size)
        self.mb = self._mb_draw = mini_batch_size               # (host value for the coefficients, what the draws take)
        self._draw_kw = {}
        if np.ndim(mini_batch_size) != 0 or draw_id is not None:
            if not batch.per_problem:                           # (a CsmriBatch, or a PrBatch tiled on shared matrices)
                raise ValueError(f'per-problem mini_batch_size / draw_id need a CsmriBatch (got {batch.kind!r})')
            dev = batch.xrec.device
            if np.ndim(mini_batch_size) != 0:
                self.mb = np.ascontiguousarray(mini_batch_size, np.int32)
                self._mb_draw = torch.from_numpy(self.mb).to(dev)
            if draw_id is not None:                             # the 32-bit ids the minibatch streams absorb
                ids = np.array([int(v) & 0xFFFFFFFF for v in np.ravel(draw_id)], np.uint32)
                if ids.shape != (batch.B,):
                    raise ValueError(f'draw_id: {batch.B} values, got {ids.shape}')
                self._draw_kw = dict(draw_id=torch.from_numpy(ids.view(np.int32)).to(dev))
        self._window = n_slots is None                          # one draw launch per AHEAD steps (else: the subclass draws)
        self.mbs = batch.minibatches(self.AHEAD if n_slots is None else n_slots)
        self._drawn_base = None                                 # first step of the window the slots currently hold
        self._hostbits = None                                   # one-kernel forms: the packed bits of a host-fed slot

    def _slot_bits(self, j):
        """The selector bits of slot j as the one-kernel forms take them."""
        if self.mbs.host[j] is not None:                        # host-drawn selector: pack it to bits (a 5 us launch)
            self._hostbits = self.b.plan.pack_mask(self.mbs.host[j], out=self._hostbits)
            return self._hostbits
        return self.mbs.selbits[j]

    def _minibatch(self, idx_s, step_id):
        """Bind a slot to this step's minibatch and return it: host index lists when given (slot 0), else a device draw."""
        if idx_s is not None:
            self.b.set_host(self.mbs, 0, idx_s)
            self._drawn_base = None
            return 0
        if not self._window or step_id >= 0xFFFFFFF0:          # (0xFFFFFFFF: the table-filling draw of pnp_saga)
            self.b.draw(self.mbs, self._mb_draw, self.seed, step_id, 1, **self._draw_kw)
            self._drawn_base = None
            return 0
        base = step_id - step_id % self.AHEAD
        if self._drawn_base != base:
            self.b.draw(self.mbs, self._mb_draw, self.seed, base, self.AHEAD, **self._draw_kw)
            self._drawn_base = base
        return step_id - base

    def _draw_slot(self, slot, step_id):
        self.b.draw(self.mbs.slot(slot), self._mb_draw, self.seed, step_id, 1, **self._draw_kw)
        self.mbs.host[slot] = None


class _T2PerProblem:
    """Per-problem T2 of SvrgEngine and SarahEngine, mixed into exactly those two: T2 as a [B] int64 vector and
    its int32 device vector `_t2_dev` (None with a scalar T2), and the draw slots as a window of `span` steps drawn with the absolute
    step ids: the slots hold steps [_drawn_base, _drawn_base + _drawn_n)."""
    _t2_dev = None
    _drawn_n = 0

    def _init_t2(self, batch, T2, span):
        """Before the base constructor (the window is its slot count): T2 as given, or as the checked vector.  -> whether T2 is
        per problem."""
        self.T2 = T2
        if np.ndim(T2) == 0:
            return False
        self.T2 = _int_vector(batch, 'T2', T2)
        self.span = int(self.AHEAD if span is None else span)
        if self.span < 1:
            raise ValueError(f'span: at least one step per draw window, got {span}')
        self._t2_dev = torch.from_numpy(self.T2.astype(np.int32)).to(batch.xrec.device)
        return True

    def refreshes(self, s):
        """Whether any problem refreshes at step s (the host knows s and the vector)."""
        return bool((s % self.T2 == 0).any())

    def _lr_pp(self, s):
        """(step sizes, decay exponents k_b = s // T2_b) of step s.  Each step size is the product the scalar engine forms from
        problem b's values, eta_b * lr_decay ** k_b in Python floats; lr_decay == 1 leaves eta as it was given."""
        k = s // self.T2
        if self.lr_decay == 1.0:
            return self.eta, k
        eta = np.broadcast_to(np.asarray(self.eta, np.float64), k.shape)
        return np.array([float(e) * self.lr_decay ** int(kb) for e, kb in zip(eta, k)], np.float64), k

    def _draw_span(self, m):
        """Draw the window of the m steps from self.s on."""
        self.b.draw(self.mbs, self._mb_draw, self.seed, self.s, m, **self._draw_kw)
        self._drawn_base, self._drawn_n = self.s, m

    def _slot_pp(self, idx_s):
        """The slot that holds this step's minibatch -- a new window of `span` steps when the step is outside the one the slots
        hold; host index lists go to slot 0."""
        if idx_s is not None:
            self.b.set_host(self.mbs, 0, idx_s)
            self._drawn_base = None
            return 0
        if self._drawn_base is None or not self._drawn_base <= self.s < self._drawn_base + self._drawn_n:
            self._draw_span(self.span)
        return self.s - self._drawn_base


class SgdEngine(_FusedStep, _StochEngine):
    """pnp_sgd over a batch (algorithms/pnp_sgd.py:24-70): v = grad_stoch(z, mb) / mini_batch_size.
    fused=True (opt-in): a step is ONE pnp_csmri_grad_step on the drawn slot and the raw data."""

    def __init__(self, batch, prox, eta, mini_batch_size, lr_decay=1.0, n_log=4096, seed=0, n_slots=None, draw_id=None,
                 log_objective=False, *, fused=False):
        self.fused = bool(fused)
        if self.fused:
            _check_fused('SgdEngine', batch, prox, log_objective)
        super().__init__(batch, prox, eta, mini_batch_size, lr_decay, n_log, seed, n_slots=n_slots, draw_id=draw_id,
                         log_objective=log_objective)

    def step(self, idx_s=None):
        j = self._minibatch(idx_s, self.s)
        lr = self.eta * self.lr_decay ** self.s
        if self.fused:
            b = self.b
            self._one_kernel(b.plan.grad_step, self.z, self._slot_bits(j), YT=b.YT, alpha=self._c('-lr/mb', self.s, -lr / self.mb),
                             beta=1.0, c1=self.z)
            self.s += 1
            return
        self.b.grad_stoch(self.z, self.mbs, j, out=self.z, alpha=self._c('-lr/mb', self.s, -lr / self.mb), beta=1.0, c1=self.z)
        self.z = self._prox(self.z)
        self.s += 1

    def run_span(self, n):
        """n inner iterations.  Where `span_kernel_ok()` holds they run in launches of at most AHEAD steps -- one draw of m steps from
        the absolute step id plus ONE pnp_csmri_grad_span each, in which the workgroup that owns a problem runs its steps back to
        back -- the same bits as stepping; otherwise n eager steps."""
        if not self.span_kernel_ok():
            return self._run_steps(n)
        b, px = self.b, self.prox
        while n > 0:
            m = min(n, self.AHEAD)
            b.draw(self.mbs, self._mb_draw, self.seed, self.s, m, **self._draw_kw)
            self._drawn_base = None                             # (a later eager step redraws its own window)
            lr = self.eta * self.lr_decay ** self.s             # (span_kernel_ok: lr_decay == 1)
            b.plan.grad_span(self.z, self.mbs.selbits, m, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig, YT=b.YT,
                             alpha=self._c('-lr/mb', self.s, -lr / self.mb), beta=1.0, sigma_modifier=px.sigma_modifier)
            self._launched(m, m)
            n -= m


class SvrgEngine(_T2PerProblem, _StochEngine):
    """pnp_svrg over a batch.  variant='svrg' is the true direction (pnp_svrg.py:53), 'reference' is what v1
    executes (v = mu, :54).  `step()` = one inner iteration (the outer full-gradient refresh happens inside when
    s % T2 == 0, as in the reference's loop nest).  Device draws of a whole outer iteration are ONE launch at the
    refresh (T2 descriptor slots).
    T2: an int, or a [B] integer array on a batch that takes per-problem values: problem b then refreshes at the steps
    with s % T2[b] == 0 and walks, bit for bit, the trajectory a scalar engine with T2[b] walks.  The draw slots then hold a window
    of `span` steps (default: AHEAD) drawn with the absolute step ids, `step()` refreshes with a full gradient into a scratch and
    one pnp_refresh_pp launch (the unfolded refresh, also on the one-kernel path), `run_span(n)` runs n steps in launches of at
    most `span` steps where `outer_kernel_ok()` holds, and there is no hipGraph form (`graph_ok()` is False, `run_outer` raises).
    one_pass=True (opt-in): on a uniform DeblurBatch the streaming path's correction and step are ONE
    pnp_deblur_grad_step (not the default's bits: z - w is rounded once); ValueError on any other batch and with fused=True."""
    FUSED_MIN_BATCH = 192

    def __init__(self, batch, prox, eta, T2, mini_batch_size, lr_decay=1.0, variant='svrg', n_log=4096, seed=0, fused=None,
                 fold_outer=True, draw_id=None, span=None, log_objective=False, one_pass=False):
        self.one_pass = bool(one_pass)
        if self.one_pass:
            _check_one_pass('SvrgEngine', batch, fused)
        self._diff_kw = dict(one_pass=True) if self.one_pass else {}      # (off: grad_stoch_diff gets the arguments it always got)
        if np.ndim(T2) == 0 and span is not None:
            raise ValueError('span is the draw window of a per-problem T2; a scalar T2 draws an outer iteration at a time')
        pp = self._init_t2(batch, T2, span)
        super().__init__(batch, prox, eta, mini_batch_size, lr_decay, n_log, seed, n_slots=self.span if pp else T2, draw_id=draw_id,
                         log_objective=log_objective)
        self.variant = variant
        self._mu_new = torch.empty_like(self.z) if pp else None     # per-problem T2: the refresh's scratch
        # the one-kernel inner iteration (csrc/csmri_fused.hip): CSMRI, f32, 256 x 256, true SVRG direction, a prox that
        # can follow it (TV inside the kernel, DnCNN after it)
        ok = variant == 'svrg' and not _fused_missing(batch, prox, False)
        if fused and not ok:
            raise ValueError('the one-kernel iteration needs a float32 256 x 256 CsmriBatch, variant="svrg" and a TV or DnCNN prox')
        # one workgroup per image: it pays off from about a workgroup per CU (measured: B = 120 is slower than the
        # streaming kernels, B = 256 faster), so small batches keep the four streaming kernels unless asked otherwise
        self.fused = (ok and batch.B >= self.FUSED_MIN_BATCH) if fused is None else bool(fused)
        self.fold_outer = fold_outer                            # False: refresh as launches of its own (A/B, tests)
        dev = batch.xrec.device
        self.w = torch.empty_like(self.z)
        self.mu = torch.empty_like(self.z)
        # device-resident step counter (mirrors self.s) and scratch row: a whole outer iteration can then be
        # captured once in a hipGraph and replayed (no host-side step index inside the graph)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._dev_step = 0                                      # the value step_dev currently holds
        self.sse_tmp = torch.zeros(batch.B, dtype=torch.float64, device=dev)

    def reset(self):
        super().reset()
        self.step_dev.zero_()
        self._dev_step = 0

    def step(self, idx_s=None):
        """One inner iteration for all B problems.  idx_s: int32 [B][mb] minibatch index lists (e.g. drawn from
        NumPy's legacy stream for reference-identical runs); None = device draws."""
        b, s = self.b, self.s
        if self._t2_dev is not None:
            j, (lr, k) = self._refresh_pp(idx_s), self._lr_pp(s)
        else:
            j, k = s % self.T2, s // self.T2
            lr = self.eta * self.lr_decay ** k
            if j == 0:                                          # outer: mu = grad_full(z); w = z
                if self.variant == 'svrg' and idx_s is None:
                    b.draw(self.mbs, self._mb_draw, self.seed, s, self.T2, **self._draw_kw)
                if not (self.fused and self.fold_outer):        # (folded: the first inner iteration's kernel does it)
                    b.grad_full(self.z, out=self.mu)
                    self.w.copy_(self.z)
            if self.variant == 'svrg':
                if idx_s is not None:                           # (at a folded j = 0 the minibatch is bound but cannot matter)
                    b.set_host(self.mbs, j, idx_s)
                elif self.mbs.host[j] is not None:              # a host-fed outer iteration continued with device draws
                    self._draw_slot(j, s)
        row = self.n_prox % self.n_log
        self.z = self._inner(j, lr, k, self.sse_log[row])
        if self.log_objective:
            self._log_obj(row, self.z)
        self.n_prox += 1
        self.s += 1                                             # eager steps keep the index on the host (no counter launch)

    def _refresh_pp(self, idx_s):
        """The head of `step()` with a per-problem T2: where any problem refreshes, grad_full into the scratch and ONE
        pnp_refresh_pp; -> the slot of the ordinary inner iteration that follows for all problems (at a problem's own refresh step
        w == z: its SVRG difference is exactly zero)."""
        if self.refreshes(self.s):
            self.b.grad_full(self.z, out=self._mu_new)
            ops.refresh_pp(self._mu_new, self.z, self.mu, self.w, self._t2_dev, self.s)
        return self._slot_pp(idx_s) if self.variant == 'svrg' else 0

    def _at_outer(self):
        """Whether the engine stands at the start of an outer iteration."""
        return self.s % self.T2 == 0 and self.n_prox == self.s

    def run_span(self, n):
        """n inner iterations from any step count.  With a per-problem T2, `outer_kernel_ok()` and lr_decay == 1 they run in
        launches of at most `span` steps -- one draw launch plus one pnp_csmri_svrg_span_pp each, in which the workgroup that owns
        a problem runs its steps back to back and refreshes where its own T2 says -- the same bits as stepping; otherwise eager
        steps."""
        # (pnp_csmri_svrg_span_pp holds the per-column prox only: TVProx(in_kernel=True) steps eagerly here)
        if not (self._t2_dev is not None and self.lr_decay == 1.0 and self.outer_kernel_ok() and not _in_kernel_2d(self.prox)):
            return self._run_steps(n)
        b, px = self.b, self.prox
        while n > 0:
            m = min(n, self.span)
            self._draw_span(m)
            b.plan.svrg_span(self.z, self.w, self.mu, b.bits, b.yh_full, b.inv_m0, self.mbs.selbits, self.s, m, self._t2_dev,
                             self._c('lr', 0, self.eta), self._mb_draw, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig,
                             sigma_modifier=px.sigma_modifier)
            self._launched(m, m)
            n -= m

    def _inner(self, j, lr, k, sse_out):
        """Inner iteration j of the current outer iteration: step size lr, decay exponent k (what the per-problem coefficient
        vectors are remade on), squared errors to sse_out.  Returns the tensor that holds the new iterate."""
        if self.fused:
            # folded refresh: at j = 0 the SVRG difference gs(z) - gs(w) is exactly zero (w == z), so that iteration is
            # z <- prox(z - lr * mu); ONE kernel forms mu, stores it and w, and goes on
            if j == 0 and self.fold_outer and self._t2_dev is None:     # (per-problem T2: j is a draw slot; refresh_pp came first)
                self._fused_outer(lr, sse_out, k)
            else:
                self._fused_inner(j, lr, sse_out, k)
            return self.z
        if self.variant == 'svrg':
            self.b.grad_stoch_diff(self.z, self.w, self.mbs, j, out=self.z, alpha=self._c('-lr/mb', k, -lr / self.mb), beta=1.0,
                                   c1=self.z, gamma=self._c('-lr', k, -lr), c2=self.mu, **self._diff_kw)
        else:
            self._step_along_mu(lr, k)
        return self.prox(self.z, self.b.xrec, sse_out)

    def _step_along_mu(self, lr, k):
        """variant='reference': z <- z - lr * mu, one launch: per-problem step sizes go in as the uploaded -lr vector
        (pnp_axpbypcz_pp), a scalar as itself (pnp_axpbypcz)."""
        ops.axpbypcz(1.0, self.z, self._c('-lr', k, -lr), self.mu, out=self.z)

    def _fused_outer(self, lr, sse_out, k):
        """outer refresh (mu = grad_full(z), w = z) + inner iteration 0 in one kernel (pnp_csmri_svrg_outer_step)."""
        b = self.b
        self._fused_call(b.plan.svrg_outer_step, (self.z, b.bits, b.yh_full, b.inv_m0, self._c('lr', k, lr), self.w, self.mu), self.z, sse_out)

    def _fused_inner(self, j, lr, sse_out, k):
        """step + estimate_sigma + prox + error of inner iteration j in one kernel (TV), or in one kernel + the network."""
        self._fused_call(self.b.plan.svrg_step, (self.z, self.w, self._slot_bits(j)), self.z, sse_out,
                         alpha=self._c('-lr/mb', k, -lr / self.mb), beta=1.0, c1=self.z, gamma=self._c('-lr', k, -lr), c2=self.mu)

    # ---- hipGraph form: one OUTER iteration (full-gradient refresh + T2 inner iterations) = one graph launch
    def _outer_body(self):
        b = self.b
        if not (self.fused and self.fold_outer):
            b.grad_full(self.z, out=self.mu)
            self.w.copy_(self.z)
        if self.variant == 'svrg':
            b.draw(self.mbs, self._mb_draw, self.seed, 0, self.T2, step_dev=self.step_dev, **self._draw_kw)
        for j in range(self.T2):
            if self._inner(j, self.eta, 0, self.sse_tmp) is not self.z:      # (graph_ok: lr_decay == 1)
                raise ValueError('graph capture needs an in-place prox')
            ops.log_append(self.sse_tmp, self.sse_log, self.step_dev)
            ops.counter_add(self.step_dev, 1)

    def graph_ok(self):
        """Whether one outer iteration of this engine can be captured: constant step size, a prox that works in place and keeps
        no host-side per-call state (TVProx with denoise_strength == 0, DnCNNProx; not NLMProx, which ping-pongs).  Never with a
        per-problem T2: the problems' outer iterations have no common period short of the lcm of their T2."""
        return (self._t2_dev is None and self.lr_decay == 1.0 and getattr(self.prox, 'inplace', False)
                and getattr(self.prox, 'denoise_strength', 0.0) == 0.0 and not self.log_objective)

    def capture(self):
        """Capture one outer iteration into a hipGraph (torch.cuda.CUDAGraph on ROCm).  Needs `graph_ok()`, a step count that
        is a multiple of T2 and device-side minibatch draws.  State is left untouched, also when the capture fails."""
        if not self.graph_ok():
            raise ValueError('this engine cannot be captured in a hipGraph (needs lr_decay == 1 and an in-place prox without '
                             'host-side per-call state: TVProx with denoise_strength == 0 or DnCNNProx); step it eagerly')
        if not self._at_outer():
            raise ValueError('capture() needs a step count that is a multiple of T2')
        self._set_dev_step(self.s)
        state = (self.z, self.w, self.mu, self.sse_log, self.step_dev)
        try:
            g = self._capture_graph(self._outer_body, state)
        finally:
            self.z = state[0]
        self.graph = g
        return g

    def _set_dev_step(self, s):
        """The device-resident counter is brought up to date only when a graph is about to read it."""
        if self._dev_step != s:
            self.step_dev.fill_(s)
            self._dev_step = s

    def outer_kernel_ok(self):
        """Whether whole outer iterations can run as ONE launch each (pnp_csmri_svrg_outer_iteration): the one-kernel iteration
        with the prox inside it (TV, no host-side per-call state), the outer refresh folded in, device-drawn minibatches."""
        return (self.fused and self.fold_outer and self.variant == 'svrg' and getattr(self.prox, 'fused_denoise', False)
                and getattr(self.prox, 'denoise_strength', 0.0) == 0.0 and all(h is None for h in self.mbs.host)
                and not self.log_objective)

    def run_outer(self, n_outer=1, one_launch=None):
        """n_outer outer iterations = n_outer * T2 inner iterations, from a step count that is a multiple of T2.
        one_launch (default: when `outer_kernel_ok()`): every outer iteration is ONE draw launch + ONE kernel in which the
        workgroup that owns a problem runs its T2 inner iterations back to back -- the same bits as stepping; otherwise
        replays of the captured hipGraph."""
        if self._t2_dev is not None:
            raise ValueError('run_outer: with a per-problem T2 the batch has no common outer iteration; use run_span(n_steps)')
        if one_launch is None:
            one_launch = self.outer_kernel_ok()
        if one_launch:
            if not (self.outer_kernel_ok() and self._at_outer()):
                raise ValueError('one launch per outer iteration needs the one-kernel iteration with the TV prox, the folded '
                                 'refresh, device-drawn minibatches and a step count that is a multiple of T2')
            b, px = self.b, self.prox
            for _ in range(n_outer):
                b.draw(self.mbs, self._mb_draw, self.seed, self.s, self.T2, **self._draw_kw)
                lr = self.eta * self.lr_decay ** (self.s // self.T2)
                b.plan.svrg_outer_iteration(self.z, self.w, self.mu, b.bits, b.yh_full, b.inv_m0, self.mbs.selbits, self.T2,
                                            self._c('lr', self.s // self.T2, lr), self._mb_draw, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig, sigma_modifier=px.sigma_modifier,
                                            prox_kind=_fused_kind(px))
                self._launched(self.T2, self.T2)
            return
        if self.graph is None:
            self.capture()
        self._set_dev_step(self.s)
        for _ in range(n_outer):
            self.graph.replay()
            self._launched(self.T2, self.T2)
        self._dev_step = self.s


class SarahEngine(_T2PerProblem, _StochEngine):
    """pnp_sarah over a batch (algorithms/pnp_sarah.py:28-104) with the quirks of v1: the outer step
    `w_next = prox(w_prev - eta * grad_full(z))` is logged but never adopted by z, w_next stays fixed through the
    inner loop, and the outer step ignores lr_decay.  One log row per prox: outer rows at s % T2 == 0.
    eta, mini_batch_size: scalars, or [B] arrays on a batch that takes them per problem; draw_id as in SgdEngine.
    fused=True (opt-in): the one-kernel forms -- the outer step is ONE pnp_csmri_svrg_outer_step (w_prev, v_prev and
    w_next are its three outputs), an inner iteration ONE pnp_csmri_sarah_step that updates v_prev, z and w_prev where they lie.
    Needs a float32 256 x 256 CsmriBatch, a TV or DnCNN prox and log_objective=False; `capture()` / `run_outer(n)` then replay
    one outer iteration (T2 + 1 log rows) as a hipGraph.
    T2: an int, or -- with split_log=True (opt-in) -- a [B] integer array on a batch that takes per-problem values:
    problem b then takes its outer step at the steps with s % T2[b] == 0 and walks, bit for bit, the trajectory a scalar engine with
    T2[b] walks on the same path.  The log is split: `sse_log` row s % n_log holds inner iteration s of every problem (n_prox == s),
    a second ring `outer_log` holds in the same row the squared error of the outer prox a problem made at step s, NaN elsewhere
    (`outer_trace()`, `psnr_trace_of(b)`).  At a step where any problem refreshes `step()` makes the outer step for the WHOLE batch
    into scratch buffers and adopts it per problem with one pnp_refresh_pp and one pnp_select_pp launch; `run_span(n)` runs n steps in
    launches of pnp_csmri_sarah_span_pp where `outer_kernel_ok()` holds and lr_decay == 1.  `span` is the draw window as in
    SvrgEngine.  There is no hipGraph form, no objective log, and no prox whose result depends on its call count.
    one_pass=True (opt-in): on a uniform DeblurBatch v_next = v_prev + (gs(w_next) - gs(w_prev)) / mb is ONE
    pnp_deblur_grad_step (not the default's bits); ValueError on any other batch and with fused=True."""

    def __init__(self, batch, prox, eta, T2, mini_batch_size, lr_decay=1.0, n_log=4096, seed=0, draw_id=None, log_objective=False,
                 *, fused=False, split_log=False, span=None, one_pass=False):
        self.one_pass = bool(one_pass)
        if self.one_pass:
            _check_one_pass('SarahEngine', batch, fused)
        self._diff_kw = dict(one_pass=True) if self.one_pass else {}      # (off: grad_stoch_diff gets the arguments it always got)
        if np.ndim(T2) != 0:
            if not split_log:
                raise ValueError('SarahEngine takes a scalar T2 (its outer prox logs a row of its own: rows would stop lining up) '
                                 'unless split_log=True gives the outer rows a ring of their own')
        elif split_log:
            raise ValueError('split_log=True is the log layout of a per-problem T2 ([B] integers); a scalar T2 keeps the single log')
        elif span is not None:
            raise ValueError('span is the draw window of a per-problem T2; a scalar T2 draws a window of AHEAD steps (an outer '
                             'iteration with fused=True)')
        pp = self._init_t2(batch, T2, span)
        if pp:
            if log_objective:
                raise ValueError('SarahEngine with a per-problem T2 does not log the objective (log_objective=True): the objective '
                                 'ring is laid out row for row with the single log of a scalar T2')
            if getattr(prox, 'denoise_strength', 0.0) != 0.0 and getattr(prox, 'decay', 1.0) != 1.0:
                raise ValueError('SarahEngine with a per-problem T2 needs a prox whose result does not depend on its call count '
                                 '(denoise_strength != 0 with decay != 1 does): the problems would have made different numbers of '
                                 'prox calls')
        self.fused = bool(fused)
        if self.fused:
            _check_fused('SarahEngine', batch, prox, log_objective)
        # fused: the draws of a whole outer iteration are ONE launch at the outer step (T2 selector slots, as SvrgEngine)
        super().__init__(batch, prox, eta, mini_batch_size, lr_decay, n_log, seed,
                         n_slots=self.span if pp else T2 if self.fused else None, draw_id=draw_id, log_objective=log_objective)
        self.w_prev = torch.empty_like(self.z)
        self.w_next = torch.empty_like(self.z)
        self.v_prev = torch.empty_like(self.z)
        self.outer_log = None
        if pp:
            # per-problem T2: the second ring, and the scratch of the whole-batch outer step (the full gradient, the stepped image
            # the prox runs on, the kernel's w_out with fused=True, the row of its squared errors)
            dev = batch.xrec.device
            self.outer_log = torch.full((n_log, batch.B), float('nan'), dtype=torch.float64, device=dev)
            self._outer_dirty = np.zeros(n_log, bool)           # rows of outer_log that hold a value of some problem
            self._v_new = torch.empty_like(self.z)
            self._tmp = torch.empty_like(self.z)
            self._w_scr = torch.empty_like(self.z) if self.fused else None
            self.sse_tmp = torch.zeros(batch.B, dtype=torch.float64, device=dev)
        if not self.fused:
            self.v_next = torch.empty_like(self.z)
            return
        dev = batch.xrec.device
        # the hipGraph form's device-resident counters and scratch row (as SvrgEngine's).  Two counters: the draws are keyed on the
        # step count, the log on the row count -- an outer iteration appends T2 + 1 rows (log_append_inc: append and count, one launch)
        self.row_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._dev_step = 0
        self.sse_tmp = torch.zeros(batch.B, dtype=torch.float64, device=dev)

    def reset(self):
        super().reset()
        if self.fused:
            self.row_dev.zero_()
            self.step_dev.zero_()
            self._dev_step = 0
        if self._t2_dev is not None:
            self.outer_log.fill_(float('nan'))
            self._outer_dirty[:] = False
            self._drawn_base = None

    def step(self, idx_s=None):
        if self._t2_dev is not None:
            return self._step_pp(idx_s)
        if self.fused:
            return self._step_fused(idx_s)
        b, s = self.b, self.s
        if s % self.T2 == 0:
            self.w_prev.copy_(self.z)
            b.grad_full(self.z, out=self.v_prev)
            # (F6: no lr_decay here -- '-eta' is a coefficient of its own, made once whatever the decay exponent)
            ops.axpbypcz(1.0, self.w_prev, self._c('-eta', 0, -self.eta), self.v_prev, out=self.w_next)
            self.w_next = self._prox(self.w_next)
        k = s // self.T2
        self._inner(self._minibatch(idx_s, s), self.eta * self.lr_decay ** k, k)

    def _inner(self, j, lr, k):
        """The inner iteration on slot j (step size lr, decay exponent k), logged in the next row of sse_log: ONE pnp_csmri_sarah_step,
        or the difference of minibatch gradients, the step, the prox, the buffer swap and the copy w_prev <- z."""
        if self.fused:
            self._fused_inner(j, lr, k, self.sse_log[self.n_prox % self.n_log])
            self.n_prox += 1
        else:
            self.b.grad_stoch_diff(self.w_next, self.w_prev, self.mbs, j, out=self.v_next, alpha=self._c('1/mb', 0, 1.0 / self.mb),
                                   beta=1.0, c1=self.v_prev, **self._diff_kw)
            ops.axpbypcz(1.0, self.z, self._c('-lr', k, -lr), self.v_next, out=self.z)
            self.z = self._prox(self.z)
            self.v_prev, self.v_next = self.v_next, self.v_prev
            self.w_prev.copy_(self.z)
        self.s += 1

    def _at_outer(self):
        """Whether the engine stands at the start of an outer iteration: a multiple of T2 steps, each outer iteration T2 + 1 rows."""
        return self.s % self.T2 == 0 and self.n_prox == self.s + self.s // self.T2

    # ---- per-problem T2 (split_log=True)
    def _outer_row(self, s, refresh):
        """Row s % n_log of outer_log for step s.  Where some problem refreshes, pnp_select_pp (or the span kernel) writes the whole
        row, NaN included; where none does nothing is launched -- unless the ring has wrapped onto a row that holds values."""
        r = s % self.n_log
        if not refresh and self._outer_dirty[r]:
            self.outer_log[r].fill_(float('nan'))
        self._outer_dirty[r] = refresh
        return self.outer_log[r]

    def _step_pp(self, idx_s):
        """`step()` with a per-problem T2.  Where any problem refreshes: the outer step of the whole batch into scratch (streaming:
        grad_full, the axpbypcz of the scalar engine, the prox; fused: ONE pnp_csmri_svrg_outer_step), then ONE pnp_refresh_pp
        (v_prev, w_prev) and ONE pnp_select_pp (w_next and the outer log row) adopt it for the refreshing problems alone.  Then the
        ordinary inner iteration for all problems.  The whole batch pays that gradient and prox; only the refreshing problems keep
        them."""
        b, px, s = self.b, self.prox, self.s
        refresh = self.refreshes(s)
        row = self._outer_row(s, refresh)
        if refresh:
            if self.fused:
                res = self._fused_outer(self._w_scr, self._v_new, self._tmp, self.sse_tmp)
            else:
                b.grad_full(self.z, out=self._v_new)
            ops.refresh_pp(self._v_new, self.z, self.v_prev, self.w_prev, self._t2_dev, s)
            if not self.fused:
                # (F6: no lr_decay here -- '-eta' is made once; for a refreshing problem z, v_new ARE its w_prev, v_prev)
                ops.axpbypcz(1.0, self.z, self._c('-eta', 0, -self.eta), self._v_new, out=self._tmp)
                res = px(self._tmp, b.xrec, self.sse_tmp)
            ops.select_pp(res, self.w_next, self._t2_dev, s, self.sse_tmp, row)
            self._tmp = res                                     # (a prox that ping-pongs hands back the buffer that is free now)
        self._inner(self._slot_pp(idx_s), *self._lr_pp(s))      # (n_prox == s: the inner row of step s is row s % n_log)

    def run_span(self, n):
        """n inner iterations from any step count.  With a per-problem T2, `outer_kernel_ok()` and lr_decay == 1 they run in
        launches of at most `span` steps -- one draw launch plus one pnp_csmri_sarah_span_pp each, in which the workgroup that owns
        a problem runs its steps back to back and takes its outer step where its own T2 says -- the same bits as stepping;
        otherwise eager steps (TVProx(in_kernel=True) among them: the span kernel holds the per-column prox only)."""
        if not (self._t2_dev is not None and self.lr_decay == 1.0 and self.outer_kernel_ok()):
            return self._run_steps(n)
        b, px = self.b, self.prox
        while n > 0:
            m = min(n, self.span)
            self._draw_span(m)
            eta = self._c('eta', 0, self.eta)                   # (lr_decay == 1: the inner step size is eta as well)
            b.plan.sarah_span(self.z, self.w_prev, self.w_next, self.v_prev, b.bits, b.yh_full, b.inv_m0, self.mbs.selbits, self.s, m,
                              self._t2_dev, eta, eta, self._mb_draw, b.xrec, self.sse_log, self.outer_log, self.s % self.n_log, px.sig,
                              sigma_modifier=px.sigma_modifier)
            for s in range(self.s, self.s + m):                 # (the kernel writes every row it passes, NaN included)
                self._outer_dirty[s % self.n_log] = self.refreshes(s)
            self._launched(m, m)
            n -= m

    def _split_rows(self, log):
        if self._t2_dev is None:
            raise ValueError('the split log is the layout of a per-problem T2 (SarahEngine(T2=[B] ints, split_log=True))')
        return self._psnr(log)

    def outer_trace(self):
        """Per-problem T2: [steps][B] PSNR of the outer prox problem b made at each step, NaN where it made none; the rows are
        those of `psnr_trace()` (the inner iterations)."""
        return self._split_rows(self.outer_log)

    def psnr_trace_of(self, b):
        """Per-problem T2: problem b's rows in the order a scalar SarahEngine with T2[b] logs them -- at each step the outer row if
        the problem made an outer step there, then the inner row -- i.e. `psnr_trace()[:, 0]` of that engine on this problem."""
        inner, outer = self._split_rows(self.sse_log)[:, b], self._split_rows(self.outer_log)[:, b]
        rows = []
        for o, i in zip(outer, inner):
            if not np.isnan(o):
                rows.append(o)
            rows.append(i)
        return np.array(rows, inner.dtype)

    # ---- the one-kernel forms (fused=True)
    def _step_fused(self, idx_s):
        b, s = self.b, self.s
        j, k = s % self.T2, s // self.T2
        if j == 0:
            if idx_s is None:
                b.draw(self.mbs, self._mb_draw, self.seed, s, self.T2, **self._draw_kw)
            self._fused_outer(self.w_prev, self.v_prev, self.w_next, self.sse_log[self.n_prox % self.n_log])
            self.n_prox += 1
        if idx_s is not None:
            b.set_host(self.mbs, j, idx_s)
        elif self.mbs.host[j] is not None:                      # a host-fed outer iteration continued with device draws
            self._draw_slot(j, s)
        self._inner(j, self.eta * self.lr_decay ** k, k)

    def _fused_outer(self, w_out, v_out, out, sse_out):
        """w_out = z, v_out = grad_full(z), out = prox(z - eta * v_out) in one kernel (pnp_csmri_svrg_outer_step): the outer step into
        w_prev, v_prev and w_next, or into scratch (per-problem T2).  z is not touched (the outer step is logged, never adopted),
        and eta does not decay here (F6).  -> out"""
        b = self.b
        self._fused_call(b.plan.svrg_outer_step, (self.z, b.bits, b.yh_full, b.inv_m0, self._c('eta', 0, self.eta), w_out, v_out), out, sse_out)
        return out

    def _fused_inner(self, j, lr, k, sse_out):
        """v_prev <- v_next, z <- prox(z - lr * v_next), w_prev <- z in one kernel (pnp_csmri_sarah_step), all three in place; with
        a prox that follows the kernel (DnCNN, the 2-D wavelet prox) the copy to w_prev follows the prox."""
        den = self.prox.fused_denoise
        self._fused_call(self.b.plan.sarah_step, (self.w_next, self.w_prev, self._slot_bits(j)), self.z, sse_out,
                         alpha=self._c('1/mb', 0, 1.0 / self.mb), beta=1.0, c1=self.v_prev, gamma=self._c('-lr', k, -lr), c2=self.z,
                         v_out=self.v_prev, out2=self.w_prev if den else None)
        if not den:
            self.w_prev.copy_(self.z)

    # ---- hipGraph form of the fused path: one OUTER iteration (outer step + T2 inner iterations, T2 + 1 log rows) = one graph launch
    def _outer_body(self):
        b = self.b
        self._fused_outer(self.w_prev, self.v_prev, self.w_next, self.sse_tmp)
        ops.log_append_inc(self.sse_tmp, self.sse_log, self.row_dev)
        b.draw(self.mbs, self._mb_draw, self.seed, 0, self.T2, step_dev=self.step_dev, **self._draw_kw)
        for j in range(self.T2):
            self._fused_inner(j, self.eta, 0, self.sse_tmp)     # (graph_ok: lr_decay == 1)
            ops.log_append_inc(self.sse_tmp, self.sse_log, self.row_dev)
            ops.counter_add(self.step_dev, 1)

    def graph_ok(self):
        """Whether one outer iteration of this engine can be captured: the fused path (the streaming path swaps buffers and may get
        fresh tensors from its prox), constant step size, an in-place prox without host-side per-call state, device draws."""
        return (self._t2_dev is None and self.fused and self.lr_decay == 1.0 and getattr(self.prox, 'inplace', False)
                and getattr(self.prox, 'denoise_strength', 0.0) == 0.0 and not self.log_objective
                and all(h is None for h in self.mbs.host))

    def capture(self):
        """Capture one outer iteration into a hipGraph.  Needs `graph_ok()` and a step count that is a multiple of T2.  State is left
        untouched, also when the capture fails."""
        if self._t2_dev is not None:
            raise ValueError('capture: with a per-problem T2 the batch has no common outer iteration to capture in a hipGraph; use '
                             'run_span(n_steps)')
        if not self.graph_ok():
            raise ValueError('this SarahEngine cannot be captured in a hipGraph (needs fused=True, lr_decay == 1, device-drawn '
                             'minibatches and an in-place prox without host-side per-call state: TVProx with denoise_strength == 0 '
                             'or DnCNNProx); step it eagerly')
        if not self._at_outer():
            raise ValueError('capture() needs a step count that is a multiple of T2')
        self._set_dev_step()
        g = self._capture_graph(self._outer_body, (self.z, self.w_prev, self.w_next, self.v_prev, self.sse_log, self.row_dev, self.step_dev))
        self.graph = g
        return g

    def _set_dev_step(self):
        """The device-resident counters are brought up to date only when a graph is about to read them."""
        if self._dev_step != self.s:
            self.step_dev.fill_(self.s)
            self.row_dev.fill_(self.n_prox % self.n_log)
            self._dev_step = self.s

    def outer_kernel_ok(self):
        """Whether whole outer iterations can run as ONE launch each (pnp_csmri_sarah_outer_iteration): the one-kernel forms with the
        prox inside the kernel (TV, no host-side per-call state), device-drawn minibatches, no objective log."""
        return not self._outer_kernel_missing()

    def _outer_kernel_missing(self):
        missing = []
        if not self.fused:
            missing.append('fused=True')
        if not getattr(self.prox, 'fused_denoise', False):
            missing.append(f'a prox that runs inside the kernel: TVProx (got {type(self.prox).__name__})')
        elif _in_kernel_2d(self.prox):
            missing.append('the per-column TV prox (pnp_csmri_sarah_outer_iteration does not hold the 2-D prox of in_kernel=True)')
        elif getattr(self.prox, 'denoise_strength', 0.0) != 0.0:
            missing.append('denoise_strength == 0')
        if not all(h is None for h in self.mbs.host):
            missing.append('device-drawn minibatches (a slot holds a host-fed one)')
        if self.log_objective:
            missing.append('log_objective=False')
        return missing

    def run_outer(self, n_outer=1, one_launch=False):
        """n_outer outer iterations = n_outer * T2 inner iterations (n_outer * (T2 + 1) log rows), from a step count that is a
        multiple of T2 -- the same bits as stepping.  Default: replays of the captured hipGraph.  one_launch=True (opt-in, needs
        `outer_kernel_ok()`): every outer iteration is ONE draw launch + ONE pnp_csmri_sarah_outer_iteration, in which the
        workgroup that owns a problem runs the outer step (eta, no decay: F6) and its T2 inner iterations (eta * lr_decay ** k) back
        to back."""
        if self._t2_dev is not None:
            raise ValueError('run_outer: with a per-problem T2 the batch has no common outer iteration; use run_span(n_steps)')
        if one_launch:
            missing = self._outer_kernel_missing()
            if not self._at_outer():
                missing.append(f'a step count that is a multiple of T2 (s = {self.s}, T2 = {self.T2})')
            if missing:
                raise ValueError('run_outer(one_launch=True) needs ' + ', '.join(missing))
            b, px = self.b, self.prox
            for _ in range(n_outer):
                k = self.s // self.T2
                b.draw(self.mbs, self._mb_draw, self.seed, self.s, self.T2, **self._draw_kw)
                lr = self.eta * self.lr_decay ** k
                b.plan.sarah_outer_iteration(self.z, self.w_prev, self.w_next, self.v_prev, b.bits, b.yh_full, b.inv_m0,
                                             self.mbs.selbits, self.T2, self._c('eta', 0, self.eta), self._c('lr', k, lr),
                                             self._mb_draw, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig,
                                             sigma_modifier=px.sigma_modifier)
                self._launched(self.T2, self.T2 + 1)
            return
        if self.graph is None:
            self.capture()
        if not self._at_outer():
            raise ValueError('run_outer() needs a step count that is a multiple of T2')
        self._set_dev_step()
        for _ in range(n_outer):
            self.graph.replay()
            self._launched(self.T2, self.T2 + 1)
        self._dev_step = self.s


def saga_row_rng(seed):
    """The generator a SagaEngine made with `seed` draws its table rows from, one `integers(hist_size)` per step (also what
    `sweep.make_runner(mixed_scales=True)` hands each item: the rows of the engine of its default group)."""
    return np.random.default_rng(seed + 977)


class SagaEngine(_FusedStep, _StochEngine):
    """pnp_saga over a batch (algorithms/pnp_saga.py:25-72): a device table [hist][B][H][W] of minibatch
    gradients (all rows start as the first one), its running sum, and ONE fused kernel per step that replaces a
    row, updates the sum, forms v = g - prev + sum/hist and applies the step (`pnp_saga_table_update`).
    The replaced row r of every step is drawn on the host (one value per step for the whole batch; pass `r=` to
    `step` to impose the reference's `np.random.choice(hist_size, 1)` stream).
    fused=True (opt-in): a step is ONE pnp_csmri_saga_step -- minibatch gradient, table update, step and prox; the rows
    always go in as the int32 [B] device vectors of the batched update.  The table initialisation is the streaming one.
    hist_size: an int, or a [B] integer array on a batch that takes per-problem values: problem b then walks, bit for bit,
    the trajectory a scalar engine with hist_size[b] walks on the same seed, draw_id, minibatches and rows.  The table is dense,
    [max(hist_size)][B][H][W], and problem b only ever touches its rows [0, hist_size[b]); its running sum starts at hist_size[b] * g
    and is divided by hist_size[b] (`pnp_saga_table_update_hist_pp`, `pnp_csmri_saga_step_hist_pp`, `pnp_csmri_saga_span_hist`: every
    step is one batched launch).  With r=None the rows come from one generator per DISTINCT value h of the vector, each the scalar
    engine's `default_rng(seed + 977)` drawing `integers(h)` once per step: problem b takes the draw of the generator of its own
    value, which is what a scalar engine with hist_size = h draws."""

    def __init__(self, batch, prox, eta, mini_batch_size, hist_size=50, lr_decay=1.0, n_log=4096, seed=0, idx0=None, draw_id=None,
                 log_objective=False, *, fused=False):
        self.fused = bool(fused)
        if self.fused:
            _check_fused('SagaEngine', batch, prox, log_objective)
        hv = None
        if np.ndim(hist_size) != 0:                             # per-problem hist_size: checked on the host (the kernels cannot)
            if self.fused and _in_kernel_2d(prox):
                raise ValueError('SagaEngine(fused=True) with a per-problem hist_size: pnp_csmri_saga_step_hist_pp holds the per-column '
                                 'prox only -- use TVProx(multi=False) without in_kernel=True (the 2-D prox then follows the kernel)')
            hv = _int_vector(batch, 'hist_size', hist_size)
        self._row_cache = {}                                    # fused: one row for the whole batch -> its device vector, made once
        super().__init__(batch, prox, eta, mini_batch_size, lr_decay, n_log, seed, draw_id=draw_id, log_objective=log_objective)
        self.hist = hist_size if hv is None else int(hv.max())  # the table's row count
        self.hist_pp = hv                                       # per-problem history lengths (None: one for the batch)
        self.g = torch.empty_like(self.z)
        self._rng = saga_row_rng(seed)
        self._inv_hist_pp = None
        if hv is not None:                                      # one row stream per distinct value, each the scalar engine's
            self._rngs = {int(h): saga_row_rng(seed) for h in np.unique(hv)}
            # the divisors as the scalar path forms them (1.0 / hist_size in Python floats), uploaded once
            self._inv_hist_pp = torch.from_numpy(np.array([1.0 / int(h) for h in hv], np.float64)).to(self.z.device)
        self._rows = None                                       # (host rows, their int32 device vector) of the last batched update
        # pnp_saga.py:25-31: one minibatch gradient at Xinit fills the whole table
        j = self._minibatch(idx0, 0xFFFFFFFF)
        batch.grad_stoch(self.z, self.mbs, j, out=self.g, alpha=self._c('1/mb', 0, 1.0 / self.mb))
        if hv is None:
            self.table = self.g.unsqueeze(0).repeat(hist_size, 1, 1, 1).contiguous()
            self.tsum = ops.axpbypcz(float(hist_size), self.g, out=torch.empty_like(self.g))
        else:                                                   # dense over max(hist_size); tsum[b] = float(hist_size[b]) * g[b]
            self.table = self.g.unsqueeze(0).repeat(self.hist, 1, 1, 1).contiguous()
            self.tsum = ops.axpbypcz(torch.from_numpy(hv.astype(np.float64)).to(self.z.device), self.g, out=torch.empty_like(self.g))
        self.r_prev = 0

    def reset(self):
        raise NotImplementedError('build a new SagaEngine (the table initialisation is part of the constructor)')

    def _row_vec(self, r):
        """Table rows (one for the batch, or one per problem) as the int32 [B] device vector of the batched update; the vector of
        the previous step's rows is the one that step made."""
        if self._rows is not None and r is self._rows[0]:
            return self._rows[1]
        if self.fused and np.ndim(r) == 0:
            if int(r) not in self._row_cache:
                self._row_cache[int(r)] = torch.full((self.b.B,), int(r), dtype=torch.int32, device=self.z.device)
            return self._row_cache[int(r)]
        rv = np.ascontiguousarray(np.broadcast_to(np.asarray(r, np.int32), (self.b.B,)))
        return torch.from_numpy(rv).to(self.z.device)

    def _draw_rows_pp(self, n):
        """Per-problem hist_size: the rows of the next n steps, int64 [n][B] -- per step one draw from the generator of every distinct
        value, problem b taking that of its own."""
        draws = {h: [int(g.integers(h)) for _ in range(n)] for h, g in self._rngs.items()}
        return np.array([draws[int(h)] for h in self.hist_pp], np.int64).T.reshape(n, self.b.B)

    def _check_rows(self, r, bound):
        """Rows against the bound [0, bound) -- `hist`: r as it is, one message for the batch; `hist_pp`: r (a scalar, [B], or
        [n][B]) as int64 over the problems, each against its own bound, the first offender named.  -> r"""
        if np.ndim(bound) == 0:
            if (not 0 <= r < bound) if np.ndim(r) == 0 else (r.min() < 0 or r.max() >= bound):
                raise ValueError(f'SAGA row outside the table: rows in [0, {bound}), got {np.ravel(r).tolist()}')
            return r
        r = np.broadcast_to(np.asarray(r, np.int64), np.shape(r)[:-1] + (self.b.B,) if np.ndim(r) else (self.b.B,)).copy()
        bad = np.argwhere((r < 0) | (r >= bound))
        if bad.size:
            b = int(bad[0][-1])
            raise ValueError(f'SAGA row outside the table of problem {b}: rows in [0, {int(bound[b])}), got {int(r[tuple(bad[0])])}')
        return r

    def step(self, idx_s=None, r=None):
        """r: the table row this step replaces -- one value for the whole batch, or one per problem (legacy-seeded sweeps:
        every item follows its own np.random stream, and with masks of different sizes the streams drift apart)."""
        j = self._minibatch(idx_s, self.s)
        if r is None:
            r = self._draw_rows_pp(1)[0] if self.hist_pp is not None else int(self._rng.integers(self.hist))
        if self.fused or self.hist_pp is not None:
            return self._step_batched(j, r)
        self.b.grad_stoch(self.z, self.mbs, j, out=self.g, alpha=self._c('1/mb', 0, 1.0 / self.mb))
        lr = self.eta * self.lr_decay ** self.s
        if np.ndim(r) == 0 and np.ndim(self.r_prev) == 0 and np.ndim(lr) == 0:
            r = int(r)
            ops.saga_table_update(self.z, self.g, self.table[r], self.table[self.r_prev], self.tsum, lr, 1.0 / self.hist)
        else:                                                   # per-problem rows or step sizes: ONE launch for the batch
            r = self._check_rows(np.broadcast_to(np.asarray(r, np.int64), (self.b.B,)).copy(), self.hist)
            prev = self._row_vec(self.r_prev)
            self._rows = (r, self._row_vec(r))
            ops.saga_table_update_pp(self.z, self.g, self.table, self._rows[1], prev, self.tsum, self._c('lr', self.s, lr),
                                     1.0 / self.hist)
        self.r_prev = r
        self.z = self._prox(self.z)
        self.s += 1

    def _step_batched(self, j, r):
        """`step()` in ONE kernel (fused=True) and with a per-problem hist_size: the rows checked, then ONE batched launch -- the
        one-kernel step with the rows and coefficients of the streaming step (a row for the whole batch as a constant [B] vector),
        or pnp_saga_table_update_hist_pp behind the minibatch gradient; a per-problem hist_size adds the divisor vector."""
        b, kw = self.b, {}
        if self.hist_pp is not None:
            r, kw = self._check_rows(r, self.hist_pp), dict(inv_hist_pp=self._inv_hist_pp)
        else:
            r = self._check_rows(int(r) if np.ndim(r) == 0 else np.broadcast_to(np.asarray(r, np.int64), (b.B,)).copy(), self.hist)
        prev, row = self._row_vec(self.r_prev), self._row_vec(r)
        if np.ndim(r) != 0:
            self._rows = (r, row)
        lr = self.eta * self.lr_decay ** self.s
        if self.fused:
            self._one_kernel(b.plan.saga_step, self.z, self._slot_bits(j), b.YT, self.table, row, prev, self.tsum,
                             self._c('lr', self.s, lr), 1.0 / self.hist, alpha=self._c('1/mb', 0, 1.0 / self.mb), **kw)
        else:
            b.grad_stoch(self.z, self.mbs, j, out=self.g, alpha=self._c('1/mb', 0, 1.0 / self.mb))
            ops.saga_table_update_pp(self.z, self.g, self.table, row, prev, self.tsum, self._c('lr', self.s, lr), 1.0 / self.hist, **kw)
            self.z = self._prox(self.z)
        self.r_prev = r
        self.s += 1

    def run_span(self, n, r=None):
        """n inner iterations.  r: the rows they replace -- None (n values from the engine's own stream, in the order `step()` takes
        them), [n] (one per step for the whole batch) or [n][B] (one per step and problem).  Where `span_kernel_ok()` holds they run
        in launches of at most AHEAD steps -- one draw of m steps from the absolute step id plus ONE pnp_csmri_saga_span each, in
        which the workgroup that owns a problem runs its steps back to back -- the same bits as stepping, with r_prev left as
        stepping leaves it; otherwise n eager steps."""
        if r is None:
            r = self._draw_rows_pp(n) if self.hist_pp is not None else [int(self._rng.integers(self.hist)) for _ in range(n)]
        r = np.asarray(r)
        if r.shape not in ((n,), (n, self.b.B)):
            raise ValueError(f'run_span: r holds one row per step ([{n}]) or per step and problem ([{n}][{self.b.B}]), got shape {r.shape}')
        if not self.span_kernel_ok():
            for i in range(n):
                self.step(r=r[i] if r.ndim == 2 else int(r[i]))
            return
        if n < 1:
            return
        b, px = self.b, self.prox
        kw = {}
        if self.hist_pp is not None:                            # every problem's own bound; the rows are then always [n][B]
            r, kw = self._check_rows(r.reshape(n, -1), self.hist_pp), dict(inv_hist_pp=self._inv_hist_pp)
        else:
            self._check_rows(r, self.hist)
        rows = np.ascontiguousarray(np.broadcast_to(r.reshape(n, -1), (n, b.B)), np.int32)
        rows_dev = torch.from_numpy(rows).to(self.z.device)
        prev, i0 = self._row_vec(self.r_prev), 0
        while i0 < n:
            m = min(n - i0, self.AHEAD)
            b.draw(self.mbs, self._mb_draw, self.seed, self.s, m, **self._draw_kw)
            self._drawn_base = None                             # (a later eager step redraws its own window)
            lr = self.eta * self.lr_decay ** self.s             # (span_kernel_ok: lr_decay == 1)
            b.plan.saga_span(self.z, self.mbs.selbits, b.YT, self.table, rows_dev[i0:i0 + m], prev, self.tsum, self._c('lr', self.s, lr),
                             1.0 / self.hist, m, b.xrec, self.sse_log, self.n_prox % self.n_log, px.sig,
                             alpha=self._c('1/mb', 0, 1.0 / self.mb), sigma_modifier=px.sigma_modifier, **kw)
            self._launched(m, m)
            i0 += m
            prev = rows_dev[i0 - 1]
        if r.ndim == 1:                                         # as the last step leaves them: a row for the whole batch ...
            self.r_prev = int(r[-1])
        else:                                                   # ... or the rows of its batched update with their device vector
            self.r_prev = r[-1].astype(np.int64)
            self._rows = (self.r_prev, rows_dev[n - 1])


def make_engine(batch, prox, eta, T2, mini_batch_size, lr_decay=1.0, variant='svrg', algorithm='svrg', hist_size=50, **kw):
    """Engine by algorithm name: 'svrg' (default), 'sgd', 'gd', 'sarah', 'saga'.  Keywords of the engine (`fused`, `seed`,
    `draw_id`, `log_objective`, ...) pass through."""
    if algorithm == 'svrg':
        return SvrgEngine(batch, prox, eta, T2, mini_batch_size, lr_decay=lr_decay, variant=variant, **kw)
    if algorithm == 'sarah':
        return SarahEngine(batch, prox, eta, T2, mini_batch_size, lr_decay=lr_decay, **kw)
    if algorithm == 'sgd':
        return SgdEngine(batch, prox, eta, mini_batch_size, lr_decay=lr_decay, **kw)
    if algorithm == 'saga':
        return SagaEngine(batch, prox, eta, mini_batch_size, hist_size=hist_size, lr_decay=lr_decay, **kw)
    if algorithm == 'gd':
        kw.pop('seed', None)
        kw.pop('draw_id', None)
        return GdEngine(batch, prox, eta, lr_decay=lr_decay, **kw)
    raise ValueError(f'unknown algorithm {algorithm!r}')
