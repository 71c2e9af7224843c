"""Batch problems: the device-resident data of B independent reconstructions, as the engines of `engine.py` step them.

A *batch problem* (CsmriBatch, DeblurBatch, PrBatch) holds the device-resident data of B problems and offers
    grad_full(z, out, alpha, beta, c1)                         alpha * grad_full(z) + beta * c1
    grad_stoch(z, mbs, j, out, alpha, beta, c1)                alpha * grad_stoch(z, minibatch j) + beta * c1
    grad_stoch_diff(z, w, mbs, j, out, alpha, beta, c1, gamma, c2)
                                                               alpha * (gs(z) - gs(w)) + beta * c1 + gamma * c2
    objective(z, out)                                          f(z) = ||Y - forward_model(z)||^2 / 2 / M per problem, float64 [B]
    minibatches(n) / draw(mbs, mb, seed, step0, nsteps) / set_host(mbs, j, idx)
Minibatches are drawn on the device by default (counter-based keys + a threshold per (problem, step): csrc/draw.h;
the selection itself is re-derived inside the gradient kernels and never stored); for reference-identical runs pass
index lists drawn from the legacy `np.random` stream (`step(idx)`).

Every class has ONE initialiser of its state, `_init`, which takes the plan and device tensors: the NumPy `__init__` uploads and
calls it, `generate` (data made on the device) and `tile` hand it their tensors through `_of`.
"""
import numpy as np
import torch

from . import ops


class Minibatches:
    """n slots of per-problem minibatch selections: threshold descriptors of device draws (mbd: int64 [n, B, 2]; CSMRI also
    selbits, the device-drawn selections themselves, bit-packed: what the column pass reads) or host-provided selections
    (slot -> whatever the batch problem's kernels take)."""

    def __init__(self, mbd, selbits=None):
        self.n, self.mbd, self.selbits = mbd.shape[0], mbd, selbits
        self.host = [None] * self.n

    @classmethod
    def zeros(cls, n, B, device, bits_shape=None):
        return cls(torch.zeros((n, B, 2), dtype=torch.int64, device=device),
                   torch.zeros((n, B) + tuple(bits_shape), dtype=torch.int32, device=device) if bits_shape else None)

    def slot(self, j):
        """Slot j alone, as a one-slot view of the same device rows (its host selection starts empty)."""
        return Minibatches(self.mbd[j:j + 1], None if self.selbits is None else self.selbits[j:j + 1])


class _BatchBase:
    per_problem = False                                         # whether the engines may hand this batch per-problem eta / mb / draw_id

    def _init_base(self, xrec, xinit, max_mb):
        """The state every batch has, from its device tensors: xrec, xinit [B, H, W]."""
        self.B, self.H, self.W = xrec.shape
        self.N, self.dtype, self.device = self.H * self.W, xrec.dtype, xrec.device
        self.xrec, self.xinit, self.max_mb = xrec, xinit, max_mb
        self._tmp = None                                        # gradient scratch, made on first use

    @classmethod
    def _of(cls, **state):
        """A batch from the device tensors of `_init` (the NumPy arguments of `__init__` stay empty)."""
        return cls(None, None, None, None, _state=state)

    @staticmethod
    def _upload(a, dtype, device, shape=None):
        t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device, dtype)
        return t if shape is None else t.reshape(shape)

    def minibatches(self, n):
        return Minibatches.zeros(n, self.B, self.device)

    def _check_mb(self, mb):
        if np.ndim(mb) != 0:                                    # per problem: every entry against its own problem's population
            mb = np.asarray(mb)
            cap = np.broadcast_to(np.asarray(getattr(self, 'M0', self.max_mb)), (self.B,))
            if mb.shape != (self.B,) or not np.issubdtype(mb.dtype, np.integer):
                raise ValueError(f'per-problem mini_batch_size: {self.B} integers, got shape {mb.shape} of {mb.dtype}')
            bad = np.flatnonzero((mb < 1) | (mb > cap))
            if bad.size:
                b = int(bad[0])
                raise ValueError(f"Cannot take a larger sample than population when 'replace=False' (problem {b}: mini_batch_size "
                                 f'{int(mb[b])}, population {int(cap[b])}; sizes must be >= 1)')
            return
        if mb > self.max_mb:
            # np.random.choice(..., replace=False) raises the same way (problems/problem.py:110-117, CSMRI.py:66-74)
            raise ValueError(f"Cannot take a larger sample than population when 'replace=False' (mini_batch_size {mb} > {self.max_mb})")

    @staticmethod
    def upload_images(images, H=256, W=256, dtype=torch.float32, device='cuda'):
        """The image set of `generate`, each image min-max normalised in float64 (sweep._norm01), as one [n, H, W] device tensor."""
        xs = []
        for img in images:
            x = np.asarray(img, np.float64)
            if x.shape != (H, W):
                raise ValueError(f'image of shape {x.shape}: generate needs {H} x {W} images')
            xs.append((x - x.min()) / (x.max() - x.min()))
        return torch.from_numpy(np.stack(xs)).to(device, dtype).contiguous()

    @classmethod
    def _generate_inputs(cls, images, items, H, W, dtype, device):
        """What every `generate` starts from: the image set on the device and the per-item [B] parameter vectors of the
        counter-based stream (image_idx int32, snr_fac float64, seed, id as int64 holding the 64-bit values)."""
        ops.require_gpu()
        if not isinstance(images, torch.Tensor):
            images = cls.upload_images(images, H, W, dtype, device)
        if images.dtype != dtype or tuple(images.shape[1:]) != (H, W):
            raise ValueError(f'image set of dtype {images.dtype}, shape {tuple(images.shape)}: generate needs [n, {H}, {W}] {dtype}')
        if len(items) < 1 or any(not 0 <= it['image'] < images.shape[0] for it in items):
            raise ValueError('generate needs at least one item and image indices inside the image set')
        u64 = lambda v: np.array([int(x) & (2 ** 64 - 1) for x in v], np.uint64).view(np.int64)
        par = [np.array([it['image'] for it in items], np.int32),
               np.array([10.0 ** (-np.float64(it['snr']) / 10) for it in items], np.float64),
               u64([it['seed'] for it in items]), u64([it['id'] for it in items])]
        return images, [torch.from_numpy(a).to(images.device) for a in par]

    def psnr_init(self):
        """rounded PSNR of Xinit per problem (problems/problem.py:33-35)."""
        sse = ops.sse(self.xinit, self.xrec).cpu().numpy()
        with np.errstate(divide='ignore'):
            return np.around(10 * np.log10(1.0 / (sse / self.N)), 2)

    # ---- what DeblurBatch and PrBatch share: gradients that cannot add c1, c2 themselves
    def _scratch(self, z):
        if self._tmp is None:
            self._tmp = torch.empty_like(z)
        return self._tmp

    def _combine(self, g, out, beta, c1, gamma=0.0, c2=None):
        """g + beta * c1 + gamma * c2 -> out, ONE launch.  With nothing to add, a gradient that was written to `out` is the result
        as it is.  A per-problem gamma (float64 [B] device tensor) goes to pnp_axpbypcz_pp as it is: per problem the scalar call
        with its value, bit for bit."""
        if c1 is None and c2 is None:
            return g if g is out else out.copy_(g)
        return ops.axpbypcz(1.0, g, beta, c1, gamma, c2, out=out)

    def _host(self, t, fn=None):
        """The host copy of a per-problem coefficient vector (a float64 [B] device tensor the engines upload once), or fn(host copy)
        uploaded again: read back once per tensor and kept while the engine keeps passing that very tensor."""
        hit = getattr(self, '_host_cache', None)
        if hit is None or hit[0] is not t:
            hit = self._host_cache = (t, t.cpu().numpy(), {})
        if fn is None:
            return hit[1]
        if fn not in hit[2]:
            hit[2][fn] = torch.from_numpy(np.ascontiguousarray(fn(hit[1]), np.float64)).to(t.device)
        return hit[2][fn]


class CsmriBatch(_BatchBase):
    """Device-resident data of B CSMRI problems (reference problems/CSMRI.py:12-41 per problem).  Masks may have
    different numbers of sampled locations (the reference draws Bernoulli masks, CSMRI.py:43-45): grad_full's 1/M0
    is a per-problem device vector."""
    kind = 'csmri'
    per_problem = True

    def __init__(self, xrec, mask, Y, xinit, dtype=torch.float32, device='cuda', *, _state=None):
        if _state is not None:
            return self._init(**_state)
        B, H, W = xrec.shape
        plan = ops.CsmriPlan(H, W, B, dtype)
        mask_np = np.ascontiguousarray(mask, np.uint8).reshape(B, H, W)
        M0 = mask_np.reshape(B, -1).sum(1).astype(np.int64)
        maskT = plan.sel_from_dense(torch.from_numpy(mask_np).to(device))
        YT = torch.from_numpy(np.ascontiguousarray(np.swapaxes(Y, 1, 2))).to(device, ops._CDT[dtype]).contiguous()
        self._init(plan, self._upload(xrec, dtype, device), self._upload(xinit, dtype, device, (B, H, W)), maskT,
                   plan.pack_mask(maskT), YT, plan.pack_y(YT, maskT), self._upload(1.0 / M0.astype(np.float64), dtype, device), M0,
                   mask_np=mask_np)

    def _init(self, plan, xrec, xinit, maskT, bits, YT, yh_full, inv_m0, M0, sigma=None, mask_np=None):
        """M0: int64 [B] on the host; sigma: [B] float64 noise levels (a generated batch), mask_np: the host masks when known."""
        self._init_base(xrec, xinit, int(M0.min()))
        self.plan, self.maskT, self.bits, self.YT, self.yh_full, self.inv_m0 = plan, maskT, bits, YT, yh_full, inv_m0
        self.M0, self.sigma, self._mask_np = M0, sigma, mask_np

    @classmethod
    def synthetic(cls, B, H=256, W=256, sample_prob=0.2, snr=20.0, seed=0, dtype=torch.float32, bernoulli=True):
        """B synthetic problems: smoothed-noise images, complex data with real noise on the support.
        bernoulli=True draws each mask entry with probability p like the reference (CSMRI.py:43-45; the number of
        sampled points then differs per problem), False draws exactly round(p*N) points."""
        rng = np.random.default_rng(seed)
        N = H * W
        xrec = np.empty((B, H, W))
        mask = np.zeros((B, N), np.uint8)
        Y = np.empty((B, H, W), np.complex128)
        xinit = np.empty((B, N))
        for b in range(B):
            x = rng.random((H, W))
            p = np.pad(x, 2, mode='wrap')
            y = sum(p[i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
            y = (y - y.min()) / (y.max() - y.min())
            xrec[b] = np.round(y * 255) / 255.0
            xrec[b] = (xrec[b] - xrec[b].min()) / (xrec[b].max() - xrec[b].min())
            if bernoulli:
                mask[b] = rng.random(N) < sample_prob
            else:
                mask[b, rng.choice(N, int(round(sample_prob * N)), replace=False)] = 1
            mk = mask[b].reshape(H, W)
            Y0 = mk * np.fft.fft2(xrec[b])
            sigma = np.sqrt(np.linalg.norm(Y0.ravel()) / 10 ** (snr / 10) / H / W)     # problem.py:58-61
            Y[b] = Y0 + mk * rng.normal(0, sigma, (H, W))
            xi = np.absolute(np.fft.ifft2(Y[b])).ravel()
            xinit[b] = (xi - xi.min()) / (xi.max() - xi.min())
        return cls(xrec, mask.reshape(B, H, W), Y, xinit, dtype=dtype)

    @property
    def mask_np(self):
        """[B, H, W] uint8 sampling masks on the host; a generated batch reads them back on first use."""
        if self._mask_np is None:
            self._mask_np = np.ascontiguousarray(self.maskT.cpu().numpy().swapaxes(1, 2))
        return self._mask_np

    @mask_np.setter
    def mask_np(self, m):
        self._mask_np = m

    @classmethod
    def generate(cls, images, items, H=256, W=256, dtype=torch.float32, device='cuda'):
        """The problems of `items` (dicts of sweep.make_items: id, image, alpha, snr, seed) generated ON THE DEVICE from the
        counter-based stream of include/pnp_hip.h (pnp_csmri_generate): Bernoulli mask, masked spectrum, real noise on the
        support, Xinit -- problems/CSMRI.py:12-59 per item, NOT NumPy's streams.  images: a list of H x W arrays, or the
        tensor `upload_images` made of them (upload once, generate many batches).  Host work: the [B] parameter vectors and
        one read-back of M0."""
        images, (image_idx, *par) = cls._generate_inputs(images, items, H, W, dtype, device)
        thr = [min(max(int(np.floor(np.float64(it['alpha']) * 2.0 ** 32)), 0), 2 ** 32) for it in items]
        plan = ops.CsmriPlan(H, W, len(items), dtype)
        o = plan.generate(images, image_idx, torch.from_numpy(np.array(thr, np.int64)).to(images.device), *par)
        return cls._of(plan=plan, M0=o.pop('M0').cpu().numpy().astype(np.int64), **o)

    def tile(self, n):
        """A batch of n * B problems whose data is this batch's repeated n times along B (problem t * B + i = this batch's
        problem i): device copies only, no regeneration and no host round trip -- what a trial-batched grid runs on."""
        n = int(n)
        if n < 1:
            raise ValueError('tile(n) needs n >= 1')
        rep = lambda v: None if v is None else v.repeat((n,) + (1,) * (v.dim() - 1)).contiguous()
        dev = {name: rep(getattr(self, name)) for name in ('xrec', 'xinit', 'maskT', 'bits', 'YT', 'yh_full', 'inv_m0', 'sigma')}
        return self._of(plan=ops.CsmriPlan(self.H, self.W, self.B * n, self.dtype), M0=np.tile(self.M0, n),
                        mask_np=None if self._mask_np is None else np.tile(self._mask_np, (n, 1, 1)), **dev)

    @classmethod
    def from_problems(cls, probs, dtype=torch.float32, device='cuda'):
        """From reference-style problem objects (anything with Xrec, mask, Y, Xinit: problems.CSMRI, the oracle's)."""
        return cls(np.stack([p.Xrec for p in probs]), np.stack([p.mask for p in probs]), np.stack([p.Y for p in probs]),
                   np.stack([p.Xinit for p in probs]), dtype=dtype, device=device)

    def draw_minibatches(self, n_steps, mb, seed=1):
        """[n_steps][B][mb] int32 flat k-space indices, each row a uniform draw without replacement
        from that problem's mask support (CSMRI.py:66-74 semantics, fast Generator stream)."""
        self._check_mb(mb)
        rng = np.random.default_rng(seed)
        out = np.empty((n_steps, self.B, mb), np.int32)
        for b in range(self.B):
            locs = np.flatnonzero(self.mask_np[b]).astype(np.int32)
            for s in range(n_steps):
                out[s, b] = rng.choice(locs, mb, replace=False)
        return torch.from_numpy(out).to(self.device)

    # ---- minibatch slots
    def minibatches(self, n):
        return Minibatches.zeros(n, self.B, self.device, bits_shape=(self.W, self.H // 32))

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        """mb: an int, or per problem: [B] integers on the host (checked against each problem's population, then uploaded) or an
        int32 [B] device tensor (taken as checked: the engines check their host copy once).  draw_id: int32 [B] device tensor,
        the ids the minibatch streams absorb in place of the batch index."""
        if not isinstance(mb, torch.Tensor):
            self._check_mb(mb)
            if np.ndim(mb) != 0:
                mb = torch.from_numpy(np.ascontiguousarray(mb, np.int32)).to(self.device)
        self.plan.draw_thresholds(self.bits, mb, seed, step0, nsteps, out=mbs.mbd[:nsteps], step_dev=step_dev,
                                  selbits=mbs.selbits[:nsteps], draw_id=draw_id)
        for j in range(nsteps):
            mbs.host[j] = None

    def set_host(self, mbs, j, idx):
        """idx: int32 [B, mb] flat row-major k-space positions (np.flatnonzero(mask o minibatch))."""
        mbs.host[j] = self.plan.sel_from_indices(idx, out=mbs.host[j] if isinstance(mbs.host[j], torch.Tensor) else None)

    def _sel(self, mbs, j):
        if mbs.host[j] is not None:
            return dict(selT=mbs.host[j])
        return dict(bits=mbs.selbits[j])

    def objective(self, z, out=None):
        """f(z) = ||Y - mask o fft2(z)||^2 / 2 / N per problem (problems/CSMRI.py:61-64) -> float64 [B] on the device: the forward row
        pass and a column pass that ends in the sum over the full spectrum (pnp_csmri_objective); nothing is read back."""
        return self.plan.objective(z, self.YT, self.bits, 0.5 / self.N, out=out)

    # ---- gradients
    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        return self.plan.grad(z, bits=self.bits, yh=self.yh_full, alpha=alpha, alpha_vec=self.inv_m0, beta=beta, c1=c1, out=out)

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        return self.plan.grad(z, YT=self.YT, alpha=alpha, beta=beta, c1=c1, out=out, **self._sel(mbs, j))

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        # one FFT pair: the data terms cancel
        return self.plan.grad(z, b=w, alpha=alpha, beta=beta, c1=c1, gamma=gamma, c2=c2, out=out, **self._sel(mbs, j))


class DeblurBatch(_BatchBase):
    """B Deblur / super-resolution problems sharing one blur kernel (reference problems/DeblurSR.py:17-147 per problem).
    By default they also share one down-sampler: the sweeps that vary image, noise and seed.  With a SEQUENCE of B `scale_percent`
    values (the sampling-ratio sweep) every problem has a down-sampler and a measurement count of its own: `M_vec`
    ([B] ints) holds them, `M` is their maximum, and Y, the indicators and the forward output are [B, M] with entries m >= M_vec[b]
    of a row as padding (zero in Y, read by no kernel).  A problem of such a batch with scale_percent < 100 walks, bit for bit,
    what it walks in a uniform batch of its scale; one with scale_percent == 100 agrees to rounding."""
    kind = 'deblur'
    per_problem = True
    M_vec = None                                                # mixed scales: per-problem measurement counts, host int32 [B]
    draw_seeds = None                                           # mixed scales: per-problem seeds of the device draws (see `draw`)

    def __init__(self, xrec, Bk, Y, xinit, dtype=torch.float32, device='cuda', bilinear=None, *, scale_percent=None, _state=None):
        if _state is not None:
            return self._init(**_state)
        B, H, W = xrec.shape
        if scale_percent is not None and np.ndim(scale_percent) != 0:
            # mixed scales: Y as B per-problem arrays of M_b entries, or as one padded [B, Mmax] array
            from .problems import deblur_operator_sets
            if bilinear is not None:
                raise ValueError('DeblurBatch: pass either bilinear (one down-sampler) or a sequence of scale_percent, not both')
            if len(scale_percent) != B:
                raise ValueError(f'DeblurBatch: {B} problems need {B} scale_percent values, got {len(scale_percent)}')
            sets, set_of, M_vec = deblur_operator_sets(H, W, scale_percent)
            Mmax = int(M_vec.max())
            if isinstance(Y, np.ndarray) and Y.ndim == 2:
                if Y.shape != (B, Mmax):
                    raise ValueError(f'DeblurBatch: a padded Y must be [{B}, {Mmax}], got {Y.shape}')
                Yp = np.array(Y, np.float64)
            else:
                if len(Y) != B or any(np.size(y) != m for y, m in zip(Y, M_vec)):
                    raise ValueError(f'DeblurBatch: per-problem Y arrays must hold {M_vec.tolist()} entries, got '
                                     f'{[int(np.size(y)) for y in Y]}')
                Yp = np.zeros((B, Mmax))
                for b, y in enumerate(Y):
                    Yp[b, :M_vec[b]] = np.ravel(y)
            for b in range(B):
                Yp[b, M_vec[b]:] = 0.0                          # the padding is zero by definition
            plan = ops.DeblurPlan.mixed(H, W, dtype, Bk, sets, set_of, M_vec, device=device)
            return self._init(plan, self._upload(xrec, dtype, device), self._upload(xinit, dtype, device, (B, H, W)),
                              self._upload(Yp, dtype, device, (B, Mmax)))
        if scale_percent is not None:                           # an int: exactly the batch `bilinear=` of that scale builds
            from .problems import _deblur_taps
            if bilinear is not None:
                raise ValueError('DeblurBatch: pass either bilinear or scale_percent, not both')
            bilinear = _deblur_taps(H, W, int(scale_percent))
        plan = ops.DeblurPlan(H, W, B, dtype, Bk, bilinear=bilinear)
        self._init(plan, self._upload(xrec, dtype, device), self._upload(xinit, dtype, device, (B, H, W)),
                   self._upload(Y, dtype, device, (B, plan.M)))

    def _init(self, plan, xrec, xinit, Y, sigma=None):
        """sigma: [B] float64 noise levels (a generated batch)."""
        self._init_base(xrec, xinit, plan.M if plan.M_vec is None else plan.M_vec)
        self.plan, self.M, self.Y, self.sigma = plan, plan.M, Y, sigma
        self.M_vec = plan.M_vec
        self._scale_cache, self._mb_cache, self._pinned = {}, {}, set()

    def _check_mb(self, mb):
        if self.M_vec is not None and np.ndim(mb) == 0:         # mixed scales: a scalar against every problem's own M_b
            mb = np.full(self.B, int(mb), np.int64)
        return super()._check_mb(mb)

    @classmethod
    def generate(cls, images, items, H=256, W=256, dtype=torch.float32, kernel='Minimal', scale_percent=100, device='cuda'):
        """The problems of `items` (dicts of sweep.make_items; their alpha is NOT read: the operator comes from `kernel` and
        `scale_percent`) generated ON THE DEVICE from the counter-based stream of include/pnp_hip.h (pnp_deblur_generate):
        Y = S B x + noise, Xinit uniform in [0, 1) -- problems/DeblurSR.py:38-57 per item, NOT NumPy's streams.  images: a list of
        H x W arrays, or the tensor `upload_images` made of them.  Also sets `sigma` ([B] float64, device).
        scale_percent: an int, or one int per item (a mixed-scale batch): an item's Y[:M_b], xinit, xrec and sigma are then those a
        uniform `generate` of its scale gives, bit for bit, and the padding of Y is zero."""
        from .problems import _deblur_taps, deblur_operator_sets
        from .sweep import _minimal_kernel
        if np.ndim(scale_percent) != 0:
            if len(scale_percent) != len(items):
                raise ValueError(f'generate: {len(items)} items need {len(items)} scale_percent values, got {len(scale_percent)}')
            sets, set_of, M_vec = deblur_operator_sets(H, W, scale_percent)
            images, par = cls._generate_inputs(images, items, H, W, dtype, device)
            plan = ops.DeblurPlan.mixed(H, W, dtype, _minimal_kernel(H, W, kernel), sets, set_of, M_vec, device=images.device)
            return cls._of(plan=plan, **plan.generate(images, *par))
        images, par = cls._generate_inputs(images, items, H, W, dtype, device)
        plan = ops.DeblurPlan(H, W, len(items), dtype, _minimal_kernel(H, W, kernel), bilinear=_deblur_taps(H, W, scale_percent))
        return cls._of(plan=plan, **plan.generate(images, *par))

    @classmethod
    def from_problems(cls, probs, dtype=torch.float32, device='cuda'):
        p0 = probs[0]
        scales = [getattr(p, 'scale_percent', None) for p in probs]
        if any(s != scales[0] for s in scales):                 # problems of different scales: a mixed-scale batch
            return cls(np.stack([p.Xrec for p in probs]), p0.B, [p.Y for p in probs], np.stack([p.Xinit for p in probs]),
                       dtype=dtype, device=device, scale_percent=scales)
        return cls(np.stack([p.Xrec for p in probs]), p0.B, np.stack([p.Y for p in probs]),
                   np.stack([p.Xinit for p in probs]), dtype=dtype, device=device,
                   bilinear=getattr(p0, 'Bop', None) if isinstance(getattr(p0, 'Bop', None), tuple) else None)

    @classmethod
    def synthetic(cls, B, H=256, W=256, kernel='Minimal', snr=20.0, seed=0, dtype=torch.float32):
        """B synthetic Deblur problems (scale_percent = 100): smoothed-noise images, the reference's "Minimal" or
        "Identity" kernel (DeblurSR.py:80-89), noise and U(0,1) initialisation from a Generator stream."""
        rng = np.random.default_rng(seed)
        N = H * W
        if kernel == 'Minimal':
            Bk = np.zeros((H, W))
            Bk[0, 0] = Bk[H // 2, H // 2] = Bk[H // 2, H // 3] = Bk[H // 2, H // 4] = 0.25
        else:
            Bk = np.zeros((H, W))
            Bk[0, 0] = 1
        Bk = Bk.ravel() / N
        FB = np.fft.fft(Bk)
        xrec = np.empty((B, H, W))
        Y = np.empty((B, N))
        for b in range(B):
            x = rng.random((H, W))
            p = np.pad(x, 2, mode='wrap')
            y = sum(p[i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
            xrec[b] = (y - y.min()) / (y.max() - y.min())
            Y0 = np.real(np.fft.ifft(np.fft.fft(xrec[b].ravel()) * FB)) * np.sqrt(N)       # DeblurSR.py:119-120
            sigma = np.sqrt(np.linalg.norm(Y0) / 10 ** (snr / 10) / H / W)
            Y[b] = Y0 + rng.normal(0, sigma, N)
        return cls(xrec, Bk, Y, rng.uniform(0.0, 1.0, (B, N)), dtype=dtype)

    def draw_minibatches(self, n_steps, mb, seed=1):
        if self.M_vec is not None:
            raise ValueError('draw_minibatches draws from one population for all problems; a mixed-scale DeblurBatch has one per '
                             'problem: use device draws (draw), or set_host with indices below every M_vec[b]')
        self._check_mb(mb)
        rng = np.random.default_rng(seed)
        out = np.stack([[rng.choice(self.M, mb, replace=False) for _ in range(self.B)] for _ in range(n_steps)]).astype(np.int32)
        return torch.from_numpy(out).to(self.device)

    def tile(self, n):
        """A batch of n * B problems (problem t * B + i = this batch's problem i) on the same kernel spectrum and down-sampler: a plan
        for n * B problems, xrec, xinit, Y and sigma repeated by device copies -- what a trial-batched grid runs on."""
        n = int(n)
        if n < 1:
            raise ValueError('tile(n) needs n >= 1')
        rep = lambda v: None if v is None else v.repeat((n,) + (1,) * (v.dim() - 1)).contiguous()
        t = self._of(plan=self.plan.resized(self.B * n), xrec=rep(self.xrec), xinit=rep(self.xinit), Y=rep(self.Y),
                     sigma=rep(self.sigma))
        t.draw_seeds = rep(self.draw_seeds)
        return t

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        """mb: an int, or per problem: [B] integers on the host (checked, then uploaded) or an int32 [B] device tensor (taken as
        checked: the engines check their host copy once).  draw_id: int32 [B] device tensor, the ids the minibatch streams absorb in
        place of the batch index.  On a mixed-scale batch `draw_seeds` (int64 [B] device tensor, or None) gives every problem a seed
        of its own in place of `seed`: in a sweep an item keeps the stream of the group it would have run in."""
        if not isinstance(mb, torch.Tensor):
            self._check_mb(mb)
            if np.ndim(mb) != 0:
                mb = torch.from_numpy(np.ascontiguousarray(mb, np.int32)).to(self.device)
        if self.M_vec is not None:                              # mixed scales: problem b draws among its own M_vec[b] measurements
            if not isinstance(mb, torch.Tensor):                # (the int32 vector of a scalar: made once per value)
                mb = self._cached(self._mb_cache, int(mb), lambda: torch.full((self.B,), int(mb), dtype=torch.int32, device=self.device))
            ops.draw_thresholds_mpp(self.plan.M_dev, mb, seed, step0, nsteps, out=mbs.mbd[:nsteps], step_dev=step_dev, draw_id=draw_id,
                                    seed_vec=self.draw_seeds)
        else:
            ops.draw_thresholds(self.M, self.B, mb, seed, step0, nsteps, out=mbs.mbd[:nsteps], step_dev=step_dev, draw_id=draw_id)
        for j in range(nsteps):
            mbs.host[j] = None

    def set_host(self, mbs, j, idx):
        """idx: int32 [B, mb] measurement indices (np.flatnonzero of Problem.select_mb's indicator); on a mixed-scale batch row b
        holds indices below M_vec[b] and the indicator has the row stride M."""
        mbs.host[j] = ops.indicator_from_indices(idx, self.M, out=mbs.host[j] if isinstance(mbs.host[j], torch.Tensor) else None)

    def _sel(self, mbs, j):
        if mbs.host[j] is not None:
            return dict(sel=mbs.host[j])
        return dict(mbd=mbs.mbd[j])

    def objective(self, z, out=None):
        """f(z) = ||Y - S B z||^2 / 2 / M per problem (problems/DeblurSR.py:114-117) -> float64 [B] on the device
        (pnp_deblur_objective); nothing is read back."""
        if self.M_vec is not None:                              # mixed scales: the kernel divides 1/2 by each problem's own M_b
            return self.plan.objective(z, self.Y, 0.5, out=out)
        return self.plan.objective(z, self.Y, 0.5 / self.M, out=out)

    # alpha (and gamma of grad_stoch_diff): a scalar -> the plain calls; a float64 [B] device tensor -> the `_pp` entry points
    def _over_m(self, a):
        return a / (self.M if self.M_vec is None else self.M_vec)     # (mixed scales: per problem, alpha_b / M_b)

    def _cached(self, cache, key, make):
        """cache[key], made on first use.  A value looked up while the stream captures is pinned for the life of the batch: the
        captured graph points to its tensor.  Of the others at most 16 are kept per cache, the oldest dropped first (a decaying
        step size makes a new value every step)."""
        if key not in cache:
            loose = [k for k in cache if (id(cache), k) not in self._pinned]
            for k in loose[:max(0, len(loose) - 15)]:
                del cache[k]
            cache[key] = make()
        if torch.cuda.is_current_stream_capturing():
            self._pinned.add((id(cache), key))
        return cache[key]

    def _scalar_over_m(self, alpha):
        """Mixed scales: a scalar alpha over every problem's own M_b -- each quotient the float64 one a uniform batch takes on the
        host -- as a float64 [B] device tensor, uploaded once per value (so a replayed capture sees no upload)."""
        key = float(alpha)
        return self._cached(self._scale_cache, key,
                            lambda: torch.from_numpy(np.array([key / int(m) for m in self.M_vec], np.float64)).to(self.device))

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        # (per problem: alpha_b / M taken on the host in float64, as the scalar's quotient is; mixed scales: alpha / M_b)
        if isinstance(alpha, torch.Tensor):
            scale = self._host(alpha, self._over_m)
        else:
            scale = alpha / self.M if self.M_vec is None else self._scalar_over_m(alpha)
        g = self.plan.grad(z, self.Y, scale=scale, out=out if c1 is None else self._scratch(z))
        return self._combine(g, out, beta, c1)

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        g = self.plan.grad(z, self.Y, scale=alpha, out=out if c1 is None else self._scratch(z), **self._sel(mbs, j))
        return self._combine(g, out, beta, c1)

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None, one_pass=False):
        # gs(z) - gs(w) = B^T S^T sel (S B (z - w)) + (terms in y cancel): two gradients, one combine
        # one_pass=True (opt-in): exactly that, and the step's addends, as ONE pnp_deblur_grad_step -- nothing allocated;
        # it rounds z - w once instead of two gradients, so it is not the default's bits
        if one_pass:
            if self.M_vec is not None:
                raise ValueError('grad_stoch_diff(one_pass=True): a mixed-scale DeblurBatch has no one-pass step (uniform batches only)')
            return self.plan.grad_step(z, b=w, scale=alpha, beta=beta, c1=c1, gamma=gamma, c2=c2, out=out, **self._sel(mbs, j))
        g1 = self.plan.grad(z, self.Y, scale=alpha, out=torch.empty_like(z), **self._sel(mbs, j))
        g2 = self.plan.grad(w, self.Y, scale=alpha, out=self._scratch(z), **self._sel(mbs, j))
        return self._combine(ops.axpbypcz(1.0, g1, -1.0, g2, out=g1), out, beta, c1, gamma, c2)


class PrBatch(_BatchBase):
    """B phase-retrieval problems (reference problems/PR.py:13-87 per problem), each with its own dense M x N matrix.
    `tile(n)` gives the trial-batched form: n * B problems that SHARE the B matrices (problem t * B + i works on A[i]; nothing of
    A is copied), whose gradients are one pnp_pr_grad_shared call each (csrc/pr_shared.hip: A is streamed twice per call whatever
    n is) and which takes per-problem eta, mini_batch_size and draw_id from the engines."""
    kind = 'pr'

    def __init__(self, xrec, A, Y, xinit, dtype=torch.float32, device='cuda', *, _state=None):
        if _state is not None:
            return self._init(**_state)
        ops.require_gpu()
        B, H, W = xrec.shape
        self._init(self._upload(xrec, dtype, device), self._upload(xinit, dtype, device, (B, H, W)),
                   self._upload(A, dtype, device).contiguous(), self._upload(Y, dtype, device, (B, A.shape[1])))

    def _init(self, xrec, xinit, A, Y, sigma=None, spec_iters=None, items=None):
        """A: [B, M, N]; sigma ([B] float64 noise levels) and spec_iters (power-iteration steps per item): a generated batch.
        items: a tiled batch -- A is [items, M, N] and problem b of the B = n * items works on A[b % items]."""
        self._init_base(xrec, xinit, A.shape[1])
        self.M, self.A, self.Y, self.sigma, self.spec_iters = A.shape[1], A, Y, sigma, spec_iters
        self.items, self.shared = (self.B, False) if items is None else (int(items), True)
        self.per_problem = self.shared
        if self.shared:
            self._ws = ops.pr_shared_workspace(self.M, self.N, self.dtype, self.device, self.B)
        else:
            self._ws = ops.pr_workspace(self.M, self.N, self.dtype, self.device, self.B)
        self._mb = None                                         # size of the last device draw (the row lists' width)
        self._obj_ws = None                                     # scratch of `objective`, made on first use

    def tile(self, n):
        """A batch of n * B problems (problem t * B + i = this batch's problem i) on THIS batch's matrices: xrec, xinit, Y and sigma
        are repeated by device copies, A is the same tensor -- what a trial-batched grid runs on (sweep.make_runner(...,
        shared_matrix=True)).  Its gradients go through pnp_pr_grad_shared."""
        n = int(n)
        if n < 1:
            raise ValueError('tile(n) needs n >= 1')
        rep = lambda v: None if v is None else v.repeat((n,) + (1,) * (v.dim() - 1)).contiguous()
        return self._of(xrec=rep(self.xrec), xinit=rep(self.xinit), A=self.A, Y=rep(self.Y), sigma=rep(self.sigma),
                        spec_iters=None if self.spec_iters is None else np.tile(self.spec_iters, n), items=self.items)

    @classmethod
    def generate(cls, images, items, H, W, M, dtype=torch.float32, max_iters=1000, check_every=8, device='cuda'):
        """The problems of `items` (dicts of sweep.make_items; their alpha is NOT read: `M` is the number of measurements)
        generated ON THE DEVICE from the counter-based stream of include/pnp_hip.h: the Gaussian A in HBM, Y = |A x| + noise
        (pnp_pr_generate) and the spectral initialisation of all items at once with the stopping rule evaluated per item on the
        device (pnp_pr_spectral_init_batch; one host synchronisation per `check_every` steps) -- problems/PR.py:26-63 per item,
        NOT NumPy's streams.  Also sets `sigma` ([B] float64, device) and `spec_iters` ([B] int array: power-iteration steps per
        item).  Raises ValueError naming the items that have not met the rule after `max_iters` steps."""
        images, par = cls._generate_inputs(images, items, H, W, dtype, device)
        o = ops.pr_generate(images, *par, int(M))
        xinit, iters, active = ops.pr_spectral_init_batch(o['A'], o['Y'], o['xrec'], max_iters, check_every)
        spec_iters = iters.cpu().numpy().astype(np.int64)
        late = np.flatnonzero(active.cpu().numpy())
        if late.size:
            raise ValueError(f'spectral initialisation: items {[items[j]["id"] for j in late]} (batch positions {late.tolist()}) '
                             f'still active after max_iters = {max_iters} steps')
        return cls._of(xinit=xinit, spec_iters=spec_iters, **o)

    @classmethod
    def from_problems(cls, probs, dtype=torch.float32, device='cuda'):
        return cls(np.stack([p.Xrec for p in probs]), np.stack([p.A for p in probs]), np.stack([p.Y for p in probs]),
                   np.stack([p.Xinit for p in probs]), dtype=dtype, device=device)

    def draw_minibatches(self, n_steps, mb, seed=1):
        self._check_mb(mb)
        rng = np.random.default_rng(seed)
        out = np.stack([[np.sort(rng.choice(self.M, mb, replace=False)) for _ in range(self.B)] for _ in range(n_steps)]).astype(np.int32)
        return torch.from_numpy(out).to(self.device)

    def draw(self, mbs, mb, seed, step0, nsteps=1, step_dev=None, draw_id=None):
        """mb: an int; on a tiled batch also per problem ([B] integers on the host, or an int32 [B] device tensor taken as
        checked), with draw_id (int32 [B] device tensor): the ids the minibatch streams absorb in place of the batch index."""
        if not isinstance(mb, torch.Tensor):
            self._check_mb(mb)
            if np.ndim(mb) != 0:
                mb = torch.from_numpy(np.ascontiguousarray(mb, np.int32)).to(self.device)
        if (isinstance(mb, torch.Tensor) or draw_id is not None) and not self.shared:
            raise ValueError('per-problem mini_batch_size / draw_id need a tiled PrBatch (PrBatch.tile)')
        self._mb = mb
        ops.draw_thresholds(self.M, self.B, mb, seed, step0, nsteps, out=mbs.mbd[:nsteps], step_dev=step_dev, draw_id=draw_id)
        for j in range(nsteps):
            mbs.host[j] = None

    def set_host(self, mbs, j, idx):
        """idx: int32 [B, mb] row ids (np.flatnonzero of the indicator: ascending, like A[idx] in PR.py:82-83).  A tiled batch keeps
        them as the uint8 [B, M] indicator its kernel takes."""
        if self.shared:
            mbs.host[j] = ops.indicator_from_indices(idx.contiguous(), self.M,
                                                     out=mbs.host[j] if isinstance(mbs.host[j], torch.Tensor) else None)
        else:
            mbs.host[j] = idx.contiguous()

    def _rows(self, mbs, j):
        if mbs.host[j] is not None:
            return mbs.host[j]
        key = ('rows', j)
        buf = getattr(mbs, '_rows', None)
        if buf is None:
            buf = mbs._rows = {}
        if key not in buf:
            buf[key] = torch.empty((self.B, self._mb), dtype=torch.int32, device=self.device)
        return ops.rows_from_thresholds(self.M, self._mb, mbs.mbd[j], out=buf[key])

    def objective(self, z, out=None):
        """f(z) = ||Y - |A z|||^2 / 2 / M per problem (problems/PR.py:70-73) -> float64 [B] on the device (pnp_pr_objective: A is
        streamed once; a tiled batch reads the matrix of its item, A[b % items]); nothing is read back."""
        if self._obj_ws is None:
            self._obj_ws = ops.pr_objective_workspace(self.M, self.B, self.device)
        return ops.pr_objective(self.A, z.reshape(self.B, self.N), self.Y, 0.5 / self.M, workspace=self._obj_ws, out=out)

    def _g(self, z, rows, scale, out):
        ops.pr_grad_batch(self.A, z.reshape(self.B, self.N), self.Y, rows=rows, scale=scale, workspace=self._ws,
                          out=out.reshape(self.B, self.N))
        return out

    def _shared(self, z, w, mbs, j, out, alpha, alpha_div, beta, c1, gamma=0.0, c2=None):
        """One pnp_pr_grad_shared call: the selection of slot j (None: all rows) goes in as descriptors or as an indicator."""
        v = lambda t: None if t is None else t.reshape(self.B, self.N)
        sel = {} if mbs is None else (dict(ind=mbs.host[j]) if mbs.host[j] is not None else dict(mbd=mbs.mbd[j]))
        ops.pr_grad_shared(self.A, self.Y[:self.items], v(z), v(w), alpha=alpha, alpha_div=alpha_div, beta=beta, c1=v(c1), gamma=gamma,
                           c2=v(c2), workspace=self._ws, out=v(out), **sel)
        return out

    def grad_full(self, z, out, alpha=1.0, beta=0.0, c1=None):
        if self.shared:
            return self._shared(z, None, None, 0, out, alpha, self.M, beta, c1)
        g = self._g(z, None, alpha / self.M, out if c1 is None else self._scratch(z))
        return self._combine(g, out, beta, c1)

    def grad_stoch(self, z, mbs, j, out, alpha=1.0, beta=0.0, c1=None):
        if self.shared:
            return self._shared(z, None, mbs, j, out, alpha, 1.0, beta, c1)
        g = self._g(z, self._rows(mbs, j), alpha, out if c1 is None else self._scratch(z))
        return self._combine(g, out, beta, c1)

    def grad_stoch_diff(self, z, w, mbs, j, out, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None):
        if self.shared:
            return self._shared(z, w, mbs, j, out, alpha, 1.0, beta, c1, gamma, c2)
        rows = self._rows(mbs, j)
        g1 = self._g(z, rows, alpha, torch.empty_like(z))
        g2 = self._g(w, rows, alpha, self._scratch(z))
        return self._combine(ops.axpbypcz(1.0, g1, -1.0, g2, out=g1), out, beta, c1, gamma, c2)
