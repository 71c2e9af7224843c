"""Prox adapters of the engines: a denoiser of the reference (denoisers/TV.py, RealSN_DnCNN.py, NLM.py) as the engines call it.

A prox is bound to a batch once (`bind(batch)`), then called as `prox(z, xrec, sse_out)`: it denoises the iterate z [B, H, W],
writes the squared errors against xrec to sse_out and returns the tensor that holds the result (`inplace`: z itself).  The
one-kernel iteration of SvrgEngine asks for `fused_args()` / `after_fused()` / `fused_denoise` as well.
"""
import numpy as np
import torch

from . import ops


class TVProx:
    """denoisers/TV.py semantics for the engines (fused estimate_sigma + BayesShrink + error sum).
    multi=True: the per-column 1-D prox (pnp_prox_tv), which the one-kernel iteration holds inside the gradient kernel.
    multi=False: the 2-D wavelet prox (pnp_prox_wavelet2d): a kernel of its own after the gradient kernel, which in the
    one-kernel iteration makes step + noise estimate (the DnCNNProx pattern) -- the engine then steps per iteration.
    multi=False, in_kernel=True (opt-in): the one-kernel iteration holds the 2-D prox as well (`denoise = 2` of the step entry
    points, pnp_csmri_svrg_outer_iteration_prox): one launch per step, SvrgEngine's one-launch outer iteration.  Its 15 sub-band
    sums are taken in another order than pnp_prox_wavelet2d's, so the two forms agree to a few ulps of the thresholds, not bit
    for bit; outside the one-kernel iteration (fused=False engines) the prox is pnp_prox_wavelet2d as before."""

    def __init__(self, sigma_modifier=1.0, decay=1.0, denoise_strength=0.0, multi=True, in_kernel=False):
        if in_kernel and multi:
            raise ValueError('TVProx(in_kernel=True) selects the in-kernel form of the 2-D prox: it needs multi=False '
                             '(the per-column prox, multi=True, always runs inside the one-kernel iteration)')
        self.sigma_modifier, self.decay, self.denoise_strength, self.t = sigma_modifier, decay, denoise_strength, 0
        self.multi, self.in_kernel = multi, bool(in_kernel)
        self.fused_denoise = bool(multi) or self.in_kernel      # one-kernel iteration: does the prox run inside it
        self.fused_kind = 2 if self.in_kernel else 1            # ... and which: `int denoise` of the step entry points

    def bind(self, batch):
        self.sig = torch.empty(batch.B, dtype=batch.dtype, device=batch.xrec.device)
        if not isinstance(self.sigma_modifier, torch.Tensor) and np.ndim(self.sigma_modifier) != 0:
            sm = np.ascontiguousarray(self.sigma_modifier, np.float64)      # per problem: a float64 [B] device vector, uploaded once
            if sm.shape != (batch.B,):
                raise ValueError(f'per-problem sigma_modifier: {batch.B} values, got shape {sm.shape}')
            self.sigma_modifier = torch.from_numpy(sm).to(batch.xrec.device)

    def __call__(self, z, xrec, sse_out):
        self.t += 1
        prox = ops.prox_tv if self.multi else ops.prox_wavelet2d
        prox(z, sigma_modifier=self.sigma_modifier, fallback_sigma=self.denoise_strength * self.decay ** self.t,
             xrec=xrec, out=z, sse=sse_out, sigma_out=self.sig)
        return z

    inplace = True                                              # writes its result into the iterate it was given

    # one-kernel iteration (pnp_csmri_svrg_step): the 1-D prox runs inside the gradient kernel (fused_denoise); for the
    # 2-D prox that kernel stops after the noise estimate and after_fused shrinks with it
    def fused_args(self):
        if not self.fused_denoise:
            return dict(sigma_out=self.sig)
        self.t += 1
        return dict(sigma_modifier=self.sigma_modifier, fallback_sigma=self.denoise_strength * self.decay ** self.t, sigma_out=self.sig)

    def after_fused(self, z, xrec, sse_out):
        if not self.fused_denoise:
            self.t += 1
            ops.prox_wavelet2d(z, sigma_in=self.sig, sigma_modifier=self.sigma_modifier,
                               fallback_sigma=self.denoise_strength * self.decay ** self.t, xrec=xrec, out=z, sse=sse_out,
                               sigma_out=self.sig)
        return z


class DnCNNProx:
    """denoisers/RealSN_DnCNN.py semantics for the engines.  The loop's estimate_sigma is still
    evaluated (the reference computes it every iteration and this denoiser ignores it, F12)."""

    def __init__(self, weights, sigma):
        self.weights, self.sigma = weights, sigma

    def bind(self, batch):
        self.plan = ops.DncnnPlan(self.weights, batch.H, batch.W, batch.B)
        self.sig = torch.empty(batch.B, dtype=batch.dtype, device=batch.xrec.device)

    def __call__(self, z, xrec, sse_out):
        ops.sigma_est(z, out=self.sig)
        self.plan.denoise(z, self.sigma, xrec=xrec, out=z, sse=sse_out)
        return z

    inplace = True
    # one-kernel iteration: the gradient kernel makes the (ignored, F12) noise estimate; the network follows
    fused_denoise = False

    def fused_args(self):
        return dict(sigma_out=self.sig)

    def after_fused(self, z, xrec, sse_out):
        self.plan.denoise(z, self.sigma, xrec=xrec, out=z, sse=sse_out)
        return z


class NLMProx:
    """denoisers/NLM.py:22-27 semantics for the engines: h = sigma = estimate_sigma * sigma_modifier when
    `self.sigma > 0` (the attribute the reference reads; default 1.0 here), else the decaying fixed strength.
    NLM cannot run in place: the prox ping-pongs between the engine's iterate and a buffer of its own and RETURNS the
    tensor that holds the result.  sigma_modifier: a scalar, or [B] values (per problem: pnp_nlm2d_pp)."""

    inplace = False                                             # ping-pongs: a hipGraph of an outer iteration cannot hold it

    def __init__(self, sigma=1.0, sigma_modifier=1.0, decay=1.0, denoise_strength=0.0, patch_size=4, patch_distance=5):
        self.sigma, self.sigma_modifier, self.decay, self.denoise_strength = sigma, sigma_modifier, decay, denoise_strength
        self.patch_size, self.patch_distance, self.t = patch_size, patch_distance, 0

    def bind(self, batch):
        self.sig = torch.empty(batch.B, dtype=batch.dtype, device=batch.xrec.device)
        self.buf = torch.empty_like(batch.xinit)
        if not isinstance(self.sigma_modifier, torch.Tensor) and np.ndim(self.sigma_modifier) != 0:
            sm = np.ascontiguousarray(self.sigma_modifier, np.float64)      # per problem: a float64 [B] device vector, uploaded once
            if sm.shape != (batch.B,):
                raise ValueError(f'per-problem sigma_modifier: {batch.B} values, got shape {sm.shape}')
            self.sigma_modifier = torch.from_numpy(sm).to(batch.xrec.device)

    def __call__(self, z, xrec, sse_out):
        self.t += 1
        if self.sigma > 0:
            ops.sigma_est(z, out=self.sig)
            ops.nlm2d(z, sigma_in=self.sig, sigma_modifier=self.sigma_modifier, patch_size=self.patch_size,
                      patch_distance=self.patch_distance, xrec=xrec, out=self.buf, sse=sse_out)
        else:
            ops.nlm2d(z, fixed_h=self.denoise_strength * self.decay ** self.t, patch_size=self.patch_size,
                      patch_distance=self.patch_distance, xrec=xrec, out=self.buf, sse=sse_out)
        out, self.buf = self.buf, z
        return out
