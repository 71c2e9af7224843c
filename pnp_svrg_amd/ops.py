"""Torch-tensor front end of the C-ABI calls.  PyTorch is plumbing here: it owns HBM
allocations and the HIP stream; every op below is one call into libpnp_hip.so."""
import contextlib
import ctypes
import gc
import numpy as np
import torch
from . import _native as N

_DT = {torch.float32: N.F32, torch.float64: N.F64}
_CDT = {torch.float32: torch.complex64, torch.float64: torch.complex128}


def _stream():
    """The current HIP stream of the current device as a raw pointer (capture-aware: inside torch.cuda.graph it is the
    capture stream).  Through torch._C directly: torch.cuda.current_stream() costs 5-6 us of Python per call, which at five
    launches per inner iteration is as much as a kernel of the B = 1 loops."""
    try:
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:                                      # (private API moved: the public, slower way)
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), 'device-resident contiguous tensors only'
    return ctypes.c_void_p(t.data_ptr())


def _dn(denoise):
    """`int denoise` of the one-kernel step entry points: 0 = store the stepped image, 1 = the per-column prox, 2 = the 2-D wavelet
    prox inside the kernel (True / False keep their meaning: 1 / 0)."""
    return 2 if (denoise is not True and denoise == 2) else (1 if denoise else 0)


class _PP(tuple):
    """(scalar, device array or None): a hyper-parameter marked as per-problem capable in an argument list for `_route`."""
    __slots__ = ()


def _pp(v, B, dtype=torch.float64):
    """A hyper-parameter that may be per problem -> _PP(scalar, device array or None): a tensor ([B], float64 -- int32 for minibatch
    sizes) goes to the `_pp` entry point's array argument, anything else is the scalar of the plain call."""
    if isinstance(v, torch.Tensor):
        assert v.dtype == dtype and tuple(v.shape) == (B,), f'per-problem values: a [{B}] {dtype} device tensor'
        return _PP(((0 if dtype == torch.int32 else 0.0), v))
    return _PP(((int(v) if dtype == torch.int32 else float(v)), None))


def _route(name, args, ptr=None):
    """Call entry point `name` with `args`, the `_pp()` values among them as their scalars -- exactly the plain call -- unless one
    of them holds a per-problem array: then `name_pp`, where every `_pp()` value is a (scalar, array pointer or None) pair.
    ptr: what turns an array into the pointer argument (default: `_p`)."""
    ptr = ptr or _p
    if any(type(a) is _PP and a[1] is not None for a in args):
        flat = []
        for a in args:
            if type(a) is _PP:
                flat += (a[0], ptr(a[1]))
            else:
                flat.append(a)
        N.call(name + '_pp', *flat)
    else:
        N.call(name, *[a[0] if type(a) is _PP else a for a in args])


def _mb_vec(mb, draw_id, B, device):
    """What the `_pp` draw entry points take for `mb` (an int, or an int32 [B] device tensor) once either it or `draw_id` is per
    problem: the int32 [B] device vector (they have no scalar form); None when the plain entry point takes the int."""
    if not isinstance(mb, torch.Tensor):
        if draw_id is None:
            return None
        mb = torch.full((B,), int(mb), dtype=torch.int32, device=device)
    assert mb.dtype == torch.int32 and tuple(mb.shape) == (B,)
    assert draw_id is None or (draw_id.dtype == torch.int32 and tuple(draw_id.shape) == (B,))
    return mb


def require_gpu():
    if not torch.cuda.is_available():
        raise N.NativeError('no MI355X visible (torch.cuda.is_available() is False); the hot path has no CPU fallback')
    N.lib()


@contextlib.contextmanager
def collector_held():
    """Around a hipGraph capture.  A plan frees its device buffers when it is destroyed (hipFree), and a hipFree while a stream
    captures invalidates the capture.  A plan that died inside a reference cycle goes whenever the cyclic collector next runs, and
    torch.cuda.graph does not collect before it begins: collect now, and hold the collector off until the block ends."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


def _f_out(out, B, device):
    """The float64 [B] result vector of the objective calls (as pnp_sse's)."""
    if out is None:
        return torch.empty(B, dtype=torch.float64, device=device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B,)
    return out


class CsmriPlan:
    """pnp_csmri_plan_*: masked-FFT gradient of B independent H x W CSMRI problems."""

    def __init__(self, H, W, batch, dtype=torch.float32):
        require_gpu()
        self.H, self.W, self.B, self.dtype = H, W, batch, dtype
        h = ctypes.c_void_p()
        N.call('pnp_csmri_plan_create', ctypes.byref(h), H, W, batch, _DT[dtype])
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                N.lib().pnp_csmri_plan_destroy(h)
            except Exception:
                pass

    def sel_from_indices(self, idx, out=None):
        """idx: int32 [B, n] flat row-major k-space positions -> uint8 [B, W, H] (transposed)."""
        assert idx.dtype == torch.int32 and idx.shape[0] == self.B
        out = out if out is not None else torch.empty((self.B, self.W, self.H), dtype=torch.uint8, device=idx.device)
        N.call('pnp_csmri_sel_from_indices', self._h, _p(idx), idx.shape[1], _p(out), _stream())
        return out

    def pack_mask(self, selT, out=None):
        """uint8 transposed selector [B, W, H] -> bit-packed mask int32 [B, W, H/32] (pnp_csmri_pack_mask)."""
        assert selT.dtype == torch.uint8 and tuple(selT.shape) == (self.B, self.W, self.H)
        out = out if out is not None else torch.empty((self.B, self.W, self.H // 32), dtype=torch.int32, device=selT.device)
        N.call('pnp_csmri_pack_mask', self._h, _p(selT), _p(out), _stream())
        return out

    def draw_thresholds(self, bits, mb, seed, step0, nsteps=1, out=None, step_dev=None, selbits=None, draw_id=None):
        """Device-side minibatch draws for steps step0 .. step0+nsteps-1 of every problem: threshold descriptors
        (int64 [nsteps, B, 2] = 16 bytes per (step, problem)) and, when `selbits` (int32 [nsteps, B, W, H/32]) is given,
        mask o minibatch as bit-packed selectors -- `grad(bits=selbits[j])` consumes a step's row.
        mb: an int, or an int32 [B] device tensor (problem b draws mb[b]); draw_id: int32 [B] device tensor holding the 32-bit
        ids the streams absorb in place of the batch index (pnp_csmri_draw_thresholds_pp)."""
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        out = out if out is not None else torch.empty((nsteps, self.B, 2), dtype=torch.int64, device=bits.device)
        assert out.dtype == torch.int64 and tuple(out.shape) == (nsteps, self.B, 2)
        assert selbits is None or (selbits.dtype == torch.int32 and tuple(selbits.shape) == (nsteps, self.B, self.W, self.H // 32))
        mb_vec = _mb_vec(mb, draw_id, self.B, bits.device)
        if mb_vec is not None:
            N.call('pnp_csmri_draw_thresholds_pp', self._h, _p(bits), _p(mb_vec), _p(draw_id), int(seed) & (2 ** 64 - 1),
                   int(step0) & 0xFFFFFFFF, int(nsteps), _p(step_dev), _p(out), _p(selbits), _stream())
            return out
        N.call('pnp_csmri_draw_thresholds', self._h, _p(bits), int(mb), int(seed) & (2 ** 64 - 1), int(step0) & 0xFFFFFFFF,
               int(nsteps), _p(step_dev), _p(out), _p(selbits), _stream())
        return out

    def sel_from_thresholds(self, bits, mbd, out=None):
        """mask o minibatch of one step (mbd: int64 [B, 2]) as an explicit transposed uint8 selector."""
        assert mbd.dtype == torch.int64 and tuple(mbd.shape) == (self.B, 2)
        out = out if out is not None else torch.empty((self.B, self.W, self.H), dtype=torch.uint8, device=bits.device)
        N.call('pnp_csmri_sel_from_thresholds', self._h, _p(bits), _p(mbd), _p(out), _stream())
        return out

    def draw_minibatch(self, bits, mb, seed, step, out=None, step_dev=None):
        """Device-side uniform draw of `mb` of each problem's sampled locations -> explicit transposed selector.
        bits: int32 [B, W, H/32] bit-packed mask (pack_mask)."""
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        out = out if out is not None else torch.empty((self.B, self.W, self.H), dtype=torch.uint8, device=bits.device)
        N.call('pnp_csmri_draw_minibatch', self._h, _p(bits), int(mb), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF,
               _p(step_dev), _p(out), _stream())
        return out

    def sel_from_dense(self, sel, out=None):
        assert sel.dtype == torch.uint8 and tuple(sel.shape) == (self.B, self.H, self.W)
        out = out if out is not None else torch.empty((self.B, self.W, self.H), dtype=torch.uint8, device=sel.device)
        N.call('pnp_csmri_sel_from_dense', self._h, _p(sel), _p(out), _stream())
        return out

    def pack_y(self, YT, selT, out=None):
        """YT: complex [B, W, H] (Y transposed); returns packed data term complex [B, W/2, H]."""
        assert YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H)
        out = out if out is not None else torch.empty((self.B, self.W // 2, self.H), dtype=YT.dtype, device=YT.device)
        N.call('pnp_csmri_pack_y', self._h, _p(YT), _p(selT), _p(out), _stream())
        return out

    def grad(self, a, selT=None, b=None, yh=None, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None, out=None, *,
             bits=None, alpha_vec=None, YT=None):
        """out = alpha * alpha_vec[b] * Re ifft2(sel o fft2(a - b) - sel o Y) + beta*c1 + gamma*c2.
        Selector: `selT` (explicit uint8 [B, W, H]) or `bits` (bit-packed int32 [B, W, H/32]: the mask, or one step's
        row of draw_thresholds' selbits).  Data term: `yh` (packed for this
        selector) or `YT` (complex [B, W, H], masked by the selector inside the kernel)."""
        for t in (a, b, c1, c2, out):
            assert t is None or (t.dtype == self.dtype and t.numel() == self.B * self.H * self.W)
        assert (selT is None) != (bits is None), 'pass selT or bits'
        assert alpha_vec is None or (alpha_vec.dtype == self.dtype and alpha_vec.numel() == self.B)
        out = out if out is not None else torch.empty_like(a)
        assert YT is None or (YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H))
        _route('pnp_csmri_grad_sel', [self._h, _p(a), _p(b), _p(selT), _p(bits), _p(yh), _p(YT), _pp(alpha, self.B), _p(alpha_vec),
                                      float(beta), _p(c1), _pp(gamma, self.B), _p(c2), _p(out), _stream()])
        return out

    def objective(self, z, YT, bits, scale, out=None):
        """pnp_csmri_objective: scale * sum over the full spectrum of mask |fft2(z) - Y|^2 per problem -> float64 [B].
        YT: complex [B, W, H] (Y transposed), bits: the bit-packed mask int32 [B, W, H/32]."""
        assert z.dtype == self.dtype and z.numel() == self.B * self.H * self.W
        assert YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H)
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        out = _f_out(out, self.B, z.device)
        N.call('pnp_csmri_objective', self._h, _p(z), _p(YT), _p(bits), float(scale), _p(out), _stream())
        return out

    def generate(self, images, image_idx, thresh, snr_fac, seed, item_id, with_mask=True):
        """pnp_csmri_generate: the B problems of this plan generated on the device from the counter-based stream of
        include/pnp_hip.h.  images: [n, H, W] of the plan's dtype (normalised); per item device vectors image_idx (int32),
        thresh (int64 holding T = floor(alpha 2^32)), snr_fac (float64, 10^(-snr/10)), seed, item_id (int64 holding the
        64-bit values).  Returns a dict of device tensors: xrec, bits, maskT (None without with_mask), YT, yh_full, xinit,
        M0 (int32), inv_m0, sigma (float64)."""
        B, H, W, dt, dev = self.B, self.H, self.W, self.dtype, images.device
        assert images.dtype == dt and images.dim() == 3 and tuple(images.shape[1:]) == (H, W)
        for t, d in ((image_idx, torch.int32), (thresh, torch.int64), (snr_fac, torch.float64), (seed, torch.int64),
                     (item_id, torch.int64)):
            assert t.dtype == d and tuple(t.shape) == (B,)
        o = dict(xrec=torch.empty((B, H, W), dtype=dt, device=dev),
                 bits=torch.empty((B, W, H // 32), dtype=torch.int32, device=dev),
                 maskT=torch.empty((B, W, H), dtype=torch.uint8, device=dev) if with_mask else None,
                 YT=torch.empty((B, W, H), dtype=_CDT[dt], device=dev),
                 yh_full=torch.empty((B, W // 2, H), dtype=_CDT[dt], device=dev),
                 xinit=torch.empty((B, H, W), dtype=dt, device=dev),
                 M0=torch.empty(B, dtype=torch.int32, device=dev),
                 inv_m0=torch.empty(B, dtype=dt, device=dev),
                 sigma=torch.empty(B, dtype=torch.float64, device=dev))
        N.call('pnp_csmri_generate', self._h, _p(images), images.shape[0], _p(image_idx), _p(thresh), _p(snr_fac), _p(seed),
               _p(item_id), _p(o['xrec']), _p(o['bits']), _p(o['maskT']), _p(o['YT']), _p(o['yh_full']), _p(o['xinit']),
               _p(o['M0']), _p(o['inv_m0']), _p(o['sigma']), _stream())
        return o

    def svrg_step(self, a, b, bits, alpha=1.0, beta=0.0, c1=None, gamma=0.0, c2=None, out=None, *, alpha_vec=None, denoise=True,
                  sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, sse=None, sigma_out=None):
        """pnp_csmri_svrg_step: gradient step + noise estimate (+ TV prox) + PSNR error of one inner iteration in ONE
        kernel (f32, 256 x 256).  out = prox_TV(alpha * Re ifft2(bits o fft2(a - b)) + beta*c1 + gamma*c2)."""
        assert self.dtype == torch.float32 and self.H == 256 and self.W == 256
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        out = out if out is not None else torch.empty_like(a)
        sigma_out = sigma_out if sigma_out is not None else torch.empty(self.B, dtype=a.dtype, device=a.device)
        _route('pnp_csmri_svrg_step', [self._h, _p(a), _p(b), _p(bits), _pp(alpha, self.B), _p(alpha_vec), float(beta), _p(c1),
                                       _pp(gamma, self.B), _p(c2), _p(out), _dn(denoise), _pp(sigma_modifier, self.B),
                                       float(fallback_sigma), _p(xrec), _p(sse), _p(sigma_out), _stream()])
        return out, sse, sigma_out

    def sarah_step(self, a, b, bits, alpha=1.0, beta=1.0, c1=None, gamma=0.0, c2=None, v_out=None, out=None, out2=None, *,
                   alpha_vec=None, denoise=True, sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, sse=None, sigma_out=None):
        """pnp_csmri_sarah_step: one inner iteration of pnp_sarah in ONE kernel (f32, 256 x 256):
        v_out = alpha * Re ifft2(bits o fft2(a - b)) + beta*c1 (stored), out = prox_TV(c2 + gamma * v_out), out2 = out.
        v_out may be c1, out may be c2, out2 may be b; denoise=False stores c2 + gamma * v_out and takes no out2.
        Returns (out, sse, sigma_out, v_out)."""
        if self.dtype != torch.float32 or self.H != 256 or self.W != 256:
            raise ValueError(f'sarah_step: the one-kernel iteration exists for float32 plans of 256 x 256 (this plan: {self.dtype}, '
                             f'{self.H} x {self.W})')
        if out2 is not None and not denoise:
            raise ValueError('sarah_step: out2 needs denoise=True (without the prox the stored image is not the iterate)')
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        assert c1 is not None and c2 is not None, 'sarah_step: c1 (v_prev) and c2 (z) are required'
        for t in (a, b, c1, c2, v_out, out, out2, xrec):
            assert t is None or (t.dtype == self.dtype and t.numel() == self.B * self.H * self.W)
        out = out if out is not None else torch.empty_like(a)
        v_out = v_out if v_out is not None else torch.empty_like(a)
        if any(v_out.data_ptr() == t.data_ptr() for t in (a, b, c2, out, out2) if t is not None):
            raise ValueError('sarah_step: v_out may alias c1 only (not a, b, c2, out or out2)')
        sigma_out = sigma_out if sigma_out is not None else torch.empty(self.B, dtype=a.dtype, device=a.device)
        _route('pnp_csmri_sarah_step', [self._h, _p(a), _p(b), _p(bits), _pp(alpha, self.B), _p(alpha_vec), float(beta), _p(c1),
                                        _pp(gamma, self.B), _p(c2), _p(v_out), _p(out), _p(out2), _dn(denoise),
                                        _pp(sigma_modifier, self.B), float(fallback_sigma), _p(xrec), _p(sse), _p(sigma_out),
                                        _stream()])
        return out, sse, sigma_out, v_out

    def _one_kernel_plan(self, what):
        if self.dtype != torch.float32 or self.H != 256 or self.W != 256:
            raise ValueError(f'{what}: the one-kernel iteration exists for float32 plans of 256 x 256 (this plan: {self.dtype}, '
                             f'{self.H} x {self.W})')

    def grad_step(self, a, bits, yh=None, YT=None, alpha=1.0, beta=1.0, c1=None, out=None, *, alpha_vec=None, denoise=True,
                  sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, sse=None, sigma_out=None):
        """pnp_csmri_grad_step: one GD or SGD inner iteration in ONE kernel (f32, 256 x 256):
        out = prox_TV(alpha * alpha_vec[b] * Re ifft2(bits o fft2(a) - bits o Y) + beta * c1).  Data term: `yh` (packed for `bits` = the
        mask: the GD step) or `YT` (complex [B, W, H], masked by `bits` = a drawn slot inside the kernel: the SGD step) -- exactly one.
        out may be a and c1; denoise=False stores the stepped image.  Returns (out, sse, sigma_out)."""
        self._one_kernel_plan('grad_step')
        if (yh is None) == (YT is None):
            raise ValueError('grad_step: pass the packed data term (yh) or the raw data (YT), exactly one of them')
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        assert c1 is not None, 'grad_step: c1 is required'
        for t in (a, c1, out, xrec):
            assert t is None or (t.dtype == self.dtype and t.numel() == self.B * self.H * self.W)
        assert YT is None or (YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H))
        assert yh is None or (yh.dtype == _CDT[self.dtype] and tuple(yh.shape) == (self.B, self.W // 2, self.H))
        out = out if out is not None else torch.empty_like(a)
        sigma_out = sigma_out if sigma_out is not None else torch.empty(self.B, dtype=a.dtype, device=a.device)
        _route('pnp_csmri_grad_step', [self._h, _p(a), _p(bits), _p(yh), _p(YT), _pp(alpha, self.B), _p(alpha_vec), float(beta), _p(c1),
                                       _p(out), _dn(denoise), _pp(sigma_modifier, self.B), float(fallback_sigma), _p(xrec),
                                       _p(sse), _p(sigma_out), _stream()])
        return out, sse, sigma_out

    def saga_step(self, z, bits, YT, table, row, prev_row, tsum, lr, inv_hist, alpha=1.0, out=None, *, alpha_vec=None, denoise=True,
                  sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, sse=None, sigma_out=None, inv_hist_pp=None):
        """pnp_csmri_saga_step: one SAGA inner iteration in ONE kernel (f32, 256 x 256): g = alpha * Re ifft2(bits o fft2(z) - bits o Y);
        s = tsum + g - table[row[b]][b]; out = prox_TV(z - lr * ((g - table[prev_row[b]][b]) + s * inv_hist)); table[row[b]][b] = g;
        tsum = s.  table: [hist, B, H, W]; row, prev_row: int32 [B] device tensors; out may be z.  Returns (out, sse, sigma_out).
        inv_hist_pp: a float64 [B] device tensor of per-problem divisors 1 / hist[b] -> pnp_csmri_saga_step_hist_pp (table: [max hist, B,
        H, W]); None: the calls above, unchanged."""
        self._one_kernel_plan('saga_step')
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (self.B, self.W, self.H // 32)
        assert YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H)
        for t in (z, tsum, out, xrec):
            assert t is None or (t.dtype == self.dtype and t.numel() == self.B * self.H * self.W)
        assert table.dtype == self.dtype and table.dim() >= 2 and table.shape[1] == self.B and table.numel() == table.shape[0] * z.numel()
        for rv in (row, prev_row):
            assert rv.dtype == torch.int32 and tuple(rv.shape) == (self.B,)
        out = out if out is not None else torch.empty_like(z)
        sigma_out = sigma_out if sigma_out is not None else torch.empty(self.B, dtype=z.dtype, device=z.device)
        if inv_hist_pp is not None:                             # (scalar, array or NULL) pairs: the entry point has the _pp form only
            a, l, sm, ih = _pp(alpha, self.B), _pp(lr, self.B), _pp(sigma_modifier, self.B), _pp(inv_hist_pp, self.B)
            assert ih[1] is not None, 'inv_hist_pp: a [B] float64 device tensor'
            N.call('pnp_csmri_saga_step_hist_pp', self._h, _p(z), _p(bits), _p(YT), a[0], _p(a[1]), _p(alpha_vec), _p(table), _p(row),
                   _p(prev_row), _p(tsum), l[0], _p(l[1]), float(inv_hist), _p(ih[1]), int(table.shape[0]), _p(out), _dn(denoise),
                   sm[0], _p(sm[1]), float(fallback_sigma), _p(xrec), _p(sse), _p(sigma_out), _stream())
            return out, sse, sigma_out
        _route('pnp_csmri_saga_step', [self._h, _p(z), _p(bits), _p(YT), _pp(alpha, self.B), _p(alpha_vec), _p(table), _p(row),
                                       _p(prev_row), _p(tsum), _pp(lr, self.B), float(inv_hist), int(table.shape[0]), _p(out),
                                       _dn(denoise), _pp(sigma_modifier, self.B), float(fallback_sigma), _p(xrec), _p(sse),
                                       _p(sigma_out), _stream()])
        return out, sse, sigma_out

    def svrg_outer_step(self, z, mask_bits, yh, alpha_vec, lr, w_out, mu_out, out=None, *, denoise=True, sigma_modifier=1.0,
                        fallback_sigma=0.0, xrec=None, sse=None, sigma_out=None):
        """pnp_csmri_svrg_outer_step: the outer refresh of pnp_svrg folded into its first inner iteration, one kernel:
        mu_out = alpha_vec[b] * Re ifft2(mask o fft2(z) - yh), w_out = z, out = prox_TV(z - lr * mu_out)."""
        assert self.dtype == torch.float32 and self.H == 256 and self.W == 256
        assert mask_bits.dtype == torch.int32 and tuple(mask_bits.shape) == (self.B, self.W, self.H // 32)
        for t in (z, w_out, mu_out, out):
            assert t is None or (t.dtype == self.dtype and t.numel() == self.B * self.H * self.W)
        out = out if out is not None else torch.empty_like(z)
        sigma_out = sigma_out if sigma_out is not None else torch.empty(self.B, dtype=z.dtype, device=z.device)
        _route('pnp_csmri_svrg_outer_step', [self._h, _p(z), _p(mask_bits), _p(yh), _p(alpha_vec), _pp(lr, self.B), _p(w_out),
                                             _p(mu_out), _p(out), _dn(denoise), _pp(sigma_modifier, self.B),
                                             float(fallback_sigma), _p(xrec), _p(sse), _p(sigma_out), _stream()])
        return out, sse, sigma_out

    def svrg_outer_iteration(self, z, w, mu, mask_bits, yh, alpha_vec, selbits, T2, lr, mini_batch_size, xrec, sse_log, log_row0,
                             sigma_out, *, sigma_modifier=1.0, fallback_sigma=0.0, prox_kind=1):
        """pnp_csmri_svrg_outer_iteration: refresh + T2 inner iterations with the TV prox in ONE launch (z in place; w, mu out).
        prox_kind: 1 = the per-column prox (the calls above, unchanged); 2 = the 2-D wavelet prox inside the kernel
        (pnp_csmri_svrg_outer_iteration_prox)."""
        if prox_kind not in (1, 2):
            raise ValueError(f'svrg_outer_iteration: prox_kind must be 1 (per-column) or 2 (2-D wavelet), not {prox_kind!r}')
        assert self.dtype == torch.float32 and self.H == 256 and self.W == 256
        for t in (z, w, mu, xrec):
            assert t.dtype == self.dtype and t.numel() == self.B * self.H * self.W
        assert selbits.dtype == torch.int32 and tuple(selbits.shape) == (T2, self.B, self.W, self.H // 32)
        assert sse_log.dtype == torch.float64 and sse_log.dim() == 2 and sse_log.shape[1] == self.B and sse_log.is_contiguous()
        if prox_kind == 2:                                      # (scalar, array or NULL) pairs: the entry point has the _pp form only
            l, mb, sm = _pp(lr, self.B), _pp(mini_batch_size, self.B, torch.int32), _pp(sigma_modifier, self.B)
            N.call('pnp_csmri_svrg_outer_iteration_prox', self._h, _p(z), _p(w), _p(mu), _p(mask_bits), _p(yh), _p(alpha_vec), _p(selbits),
                   int(T2), l[0], _p(l[1]), mb[0], _p(mb[1]), sm[0], _p(sm[1]), float(fallback_sigma), _p(xrec), _p(sse_log),
                   int(log_row0), int(sse_log.shape[0]), _p(sigma_out), 2, _stream())
            return
        _route('pnp_csmri_svrg_outer_iteration',
               [self._h, _p(z), _p(w), _p(mu), _p(mask_bits), _p(yh), _p(alpha_vec), _p(selbits), int(T2), _pp(lr, self.B),
                _pp(mini_batch_size, self.B, torch.int32), _pp(sigma_modifier, self.B), float(fallback_sigma), _p(xrec), _p(sse_log),
                int(log_row0), int(sse_log.shape[0]), _p(sigma_out), _stream()])

    def svrg_span(self, z, w, mu, mask_bits, yh, alpha_vec, selbits, step0, n_steps, T2, lr, mini_batch_size, xrec, sse_log, log_row0,
                  sigma_out, *, sigma_modifier=1.0, fallback_sigma=0.0):
        """pnp_csmri_svrg_span_pp: inner iterations step0 .. step0 + n_steps - 1 with the TV prox in ONE launch, every problem
        refreshing at the steps its own T2 names (z in place; w, mu updated where a problem refreshes).  T2: an int32 [B] device
        tensor (or an int); selbits: int32 [>= n_steps, B, W, H/32], slot i = step step0 + i."""
        assert self.dtype == torch.float32 and self.H == 256 and self.W == 256
        for t in (z, w, mu, xrec):
            assert t.dtype == self.dtype and t.numel() == self.B * self.H * self.W
        assert selbits.dtype == torch.int32 and selbits.shape[0] >= n_steps and tuple(selbits.shape[1:]) == (self.B, self.W, self.H // 32)
        assert sse_log.dtype == torch.float64 and sse_log.dim() == 2 and sse_log.shape[1] == self.B and sse_log.is_contiguous()
        args = [self._h, _p(z), _p(w), _p(mu), _p(mask_bits), _p(yh), _p(alpha_vec), _p(selbits), int(step0), int(n_steps)]
        for v in (_pp(T2, self.B, torch.int32), _pp(lr, self.B), _pp(mini_batch_size, self.B, torch.int32), _pp(sigma_modifier, self.B)):
            args += (v[0], _p(v[1]))                            # (scalar, array or NULL): the entry point has the _pp form only
        N.call('pnp_csmri_svrg_span_pp', *args, float(fallback_sigma), _p(xrec), _p(sse_log), int(log_row0), int(sse_log.shape[0]),
               _p(sigma_out), _stream())

    def _span_log(self, what, sse_log, sigma_out, *images):
        """What the one-launch forms share: a float32 256 x 256 plan, whole-batch images, the [n_log, B] float64 log ring."""
        self._one_kernel_plan(what)
        for t in images:
            assert t.dtype == self.dtype and t.numel() == self.B * self.H * self.W
        assert sse_log.dtype == torch.float64 and sse_log.dim() == 2 and sse_log.shape[1] == self.B and sse_log.is_contiguous()
        assert sigma_out.dtype == self.dtype and sigma_out.numel() == self.B

    def sarah_outer_iteration(self, z, w_prev, w_next, v_prev, mask_bits, yh, alpha_vec, selbits, T2, eta, lr, mini_batch_size, xrec,
                              sse_log, log_row0, sigma_out, *, sigma_modifier=1.0, fallback_sigma=0.0):
        """pnp_csmri_sarah_outer_iteration: the outer step of pnp_sarah (w_prev = z, v_prev = grad_full(z), w_next = prox_TV(z - eta *
        v_prev); z not written) + T2 inner iterations with the TV prox in ONE launch (z, w_prev, v_prev in place; w_next out).  T2 + 1
        log rows from log_row0 on.  eta, lr, mini_batch_size, sigma_modifier: scalars, or [B] device tensors (float64; int32 for
        mini_batch_size) -> the _pp entry point."""
        self._span_log('sarah_outer_iteration', sse_log, sigma_out, z, w_prev, w_next, v_prev, xrec)
        assert mask_bits.dtype == torch.int32 and tuple(mask_bits.shape) == (self.B, self.W, self.H // 32)
        assert selbits.dtype == torch.int32 and tuple(selbits.shape) == (T2, self.B, self.W, self.H // 32)
        if len({t.data_ptr() for t in (z, w_prev, w_next, v_prev)}) != 4:
            raise ValueError('sarah_outer_iteration: z, w_prev, w_next and v_prev must be buffers of their own')
        _route('pnp_csmri_sarah_outer_iteration',
               [self._h, _p(z), _p(w_prev), _p(w_next), _p(v_prev), _p(mask_bits), _p(yh), _p(alpha_vec), _p(selbits), int(T2),
                _pp(eta, self.B), _pp(lr, self.B), _pp(mini_batch_size, self.B, torch.int32), _pp(sigma_modifier, self.B),
                float(fallback_sigma), _p(xrec), _p(sse_log), int(log_row0), int(sse_log.shape[0]), _p(sigma_out), _stream()])

    def sarah_span(self, z, w_prev, w_next, v_prev, mask_bits, yh, alpha_vec, selbits, step0, n_steps, T2, eta, lr, mini_batch_size,
                   xrec, sse_log, outer_log, log_row0, sigma_out, *, sigma_modifier=1.0, fallback_sigma=0.0):
        """pnp_csmri_sarah_span_pp: inner iterations step0 .. step0 + n_steps - 1 of pnp_sarah with the TV prox in ONE launch, every
        problem taking its outer step (w_prev = z, v_prev = grad_full(z), w_next = prox_TV(z - eta * v_prev)) at the steps its own T2
        names.  T2: an int32 [B] device tensor (or an int); selbits: int32 [>= n_steps, B, W, H/32], slot i = step step0 + i; sse_log
        and outer_log: float64 [n_log, B] rings of their own, row (log_row0 + i) % n_log (outer_log: NaN where no outer step was made).
        eta, lr, mini_batch_size, sigma_modifier: scalars or [B] device tensors."""
        self._span_log('sarah_span', sse_log, sigma_out, z, w_prev, w_next, v_prev, xrec)
        assert mask_bits.dtype == torch.int32 and tuple(mask_bits.shape) == (self.B, self.W, self.H // 32)
        assert selbits.dtype == torch.int32 and selbits.shape[0] >= n_steps and tuple(selbits.shape[1:]) == (self.B, self.W, self.H // 32)
        assert outer_log.dtype == torch.float64 and outer_log.shape == sse_log.shape and outer_log.is_contiguous()
        if len({t.data_ptr() for t in (z, w_prev, w_next, v_prev)}) != 4:
            raise ValueError('sarah_span: z, w_prev, w_next and v_prev must be buffers of their own')
        args = [self._h, _p(z), _p(w_prev), _p(w_next), _p(v_prev), _p(mask_bits), _p(yh), _p(alpha_vec), _p(selbits), int(step0),
                int(n_steps)]
        for v in (_pp(T2, self.B, torch.int32), _pp(eta, self.B), _pp(lr, self.B), _pp(mini_batch_size, self.B, torch.int32),
                  _pp(sigma_modifier, self.B)):
            args += (v[0], _p(v[1]))                            # (scalar, array or NULL): the entry point has the _pp form only
        N.call('pnp_csmri_sarah_span_pp', *args, float(fallback_sigma), _p(xrec), _p(sse_log), _p(outer_log), int(log_row0),
               int(sse_log.shape[0]), _p(sigma_out), _stream())

    def grad_span(self, z, bits, n_steps, xrec, sse_log, log_row0, sigma_out, *, yh=None, YT=None, alpha=1.0, beta=1.0, alpha_vec=None,
                  sigma_modifier=1.0, fallback_sigma=0.0):
        """pnp_csmri_grad_span: n_steps GD or SGD inner iterations with the TV prox in ONE launch, z in place.  yh with bits = the mask
        [B, W, H/32] (GD, the same at every step) or YT with bits = drawn selbits [>= n_steps, B, W, H/32], slot i = step i (SGD) --
        exactly one.  alpha, sigma_modifier: scalars or [B] float64 device tensors.  n_steps log rows from log_row0 on."""
        self._span_log('grad_span', sse_log, sigma_out, z, xrec)
        if (yh is None) == (YT is None):
            raise ValueError('grad_span: pass the packed data term (yh) or the raw data (YT), exactly one of them')
        assert bits.dtype == torch.int32
        if yh is not None:
            assert tuple(bits.shape) == (self.B, self.W, self.H // 32)
            assert yh.dtype == _CDT[self.dtype] and tuple(yh.shape) == (self.B, self.W // 2, self.H)
        else:
            assert bits.dim() == 4 and bits.shape[0] >= n_steps and tuple(bits.shape[1:]) == (self.B, self.W, self.H // 32)
            assert YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H)
        assert alpha_vec is None or (alpha_vec.dtype == self.dtype and alpha_vec.numel() == self.B)
        a, sm = _pp(alpha, self.B), _pp(sigma_modifier, self.B)  # (scalar, array or NULL): the entry point has the _pp form only
        N.call('pnp_csmri_grad_span', self._h, _p(z), _p(bits), _p(yh), _p(YT), a[0], _p(a[1]), _p(alpha_vec), float(beta), 1, sm[0],
               _p(sm[1]), float(fallback_sigma), _p(xrec), int(n_steps), _p(sse_log), int(log_row0), int(sse_log.shape[0]),
               _p(sigma_out), _stream())

    def saga_span(self, z, bits, YT, table, rows, prev_row0, tsum, lr, inv_hist, n_steps, xrec, sse_log, log_row0, sigma_out, *,
                  alpha=1.0, alpha_vec=None, sigma_modifier=1.0, fallback_sigma=0.0, inv_hist_pp=None):
        """pnp_csmri_saga_span: n_steps SAGA inner iterations with the TV prox in ONE launch; table, tsum and z in place.  bits: drawn
        selbits [>= n_steps, B, W, H/32], slot i = step i; rows: int32 [n_steps, B] device tensor (step i replaces rows[i][b]);
        prev_row0: int32 [B] (the row the step before the span replaced).  Row values must lie in [0, hist): the caller checks its
        host copy.  alpha, lr, sigma_modifier: scalars or [B] float64 device tensors.  inv_hist_pp: a float64 [B] device tensor of
        per-problem divisors 1 / hist[b] -> pnp_csmri_saga_span_hist (table: [max hist, B, H, W]); None: the call above, unchanged."""
        self._span_log('saga_span', sse_log, sigma_out, z, tsum, xrec)
        assert bits.dtype == torch.int32 and bits.dim() == 4 and bits.shape[0] >= n_steps
        assert tuple(bits.shape[1:]) == (self.B, self.W, self.H // 32)
        assert YT.dtype == _CDT[self.dtype] and tuple(YT.shape) == (self.B, self.W, self.H)
        assert table.dtype == self.dtype and table.dim() >= 2 and table.shape[1] == self.B and table.numel() == table.shape[0] * z.numel()
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (n_steps, self.B)
        assert prev_row0.dtype == torch.int32 and tuple(prev_row0.shape) == (self.B,)
        assert alpha_vec is None or (alpha_vec.dtype == self.dtype and alpha_vec.numel() == self.B)
        a, l, sm = _pp(alpha, self.B), _pp(lr, self.B), _pp(sigma_modifier, self.B)
        if inv_hist_pp is not None:
            ih = _pp(inv_hist_pp, self.B)
            assert ih[1] is not None, 'inv_hist_pp: a [B] float64 device tensor'
            N.call('pnp_csmri_saga_span_hist', self._h, _p(z), _p(bits), _p(YT), a[0], _p(a[1]), _p(alpha_vec), _p(table), _p(rows),
                   _p(prev_row0), _p(tsum), l[0], _p(l[1]), float(inv_hist), _p(ih[1]), int(table.shape[0]), 1, sm[0], _p(sm[1]),
                   float(fallback_sigma), _p(xrec), int(n_steps), _p(sse_log), int(log_row0), int(sse_log.shape[0]), _p(sigma_out),
                   _stream())
            return
        N.call('pnp_csmri_saga_span', self._h, _p(z), _p(bits), _p(YT), a[0], _p(a[1]), _p(alpha_vec), _p(table), _p(rows), _p(prev_row0),
               _p(tsum), l[0], _p(l[1]), float(inv_hist), int(table.shape[0]), 1, sm[0], _p(sm[1]), float(fallback_sigma), _p(xrec),
               int(n_steps), _p(sse_log), int(log_row0), int(sse_log.shape[0]), _p(sigma_out), _stream())


class DncnnPlan:
    """pnp_dncnn_plan_*: DnCNN-17 prox for B images of H x W (fp32 network on the f32 matrix cores).

    `weights`: dict of NumPy arrays in the reference's layer order -- conv{i}.weight (i = 0..n-1) and
    bn{i}.{weight,bias,mean,var} for the middle layers -- exactly what tests/golden/dncnn_noise15.npz
    holds or what `load_dncnn_state_dict` extracts from a reference .pth.  BatchNorm (eval) is folded here.
    Optional `conv{i}.bias` arrays (any layer), `negative_slope` (LeakyReLU instead of ReLU) and
    `transpose_taps` (every 3x3 kernel transposed) cover the MMO `simple_CNN` (denoisers/MMODenoise.py:73-101)."""

    def __init__(self, weights, H, W, batch, winograd=None):
        """winograd: 5 = Winograd F(4x4,3x3) conv kernel (default where H % 8 == 0 and W % 64 == 0; fp32, a quarter of the
        matrix-core work), True / 1 = F(2,3) along x (two thirds; the default elsewhere), False / 0 = direct implicit GEMM
        (bit-for-bit an fmaf chain), 6 = opt-in F(4x4,3x3) on the bf16 matrix cores with three-way exact splits (fp32-class accuracy,
        currently slower than 5), None = env PNP_DNCNN_WINOGRAD or the default."""
        import numpy as np
        require_gpu()
        n = int(weights['n_layers'])
        self.H, self.W, self.B, self.n_mid = H, W, batch, n - 2
        tr = bool(weights.get('transpose_taps', False))

        def taps(name, shape):
            w = np.asarray(weights[name], dtype=np.float64).reshape(shape + (3, 3))
            return (w.swapaxes(-1, -2) if tr else w).reshape(shape + (9,))

        w_first = np.ascontiguousarray(taps('conv0.weight', (64,)), dtype=np.float32)
        w_last = np.ascontiguousarray(taps(f'conv{n - 1}.weight', (64,)), dtype=np.float32)
        w_mid = np.empty((n - 2, 64, 64, 9), dtype=np.float32)
        b_mid = np.zeros((n - 2, 64), dtype=np.float32)
        for i in range(1, n - 1):
            w = taps(f'conv{i}.weight', (64, 64))
            b = np.asarray(weights[f'conv{i}.bias'], np.float64) if f'conv{i}.bias' in weights else np.zeros(64)
            if f'bn{i}.weight' in weights:
                s = np.asarray(weights[f'bn{i}.weight'], np.float64) / np.sqrt(np.asarray(weights[f'bn{i}.var'], np.float64) + 1e-5)
                w = w * s[:, None, None]
                b = np.asarray(weights[f'bn{i}.bias'], np.float64) + (b - np.asarray(weights[f'bn{i}.mean'], np.float64)) * s
            b_mid[i - 1] = b
            w_mid[i - 1] = w
        h = ctypes.c_void_p()
        N.call('pnp_dncnn_plan_create', ctypes.byref(h), n - 2, w_first.ctypes.data_as(ctypes.c_void_p),
               w_mid.ctypes.data_as(ctypes.c_void_p), b_mid.ctypes.data_as(ctypes.c_void_p),
               w_last.ctypes.data_as(ctypes.c_void_p), H, W, batch)
        self._h = h
        slope = float(weights.get('negative_slope', 0.0))
        if slope != 0.0 or 'conv0.bias' in weights or f'conv{n - 1}.bias' in weights:
            b_first = np.ascontiguousarray(weights.get('conv0.bias', np.zeros(64)), dtype=np.float32)
            b_last = float(np.asarray(weights.get(f'conv{n - 1}.bias', 0.0)).reshape(-1)[0])
            N.call('pnp_dncnn_set_affine', self._h, b_first.ctypes.data_as(ctypes.c_void_p), b_last, slope)
        if winograd is not None:
            N.call('pnp_dncnn_set_winograd', self._h, int(winograd))

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                N.lib().pnp_dncnn_plan_destroy(h)
            except Exception:
                pass

    def profile_begin(self, max_calls=4096):
        N.call('pnp_dncnn_profile_begin', self._h, int(max_calls))

    def profile_end(self):
        """-> (mean ms of one 64->64 conv launch, number of launches timed)"""
        ms, n = ctypes.c_double(), ctypes.c_long()
        N.call('pnp_dncnn_profile_end', self._h, ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    def debug_w44_weights(self, layer):
        """packed F(4x4,3x3) weights of one middle layer as a device tensor (test hook)"""
        n = N.lib().pnp_dncnn_debug_w44_floats()
        dst = torch.empty(n, dtype=torch.float32, device='cuda')
        N.call('pnp_dncnn_debug_w44_weights', self._h, int(layer), _p(dst), _stream())
        return dst

    def debug_mid_layer(self, layer, x, out, w44=None, rows=0):
        """one 64->64 layer on caller-provided activations [B,64,H,W] (test hook: guard bands around the buffers)"""
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, 64, self.H, self.W) and tuple(out.shape) == tuple(x.shape)
        N.call('pnp_dncnn_debug_mid_layer', self._h, int(layer), _p(x), _p(out), _p(w44), int(rows), _stream())
        return out

    def debug_fused_last(self, x, part, rows=0):
        """the last middle layer with the output conv fused in, on caller-provided buffers (test hook): x [B,64,H,W] ->
        part [B,H/4,W/4,6,6], the output partials of every 4 x 4 block (pixel (4 by + py - 1, 4 bx + px - 1))"""
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, 64, self.H, self.W)
        assert part.dtype == torch.float32 and part.numel() == self.B * (self.H // 4) * (self.W // 4) * 36
        N.call('pnp_dncnn_debug_fused_last', self._h, _p(x), _p(part), int(rows), _stream())
        return part

    def forward(self, x, out=None):
        """raw network residual; x: float32 [B,H,W]."""
        assert x.dtype == torch.float32 and tuple(x.shape) == (self.B, self.H, self.W)
        out = out if out is not None else torch.empty_like(x)
        N.call('pnp_dncnn_forward', self._h, _p(x), _p(out), _stream())
        return out

    def denoise(self, z, sigma_net, xrec=None, out=None, sse=None):
        assert tuple(z.shape) == (self.B, self.H, self.W)
        out = out if out is not None else torch.empty_like(z)
        if xrec is not None and sse is None:
            sse = torch.empty(self.B, dtype=torch.float64, device=z.device)
        N.call('pnp_dncnn_denoise', self._h, _p(z), _p(out), _DT[z.dtype], float(sigma_net), _p(xrec), _p(sse), _stream())
        return out, sse


    def mmo_denoise(self, z, xrec=None, out=None, sse=None):
        """pnp_mmo_denoise: clip(xc + net(xc), 0, 1), xc = clip(z, 0, 1) (reference MMODenoise.py:18-40,88-101)."""
        assert tuple(z.shape) == (self.B, self.H, self.W)
        out = out if out is not None else torch.empty_like(z)
        if xrec is not None and sse is None:
            sse = torch.empty(self.B, dtype=torch.float64, device=z.device)
        N.call('pnp_mmo_denoise', self._h, _p(z), _p(out), _DT[z.dtype], _p(xrec), _p(sse), _stream())
        return out, sse


def sigma_est(z, out=None):
    """z: [B, H, W] -> [B] (estimate_sigma(multichannel=True, average_sigmas=True))."""
    require_gpu()
    B, H, W = z.shape
    out = out if out is not None else torch.empty(B, dtype=z.dtype, device=z.device)
    N.call('pnp_sigma_est', _p(z), H, W, B, _DT[z.dtype], _p(out), _stream())
    return out


def _prox(name, z, sigma_in, sigma_modifier, fallback_sigma, xrec, out, sse, sigma_out):
    """prox_tv / prox_wavelet2d: two entry points with one signature (sigma_modifier: a scalar, or float64 [B] per problem)."""
    require_gpu()
    B, H, W = z.shape
    out = out if out is not None else torch.empty_like(z)
    if xrec is not None and sse is None:
        sse = torch.empty(B, dtype=torch.float64, device=z.device)
    sigma_out = sigma_out if sigma_out is not None else torch.empty(B, dtype=z.dtype, device=z.device)
    _route(name, [_p(z), _p(out), H, W, B, _DT[z.dtype], _p(sigma_in), _pp(sigma_modifier, B), float(fallback_sigma), _p(xrec),
                  _p(sse), _p(sigma_out), _stream()])
    return out, sse, sigma_out


def prox_tv(z, sigma_in=None, sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, out=None, sse=None, sigma_out=None):
    """Fused estimate_sigma + Haar-BayesShrink prox (+ squared error vs xrec).
    Returns (denoised [B,H,W], sse [B] float64 or None, sigma_est [B])."""
    return _prox('pnp_prox_tv', z, sigma_in, sigma_modifier, fallback_sigma, xrec, out, sse, sigma_out)


def prox_wavelet2d(z, sigma_in=None, sigma_modifier=1.0, fallback_sigma=0.0, xrec=None, out=None, sse=None, sigma_out=None):
    """Fused estimate_sigma + 2-D multi-level Haar BayesShrink prox (TVDenoiser(multi=False)) (+ squared error vs xrec).
    Signature and result of `prox_tv`: (denoised [B,H,W], sse [B] float64 or None, sigma_est [B])."""
    return _prox('pnp_prox_wavelet2d', z, sigma_in, sigma_modifier, fallback_sigma, xrec, out, sse, sigma_out)


def sse(z, xrec, out=None):
    require_gpu()
    B = z.shape[0]
    out = out if out is not None else torch.empty(B, dtype=torch.float64, device=z.device)
    N.call('pnp_sse', _p(z), _p(xrec), z.numel() // B, B, _DT[z.dtype], _p(out), _stream())
    return out


def minmax(z):
    require_gpu()
    B = z.shape[0]
    out = torch.empty((B, 2), dtype=z.dtype, device=z.device)
    N.call('pnp_minmax', _p(z), z.numel() // B, B, _DT[z.dtype], _p(out), _stream())
    return out


def axpbypcz(a, x, b=0.0, y=None, c=0.0, w=None, out=None):
    """out = a * x + b * y + c * w (y, w may be None; out may be x, y or w).  a, b, c: scalars -- the plain pnp_axpbypcz call -- or
    float64 [B] device tensors with B = x.shape[0]: problem p = x[p] takes its own value, ONE pnp_axpbypcz_pp launch, bit for bit
    the plain call on p's views with float(coef[p])."""
    require_gpu()
    out = out if out is not None else torch.empty_like(x)
    B = x.shape[0] if x.dim() else 1
    args = [_pp(a, B), _p(x), _pp(b, B), _p(y), _pp(c, B), _p(w), _p(out), x.numel(), _DT[x.dtype], _stream()]
    if any(v[1] is not None for v in args[0:5:2]):              # the `_pp` call alone takes the number of problems, behind n
        args.insert(8, int(B))
    _route('pnp_axpbypcz', args)
    return out


def refresh_pp(mu_new, z, mu, w, t2_vec, step):
    """pnp_refresh_pp: mu[p] = mu_new[p], w[p] = z[p] for every problem p = row p of the [B, ...] tensors with step % t2_vec[p] == 0
    (t2_vec: int32 [B] device tensor, entries >= 1; step: a host int); the other problems' mu and w stay untouched.  ONE launch."""
    require_gpu()
    B = z.shape[0]
    assert t2_vec.dtype == torch.int32 and tuple(t2_vec.shape) == (B,), f'per-problem T2: an int32 [{B}] device tensor'
    for t in (mu_new, mu, w):
        assert t.dtype == z.dtype and t.shape == z.shape
    N.call('pnp_refresh_pp', _p(mu_new), _p(z), _p(mu), _p(w), _p(t2_vec), int(step), z.numel(), int(B), _DT[z.dtype], _stream())


def select_pp(src, dst, t2_vec, step, row_in=None, row_out=None):
    """pnp_select_pp: dst[p] = src[p] and row_out[p] = row_in[p] for every problem p = row p of the [B, ...] tensors with
    step % t2_vec[p] == 0; the other problems' dst stays untouched and their row_out[p] becomes NaN (t2_vec: int32 [B] device tensor,
    entries >= 1; step: a host int; row_in, row_out: float64 [B], both or neither).  ONE launch."""
    require_gpu()
    B = src.shape[0]
    assert t2_vec.dtype == torch.int32 and tuple(t2_vec.shape) == (B,), f'per-problem T2: an int32 [{B}] device tensor'
    assert dst.dtype == src.dtype and dst.shape == src.shape
    if (row_in is None) != (row_out is None):
        raise ValueError('select_pp: row_in and row_out go together (both or neither)')
    for r in (row_in, row_out):
        assert r is None or (r.dtype == torch.float64 and tuple(r.shape) == (B,) and r.is_contiguous())
    N.call('pnp_select_pp', _p(src), _p(dst), _p(row_in), _p(row_out), _p(t2_vec), int(step), src.numel(), int(B), _DT[src.dtype], _stream())


_NLM_W0 = {}


def _nlm_w0(side, device):
    """exp(-(x^2+y^2)/(2A^2)), A=(side-1)/4, and its NumPy sum (skimage non_local_means.py:150-153)."""
    key = (side, str(device))
    if key not in _NLM_W0:
        import numpy as np
        off = side // 2
        A = (side - 1.0) / 4.0
        g = np.arange(-off, off + 1)
        gr, gc = np.meshgrid(g, g, indexing='ij')
        w = np.exp(-(gr * gr + gc * gc) / (2 * A * A))
        _NLM_W0[key] = (torch.from_numpy(np.ascontiguousarray(w.ravel())).to(device), float(np.sum(w)))
    return _NLM_W0[key]


def nlm2d(z, sigma_in=None, sigma_modifier=1.0, fixed_h=0.0, patch_size=4, patch_distance=5, xrec=None, out=None, sse=None):
    """skimage denoise_nl_means(slow mode) semantics on [B,H,W]; returns (denoised, sse or None).
    sigma_modifier: a scalar, or a float64 [B] device tensor (per image: pnp_nlm2d_pp)."""
    B, H, W = z.shape
    side = patch_size + 1 if patch_size % 2 == 0 else patch_size
    if min(H, W) < side // 2 + 1:                               # nlm2d() in nlm.hip refuses it too: the border is reflected once
        raise N.NativeError(f'pnp_nlm2d: H and W must be at least {side // 2 + 1} for patch side {side} (got {H} x {W})')
    require_gpu()
    w0, w0_sum = _nlm_w0(side, z.device)
    out = out if out is not None else torch.empty_like(z)
    ws = None
    if xrec is not None:
        sse = sse if sse is not None else torch.empty(B, dtype=torch.float64, device=z.device)
        ws = torch.empty(B * ((H + 15) // 16) * ((W + 15) // 16), dtype=torch.float64, device=z.device)
    _route('pnp_nlm2d', [_p(z), _p(out), H, W, B, _DT[z.dtype], int(patch_size), int(patch_distance), _p(sigma_in),
                         _pp(sigma_modifier, B), float(fixed_h), _p(w0), w0_sum, _p(xrec), _p(sse), _p(ws), _stream()])
    return out, sse


class DeblurPlan:
    """pnp_deblur_plan_*: B^T S^T (S B z - y) for B problems of H x W (H*W in {4096, 65536})."""

    def __init__(self, H, W, batch, dtype, Bk, bilinear=None):
        import numpy as np
        require_gpu()
        self.H, self.W, self.N, self.B, self.dtype = H, W, H * W, batch, dtype
        npdt = np.float32 if dtype == torch.float32 else np.float64
        Bk = np.ascontiguousarray(Bk, dtype=npdt)
        self._Bk, self._bilinear = Bk, bilinear                 # (host arrays: what `resized` builds the next plan from)
        h = ctypes.c_void_p()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if bilinear is None:
            self.M = self.N
            N.call('pnp_deblur_plan_create', ctypes.byref(h), H, W, batch, _DT[dtype], vp(Bk), self.M, None, None, None, None, None)
        else:
            g_idx, g_w, a_rowptr, a_col, a_val = bilinear
            self.M = g_idx.shape[0]
            keep = [np.ascontiguousarray(g_idx, np.int32), np.ascontiguousarray(g_w, npdt), np.ascontiguousarray(a_rowptr, np.int32),
                    np.ascontiguousarray(a_col, np.int32), np.ascontiguousarray(a_val, npdt)]
            N.call('pnp_deblur_plan_create', ctypes.byref(h), H, W, batch, _DT[dtype], vp(Bk), self.M, *[vp(k) for k in keep])
        self._h = h

    M_vec = None                                                # mixed-scale plans: the per-problem measurement counts (host int32 [B])

    @classmethod
    def mixed(cls, H, W, dtype, Bk, sets, set_of, M_vec, device='cuda'):
        """pnp_deblur_plan_create_mixed: a plan whose problems each have a down-sampler of their own.  sets, set_of, M_vec: what
        `problems.deblur_operator_sets` returns (the distinct down-samplers, problem -> set, problem -> M_b).  M is Mmax = max M_b:
        Y, sel and the forward output are [B, Mmax], entries m >= M_b of a row are padding."""
        require_gpu()
        self = cls.__new__(cls)
        set_of, M_vec = np.ascontiguousarray(set_of, np.int32), np.ascontiguousarray(M_vec, np.int32)
        batch = int(set_of.shape[0])
        self.H, self.W, self.N, self.B, self.dtype = H, W, H * W, batch, dtype
        npdt = np.float32 if dtype == torch.float32 else np.float64
        Bk = np.ascontiguousarray(Bk, dtype=npdt)
        self._Bk, self._bilinear, self._sets, self._set_of = Bk, None, list(sets), set_of
        self.M_vec, self.M = M_vec, int(M_vec.max())
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
        taps = [t for _, _, t in sets if t is not None]
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(t[k]).reshape(-1) for t in taps]), dt) if taps else None
        M_set = np.array([m for _, m, _ in sets], np.int32)
        g_off = np.cumsum([0] + [0 if t is None else t[0].shape[0] for _, _, t in sets]).astype(np.int32)
        nz_off = np.cumsum([0] + [0 if t is None else t[3].shape[0] for _, _, t in sets]).astype(np.int32)
        keep = [cat(0, np.int32), cat(1, npdt), nz_off, cat(2, np.int32), cat(3, np.int32), cat(4, npdt)]
        h = ctypes.c_void_p()
        N.call('pnp_deblur_plan_create_mixed', ctypes.byref(h), H, W, batch, _DT[dtype], vp(Bk), len(sets), vp(M_set), vp(g_off),
               *[vp(k) for k in keep], vp(set_of), vp(M_vec))
        self._h = h
        self.M_dev = torch.from_numpy(M_vec).to(device)          # what the draws and indicators take
        return self

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                N.lib().pnp_deblur_plan_destroy(h)
            except Exception:
                pass

    def grad(self, z, Y, sel=None, scale=1.0, out=None, mbd=None):
        """scale * B^T S^T (sel o (S B z - Y)); sel: uint8 [B, M] indicator, or mbd: int64 [B, 2] = one step's
        device-drawn minibatch descriptors (draw_thresholds), or neither (all measurements).
        scale: a scalar, or a float64 [B] device tensor (per problem: pnp_deblur_grad_pp / pnp_deblur_grad_mb_pp)."""
        assert z.dtype == self.dtype and z.numel() == self.B * self.N and Y.numel() == self.B * self.M
        assert sel is None or mbd is None
        out = out if out is not None else torch.empty_like(z)
        if self.M_vec is not None:                              # mixed scales: one entry point takes the scalar and the array
            assert Y.dtype == self.dtype and (sel is None or (sel.dtype == torch.uint8 and sel.numel() == self.B * self.M))
            sc = _pp(scale, self.B)
            if mbd is not None:
                assert mbd.dtype == torch.int64 and tuple(mbd.shape) == (self.B, 2)
                N.call('pnp_deblur_grad_mb_mixed', self._h, _p(z), _p(Y), _p(mbd), sc[0], _p(sc[1]), _p(out), _stream())
            else:
                N.call('pnp_deblur_grad_mixed', self._h, _p(z), _p(Y), _p(sel), sc[0], _p(sc[1]), _p(out), _stream())
            return out
        if mbd is not None:
            assert mbd.dtype == torch.int64 and tuple(mbd.shape) == (self.B, 2)
            _route('pnp_deblur_grad_mb', [self._h, _p(z), _p(Y), _p(mbd), _pp(scale, self.B), _p(out), _stream()])
        else:
            _route('pnp_deblur_grad', [self._h, _p(z), _p(Y), _p(sel), _pp(scale, self.B), _p(out), _stream()])
        return out

    def grad_step(self, a, b=None, Y=None, sel=None, mbd=None, scale=1.0, beta=0.0, c1=None, gamma=0.0, c2=None, out=None):
        """pnp_deblur_grad_step: beta * c1 + gamma * c2 + scale * B^T S^T (sel o (S B (a - b) - Y)) in one gradient pass (DESIGN
        9.12).  b, Y, c1, c2: None = absent; sel / mbd as in `grad`; scale, gamma: a scalar or a float64 [B] device tensor (per
        problem).  out may be a, b, c1 or c2.  Uniform plans only."""
        assert a.dtype == self.dtype and a.numel() == self.B * self.N and (Y is None or Y.numel() == self.B * self.M)
        assert sel is None or mbd is None
        if self.M_vec is not None:
            raise ValueError('grad_step: a mixed-scale plan has no one-pass step (uniform plans only)')
        assert mbd is None or (mbd.dtype == torch.int64 and tuple(mbd.shape) == (self.B, 2))
        for t in (b, c1, c2):
            assert t is None or (t.dtype == self.dtype and t.numel() == a.numel())
        assert (Y is None or Y.dtype == self.dtype) and (sel is None or (sel.dtype == torch.uint8 and sel.numel() == self.B * self.M))
        out = out if out is not None else torch.empty_like(a)
        assert out.dtype == self.dtype and out.numel() == a.numel()
        sc, ga = _pp(scale, self.B), _pp(gamma, self.B)
        N.call('pnp_deblur_grad_step', self._h, _p(a), _p(b), _p(Y), _p(sel), _p(mbd), sc[0], _p(sc[1]), float(beta), _p(c1),
               ga[0], _p(ga[1]), _p(c2), _p(out), _stream())
        return out

    def resized(self, batch):
        """A plan for `batch` problems on this plan's kernel spectrum and down-sampler (DeblurBatch.tile).  A mixed-scale plan
        repeats its problems' sets: batch = n * B, problem t * B + i on the set of problem i."""
        if self.M_vec is not None:
            n, r = divmod(int(batch), self.B)
            if n < 1 or r:
                raise ValueError(f'a mixed-scale plan of {self.B} problems resizes to multiples of {self.B}, got {batch}')
            return DeblurPlan.mixed(self.H, self.W, self.dtype, self._Bk, self._sets, np.tile(self._set_of, n), np.tile(self.M_vec, n),
                                    device=self.M_dev.device)
        return DeblurPlan(self.H, self.W, int(batch), self.dtype, self._Bk, bilinear=self._bilinear)

    def forward(self, x, out=None):
        out = out if out is not None else torch.empty(self.B * self.M, dtype=self.dtype, device=x.device)
        if self.M_vec is not None:                              # mixed scales: out [B, Mmax], zero in the padding
            assert x.dtype == self.dtype and out.dtype == self.dtype and x.numel() == self.B * self.N and out.numel() == self.B * self.M
            N.call('pnp_deblur_forward_mixed', self._h, _p(x), _p(out), _stream())
            return out
        N.call('pnp_deblur_forward', self._h, _p(x), _p(out), _stream())
        return out

    def objective(self, z, Y, scale, out=None):
        """pnp_deblur_objective: scale * sum over the M measurements of (S B z - Y)^2 per problem -> float64 [B].  A mixed-scale
        plan (pnp_deblur_objective_mixed) sums over m < M_b and divides `scale` by M_b itself: pass 1/2 for f."""
        assert z.dtype == self.dtype and Y.dtype == self.dtype and z.numel() == self.B * self.N and Y.numel() == self.B * self.M
        out = _f_out(out, self.B, z.device)
        N.call('pnp_deblur_objective_mixed' if self.M_vec is not None else 'pnp_deblur_objective', self._h, _p(z), _p(Y), float(scale),
               _p(out), _stream())
        return out

    def generate(self, images, image_idx, snr_fac, seed, item_id):
        """pnp_deblur_generate: the B problems of this plan generated on the device from the counter-based stream of
        include/pnp_hip.h.  images: [n, H, W] of the plan's dtype (normalised); per item device vectors image_idx (int32),
        snr_fac (float64, 10^(-snr/10)), seed, item_id (int64 holding the 64-bit values).  Returns a dict of device tensors:
        xrec [B, H, W], Y [B, M], xinit [B, H, W], sigma [B] (float64)."""
        B, dt, dev = self.B, self.dtype, images.device
        assert images.dtype == dt and images.dim() == 3 and tuple(images.shape[1:]) == (self.H, self.W) and images.is_contiguous()
        _check_item_vectors(B, image_idx, snr_fac, seed, item_id)
        o = dict(xrec=torch.empty((B, self.H, self.W), dtype=dt, device=dev), Y=torch.empty((B, self.M), dtype=dt, device=dev),
                 xinit=torch.empty((B, self.H, self.W), dtype=dt, device=dev), sigma=torch.empty(B, dtype=torch.float64, device=dev))
        N.call('pnp_deblur_generate', self._h, _p(images), images.shape[0], _p(image_idx), _p(snr_fac), _p(seed), _p(item_id),
               _p(o['xrec']), _p(o['Y']), _p(o['xinit']), _p(o['sigma']), _stream())
        return o


def _check_item_vectors(B, image_idx, snr_fac, seed, item_id):
    for t, d in ((image_idx, torch.int32), (snr_fac, torch.float64), (seed, torch.int64), (item_id, torch.int64)):
        assert t.dtype == d and tuple(t.shape) == (B,)


def pr_generate(images, image_idx, snr_fac, seed, item_id, M):
    """pnp_pr_generate: B phase-retrieval problems with M measurements each generated on the device from the counter-based
    stream of include/pnp_hip.h.  images: [n, H, W] (normalised; its dtype is the problems'); per item device vectors as in
    DeblurPlan.generate.  Returns a dict of device tensors: A [B, M, H*W], xrec [B, H, W], Y [B, M], sigma [B] (float64)."""
    require_gpu()
    B, dt, dev = image_idx.shape[0], images.dtype, images.device
    assert images.dim() == 3 and images.is_contiguous()
    _check_item_vectors(B, image_idx, snr_fac, seed, item_id)
    H, W = int(images.shape[1]), int(images.shape[2])
    if int(M) * H * W > 2 ** 32:
        raise ValueError(f'M * N = {int(M) * H * W} > 2^32: the matrix stream has a 32-bit pair index')
    o = dict(A=torch.empty((B, int(M), H * W), dtype=dt, device=dev), xrec=torch.empty((B, H, W), dtype=dt, device=dev),
             Y=torch.empty((B, int(M)), dtype=dt, device=dev), sigma=torch.empty(B, dtype=torch.float64, device=dev))
    N.call('pnp_pr_generate', _p(images), images.shape[0], _p(image_idx), _p(snr_fac), _p(seed), _p(item_id), H, W, int(M), B,
           _DT[dt], _p(o['A']), _p(o['xrec']), _p(o['Y']), _p(o['sigma']), _stream())
    return o


def pr_spectral_init_batch(A, Y, xrec, max_iters=1000, check_every=8):
    """pnp_pr_spectral_init_batch: PhaseRetrieval.spec_init + min-max normalisation (PR.py:50-63, :38) of B problems at once,
    the stopping rule evaluated per item on the device; one host synchronisation per `check_every` steps.  A [B, M, N],
    Y [B, M], xrec [B, ...] of one dtype.  Returns (xinit like xrec, iters int32 [B], active int32 [B]): `active` is nonzero
    for an item that had not met its rule after `max_iters` steps."""
    require_gpu()
    B, M, Nn = A.shape
    assert Y.dtype == A.dtype and xrec.dtype == A.dtype and tuple(Y.shape) == (B, M) and xrec.numel() == B * Nn
    ws = torch.empty(N.lib().pnp_pr_spectral_workspace_bytes(M, Nn, B) // 8, dtype=torch.float64, device=A.device)
    xinit = torch.empty_like(xrec)
    iters = torch.empty(B, dtype=torch.int32, device=A.device)
    active = torch.empty(B, dtype=torch.int32, device=A.device)
    N.call('pnp_pr_spectral_init_batch', _p(A), _p(Y), _p(xrec), M, Nn, B, _DT[A.dtype], int(max_iters), int(check_every), _p(ws),
           _p(xinit), _p(iters), _p(active), _stream())
    return xinit, iters, active


def pr_workspace(M, Nn, dtype, device, B=1):
    """Scratch of the pnp_pr_* gradient / spectral kernels for B problems of an M x Nn matrix."""
    return torch.empty(B * N.lib().pnp_pr_workspace_elems(M, Nn), dtype=dtype, device=device)


def pr_grad(A, w, y, rows=None, scale=1.0, workspace=None, out=None):
    """scale * A_sel^T(((|A_sel w| - y_sel)/|A_sel w|) o A_sel w); A [M,N], rows int32 [nsel] or None."""
    require_gpu()
    M, Nn = A.shape
    if workspace is None:
        workspace = pr_workspace(M, Nn, A.dtype, A.device)
    out = out if out is not None else torch.empty(Nn, dtype=A.dtype, device=A.device)
    nsel = M if rows is None else rows.numel()
    N.call('pnp_pr_grad', _p(A), _p(w), _p(y), _p(rows), nsel, M, Nn, _DT[A.dtype], float(scale), _p(workspace), _p(out), _stream())
    return out


def pr_grad_batch(A, w, y, rows=None, scale=1.0, workspace=None, out=None):
    """B independent problems: A [B,M,N], w [B,N], y [B,M], rows int32 [B,nsel] or None -> [B,N]."""
    require_gpu()
    B, M, Nn = A.shape
    if workspace is None:
        workspace = pr_workspace(M, Nn, A.dtype, A.device, B)
    out = out if out is not None else torch.empty((B, Nn), dtype=A.dtype, device=A.device)
    nsel = M if rows is None else rows.shape[1]
    N.call('pnp_pr_grad_batch', _p(A), _p(w), _p(y), _p(rows), nsel, M, Nn, B, _DT[A.dtype], float(scale), _p(workspace),
           _p(out), _stream())
    return out


def pr_shared_workspace(M, Nn, dtype, device, B):
    """Scratch of pnp_pr_grad_shared for B problems on shared M x Nn matrices (any number of items)."""
    return torch.empty(N.lib().pnp_pr_shared_workspace_elems(M, Nn, B), dtype=dtype, device=device)


def pr_grad_shared(A, Y, W, W2=None, mbd=None, ind=None, alpha=1.0, alpha_div=1.0, beta=0.0, c1=None, gamma=0.0, c2=None,
                   workspace=None, out=None):
    """B = G * items problems on `items` shared matrices (problem b works on A[b % items], Y[b % items]): A [items, M, N],
    Y [items, M], W, W2 (or None), c1, c2 (or None), out [B, N]:
        out[b] = (alpha_b / alpha_div) * (g_b(W[b]) - g_b(W2[b])) + beta * c1[b] + gamma_b * c2[b]
    alpha, gamma: scalars, or float64 [B] device tensors (per problem).  Rows per problem: mbd (int64 [B, 2], one step's device-drawn
    descriptors), ind (uint8 [B, M]) or neither (all rows).  out may alias W, c1 or c2."""
    require_gpu()
    items, M, Nn = A.shape
    B = W.numel() // Nn
    for t in (Y, W, W2, c1, c2, out):
        assert t is None or t.dtype == A.dtype
    assert B * Nn == W.numel() and Y.numel() == items * M and all(t is None or t.numel() == B * Nn for t in (W2, c1, c2, out))
    assert mbd is None or (mbd.dtype == torch.int64 and tuple(mbd.shape) == (B, 2))
    assert ind is None or (ind.dtype == torch.uint8 and tuple(ind.shape) == (B, M))
    if workspace is None:
        workspace = pr_shared_workspace(M, Nn, A.dtype, A.device, B)
    assert workspace.dtype == A.dtype and workspace.numel() >= N.lib().pnp_pr_shared_workspace_elems(M, Nn, B)
    out = out if out is not None else torch.empty((B, Nn), dtype=A.dtype, device=A.device)
    _route('pnp_pr_grad_shared', [_p(A), _p(Y), _p(W), _p(W2), _p(mbd), _p(ind), M, Nn, B, items, _DT[A.dtype], _pp(alpha, B),
                                  float(alpha_div), float(beta), _p(c1), _pp(gamma, B), _p(c2), _p(workspace), _p(out), _stream()])
    return out


def pr_objective_workspace(M, B, device):
    """Scratch of pnp_pr_objective for B problems of M measurements (float64: the per-workgroup partial sums)."""
    return torch.empty(max(1, N.lib().pnp_pr_objective_workspace_bytes(int(M), int(B)) // 8), dtype=torch.float64, device=device)


def pr_objective(A, w, y, scale, workspace=None, out=None):
    """pnp_pr_objective: scale * sum over the M rows of (|A w| - y)^2 per problem -> float64 [B].  A [n_mat, M, N] with n_mat == B
    or a divisor of B (problem b works on A[b % n_mat]: the tiled batches of pr_grad_shared); w [B, N]; y [B, M]."""
    require_gpu()
    n_mat, M, Nn = A.shape
    B = w.numel() // Nn
    assert w.dtype == A.dtype and y.dtype == A.dtype and w.numel() == B * Nn and y.numel() == B * M
    if B % n_mat != 0:
        raise ValueError(f'pr_objective: {B} problems on {n_mat} matrices (the number of matrices must divide the batch)')
    if workspace is None:
        workspace = pr_objective_workspace(M, B, A.device)
    assert workspace.dtype == torch.float64 and workspace.numel() * 8 >= N.lib().pnp_pr_objective_workspace_bytes(M, B)
    out = _f_out(out, B, A.device)
    N.call('pnp_pr_objective', _p(A), _p(w), _p(y), M, Nn, B, n_mat, _DT[A.dtype], float(scale), _p(workspace), _p(out), _stream())
    return out


def draw_thresholds(M, B, mb, seed, step0, nsteps=1, out=None, step_dev=None, device='cuda', draw_id=None):
    """Device-side draws of `mb` of M measurements for B problems and `nsteps` steps -> descriptors int64 [nsteps, B, 2].
    mb: an int, or an int32 [B] device tensor; draw_id: int32 [B] ids absorbed in place of the batch index (pnp_draw_thresholds_pp)."""
    require_gpu()
    out = out if out is not None else torch.empty((nsteps, B, 2), dtype=torch.int64, device=device)
    mb_vec = _mb_vec(mb, draw_id, B, out.device)
    if mb_vec is not None:
        N.call('pnp_draw_thresholds_pp', int(M), int(B), _p(mb_vec), _p(draw_id), int(seed) & (2 ** 64 - 1), int(step0) & 0xFFFFFFFF,
               int(nsteps), _p(step_dev), _p(out), _stream())
        return out
    N.call('pnp_draw_thresholds', int(M), int(B), int(mb), int(seed) & (2 ** 64 - 1), int(step0) & 0xFFFFFFFF, int(nsteps),
           _p(step_dev), _p(out), _stream())
    return out


def indicator_from_thresholds(M, mbd, out=None):
    require_gpu()
    B = mbd.shape[0]
    out = out if out is not None else torch.empty((B, M), dtype=torch.uint8, device=mbd.device)
    N.call('pnp_indicator_from_thresholds', int(M), int(B), _p(mbd), _p(out), _stream())
    return out


def draw_thresholds_mpp(M_vec, mb, seed, step0, nsteps=1, out=None, step_dev=None, draw_id=None, seed_vec=None):
    """pnp_draw_thresholds_mpp: `draw_thresholds` with a population per problem (mixed-scale Deblur batches) -- problem b draws
    mb_b of its M_vec[b] measurements (M_vec: int32 [B] device tensor) -> descriptors int64 [nsteps, B, 2], problem b's equal to
    those of draw_thresholds(M_vec[b], ...) with the same id, mb, seed and step.  seed_vec: int64 [B] device tensor holding
    64-bit seeds; problem b's stream then absorbs seed_vec[b] in place of `seed`."""
    require_gpu()
    assert M_vec.dtype == torch.int32 and M_vec.dim() == 1
    B = M_vec.shape[0]
    out = out if out is not None else torch.empty((nsteps, B, 2), dtype=torch.int64, device=M_vec.device)
    if not isinstance(mb, torch.Tensor):
        mb = torch.full((B,), int(mb), dtype=torch.int32, device=M_vec.device)
    assert mb.dtype == torch.int32 and tuple(mb.shape) == (B,) and tuple(out.shape[1:]) == (B, 2) and out.shape[0] >= nsteps
    assert draw_id is None or (draw_id.dtype == torch.int32 and tuple(draw_id.shape) == (B,))
    assert seed_vec is None or (seed_vec.dtype == torch.int64 and tuple(seed_vec.shape) == (B,))
    N.call('pnp_draw_thresholds_mpp', _p(M_vec), int(B), _p(mb), _p(draw_id), int(seed) & (2 ** 64 - 1), _p(seed_vec), int(step0) & 0xFFFFFFFF,
           int(nsteps), _p(step_dev), _p(out), _stream())
    return out


def indicator_from_thresholds_m(M_vec, Mmax, mbd, out=None):
    """pnp_indicator_from_thresholds_m: uint8 [B, Mmax], problem b's minibatch among m < M_vec[b], zero in the padding."""
    require_gpu()
    B = mbd.shape[0]
    assert M_vec.dtype == torch.int32 and tuple(M_vec.shape) == (B,)
    out = out if out is not None else torch.empty((B, Mmax), dtype=torch.uint8, device=mbd.device)
    N.call('pnp_indicator_from_thresholds_m', _p(M_vec), int(Mmax), int(B), _p(mbd), _p(out), _stream())
    return out


def rows_from_thresholds(M, mb, mbd, out=None):
    require_gpu()
    B = mbd.shape[0]
    out = out if out is not None else torch.empty((B, mb), dtype=torch.int32, device=mbd.device)
    N.call('pnp_rows_from_thresholds', int(M), int(B), int(mb), _p(mbd), _p(out), _stream())
    return out


def indicator_from_indices(idx, M, out=None):
    """idx int32 [B, n] -> uint8 [B, M] (Problem.select_mb's 0/1 indicator, problems/problem.py:110-117)."""
    require_gpu()
    assert idx.dtype == torch.int32
    B, n = idx.shape
    out = out if out is not None else torch.empty((B, M), dtype=torch.uint8, device=idx.device)
    N.call('pnp_indicator_from_indices', _p(idx), int(n), int(M), int(B), _p(out), _stream())
    return out


def saga_table_update(z, g, slot, prev, tsum, lr, inv_hist):
    """pnp_saga_table_update: one SAGA step over all elements (z, slot, tsum updated in place)."""
    require_gpu()
    for t in (g, slot, prev, tsum):
        assert t.dtype == z.dtype and t.numel() == z.numel()
    N.call('pnp_saga_table_update', _p(z), _p(g), _p(slot), _p(prev), _p(tsum), float(lr), float(inv_hist), z.numel(),
           _DT[z.dtype], _stream())


def saga_table_update_pp(z, g, table, row, prev_row, tsum, lr, inv_hist, inv_hist_pp=None):
    """pnp_saga_table_update_pp: one SAGA step of a whole batch in ONE launch.  z, g, tsum [B, ...]; table [hist, B, ...]; row, prev_row:
    int32 [B] device tensors (problem b replaces table[row[b], b]; its previous step wrote table[prev_row[b], b]); lr: a scalar, or
    a float64 [B] device tensor.  inv_hist_pp: a float64 [B] device tensor of per-problem divisors 1 / hist[b] ->
    pnp_saga_table_update_hist_pp (table [max hist, B, ...]); None: the call above, unchanged."""
    require_gpu()
    B, hist = z.shape[0], table.shape[0]
    n = z.numel() // B
    for t in (g, tsum):
        assert t.dtype == z.dtype and t.numel() == z.numel()
    assert table.dtype == z.dtype and table.numel() == hist * z.numel() and table.shape[1] == B
    for t in (row, prev_row):
        assert t.dtype == torch.int32 and tuple(t.shape) == (B,)
    lr = _pp(lr, B)
    if inv_hist_pp is not None:
        ih = _pp(inv_hist_pp, B)
        assert ih[1] is not None, 'inv_hist_pp: a [B] float64 device tensor'
        N.call('pnp_saga_table_update_hist_pp', _p(z), _p(g), _p(table), _p(row), _p(prev_row), _p(tsum), lr[0], _p(lr[1]), float(inv_hist),
               _p(ih[1]), int(hist), int(B), int(n), _DT[z.dtype], _stream())
        return
    N.call('pnp_saga_table_update_pp', _p(z), _p(g), _p(table), _p(row), _p(prev_row), _p(tsum), lr[0], _p(lr[1]), float(inv_hist),
           int(hist), int(B), int(n), _DT[z.dtype], _stream())


def pr_spectral_apply(A, v, y, scale=1.0, workspace=None, out=None):
    """scale * A^T (y o (A v)): one power-iteration step of the PR spectral initialisation; A [M,N]."""
    require_gpu()
    M, Nn = A.shape
    if workspace is None:
        workspace = pr_workspace(M, Nn, A.dtype, A.device)
    out = out if out is not None else torch.empty(Nn, dtype=A.dtype, device=A.device)
    N.call('pnp_pr_spectral_apply', _p(A), _p(v), _p(y), M, Nn, _DT[A.dtype], float(scale), _p(workspace), _p(out), _stream())
    return out


def counter_add(counter, inc=1):
    """counter: int32 device tensor with one element (device-resident step counter)."""
    require_gpu()
    N.call('pnp_counter_add', _p(counter), int(inc), _stream())


def log_append(src, log, step_dev):
    """log[(step % n_log)] = src; src: float64 [n], log: float64 [n_log, n], step_dev: device counter."""
    require_gpu()
    N.call('pnp_log_append', _p(src), src.numel(), _p(log), log.shape[0], _p(step_dev), _stream())


def log_append_inc(src, log, counter):
    """log[(counter % n_log)] = src; counter += 1 (one launch; counter: int32 device tensor with one element)."""
    require_gpu()
    N.call('pnp_log_append_inc', _p(src), src.numel(), _p(log), log.shape[0], _p(counter), _stream())
