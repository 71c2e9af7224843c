"""CPU-only checks of the 2-D wavelet prox inside the one-kernel CSMRI iteration: the new symbol
pnp_csmri_svrg_outer_iteration_prox in the header, in `_native`'s table and in the built library; the PNP_ERR_ARG answers to
`denoise = 2` of the multi-step entry points (made before any device work, on a plan filled on the host as in
test_cpu_outer_forms.py); the attribute semantics of TVProx(in_kernel=...); `make_prox` passing the keyword through; what `ops` hands
to the library for `denoise`."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = 'pnp_csmri_svrg_outer_iteration_prox'


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_symbol_exported_declared_and_bound():
    from pnp_svrg_amd import _native, ops
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    assert hasattr(h, NEW) and NEW in _native.SIGNATURES and f'int {NEW}(' in hdr
    # the argument list of the _pp entry point plus `int denoise` in front of the stream
    pp = _native.SIGNATURES['pnp_csmri_svrg_outer_iteration_pp'][1]
    assert _native.SIGNATURES[NEW][1] == pp[:-1] + [ctypes.c_int] + pp[-1:]
    assert 'prox_kind' in ops.CsmriPlan.svrg_outer_iteration.__kwdefaults__
    assert ops.CsmriPlan.svrg_outer_iteration.__kwdefaults__['prox_kind'] == 1


class _Plan(ctypes.Structure):
    """The fields of csrc/csmri_plan.h, filled on the host: enough for the argument checks, which answer before any of the device
    pointers is used."""
    _fields_ = [('H', ctypes.c_int), ('W', ctypes.c_int), ('batch', ctypes.c_int), ('dtype', ctypes.c_int), ('NL', ctypes.c_int),
                ('work', ctypes.c_void_p), ('twtab', ctypes.c_void_p), ('mbd', ctypes.c_void_p), ('fused_min_batch', ctypes.c_int)]


def test_multi_step_entry_points_refuse_denoise_2():
    from pnp_svrg_amd import _native
    lib = _lib()
    plan = _Plan(256, 256, 2, _native.F32, 16, None, None, None, 192)
    h = ctypes.cast(ctypes.pointer(plan), ctypes.c_void_p)
    # distinct non-NULL addresses that are never dereferenced: images 1 MiB apart, the table far from them
    P = lambda k: ctypes.c_void_p(0x10000000 + k * 0x100000)
    z, bits, yt, yh, tsum, xrec, log, sig, rows, prev, ih, table = (P(k) for k in range(12))
    table = ctypes.c_void_p(0x40000000)
    calls = {
        'pnp_csmri_grad_span': lambda d: (h, z, bits, yh, None, -1.0, None, None, 1.0, d, 1.0, None, 0.0, xrec, 1, log, 0, 2, sig, None),
        'pnp_csmri_saga_span': lambda d: (h, z, bits, yt, 1e-3, None, None, table, rows, prev, tsum, 1.0, None, 0.5, 2, d, 1.0, None, 0.0,
                                          xrec, 1, log, 0, 2, sig, None),
        'pnp_csmri_saga_span_hist': lambda d: (h, z, bits, yt, 1e-3, None, None, table, rows, prev, tsum, 1.0, None, 0.5, ih, 2, d, 1.0,
                                               None, 0.0, xrec, 1, log, 0, 2, sig, None),
        'pnp_csmri_saga_step_hist_pp': lambda d: (h, z, bits, yt, 1e-3, None, None, table, rows, prev, tsum, 1.0, None, 0.5, ih, 2, z, d,
                                                  1.0, None, 0.0, xrec, log, sig, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args(2)) == 1, name          # PNP_ERR_ARG
        assert b'denoise' in lib.pnp_last_error(), name
    # the new entry point takes 1 or 2 only
    for d in (0, 3, -1):
        assert getattr(lib, NEW)(h, z, tsum, xrec, bits, yh, sig, rows, 2, 1.0, None, 100, None, 1.0, None, 0.0, xrec, log, 0, 2, sig, d,
                                 None) == 1
        assert b'denoise' in lib.pnp_last_error()
    # ... and checks the rest as the _pp call does: z, w and mu must be buffers of their own, with either prox kind
    for d in (1, 2):
        assert getattr(lib, NEW)(h, z, z, xrec, bits, yh, sig, rows, 2, 1.0, None, 100, None, 1.0, None, 0.0, xrec, log, 0, 2, sig, d,
                                 None) == 1
        assert b'buffers of their own' in lib.pnp_last_error()


def test_tvprox_attribute_semantics():
    from pnp_svrg_amd.engine import TVProx
    from pnp_svrg_amd import engine
    d = TVProx()
    assert d.multi and d.fused_denoise and not d.in_kernel and d.fused_kind == 1
    two = TVProx(multi=False)
    assert not two.multi and not two.fused_denoise and not two.in_kernel          # the default: today's two-launch behaviour
    ink = TVProx(multi=False, in_kernel=True, sigma_modifier=1.2, denoise_strength=0.05, decay=0.9)
    assert not ink.multi and ink.fused_denoise and ink.in_kernel and ink.fused_kind == 2 and ink.inplace
    for bad in (dict(multi=True, in_kernel=True), dict(in_kernel=True)):
        with pytest.raises(ValueError, match='multi=False'):
            TVProx(**bad)
    assert [engine._fused_kind(p) for p in (d, two, ink)] == [1, 0, 2]
    assert [engine._in_kernel_2d(p) for p in (d, two, ink)] == [False, False, True]
    # the in-kernel prox advances its step count in fused_args, as the per-column prox does, and after_fused does nothing
    ink.sig = None
    kw = ink.fused_args()
    assert ink.t == 1 and kw['sigma_modifier'] == 1.2 and kw['fallback_sigma'] == 0.05 * 0.9
    marker = object()
    assert ink.after_fused(marker, None, None) is marker and ink.t == 1
    two.sig = None
    assert two.fused_args() == dict(sigma_out=None) and two.t == 0


def test_make_prox_passes_the_keyword_through():
    from pnp_svrg_amd import sweep
    p = sweep.make_prox('tv', multi=False, in_kernel=True)
    assert p.fused_denoise and p.fused_kind == 2
    assert not sweep.make_prox('tv', multi=False).fused_denoise
    with pytest.raises(ValueError, match='multi=False'):
        sweep.make_prox('tv', in_kernel=True)


def test_ops_hands_denoise_through_as_0_1_2():
    from pnp_svrg_amd import ops
    assert [ops._dn(v) for v in (False, 0, True, 1, 2, 3)] == [0, 0, 1, 1, 2, 1]
