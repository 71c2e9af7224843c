"""CPU-only checks of the mixed-scale Deblur batches: the operator sets, the new symbols, and every refusal that is
raised before any device work."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = ['pnp_deblur_plan_create_mixed', 'pnp_deblur_grad_mixed', 'pnp_deblur_grad_mb_mixed', 'pnp_deblur_forward_mixed',
         'pnp_deblur_objective_mixed', 'pnp_draw_thresholds_mpp', 'pnp_indicator_from_thresholds_m']


def _lib():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.lib()


def test_operator_sets_dedupe_order_and_counts():
    from pnp_svrg_amd.problems import deblur_operator_sets, _deblur_taps
    sets, set_of, M_vec = deblur_operator_sets(64, 64, [50, 10, 100, 75, 50, 10])
    assert [s[0] for s in sets] == [50, 10, 100, 75]            # distinct, in order of first appearance
    assert [s[1] for s in sets] == [1024, 36, 4096, 2304]
    assert set_of.dtype == np.int32 and set_of.tolist() == [0, 1, 2, 3, 0, 1]
    assert M_vec.dtype == np.int32 and M_vec.tolist() == [1024, 36, 4096, 2304, 1024, 36]
    assert sets[2][2] is None                                   # 100: the identity, no tables
    for sp, M, taps in sets:
        if sp == 100:
            continue
        ref = _deblur_taps(64, 64, sp)
        assert taps[0].shape == (M, 4) and all(np.array_equal(a, b) for a, b in zip(taps, ref))
    # scale 75: adjoint rows with up to 4 entries (the CSR sum has an order)
    assert int(np.diff(sets[3][2][2]).max()) == 4
    with pytest.raises(ValueError, match='scale_percent'):
        deblur_operator_sets(64, 64, [50, 101])
    with pytest.raises(ValueError, match='at least one'):
        deblur_operator_sets(64, 64, [])


def test_mixed_symbols_exported_and_declared():
    from pnp_svrg_amd import _native
    h = ctypes.CDLL(_lib()._name)
    hdr = open(os.path.join(ROOT, 'include', 'pnp_hip.h')).read()
    for name in MIXED:
        assert hasattr(h, name) and name in _native.SIGNATURES and f'int {name}(' in hdr, name


def _create_args(n_sets=2, M_set=(36, 4096), set_of=(0, 1), M_vec=(36, 4096), bad_idx=False, bad_col=False):
    from pnp_svrg_amd.problems import _deblur_taps
    g_idx, g_w, rp, col, val = _deblur_taps(64, 64, 10)
    g_idx, col = g_idx.copy(), col.copy()
    if bad_idx:
        g_idx[5, 2] = 4096
    if bad_col:
        col[7] = 36
    arr = [np.zeros(4096), np.array(M_set, np.int32), np.array([0, 36, 36], np.int32), np.ascontiguousarray(g_idx, np.int32),
           np.ascontiguousarray(g_w, np.float64), np.array([0, len(col), len(col)], np.int32), np.ascontiguousarray(rp, np.int32),
           np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float64), np.array(set_of, np.int32),
           np.array(M_vec, np.int32)]
    return arr


def _create(h, arr, H=64, W=64, batch=2, n_sets=2, null=None):
    vp = [a.ctypes.data_as(ctypes.c_void_p) for a in arr]
    if null is not None:
        vp[null] = None
    out = ctypes.c_void_p()
    return h.pnp_deblur_plan_create_mixed(ctypes.byref(out), H, W, batch, 1, vp[0], n_sets, *vp[1:])


def test_create_mixed_argument_errors_without_gpu():
    """PNP_ERR_ARG (1), each raised before any device work (this machine has no GPU: a device call would fail otherwise)."""
    h = _lib()
    for null in (0, 1, 2, 5, 9, 10):                            # Bk, M_set, g_off, nz_off, set_of, M_vec
        assert _create(h, _create_args(), null=null) == 1 and b'null' in h.pnp_last_error()
    assert _create(h, _create_args(), null=3) == 1 and b'five arrays' in h.pnp_last_error()
    assert _create(h, _create_args(set_of=(0, 2))) == 1 and b'set_of out of range' in h.pnp_last_error()
    assert _create(h, _create_args(set_of=(0, -1))) == 1 and b'set_of out of range' in h.pnp_last_error()
    assert _create(h, _create_args(M_vec=(36, 1024))) == 1 and b'M_vec' in h.pnp_last_error()
    assert _create(h, _create_args(M_set=(36, 4097), M_vec=(36, 4097))) == 1 and b'M_s outside' in h.pnp_last_error()
    assert _create(h, _create_args(M_set=(0, 4096), M_vec=(0, 4096))) == 1 and b'M_s outside' in h.pnp_last_error()
    assert _create(h, _create_args(M_set=(36, 1024), M_vec=(36, 1024))) == 1 and b'identity' in h.pnp_last_error()
    assert _create(h, _create_args(bad_idx=True)) == 1 and b'g_idx outside' in h.pnp_last_error()
    assert _create(h, _create_args(bad_col=True)) == 1 and b'a_col outside' in h.pnp_last_error()
    assert _create(h, _create_args(), H=60) == 1 and b'H*W' in h.pnp_last_error()


def test_mixed_entry_points_null_arguments_without_gpu():
    h = _lib()
    one = ctypes.c_void_p(1)
    assert h.pnp_deblur_grad_mixed(None, one, one, None, 1.0, None, one, None) == 1 and b'null' in h.pnp_last_error()
    assert h.pnp_deblur_grad_mb_mixed(None, one, one, one, 1.0, None, one, None) == 1 and b'null' in h.pnp_last_error()
    assert h.pnp_deblur_forward_mixed(None, one, one, None) == 1 and b'null' in h.pnp_last_error()
    assert h.pnp_deblur_objective_mixed(None, one, one, 0.5, one, None) == 1 and b'null' in h.pnp_last_error()
    assert h.pnp_draw_thresholds_mpp(None, 2, one, None, 1, None, 0, 1, None, one, None) == 1 and b'null' in h.pnp_last_error()
    assert h.pnp_draw_thresholds_mpp(one, 2, None, None, 1, None, 0, 1, None, one, None) == 1
    assert h.pnp_draw_thresholds_mpp(one, 2, one, None, 1, None, 0, 0, None, one, None) == 1           # nsteps >= 1
    assert h.pnp_indicator_from_thresholds_m(None, 64, 2, one, one, None) == 1
    assert h.pnp_indicator_from_thresholds_m(one, 0, 2, one, one, None) == 1


def test_deblur_batch_refusals_before_device_work():
    """The mixed constructor checks its host arguments before it touches the device."""
    import torch
    from pnp_svrg_amd.batches import DeblurBatch
    x = np.zeros((2, 64, 64))
    Bk = np.zeros(4096)
    with pytest.raises(ValueError, match='2 scale_percent values'):
        DeblurBatch(x, Bk, [np.zeros(36)], x.reshape(2, -1), dtype=torch.float64, scale_percent=[10])
    with pytest.raises(ValueError, match=r'must hold \[36, 4096\] entries'):
        DeblurBatch(x, Bk, [np.zeros(36), np.zeros(1024)], x.reshape(2, -1), dtype=torch.float64, scale_percent=[10, 100])
    with pytest.raises(ValueError, match=r'padded Y must be \[2, 4096\]'):
        DeblurBatch(x, Bk, np.zeros((2, 1024)), x.reshape(2, -1), dtype=torch.float64, scale_percent=[10, 100])
    with pytest.raises(ValueError, match='not both'):
        DeblurBatch(x, Bk, [np.zeros(36), np.zeros(4096)], x.reshape(2, -1), dtype=torch.float64, scale_percent=[10, 100],
                    bilinear=(None,) * 5)
    with pytest.raises(ValueError, match='scale_percent must be an integer'):
        DeblurBatch(x, Bk, [np.zeros(36), np.zeros(4096)], x.reshape(2, -1), dtype=torch.float64, scale_percent=[10, 0])
    with pytest.raises(ValueError, match='2 items need 2 scale_percent'):
        DeblurBatch.generate(None, [{}, {}], 64, 64, scale_percent=[10])


def test_check_mb_caps_every_problem_at_its_own_m():
    """_check_mb of a mixed batch: cap[b] = M_b for a scalar and for a per-problem vector; the message names the problem."""
    from pnp_svrg_amd.batches import DeblurBatch
    b = DeblurBatch.__new__(DeblurBatch)
    b.B, b.M_vec = 3, np.array([1024, 36, 4096], np.int32)
    b.max_mb = b.M_vec
    b._check_mb(36)
    b._check_mb(np.array([1024, 36, 4096]))
    with pytest.raises(ValueError, match=r'larger sample than population.*problem 1: mini_batch_size 37, population 36'):
        b._check_mb(37)
    with pytest.raises(ValueError, match=r'larger sample than population.*problem 0: mini_batch_size 1025, population 1024'):
        b._check_mb(np.array([1025, 36, 4096]))
    with pytest.raises(ValueError, match='one per\n? ?problem|one per problem'):
        b.draw_minibatches(1, 8)


def test_make_runner_mixed_scales_refusals_before_device_work():
    from pnp_svrg_amd import sweep
    imgs = [np.random.default_rng(0).random((64, 64))]
    kw = dict(eta=0.5, n_inner=2, mini_batch_size=8, T2=2, H=64, W=64)
    for prob in ('csmri', 'pr'):
        with pytest.raises(ValueError, match=f"mixed_scales=True is for problem='deblur' \\(got '{prob}'\\)"):
            sweep.make_runner(imgs, problem=prob, mixed_scales=True, **kw)
    with pytest.raises(ValueError, match='mixed_scales: True or False'):
        sweep.make_runner(imgs, problem='deblur', mixed_scales=1, **kw)
    # seeding='generator' keeps its scale-100 rule, also for an item that is not the first of its batch
    run = sweep.make_runner(imgs, problem='deblur', seeding='generator', mixed_scales=True, **kw)
    items = sweep.make_items(1, [1.0, 0.5], [20.0])
    with pytest.raises(ValueError, match='generator seeding builds scale_percent == 100 Deblur items'):
        run.prepare_data(items)
    sweep.make_runner(imgs, problem='deblur', **kw)             # the default is untouched and needs no device to be made
