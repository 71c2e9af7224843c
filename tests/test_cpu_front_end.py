"""CPU-only checks of the Python front end: engine.py's re-exports and the scalar / per-problem routing of ops.py."""
import pytest
import torch

MOVED = {'batches': ['Minibatches', '_BatchBase', 'CsmriBatch', 'DeblurBatch', 'PrBatch'],
         'prox': ['TVProx', 'DnCNNProx', 'NLMProx']}
KEPT = ['LoopEngine', '_StochEngine', 'GdEngine', 'SgdEngine', 'SvrgEngine', 'SarahEngine', 'SagaEngine', 'make_engine']


def test_engine_reexports_the_moved_names_as_the_same_objects():
    import importlib
    from pnp_svrg_amd import engine
    for mod, names in MOVED.items():
        home = importlib.import_module('pnp_svrg_amd.' + mod)
        for name in names:
            assert getattr(engine, name) is getattr(home, name), name
            assert getattr(home, name).__module__ == home.__name__, name         # defined there, not wrapped
    for name in KEPT:
        assert getattr(engine, name).__module__ == engine.__name__, name


def test_ops_router_scalars_plain_one_tensor_pp_pairs(monkeypatch):
    from pnp_svrg_amd import _native, ops
    calls = []
    monkeypatch.setattr(_native, 'call', lambda name, *args: calls.append((name, args)))
    ptr = lambda t: None if t is None else ('ptr', t)            # noqa: E731  (_p for CPU tensors: no device pointer to take)

    # all scalars: the plain entry point, the scalars alone, in order, as the Python types the plain calls convert to
    ops._route('pnp_x', ['h', ops._pp(2, 3), 7, ops._pp(5, 3, torch.int32), None, ops._pp(0.5, 3)], ptr=ptr)
    name, args = calls.pop()
    assert name == 'pnp_x' and args == ('h', 2.0, 7, 5, None, 0.5)
    assert [type(a) for a in args] == [str, float, int, int, type(None), float]

    # one tensor: name_pp, every marked value a (scalar, pointer) pair, None for the scalars that stayed scalar
    v = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    ops._route('pnp_x', ['h', ops._pp(2, 3), 7, ops._pp(5, 3, torch.int32), ops._pp(v, 3)], ptr=ptr)
    name, args = calls.pop()
    assert name == 'pnp_x_pp' and len(args) == 8
    assert args[:6] == ('h', 2.0, None, 7, 5, None) and args[6] == 0.0 and args[7][0] == 'ptr' and args[7][1] is v
    m = torch.tensor([4, 5, 6], dtype=torch.int32)
    ops._route('pnp_y', [ops._pp(m, 3, torch.int32), ops._pp(1.5, 3)], ptr=ptr)
    name, args = calls.pop()
    assert name == 'pnp_y_pp' and args[0] == 0 and isinstance(args[0], int) and args[1][1] is m and args[2:] == (1.5, None)

    # a tensor of the wrong dtype or shape: the assertion of _pp(), before anything is called
    for bad, dtype in ((torch.zeros(3, dtype=torch.float32), torch.float64), (torch.zeros(4, dtype=torch.float64), torch.float64),
                       (torch.zeros((3, 1), dtype=torch.float64), torch.float64), (torch.zeros(3, dtype=torch.int64), torch.int32)):
        with pytest.raises(AssertionError, match='per-problem values'):
            ops._route('pnp_x', ['h', ops._pp(bad, 3, dtype)], ptr=ptr)
    assert calls == []
