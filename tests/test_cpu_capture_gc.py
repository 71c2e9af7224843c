"""A hipGraph capture must not meet the cyclic collector: a plan frees its device buffers in its destructor (hipFree), a hipFree while
a stream captures invalidates the capture, and a plan that died inside a reference cycle is destroyed whenever the collector next
runs.  `ops.collector_held()` collects first and holds the collector off; both capture sites take it."""
import gc
import inspect

import pytest


def test_collector_held_collects_first_and_holds_the_collector_off():
    from pnp_svrg_amd import ops

    class Plan:
        freed = []

        def __del__(self):
            Plan.freed.append(gc.isenabled())

    def cycle():
        a = Plan()
        a.me = a

    assert gc.isenabled()
    gc.collect()
    cycle()
    with ops.collector_held():
        assert Plan.freed == [True]                             # the dead cycle went before the block began, collector still on
        assert not gc.isenabled()
        cycle()
        for _ in range(5000):                                   # far past the collector's allocation threshold
            [[]]
        assert Plan.freed == [True]                             # ... and nothing is destroyed inside the block
    assert gc.isenabled()
    gc.collect()
    assert Plan.freed == [True, True]


def test_collector_held_restores_the_collector_on_errors_and_leaves_it_off_when_it_was_off():
    from pnp_svrg_amd import ops
    with pytest.raises(KeyError):
        with ops.collector_held():
            raise KeyError('x')
    assert gc.isenabled()
    gc.disable()
    try:
        with ops.collector_held():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_both_capture_sites_hold_the_collector():
    from pnp_svrg_amd import algorithms, engine
    for mod in (engine, algorithms):
        src = inspect.getsource(mod)
        assert src.count('torch.cuda.graph(') == 1
        line = next(l for l in src.splitlines() if 'torch.cuda.graph(' in l)
        assert 'ops.collector_held()' in line and line.index('ops.collector_held()') < line.index('torch.cuda.graph(')
