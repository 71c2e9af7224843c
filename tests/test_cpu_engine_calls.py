"""CPU-only: every engine path makes, call for call and argument for argument, the calls recorded in tests/golden/engine_calls.json.

The traces come from tools/record_engine_calls.py (the library replaced by a recorder, a fake batch on CPU tensors, the real front end
of `ops`): every `_native.call`, every batch and prox call, every Python-level `copy_` / `fill_`, the counters a run leaves behind, and
the text of every refusal.  The golden file was written by the same tool from the engines as they were before their shared
plumbing was folded into one copy each; a difference here is a changed trajectory or a changed message, not a style matter."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'engine_calls.json')

_spec = importlib.util.spec_from_file_location('record_engine_calls', os.path.join(ROOT, 'tools', 'record_engine_calls.py'))
TOOL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(TOOL)
WANT = TOOL.load(GOLDEN)


@pytest.fixture(scope='module')
def tool():
    return TOOL


def test_the_golden_file_holds_every_configuration_of_the_tool(tool):
    assert list(WANT) == tool.names()


@pytest.mark.parametrize('name', list(WANT))
def test_engine_makes_the_recorded_calls(tool, name):
    got, want = tool.record_one(name), WANT[name]
    for i, (g, w) in enumerate(zip(got['head'], want['head'])):
        assert g == w, f'{name}: entry {i} is the first that differs\n  got  {json.dumps(g)}\n  want {json.dumps(w)}'
    assert len(got['head']) == len(want['head']) and got['n'] == want['n'], \
        f'{name}: {got["n"]} entries, recorded {want["n"]} (the first {min(len(got["head"]), len(want["head"]))} agree)'
    assert got['sha256'] == want['sha256'], (f'{name}: the first {len(want["head"])} of {want["n"]} entries agree, a later one differs '
                                             f'(tools/record_engine_calls.py --show {name} prints them all)')
