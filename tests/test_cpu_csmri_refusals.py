"""What the one-kernel CSMRI entry points of csrc/csmri.hip answer to bad arguments, replayed from tests/golden/csmri_refusals.json
(written by tools/record_csmri_refusals.py): for every entry point, plain and _pp / _hist / _prox alike, the code and the text of
pnp_last_error() of every refusal -- Python callers see that text through NativeError --, which check answers where several are violated, and the accepted side of every bound.  The
checks run on a plan filled on the host and on fabricated pointers, before any HIP call; the replay runs in a process of its own that
sees no device (see `replay` in the tool), so nothing is ever launched."""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'record_csmri_refusals.py')
TABLE = os.path.join(ROOT, 'tests', 'golden', 'csmri_refusals.json')
N_CASES = 465
ERR_ARG, ERR_HIP = 1, 2


def _lib_path():
    from pnp_svrg_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.LIB_PATH


def _tool():
    spec = importlib.util.spec_from_file_location('record_csmri_refusals', TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_every_one_kernel_entry_point():
    rec = _tool()
    src = open(os.path.join(ROOT, 'pnp_svrg_amd', 'csrc', 'csmri.hip')).read()
    src = src[src.index('---- whole inner iteration in one kernel'):]
    entries = set(re.findall(r'extern "C" int (pnp_csmri_\w+)\(', src))
    table = json.load(open(TABLE))
    assert entries == set(rec.PROTOS) == set(table['base']) == {c['entry'] for c in table['cases']}
    assert len(table['cases']) == N_CASES
    for e in entries:
        mine = [c for c in table['cases'] if c['entry'] == e]
        assert sum(c['rc'] == ERR_ARG for c in mine) >= 6 and any(c['rc'] == ERR_HIP for c in mine), e
        assert sum(c['rc'] == ERR_ARG and len(c['set']) >= 2 for c in mine) >= 2, e        # the order of the checks
    assert all((c['error'] is None) == (c['rc'] == ERR_HIP) and c['rc'] in (ERR_ARG, ERR_HIP) for c in table['cases'])
    # a case that is let through has nothing to launch, wherever it runs
    for c in table['cases']:
        if c['rc'] == ERR_HIP:
            assert rec.arguments(table, c)[0]['batch'] == 0, (c['entry'], c['case'])


def test_every_refusal_is_the_recorded_one():
    rec = _tool()
    out = subprocess.run([sys.executable, TOOL, '--replay', '--lib', _lib_path(), '-o', TABLE], capture_output=True, text=True,
                         env=dict(os.environ, **rec.HIDE), timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    cases = json.load(open(TABLE))['cases']
    assert len(got) == len(cases)
    bad = [(c['entry'], c['case'], (c['rc'], c['error']), (rc, text)) for c, (rc, text) in zip(cases, got)
           if rc != c['rc'] or (c['error'] is not None and text != c['error'])]
    assert not bad, f'{len(bad)} of {len(cases)} differ; the first: {bad[:3]}'
