"""Every memory instruction of the F(4x4,3x3) conv kernel's main loop keeps an MFMA gap of its own (two-block-row form).

Beside an f32 MFMA one memory instruction is free and a second one in the same gap costs about an MFMA.
tools/check_w44_gaps.py compiles csrc/dncnn_wino44.hip to assembly and classifies what stands between consecutive MFMAs of
the tile loop, up to W44_EPILOGUE_BEGIN, for every production instantiation (STAMP = false, VAR = 0)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import check_w44_gaps  # noqa: E402

# gaps with more than one memory instruction in the one-block-row form (half the gaps for nearly the same memory
# instructions: it cannot reach one per gap), as counted by the same tool on commit 1cd2af1, the parent of the re-slotted step
NG1_MULTI_GAPS_1CD2AF1 = 94

# <LEAKY, NG, STAMP = false, VAR = 0, FL>: plain, LeakyReLU, fused last layer
FORMS = {'plain': 'ILb0ELi%dELb0ELi0ELb0EEEv', 'leaky': 'ILb1ELi%dELb0ELi0ELb0EEEv', 'fused_last': 'ILb0ELi%dELb0ELi0ELb1EEEv'}


@pytest.fixture(scope='module')
def kernels():
    return check_w44_gaps.analyse(check_w44_gaps.compile_asm())


def pick(kernels, form, ng):
    hits = [r for name, r in kernels.items() if FORMS[form] % ng in name]
    assert len(hits) == 1, (form, ng, sorted(kernels))
    assert hits[0]['ng'] == ng
    return hits[0]


def test_all_production_instantiations_found(kernels):
    assert len(kernels) == 6, sorted(kernels)


@pytest.mark.parametrize('form', sorted(FORMS))
def test_two_block_rows_one_memory_instruction_per_gap(kernels, form):
    r = pick(kernels, form, 2)
    print(form, r)
    assert r['mfmas'] == 1152
    assert r['multi'] == 0, r['hist']
    assert r['mixed'] == 0, r['hist']


@pytest.mark.parametrize('form', sorted(FORMS))
def test_one_block_row_no_worse_than_parent(kernels, form):
    r = pick(kernels, form, 1)
    print(form, r)
    assert r['mfmas'] == 576
    assert r['multi'] <= NG1_MULTI_GAPS_1CD2AF1, r['hist']
