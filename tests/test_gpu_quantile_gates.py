"""GPU: the segment quantiles (segment_quantiles.hip) launched next to every host gate, bit for bit
against np.sort.

The question is which kernel takes a row, not the select: a segment whose class the host does not
launch keeps the sentinel its row was filled with.  The launches are data
(tests/_segment_gate_cases.py) built from the gate model; tests/test_segment_gate_model_cpu.py
proves what each is aimed at."""
import numpy as np
import pytest

import _segment_gate_cases as C
import _segment_gate_run as R

pytestmark = pytest.mark.gpu
FAMILY = "quantiles"
KEEPS = C.gate_keeps(FAMILY)


@pytest.mark.parametrize("keep", KEEPS)
def test_strided_gates(keep):
    """begin 0..3, stride % 4 zero and non-zero, the keep through cap with the cut moving the
    phase, a base off the 16-byte grid, nseg 1 and 3..6."""
    for c in C.strided_cases(FAMILY, keep):
        R.run_case(c)


@pytest.mark.parametrize("keep", KEEPS)
def test_ragged_gates(keep):
    """max_len = keep, both segment forms, with and without aligned16."""
    for c in C.ragged_gate_cases(FAMILY, keep):
        R.run_case(c)


@pytest.mark.parametrize("keep", KEEPS)
def test_ragged_gates_through_cap(keep):
    for c in C.ragged_cap_cases(FAMILY, keep):
        R.run_case(c)


@pytest.mark.parametrize("aligned16", [False, True])
def test_every_class_under_a_tight_and_a_loose_hint(aligned16):
    tight, loose = C.all_class_cases(FAMILY, aligned16)
    host, out_t, num_t = R.run_case(tight)
    out_l, num_l = R.launch(loose, host)
    R.check(loose, host, out_l, num_l)
    assert np.array_equal(out_t.view(np.uint32), out_l.view(np.uint32)) and np.array_equal(num_t, num_l)
