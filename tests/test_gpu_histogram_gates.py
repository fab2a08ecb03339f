"""GPU: the duration histograms (segment_histogram.hip) launched next to both host gates, and the
kept-bucket counting on segments built for one event each, against np.bincount.

A segment whose kernel the host does not launch keeps the sentinel its row was filled with.  The
launches and the constructed segments are data (tests/_segment_gate_cases.py);
tests/test_segment_gate_model_cpu.py proves what each is aimed at."""
import numpy as np
import pytest
import torch

import _segment_gate_cases as C
import _segment_gate_run as R

pytestmark = pytest.mark.gpu
FAMILY = "histogram"
KEEPS = C.gate_keeps(FAMILY)
DEV = R.DEV


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
    assert np.array_equal(out_t, out_l) and np.array_equal(num_t, num_l)


@pytest.mark.parametrize("case", C.count_cases(), ids=lambda c: c.name)
def test_counting(case):
    """One constructed segment (begin = m0 puts it m0 slots into a 16-byte vector) between two
    random neighbours that share its launch."""
    n, m0 = int(case.keys.size), case.m0
    stride = (n + m0 + 7) // 4 * 4
    rng = np.random.default_rng(n)
    host = rng.integers(C.KEY_LO, C.KEY_HI, size=3 * stride + 8, dtype=np.uint32)
    host[stride + m0: stride + m0 + n] = case.keys
    out = torch.full((3, R.BINS), R.HSENT, dtype=torch.int32, device=DEV)
    num = torch.full((3,), R.NSENT, dtype=torch.int32, device=DEV)
    ops_out = R.ops.segment_histogram_strided(R._dev(host), 3, stride, m0, n, out=out, num=num)
    got = ops_out.cpu().numpy().view(np.uint32).astype(np.int64)
    assert num.cpu().tolist() == [n] * 3
    for s in range(3):
        ref = R.histogram_ref(host[s * stride + m0: s * stride + m0 + n])
        assert got[s].sum() == n, (case.name, s, int(got[s].sum()))
        assert np.array_equal(got[s], ref), (case.name, s, np.nonzero(got[s] != ref)[0][:6])


def test_accumulate_twice_over_both_kernels():
    lens = np.array(C.ACCUMULATE_LENS, np.int64)
    c = C._ragged(FAMILY, "accumulate", int(lens.max()), lens, [(3 * i + 1) % 4 for i in range(len(lens))],
                  0, int(lens.max()), False, "len")
    host = C.host_keys(c, 99)
    nseg = len(lens)
    start = (np.arange(nseg * R.BINS, dtype=np.int64) * 7 % 1000).reshape(nseg, R.BINS)   # no sentinel
    out = torch.from_numpy(start.astype(np.int32)).to(DEV)
    num = torch.full((nseg,), R.NSENT, dtype=torch.int32, device=DEV)
    for _ in range(2):
        R.ops.segment_histogram_ragged(R._dev(host), torch.from_numpy(c.off).to(DEV),
                                       torch.from_numpy(lens.astype(np.int32)).to(DEV), c.max_len,
                                       out=out, num=num, accumulate=True)
    got = out.cpu().numpy().astype(np.int64)
    segs = C.ragged_segments(c)
    assert {C.M.seg_class(FAMILY, n, ph) for n, ph in segs if n > 0} == {"wave", "block"}
    for s, (n, ph) in enumerate(segs):
        add = 2 * R.histogram_ref(C.ragged_retained(c, host, s)) if n > 0 else 0
        assert np.array_equal(got[s], start[s] + add), (s, n)
        assert int(num[s]) == (n if n >= 0 else R.NSENT)
