"""GPU: the median select of the FAST statistics kernels (`lean_core`, `hist_locate1`) on segments
built for one branch each (tests/_median_cases.py), through all four kernel families, against the
oracle's computeStats: NUM / MIN / MAX / MED bit for bit, AVG / STD by tests/_moments_ref.py `check`
(the oracle's bits where tests/_ragged_model.py `expect_exact_bits` says so).

Which branch a segment takes is proved on the CPU, from its keys, by tests/test_median_trace_cpu.py
through the control-flow model tests/_median_trace.py; the trace assertions repeated before each
launch only tie the GPU run to that proof (instantiation, exits, padding position).  All cases of
one (family, PL, n, phase) go into one launch; ragged launches start from sentinel-filled outputs,
so a row nothing wrote fails."""
import numpy as np
import pytest
import torch

import _median_cases as C
import _median_trace as T
import _moments_ref as MR
import _ragged_model as RM
import oracle as O
from nvidia_resiliency_ext.straggler import ops
from test_gpu_ragged_classes import F32_SENTINEL, NUM_SENTINEL, _sentinel_out
from test_gpu_segment_stats import _check_bulk

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 0xDEAD0000   # between segments: a key no segment has


def _bits(x):
    return np.float32(x).view(np.uint32)


def _verify(g, s, keys, exact_bits, tag):
    """Row s of the fetched outputs against computeStats of the retained keys."""
    r = O.compute_stats(O.key_to_us(keys))
    assert int(g.num[s]) == r.num_calls == keys.size, (tag, "num", int(g.num[s]))
    for f, want in (("min", r.min), ("max", r.max), ("med", r.median)):
        got = getattr(g, f)[s]
        assert _bits(got) == _bits(want), (tag, f, float(got), float(want))
    if exact_bits:
        assert _bits(g.avg[s]) == _bits(r.avg) and _bits(g.std[s]) == _bits(r.stddev), (tag, "avg/std bits")
    else:
        MR.check(g.avg[s], g.std[s], keys, tag=tag)


def _proved(cases, PL, full, kb, m0, tag):
    for c in cases:
        tr = T.lean_trace(c.keys, PL, full, kb, m0)
        assert not C.unmet(tr, c.want), (tag, c.name, C.unmet(tr, c.want))


def _numpy(st):
    g = st.cpu()
    return type("G", (), {f: getattr(g, f).numpy() for f in ("num", "min", "max", "med", "avg", "std")})


def _strided(cases, n, begin, inst, tag):
    stride = (begin + n + 3) // 4 * 4 + 4
    host = np.full(len(cases) * stride, GAP, np.uint32)
    for s, c in enumerate(cases):
        host[s * stride + begin: s * stride + begin + n] = c.keys
    ns = torch.from_numpy(host.view(np.int32)).to(DEV)
    assert ns.data_ptr() % 16 == 0
    g = _numpy(ops.segment_stats_strided(ns, len(cases), stride, begin, n, cap=0, mode=ops.STATS_FAST))
    for s, c in enumerate(cases):
        _verify(g, s, c.keys, inst is None, f"{tag} {c.name}")


@pytest.mark.parametrize("PL", T.CLASSES)
def test_strided_masked(PL):
    """seg_stats_fast_kernel<PL, false>, phases 0..3 (PL 64 / 128: 0, 1, 3).  Misaligned, a run
    needs n + 3 slots: 64 PL - 1 samples then run in the next class, with cases built for it
    (8191 samples: the EXACT kernel, the oracle's bits in every field)."""
    for n in C.lengths(PL, True) + ((C.SHORT_PL4,) if PL == 4 else ()):
        for begin in (0, 1, 2, 3) if PL <= 32 else (0, 1, 3):
            inst = T.instantiation("strided_masked", n, begin)
            crossed = begin > 0 and n + 3 > 64 * PL
            assert inst == (None if crossed and PL == 128 else (2 * PL if crossed else PL, False,
                                                                (2 * PL if crossed else PL) <= 16))
            tag = f"strided PL{PL} n{n} begin{begin}"
            if inst is None:
                cases = C.build_cases(PL, n, False, PL <= 16, 0)
            else:
                cases = C.build_cases(inst[0], n, inst[1], inst[2], begin)
                _proved(cases, inst[0], inst[1], inst[2], begin, tag)
            _strided(cases, n, begin, inst, tag)


@pytest.mark.parametrize("PL", T.CLASSES)
def test_strided_full(PL):
    """seg_stats_lean_group_kernel at group size 1: aligned runs of exactly 64 PL samples."""
    n = 64 * PL
    inst = T.instantiation("strided_full", n, 0)
    assert inst == (PL, True, PL <= 16)
    cases = C.build_cases(PL, n, True, inst[2], 0)
    _proved(cases, PL, True, inst[2], 0, f"full PL{PL}")
    _strided(cases, n, 0, inst, f"strided full PL{PL}")


def _ragged(lens, keeps, segs, phase, aligned16, cap, tag, exact_bits):
    """One sentinel-prefilled launch: segment s has lens[s] samples of which the last keeps[s] are
    segs[s]; every retained run starts `phase` slots into a 16-byte vector."""
    off = np.zeros(len(lens), np.int64)
    pos = 0
    for s, (L, k) in enumerate(zip(lens, keeps)):
        pos += (phase - (pos + L - k)) % 4
        off[s] = pos
        pos += L + 1
    host = np.full(pos + 8, GAP, np.uint32)
    for s, (L, k) in enumerate(zip(lens, keeps)):
        host[off[s]: off[s] + L - k] = 4_000_000 + np.arange(L - k)   # overwritten ring entries
        host[off[s] + L - k: off[s] + L] = segs[s]
        assert (off[s] + L - k) % 4 == phase
    ns = torch.from_numpy(host.view(np.int32)).to(DEV)
    assert ns.data_ptr() % 16 == 0
    out = _sentinel_out(len(lens))
    ops.segment_stats_ragged(ns, torch.from_numpy(off).to(DEV), torch.from_numpy(np.asarray(lens, np.int32)).to(DEV),
                             max_len=int(max(lens)), cap=cap, mode=ops.STATS_FAST, aligned16=aligned16, out=out)
    g = _numpy(out)
    assert NUM_SENTINEL not in g.num.tolist(), (tag, "rows never written", np.flatnonzero(g.num == NUM_SENTINEL)[:8])
    assert not (g.med.view(np.uint32) == F32_SENTINEL.view(np.uint32)).any(), (tag, "med never written")
    for s, keys in enumerate(segs):
        _verify(g, s, keys, exact_bits[s], f"{tag} segment {s}")


@pytest.mark.parametrize("PL", T.CLASSES)
def test_ragged_list(PL):
    """seg_stats_list_kernel<PL> (KEEPBIN only up to PL 8: PL 16 runs lean_core<16, false, false>),
    aligned16 both ways; aligned, 64 PL samples that are not the launch's FULL length run masked
    code with pad = 0 -- one longer segment keeps the launch from having a FULL length."""
    for n in C.lengths(PL, True) + (64 * PL,):
        for aligned16, phase in ((True, 0), (False, 1), (False, 3)):
            # the longest segment: no FULL length in this launch
            extra = n + 4 if n + 4 not in RM.FULL_LENS else n + 8
            full_n = RM.full_len(extra, aligned16, False)
            assert full_n == 0
            inst = T.instantiation("ragged_list", n, phase, aligned16, full_n)
            crossed = not aligned16 and n + 3 > 64 * PL
            if inst is None:
                assert crossed and PL == 128   # the workgroup class
                continue
            want_pl = 2 * PL if crossed else PL
            assert inst == (want_pl, False, want_pl <= 8)
            tag = f"ragged PL{PL} n{n} aligned{int(aligned16)} phase{phase}"
            cases = C.build_cases(inst[0], n, False, inst[2], phase)
            _proved(cases, inst[0], False, inst[2], phase, tag)
            if n == 64 * inst[0]:
                assert aligned16 and all(T.lean_trace(c.keys, inst[0], False, inst[2], 0).pad == 0 for c in cases)
            segs = [c.keys for c in cases]
            rng = np.random.default_rng(n)
            segs.append(rng.integers(2000, 2_200_000, size=extra, dtype=np.uint32))
            lens = [k.size for k in segs]
            bits = [RM.expect_exact_bits(L, aligned16, False) for L in lens]
            assert not any(bits[:-1])
            _ragged(lens, lens, segs, phase, aligned16, 0, tag, bits)


@pytest.mark.parametrize("n", RM.FULL_LENS)
def test_ragged_full(n):
    """seg_stats_list_full_kernel<PL>, PL 16..128: cap = 64 PL, aligned16; rings at capacity and
    overflowed ones (the last 64 PL pushes retained)."""
    PL = n // 64
    inst = T.instantiation("ragged_full", n, 0, True, RM.full_len(RM.keep_of(2 * n, n), True, False))
    assert inst == (PL, True, PL <= 16)
    cases = C.build_cases(PL, n, True, inst[2], 0)
    _proved(cases, PL, True, inst[2], 0, f"ragged full PL{PL}")
    segs = [c.keys for c in cases]
    lens = [n if s % 2 == 0 else n + 1 + 37 * s % n for s in range(len(segs))]
    assert max(lens) > n and min(lens) == n
    _ragged(lens, [n] * len(segs), segs, 0, True, n, f"ragged full PL{PL}", [False] * len(segs))


def test_grouped_launch_with_constructed_segments():
    """The group kernel at group size 2 with a partial last group: the PL 4 cases at the first and
    the last slot of groups, in the partial group and at segment 0, random keys elsewhere; every
    row against the oracle."""
    n, nseg = 256, 2 * 32768 + 3
    group = min(8, max(1, nseg // 32768))   # segment_stats.hip lean_group
    assert group == 2 and nseg % group == 1
    cases = C.build_cases(4, n, True, True, 0)
    _proved(cases, 4, True, True, 0, "grouped")
    rng = np.random.default_rng(n)
    host = rng.integers(2000, 2_200_000, size=nseg * n, dtype=np.uint32)
    where, which = [], []
    for i, c in enumerate(cases):
        for s in (2 * (50 + i), 2 * (9000 + 3 * i) + 1):          # first slot, last slot
            where.append(s)
            which.append(c)
    where += [0, 1, nseg - 1]                                      # segment 0; the partial group
    which += [cases[0], cases[1], cases[2]]
    assert len(set(where)) == len(where)
    for s, c in zip(where, which):
        host[s * n:(s + 1) * n] = c.keys
    ns = torch.from_numpy(host.view(np.int32)).to(DEV)
    g = _numpy(ops.segment_stats_strided(ns, nseg, n, 0, n, cap=0, mode=ops.STATS_FAST))
    ref = O.matrix_stats(host, nseg, n, 0, n, 0, nthreads=8)
    for f in ("num", "min", "max", "med"):
        a, b = getattr(g, f), ref[f]
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert bad.size == 0, (f, bad[:8], a[bad[:8]], b[bad[:8]])
    _check_bulk(g.avg, g.std, host.reshape(nseg, n), where, tag="grouped")
    for s, c in zip(where, which):
        MR.check(g.avg[s], g.std[s], c.keys, tag=f"grouped segment {s} {c.name}")
