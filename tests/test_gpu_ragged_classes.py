"""GPU: the seam between the classifier and the launch gates of segment_stats_ragged.

The classifier sorts a segment by its own retained length, the host launches class kernels from
the `max_len` hint and `cap`; a segment in a class nothing launched keeps whatever its output row
held.  So every launch here starts from sentinel-filled outputs (num -7, floats -12345.0) and
every row is checked: a retained segment against the oracle (NUM / MIN / MAX / MED bit for bit;
AVG / STD bit for bit where `_ragged_model.expect_exact_bits` says so, else `_moments_ref.check`
with its own bound), an empty one as num 0 and NaN, a skipped one as the untouched sentinel.

The launches are data (tests/_ragged_cases.py, built from tests/_ragged_model.py): (a) both sides
of every launch gate under a tight hint, through cap, under a loose hint, in both segment forms;
(b) the EXACT kernels at their own edges; (c) the classifier's count / scan / scatter with classes
confined to chosen blocks, past 64 blocks, and whole launches in one class; (d) the model's proof
that (a)-(c) miss no class, gate or kernel.  tests/native/ragged_class.hip ties the model's
seg_class to the product function."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import _moments_ref as MR
import _ragged_cases as C
import _ragged_model as M
import oracle as O
from nvidia_resiliency_ext.straggler import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "native", "ragged_class.hsaco")
FLOATS = ("min", "max", "med", "avg", "std")
NUM_SENTINEL = -7
F32_SENTINEL = np.float32(-12345.0)
PARAMS = pytest.mark.parametrize("aligned16,exact", C.PARAMS, ids=[C.tag(a, e) for a, e in C.PARAMS])


def _layout(case):
    """Segment offsets and the buffer size.  seg_len form: every segment in a slot of its own; the
    retained run starts on a 16-byte boundary (aligned16), else at 4-byte phase s % 4 (copies of
    a length are neighbours: different phases).  Offsets form: back to back from phase 1 (or 0)."""
    lens = np.maximum(case.lens, 0)
    if case.form == "off":
        off = np.zeros(lens.size + 1, np.int64)
        off[0] = 0 if case.aligned16 else 1
        off[1:] = off[0] + np.cumsum(lens)
        return off, int(off[-1]) + 4
    slot = (lens + 3) // 4 * 4 + 4
    base = np.concatenate([[0], np.cumsum(slot)[:-1]])
    keep = np.maximum(C.kept(case), 0)
    phase = (keep - lens) % 4 if case.aligned16 else np.arange(lens.size) % 4
    return base + phase, int(slot.sum())


def _data(case, off, total):
    rng = np.random.default_rng(zlib.crc32(case.lens.tobytes()) + case.cap)  # the lengths alone: tight / loose share data
    host = rng.integers(2000, 2_200_000, size=total, dtype=np.uint32)
    for s in case.dup:  # duplicate-heavy segments
        n = int(case.lens[s])
        if n > 0:
            host[off[s]:off[s] + n] = 777_000 + rng.integers(0, 3, n)
    return host


def _sentinel_out(nseg):
    out = ops.SegmentStats.empty(nseg, DEV)
    out.num.fill_(NUM_SENTINEL)
    for f in FLOATS:
        getattr(out, f).fill_(float(F32_SENTINEL))
    return out


def _launch(case):
    """One sentinel-prefilled launch; returns (host keys, offsets, {field: numpy}, col_ref or None)."""
    off, total = _layout(case)
    host = _data(case, off, total)
    nseg = case.lens.size
    ns = torch.from_numpy(host.view(np.int32)).to(DEV)
    seg_len = None if case.form == "off" else torch.from_numpy(case.lens.astype(np.int32)).to(DEV)
    col = torch.empty(2 * case.colref, dtype=torch.int32, device=DEV) if case.colref else None
    out = _sentinel_out(nseg)
    ops.segment_stats_ragged(ns, torch.from_numpy(off).to(DEV), seg_len, max_len=case.max_len, cap=case.cap,
                             mode=ops.STATS_EXACT if case.exact else ops.STATS_FAST,
                             aligned16=case.aligned16, out=out, col_ref=col, ncols=case.colref)
    g = out.cpu()
    got = {f: getattr(g, f).numpy() for f in ("num",) + FLOATS}
    return host, off, got, None if col is None else col.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def _verify(case, host, off, got):
    """Every row of the launch.  The reference of the retained segments is computed once per
    retained length over the matrix of their windows (oracle.matrix_stats, threaded)."""
    keep = C.kept(case)
    full_n = M.full_len(M.keep_of(case.max_len, case.cap), case.aligned16, case.exact)
    # the contract of the inputs: the hint bounds every length, aligned16 only when true
    assert int(case.lens.max()) <= case.max_len
    start = off[:keep.size] + np.maximum(case.lens, 0) - np.maximum(keep, 0)
    if case.aligned16:
        assert not (start[keep > 0] % 4).any(), case.name
    skipped = keep < 0
    assert (got["num"][skipped] == NUM_SENTINEL).all(), (case.name, "skipped segment: num written",
                                                         np.flatnonzero(skipped & (got["num"] != NUM_SENTINEL))[:8])
    for f in FLOATS:
        assert (_bits(got[f][skipped]) == _bits(np.array([F32_SENTINEL]))[0]).all(), \
            (case.name, "skipped segment written", f)
    empty = keep == 0
    assert (got["num"][empty] == 0).all(), (case.name, "empty segment: num",
                                            np.flatnonzero(empty & (got["num"] != 0))[:8])
    for f in FLOATS:
        assert np.isnan(got[f][empty]).all(), (case.name, "empty segment: not NaN", f)
    ref_num = np.zeros(keep.size, np.int32)
    ref_med = np.full(keep.size, np.nan, np.float32)
    for n in np.unique(keep[keep > 0]):
        n = int(n)
        idx = np.flatnonzero(keep == n)
        win = np.ascontiguousarray(host[start[idx][:, None] + np.arange(n)[None, :]])
        ref = O.matrix_stats(win.reshape(-1), idx.size, n, 0, n, 0, nthreads=min(16, idx.size))
        ref_num[idx], ref_med[idx] = ref["num"], ref["med"]
        unwritten = idx[got["num"][idx] == NUM_SENTINEL]
        assert unwritten.size == 0, (case.name, f"rows of {n} retained samples never written (class "
                                     f"{M.seg_class(n, case.aligned16, case.exact, full_n)})", unwritten[:8])
        exact_bits = M.expect_exact_bits(n, case.aligned16, case.exact)
        for f in ("num", "min", "max", "med") + (("avg", "std") if exact_bits else ()):
            bad = np.flatnonzero(_bits(got[f][idx]) != _bits(ref[f]))
            assert bad.size == 0, (case.name, f, n, idx[bad[:4]], got[f][idx][bad[:4]], ref[f][bad[:4]])
        if not exact_bits:
            for i, s in enumerate(idx):
                MR.check(got["avg"][s], got["std"][s], win[i], tag=f"{case.name} segment {s} keep {n}")
    return ref_num, ref_med


def _run(case):
    host, off, got, col = _launch(case)
    ref_num, ref_med = _verify(case, host, off, got)
    if case.colref:  # the fused column reference, as test_ragged_length_classes demands it
        K = case.colref
        want = O.kernel_ref(ref_num.reshape(-1, K), ref_med.reshape(-1, K))
        missing = col[K:] != 0
        assert np.array_equal(missing, (ref_num.reshape(-1, K) == 0).any(axis=0))
        assert (~missing).any() and missing.any()
        assert np.array_equal(col[:K].view(np.float32)[~missing], want[~missing])
    return got


# ------------------------------------------------------------------ the model is the product's rule
def test_model_seg_class_is_the_product_function():
    assert os.path.exists(PROBE), "build first: make -C tests/native (__graft_entry__.build())"
    nmax, fulls = M.SCAN_KEEPS, (0,) + M.FULL_LENS
    hip = ctypes.CDLL("libamdhip64.so")
    mod, fn = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipModuleLoad(ctypes.byref(mod), PROBE.encode()) == 0
    assert hip.hipModuleGetFunction(ctypes.byref(fn), mod, b"nvrx_ragged_class_probe") == 0
    table = torch.full((4 * len(fulls) * nmax,), 255, dtype=torch.uint8, device=DEV)
    a_table, a_nmax = ctypes.c_void_p(table.data_ptr()), ctypes.c_int(nmax)
    params = (ctypes.c_void_p * 2)(ctypes.cast(ctypes.byref(a_table), ctypes.c_void_p),
                                   ctypes.cast(ctypes.byref(a_nmax), ctypes.c_void_p))
    hip.hipModuleLaunchKernel.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * 6 + [
        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip.hipModuleLaunchKernel(fn, 1024, 1, 1, 256, 1, 1, 0, stream, params, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = table.cpu().numpy().reshape(2, 2, len(fulls), nmax)
    hip.hipModuleUnload(mod)
    index = {c: i for i, c in enumerate(M.CLASSES)}
    for a in (False, True):
        for e in (False, True):
            for f, full_n in enumerate(fulls):
                want = np.fromiter((index[M.seg_class(n, a, e, full_n)] for n in range(1, nmax + 1)),
                                   np.uint8, nmax)
                bad = np.flatnonzero(got[int(a), int(e), f] != want)
                assert bad.size == 0, (a, e, full_n, bad[:8] + 1, got[int(a), int(e), f][bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------ (a) every gate, both sides
@PARAMS
def test_every_gate_both_sides_tight_hint(aligned16, exact):
    """max_len = keep exactly, cap 0, for the keeps on both sides of every gate; the seg_len form
    and (where the alignment promise allows the lengths) the nseg + 1 offsets form."""
    cases = C.gate_cases(aligned16, exact)
    assert {c.max_len for c in cases} == set(M.all_gate_keeps(aligned16, exact))
    assert {c.form for c in cases} == {"len", "off"}
    for case in cases:
        _run(case)


@PARAMS
def test_gate_keeps_through_cap(aligned16, exact):
    """keep = cap under max_len = 50000 with overflowed segments; aligned FAST: cap 1024 / 8192
    populate the FULL class next to its neighbours."""
    for case in C.cap_cases(aligned16, exact):
        assert (case.lens > case.cap).sum() >= 4
        if aligned16 and not exact and case.cap in M.FULL_LENS:
            assert {"F", "T8"} < C.populated(case) and len(C.populated(case)) >= 8
        _run(case)


@PARAMS
def test_loose_hint_gives_the_same_bits(aligned16, exact):
    tight, loose = C.loose_cases(aligned16, exact)
    assert C.case_launched(tight) < C.case_launched(loose)
    a, b = _run(tight), _run(loose)
    for f in a:
        assert np.array_equal(_bits(a[f]), _bits(b[f])), f


# ------------------------------------------------------------------ (b) the EXACT kernels' edges
@pytest.mark.parametrize("aligned16", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("keep", C.EXACT_EDGES)
def test_exact_kernels_at_their_edges(keep, aligned16):
    case = C.exact_edge_case(keep, aligned16)
    assert (C.kept(case) == keep).sum() == 2 and C.populated(case) >= {"X", "T8", "T64"}
    _run(case)  # EXACT: all six fields bit-exact (expect_exact_bits)


@pytest.mark.parametrize("keep", C.FAST_X_EDGES)
def test_fast_unaligned_crossing_into_exact(keep):
    case = C.fast_x_case(keep)
    pop = C.populated(case)
    assert "W128" in pop and ("X" in pop) == (keep >= 8190)
    _run(case)


# ------------------------------------------------------------------ (c) the classifier's partition
@pytest.mark.parametrize("config", list(C.PARTITION))
@pytest.mark.parametrize("nseg", C.NSEGS)
def test_classifier_partition(nseg, config):
    colref = nseg == C.COLREF_NSEG and config == "fast-unaligned"
    case = C.partition_case(nseg, config, skipped=not colref, colref=C.COLREF_NCOLS if colref else 0)
    _run(case)


@pytest.mark.parametrize("i", range(3), ids=["T8", "W4", "X"])
def test_whole_launch_in_one_class(i):
    case = C.one_class_cases()[i]
    assert len(C.populated(case)) == 1
    _run(case)


# ------------------------------------------------------------------ (d) nothing is left out
def test_cases_cover_every_class_gate_and_kernel():
    cases = C.all_cases()
    # the list the model judges is the list the tests above run
    names = {c.name for c in cases}
    for a, e in C.PARAMS:
        assert {c.name for c in C.gate_cases(a, e) + C.cap_cases(a, e) + list(C.loose_cases(a, e))} <= names
    assert {C.exact_edge_case(k, a).name for k in C.EXACT_EDGES for a in (False, True)} <= names
    assert {C.fast_x_case(k).name for k in C.FAST_X_EDGES} <= names
    assert {c.name for c in C.one_class_cases()} <= names
    assert {f"partition-{cfg}-nseg{n}" for n in C.NSEGS for cfg in C.PARTITION} <= names
    print(C.format_coverage(C.coverage(cases)))
