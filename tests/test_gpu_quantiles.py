"""GPU: per-segment duration quantiles (segment_quantiles.hip) against numpy, bit for bit.

Reference for every case: np.sort of the retained u32 keys, rank k = (pm * (n - 1)) // 1000 in
Python integers, the key converted as every sample is (f32(ns) / 1000.0f).  Every result is a
sample, so there is no tolerance anywhere: float32 results are compared through their bits.
"""
import numpy as np
import pytest
import torch

import oracle as O
from nvidia_resiliency_ext.straggler import _native, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PM = (0, 1, 250, 500, 900, 990, 999, 1000)


def _us(keys):
    return O.key_to_f32(np.asarray(keys, np.uint32)).astype(np.float32) / np.float32(1000)


def _ref(retained, pm):
    """[len(pm)] float32: the quantiles of one segment's retained keys (NaN when empty)."""
    n = int(len(retained))
    if n == 0:
        return np.full(len(pm), np.nan, np.float32)
    s = np.sort(np.asarray(retained, np.uint32))
    return _us([s[(int(p) * (n - 1)) // 1000] for p in pm])


def _ref_strided(host, nseg, stride, begin, length, cap, pm):
    keep = min(length, cap) if cap > 0 else length
    cols = [_ref(host[s * stride + begin + length - keep: s * stride + begin + length], pm)
            for s in range(nseg)]
    return np.stack(cols, axis=1) if cols else np.empty((len(pm), 0), np.float32)


def _same_bits(got, ref, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (what, bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])


def _dev(host_u32):
    return torch.from_numpy(np.ascontiguousarray(host_u32, np.uint32).view(np.int32)).to(DEV)


def _run_strided(host, nseg, stride, begin, length, cap=0, pm=PM):
    num = torch.full((nseg,), -7, dtype=torch.int32, device=DEV)
    q = ops.segment_quantiles_strided(_dev(host), nseg, stride, begin, length, pm, cap=cap, num=num)
    _same_bits(q, _ref_strided(host, nseg, stride, begin, length, cap, pm),
               (nseg, stride, begin, length, cap))
    keep = min(length, cap) if cap > 0 else length
    assert num.cpu().tolist() == [keep] * nseg
    return q


LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096,
           4097, 8191, 8192]


def _aligned_case(length, begin):
    """Six segments starting `begin` slots into a stride that leaves the next one misaligned."""
    rng = np.random.default_rng(1000 * length + begin)
    stride = length + begin + (int(rng.integers(0, 5)) if begin else 0)
    if begin and stride % 4 == 0:
        stride += 1
    return rng.integers(1000, 3_000_000, size=6 * stride, dtype=np.uint32), stride


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_and_alignment(length):
    for begin in range(4):
        host, stride = _aligned_case(length, begin)
        _run_strided(host, 6, stride, begin, length)


def test_ring_retention():
    R, K, S, cap = 2, 12, 10000, 8192
    ns = synth.synth_matrix(R, K, S, device=DEV)
    q = ops.segment_quantiles_strided(ns.view(-1), R * K, S, 0, S, PM, cap=cap)
    host = ns.cpu().numpy().view(np.uint32).reshape(-1)
    _same_bits(q, _ref_strided(host, R * K, S, 0, S, cap, PM))


@pytest.mark.parametrize("nseg,length,cap,begin", [(1, 8193, 0, 0), (3, 8193, 0, 1), (1, 20000, 0, 0),
                                                   (3, 20000, 0, 3), (2, 40000, 0, 2),
                                                   (2, 40000, 20000, 0), (3, 20000, 8193, 1),
                                                   # 8190 samples misaligned by 3 do not fit a wave
                                                   (2, 8190, 0, 3)])
def test_streaming_path(nseg, length, cap, begin):
    rng = np.random.default_rng(length + cap + begin)
    stride = length + begin + 1
    host = rng.integers(1000, 3_000_000, size=nseg * stride, dtype=np.uint32)
    _run_strided(host, nseg, stride, begin, length, cap=cap)


def _values(kind, n, rng):
    if kind == "all_equal":
        return np.full(n, 123_457, np.uint32)
    if kind == "two_values_1_999":
        v = np.full(n, 2_000_000, np.uint32)
        v[rng.choice(n, max(1, n // 1000), replace=False)] = 1_000
        return v
    if kind == "two_values_999_1":
        v = np.full(n, 1_000, np.uint32)
        v[rng.choice(n, max(1, n // 1000), replace=False)] = 2_000_000
        return v
    if kind == "narrow_range":  # < 256 apart: the high 24 bits are shared
        return (np.uint32(0x00ABCD00) + rng.integers(0, 256, size=n)).astype(np.uint32)
    if kind == "ramp_up":
        return (np.uint32(5_000) + 37 * np.arange(n)).astype(np.uint32)
    if kind == "ramp_down":
        return (np.uint32(5_000) + 37 * np.arange(n)).astype(np.uint32)[::-1].copy()
    if kind == "full_span":  # every u32 up to NVRX_KEY_MAX: wide keys, the top bit set
        v = rng.integers(0, _native.KEY_MAX + 1, size=n, dtype=np.uint64).astype(np.uint32)
        v[rng.choice(n, max(2, n // 8), replace=False)] = rng.integers(
            _native.KEY_WIDE, _native.KEY_MAX + 1, size=max(2, n // 8), dtype=np.uint64).astype(np.uint32)
        v[0], v[-1] = _native.KEY_MAX, 0
        return v
    return rng.integers(1000, 3_000_000, size=n, dtype=np.uint32)  # "random"


KINDS = ["all_equal", "two_values_1_999", "two_values_999_1", "narrow_range", "ramp_up", "ramp_down",
         "full_span"]
REQUESTS = {"nq1": (990,), "repeats_descending": (1000, 990, 990, 500, 500, 0, 250)}


@pytest.mark.parametrize("length", [64, 1000, 8192, 20000])
@pytest.mark.parametrize("kind", KINDS + list(REQUESTS))
def test_adversarial_values(kind, length):
    rng = np.random.default_rng(length + len(kind))
    nseg, begin = 3, 1
    stride = length + 2
    host = np.concatenate([np.concatenate([_values(kind, length, rng), np.zeros(2, np.uint32)])
                           for _ in range(nseg)])
    # the samples sit at [begin, begin + length) of each stride
    host = np.roll(host, begin)
    _run_strided(host, nseg, stride, begin, length, pm=REQUESTS.get(kind, PM))


def test_consistent_with_segment_stats():
    for length in [n for n in LENGTHS if n % 2 == 1]:
        for begin in range(4):
            host, stride = _aligned_case(length, begin)
            ns = _dev(host)
            q = ops.segment_quantiles_strided(ns, 6, stride, begin, length, (0, 500, 1000)).cpu().numpy()
            st = ops.segment_stats_strided(ns, 6, stride, begin, length, mode=ops.STATS_FAST).cpu()
            for row, f in ((0, "min"), (1, "med"), (2, "max")):
                assert np.array_equal(q[row].view(np.uint32), getattr(st, f).numpy().view(np.uint32)), \
                    (length, begin, f)


RAGGED = [0, 1, 2, 7, 64, 65, 128, 129, 1000, 8192, 8193, 20000]


@pytest.mark.parametrize("with_len", [True, False])
def test_ragged(with_len):
    rng = np.random.default_rng(11)
    lens = np.array(RAGGED, np.int64)
    if with_len:  # gaps between the runs, every start odd
        off = np.zeros(len(lens), np.int64)
        pos = 1
        for i, n in enumerate(lens):
            off[i] = pos
            pos += int(n) + 2 * int(rng.integers(0, 3)) + (1 if n % 2 == 0 else 0)
            pos += 1 - pos % 2
        total = pos
    else:  # offsets only: back to back from an odd start
        off = 1 + np.concatenate([[0], np.cumsum(lens)])
        total = int(off[-1])
    host = rng.integers(1000, 3_000_000, size=total + 4, dtype=np.uint32)
    nseg = len(lens)
    SENT = np.float32(-12345.0)
    out = torch.full((len(PM), nseg), float(SENT), dtype=torch.float32, device=DEV)
    num = torch.full((nseg,), -7, dtype=torch.int32, device=DEV)
    seg_len = lens.astype(np.int32)
    skip = 8  # the 1000-sample segment: seg_len < 0 leaves its outputs untouched
    if with_len:
        seg_len[skip] = -5
    q = ops.segment_quantiles_ragged(_dev(host), torch.from_numpy(off).to(DEV),
                                     torch.from_numpy(seg_len).to(DEV) if with_len else None,
                                     max_len=int(lens.max()), permille=PM, aligned16=False, out=out, num=num)
    assert q is out
    ref = np.stack([_ref(host[off[i]: off[i] + lens[i]], PM) for i in range(nseg)], axis=1)
    want_num = lens.astype(np.int32)
    if with_len:
        ref[:, skip] = SENT
        want_num[skip] = -7
    _same_bits(q, ref)
    assert np.all(np.isnan(q.cpu().numpy()[:, 0]))  # the empty segment
    assert num.cpu().tolist() == want_num.tolist()


def test_ragged_cap_and_aligned16():
    # ring retention per segment (the last `cap`), runs on 16-byte boundaries as the bucketing lays them
    rng = np.random.default_rng(5)
    lens = np.array([5, 300, 9000, 0, 8192, 70], np.int64)
    cap = 4096
    off = np.zeros(len(lens), np.int64)
    pos = 0
    for i, n in enumerate(lens):
        off[i] = pos
        pos += (int(n) + 3) // 4 * 4
    host = rng.integers(1000, 3_000_000, size=pos + 4, dtype=np.uint32)
    num = torch.empty(len(lens), dtype=torch.int32, device=DEV)
    q = ops.segment_quantiles_ragged(_dev(host), torch.from_numpy(off).to(DEV),
                                     torch.from_numpy(lens.astype(np.int32)).to(DEV),
                                     max_len=int(lens.max()), permille=PM, cap=cap, aligned16=True, num=num)
    ref = np.stack([_ref(host[off[i] + max(0, lens[i] - cap): off[i] + lens[i]], PM)
                    for i in range(len(lens))], axis=1)
    _same_bits(q, ref)
    assert num.cpu().tolist() == np.minimum(lens, cap).tolist()


def test_zero_segments():
    ns = _dev(np.arange(16, dtype=np.uint32))
    q = ops.segment_quantiles_ragged(ns, torch.zeros(1, dtype=torch.int64, device=DEV), None, 0, PM)
    assert tuple(q.shape) == (len(PM), 0) and q.dtype == torch.float32
    q = ops.segment_quantiles_strided(ns, 0, 8, 0, 8, (500,))
    assert tuple(q.shape) == (1, 0)


def test_device_and_dtype_checks():
    ns = _dev(np.arange(64, dtype=np.uint32))
    with pytest.raises(ValueError, match="exceed"):
        ops.segment_quantiles_strided(ns, 9, 8, 0, 8, PM)
    with pytest.raises(TypeError):
        ops.segment_quantiles_strided(ns.float(), 8, 8, 0, 8, PM)
    with pytest.raises(ValueError, match="device"):
        ops.segment_quantiles_strided(ns.cpu(), 8, 8, 0, 8, PM)
    with pytest.raises(ValueError, match="out"):
        ops.segment_quantiles_strided(ns, 8, 8, 0, 8, PM, out=torch.empty((3, 8), device=DEV))


def test_graph_replay():
    # one strided call captured in a single-stream graph (linear: the kernels of one call follow
    # each other on the capture stream), replayed on changed input
    R, K, S, cap = 2, 12, 10000, 8192
    ns = synth.synth_matrix(R, K, S, device=DEV)
    out = torch.empty((len(PM), R * K), dtype=torch.float32, device=DEV)
    ops.segment_quantiles_strided(ns.view(-1), R * K, S, 0, S, PM, cap=cap, out=out)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.segment_quantiles_strided(ns.view(-1), R * K, S, 0, S, PM, cap=cap, out=out)
    for seed in (2024, 77):
        synth.synth_matrix(R, K, S, seed=seed, device=DEV, out=ns)
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        host = ns.cpu().numpy().view(np.uint32).reshape(-1)
        _same_bits(out, _ref_strided(host, R * K, S, 0, S, cap, PM), seed)
