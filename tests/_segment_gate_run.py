"""Runs one launch of tests/_segment_gate_cases.py on the GPU from sentinel-filled outputs and checks
every row: a retained segment bit for bit against np.sort / np.bincount of its retained keys, an
empty one as NaN / zero bins with num 0, a skipped one as the untouched sentinel.  Shared by
tests/test_gpu_quantile_gates.py and tests/test_gpu_histogram_gates.py."""
import zlib

import numpy as np
import torch

import _segment_gate_cases as C
import oracle as O
from nvidia_resiliency_ext.straggler import histograms, ops

DEV = "cuda"
PM = (0, 1, 250, 500, 900, 990, 999, 1000)
QSENT = np.float32(-12345.0)
HSENT = -123456789
NSENT = -7
BINS = histograms.BINS


def quantile_ref(retained, pm=PM):
    """[len(pm)] float32: rank (pm (n - 1)) // 1000 of the sorted keys, converted as every sample."""
    n = int(len(retained))
    s = np.sort(np.asarray(retained, np.uint32))
    keys = np.array([s[(int(p) * (n - 1)) // 1000] for p in pm], np.uint32)
    return O.key_to_f32(keys).astype(np.float32) / np.float32(1000)


def histogram_ref(retained):
    return np.bincount(histograms.bucket_of(np.asarray(retained, np.uint32)), minlength=BINS).astype(np.int64)


def _dev(host_u32):
    return torch.from_numpy(np.ascontiguousarray(host_u32, np.uint32).view(np.int32)).to(DEV)


def launch(c, host):
    """(out, num) on the host: quantiles float32 [nq, nseg], histogram int32 [nseg, 240]."""
    nseg = len(C.case_segments(c))
    num = torch.full((nseg,), NSENT, dtype=torch.int32, device=DEV)
    if c.family == "quantiles":
        out = torch.full((len(PM), nseg), float(QSENT), dtype=torch.float32, device=DEV)
    else:
        out = torch.full((nseg, BINS), HSENT, dtype=torch.int32, device=DEV)
    ns = _dev(host)
    assert ns.data_ptr() % 16 == 0
    if isinstance(c, C.Strided):
        ns = ns[c.base_off:]   # a view whose base lies base_off elements off the 16-byte grid
        args = (ns, nseg, c.stride, c.begin, c.length)
        if c.family == "quantiles":
            ops.segment_quantiles_strided(*args, PM, cap=c.cap, out=out, num=num)
        else:
            ops.segment_histogram_strided(*args, cap=c.cap, out=out, num=num)
    else:
        off = torch.from_numpy(c.off).to(DEV)
        seg_len = torch.from_numpy(c.lens.astype(np.int32)).to(DEV) if c.seg_form == "len" else None
        if c.family == "quantiles":
            ops.segment_quantiles_ragged(ns, off, seg_len, c.max_len, PM, cap=c.cap, aligned16=c.aligned16,
                                         out=out, num=num)
        else:
            ops.segment_histogram_ragged(ns, off, seg_len, c.max_len, cap=c.cap, aligned16=c.aligned16,
                                         out=out, num=num)
    return out.cpu().numpy(), num.cpu().numpy()


def check(c, host, out, num):
    strided = isinstance(c, C.Strided)
    for s, (n, ph) in enumerate(C.case_segments(c)):
        what = (c.name, s, n, ph)
        run = C.strided_retained(c, host, s) if strided else C.ragged_retained(c, host, s)
        row = out[:, s] if c.family == "quantiles" else out[s]
        if n < 0:      # skipped: untouched
            assert (row == (QSENT if c.family == "quantiles" else HSENT)).all() and num[s] == NSENT, what
            continue
        assert num[s] == n and run.size == n, what + (int(num[s]),)
        if c.family == "quantiles":
            if n == 0:
                assert np.isnan(row).all(), what
            else:
                ref = quantile_ref(run)
                assert np.array_equal(row.view(np.uint32), ref.view(np.uint32)), what + (row, ref)
        else:
            ref = histogram_ref(run) if n else np.zeros(BINS, np.int64)
            got = row.view(np.uint32).astype(np.int64)
            assert np.array_equal(got, ref), what + (np.nonzero(got != ref)[0][:4], got.sum())


def run_case(c):
    host = C.host_keys(c, zlib.crc32(c.name.encode()))
    out, num = launch(c, host)
    check(c, host, out, num)
    return host, out, num
