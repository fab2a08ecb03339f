"""A plain model of the CONTROL FLOW of csrc/segment_quantiles.hip (integers only, no GPU): which
class a segment runs in, and for every visit of quant_core's loop the window, the group of ranks
and the exit taken; for the streaming kernel the prefixes of every pass and the ranks sharing each.

tests/test_quantile_trace_cpu.py uses it to prove, from the keys alone, that a constructed segment
reaches the branch it was built for; tests/test_gpu_quantile_branches.py then runs those segments.
The model decides nothing about correctness: results are compared with np.sort, and the model's
own quantiles are checked against np.sort as well.

Constants and the source lines they restate:
    QCAND = 64                      segment_quantiles.hip  `constexpr int QCAND = 64`
    QUANT_WAVE_MAX = 64 * 128       segment_quantiles.hip  `constexpr int QUANT_WAVE_MAX`
    class PL: 32 PL < need <= 64 PL segment_quantiles.hip  `need > 64 * PL || (PL > 4 && need <= 32 * PL)`
    NB, LOG                         segment_wave.h         `struct Bins`
    sh <= 26                        segment_quantiles.hip  the two rank encodings of a compaction
"""
from collections import namedtuple

import numpy as np

from nvidia_resiliency_ext.straggler import _native

NQ = _native.NVRX_MAX_QUANTILES
QCAND = 64
QUANT_WAVE_MAX = 64 * 128
CLASSES = (4, 8, 16, 32, 64, 128)
ENC_SPLIT = 26
M32 = 0xFFFFFFFF

# one visit of quant_core's loop.  level: 1 for a window that is the whole range, + 1 per histogram
# level the group went through; count: samples in the window (the padding removed); ranks: the
# indices (positions in the permille list) of the group; exit: one_value / compact_le26 /
# compact_gt26 / histogram; padin: the padding (copies of sample 0) lies in the window.
Visit = namedtuple("Visit", "level sh lo count ranks exit padin")
WaveTrace = namedtuple("WaveTrace", "PL NB LOG pad bits keys visits")
# one pass of the streaming kernel: prefixes[h] is histogram h's prefix, share[h] the ranks using it
Pass = namedtuple("Pass", "prefixes share")
StreamTrace = namedtuple("StreamTrace", "head nvec tail keys passes")


def bins(PL):
    """(NB, LOG) of Bins<PL>: 16 bins per lane-sample up to PL 16, 8 above, within [64, 512]."""
    pb = 16 * PL if PL <= 16 else 8 * PL
    nb = min(max(pb, 64), 512)
    return nb, nb.bit_length() - 1


def wave_class(n, m0):
    """The PL whose kernel takes a segment of n samples starting m0 slots into a 16-byte vector,
    None when it streams (need = n + m0 above QUANT_WAVE_MAX)."""
    need = n + m0
    for PL in CLASSES:
        if need <= 64 * PL and (PL == 4 or need > 32 * PL):
            return PL
    assert need > QUANT_WAVE_MAX
    return None


def ranks(n, pm):
    return [(int(p) * (n - 1)) // 1000 for p in pm]


def wave_trace(keys, m0, pm):
    """quant_core on one segment's retained keys (push order: keys[0] is sample 0, the padding)."""
    k = np.asarray(keys, np.uint32).astype(np.int64)
    n, nq = int(k.size), len(pm)
    assert n >= 1 and 1 <= nq <= NQ and 0 <= m0 < 4
    PL = wave_class(n, m0)
    NB, LOG = bins(PL)
    pad = 64 * PL - n
    mn, mx = int(k.min()), int(k.max())
    d = k - mn
    cp = int(k[0]) - mn                      # the padding's d
    bits = (mx - mn).bit_length()            # 32 - clz(mx - mn)
    tq = ranks(n, pm)
    lo_, sh_, below_, cnt_, lev_ = [0] * nq, [bits] * nq, [0] * nq, [n] * nq, [1] * nq
    res = [None] * nq
    todo = list(range(nq))
    visits = []
    for _ in range(7 * NQ):                  # MAXIT
        if not todo:
            break
        q = todo[0]
        lo, sh, below, cnt, level = lo_[q], sh_[q], below_[q], cnt_[q], lev_[q]
        grp = [r for r in todo if lo_[r] == lo and sh_[r] == sh]
        wm1 = M32 if sh >= 32 else (1 << sh) - 1
        padin = pad != 0 and ((cp - lo) & M32) <= wm1
        if sh == 0:
            for r in grp:
                res[r] = lo
            visits.append(Visit(level, sh, lo, cnt, tuple(grp), "one_value", padin))
        elif cnt <= QCAND:
            cand = np.sort(d[((d - lo) & M32) <= wm1])   # the real samples of the window
            assert cand.size == cnt, (cand.size, cnt)
            for r in grp:
                res[r] = int(cand[tq[r] - below])
            visits.append(Visit(level, sh, lo, cnt, tuple(grp),
                                "compact_le26" if sh <= ENC_SPLIT else "compact_gt26", padin))
        else:
            s2 = sh - LOG if sh > LOG else 0
            rel = (d - lo) & M32
            h = np.bincount(rel[rel <= wm1] >> s2, minlength=NB)
            assert h.size == NB and int(h.sum()) == cnt
            incl = np.cumsum(h)
            for r in grp:
                b = int(np.searchsorted(incl, tq[r] - below, side="right"))
                lo_[r], sh_[r], cnt_[r], lev_[r] = lo + (b << s2), s2, int(h[b]), level + 1
                below_[r] = below + int(incl[b] - h[b])
            visits.append(Visit(level, sh, lo, cnt, tuple(grp), "histogram", padin))
            continue
        todo = [r for r in todo if r not in grp]
    assert not todo
    return WaveTrace(PL, NB, LOG, pad, bits, [mn + r for r in res], visits)


def stream_trace(keys, m0, pm):
    """seg_quantiles_stream_kernel on one segment: four 8-bit passes from the top."""
    k = np.asarray(keys, np.uint32).astype(np.int64)
    n, nq = int(k.size), len(pm)
    assert wave_class(n, m0) is None and 1 <= nq <= NQ
    head = min((4 - m0) & 3, n)
    nvec = (n - head) >> 2
    t = ranks(n, pm)
    key = [0] * nq
    prefixes, share_of = [0], [0] * nq       # s_pf, s_h
    passes = []
    for p in range(4):
        shift = 24 - 8 * p
        passes.append(Pass(tuple(prefixes), tuple(tuple(q for q in range(nq) if share_of[q] == h)
                                                  for h in range(len(prefixes)))))
        hi = k >> (shift + 8)
        dg = (k >> shift) & 255
        hists = [np.bincount(dg[hi == pf], minlength=256) for pf in prefixes]
        for q in range(nq):
            h = hists[share_of[q]]
            incl = np.cumsum(h)
            b = int(np.searchsorted(incl, t[q], side="right"))
            t[q] -= int(incl[b] - h[b])
            key[q] = (key[q] << 8) | b
        if p < 3:
            prefixes = []
            for q in range(nq):
                if key[q] not in prefixes:
                    prefixes.append(key[q])
                share_of[q] = prefixes.index(key[q])
    return StreamTrace(head, nvec, n - head - 4 * nvec, key, passes)


def trace(keys, m0, pm):
    return stream_trace(keys, m0, pm) if wave_class(len(keys), m0) is None else wave_trace(keys, m0, pm)
