"""A plain model of the CONTROL FLOW of the median select in csrc/segment_wave.h (`lean_core` and
`hist_locate1`; integers only, no torch, no GPU): per visit of lean_core's loop the level, the
window, where the padding lies, what every hist_locate1 call finds (row of lanes, lane, bin in
the lane) and the exit taken; and which instantiation `lean_core<PL, FULL, KB>` each of the four
FAST kernel families compiles for a segment (`instantiation`).

tests/test_median_trace_cpu.py uses it to prove, from the keys alone, that a constructed segment
of tests/_median_cases.py reaches the branch it was built for; tests/test_gpu_median_branches.py
then runs those segments.  The model decides nothing about correctness -- the kernels are compared
with the oracle -- and nothing about the sums (tests/_moments_ref.py `branch`), the loads or the
epilogues.  Its own two middle ranks are asserted against np.sort in every call.

Constants and the source lines they restate:
    NB, LOG, BPL                segment_wave.h  `struct Bins` (PB = 16 PL up to PL 16, 8 PL above; NB in [64, 512])
    CAND = 64                   segment_wave.h  `if (n0 <= 64u)` (the candidates fill one wave)
    LEVELS                      segment_wave.h  `constexpr int LEVELS = (32 + LOGNB - 1) / LOGNB + 1`
    B = 0x4B000000 below 2^23   segment_wave.h  `const unsigned B = range < (1u << 23) ? 0x4B000000u : 0u`
    pivot                       segment_wave.h  `median3`: p[0], p[n / 2], p[n - 1] (issue_probes; lean_core FULL)
    slot of register i, lane L  segment_wave.h  `eb + 256 (i >> 2) + (i & 3)`, eb = 4 L - m0
    strided class               segment_stats.hip  `launch_fast` (need = keep, + 3 when misaligned), KB = PL <= 16
    ragged class                tests/_ragged_model.py `seg_class`; segment_ragged_kernels.h `ListKeepBin` (PL <= 8)

Branches the model proves dead (asserted in every call, never aimed at):
    the `shift > 26` rank loop  shift starts at bits - LOG <= 32 - 6 and only falls: every
                                compaction packs (candidate - lo0) << 6 | lane into one word
    `min(..., 63)` on La        hist_locate1 is called with ta < the window's count, so in the row
                                holding ta fewer than 16 lanes have an inclusive prefix <= ta - rbase
    `found == false`            for the same reason the walk over lane La's bins passes ta
"""
from collections import namedtuple

import numpy as np

import _ragged_model as RM

CAND = 64
CLASSES = (4, 8, 16, 32, 64, 128)
B23 = 0x4B000000
M32 = 0xFFFFFFFF
EXITS = ("two_buckets", "one_value", "compact_masked", "compact_keepbin", "compact_plain", "descend")
FAMILIES = ("strided_masked", "strided_full", "ragged_list", "ragged_full")

# one hist_locate1 call: the DPP row and lane holding rank ta, the bin inside the lane, and its
# three results (bucket, samples of the window below it, its count)
Locate = namedtuple("Locate", "ta row lane j ba bfa ca")
# one visit of lean_core's loop.  wlo: the window's low end less B; pad_bin: the bin clear_bins
# pre-loads with -pad (None: no padding, or the window does not hold it -- pad_side then says
# "below" / "above"); pad_at: where the padding lies for this visit's exit: "none" (pad = 0),
# "bucket" (the median's), "window" (another bucket of the window), "below", "above"; for
# two_buckets "lt_hi0" / "ge_lo1".  The compact exits: n0, r0, r1, the lanes L0 / L1 whose
# candidates are taken, the candidates in LDS order, ties of s[t0] / s[t1] inside the bucket.
Visit = namedtuple("Visit", "level shift wlo below pad_bin pad_side pad_at locs exit n0 r0 r1 L0 L1 cands "
                            "tie0 tie1")
Trace = namedtuple("Trace", "PL full kb n m0 NB LOG BPL mn mx bits hasB pad pad_key visits d0 d1")


def bins(PL):
    """(NB, LOG, BPL) of Bins<PL>."""
    pb = 16 * PL if PL <= 16 else 8 * PL
    nb = min(max(pb, 64), 512)
    return nb, nb.bit_length() - 1, nb // 64


def levels(LOG):
    return (32 + LOG - 1) // LOG + 1


def median3(a, b, c):
    return max(min(a, b), min(max(a, b), c))


def slot_order(PL, n, m0):
    """The segment slot (push position) of every register in the order the compactions walk them
    (register i, then lane); -1 for a slot outside the segment (it holds the padding)."""
    i = np.arange(PL)[:, None]
    lane = np.arange(64)[None, :]
    e = (256 * (i >> 2) + 4 * lane + (i & 3) - m0).reshape(-1)
    return np.where((e >= 0) & (e < n), e, -1)


def _locate(h, ta, BPL):
    """hist_locate1 on the bins h (the padding's bin already net of its -pad)."""
    total = int(h.sum())
    assert 0 <= ta < total, (ta, total)
    local = h.reshape(64, BPL).sum(axis=1)
    v = np.concatenate([np.cumsum(local[r * 16:(r + 1) * 16]) for r in range(4)])
    t0 = int(v[15])
    t1 = t0 + int(v[31])
    t2 = t1 + int(v[47])
    row = 0 if ta < t0 else 1 if ta < t1 else 2 if ta < t2 else 3
    rbase = (0, t0, t1, t2)[row]
    before = int((v[16 * row:16 * row + 16] <= ta - rbase).sum())
    assert before < 16, "dead: min(..., 63) never clamps"
    La = 16 * row + before
    hs = h[La * BPL:(La + 1) * BPL]
    run = rbase + int(v[La]) - int(hs.sum())
    for j in range(BPL):
        nxt = run + int(hs[j])
        if nxt > ta:
            return Locate(ta, row, La, j, La * BPL + j, run, int(hs[j]))
        run = nxt
    raise AssertionError("dead: hist_locate1 always finds the bin")


def lean_trace(keys, PL, full, kb, m0=0):
    """lean_core<PL, full, kb> on one segment's retained keys in push order, the run starting m0
    slots into its first 16-byte vector."""
    k = np.asarray(keys, np.uint32).astype(np.int64)
    n = int(k.size)
    NB, LOG, BPL = bins(PL)
    assert 1 <= n and n + m0 <= 64 * PL and 0 <= m0 < 4
    assert not full or (n == 64 * PL and m0 == 0)
    pad = 0 if full else 64 * PL - n
    mn, mx = int(k.min()), int(k.max())
    rng = mx - mn
    B = B23 if rng < 1 << 23 else 0
    bits = rng.bit_length()
    cp = median3(int(k[0]), int(k[n // 2]), int(k[n - 1])) - mn
    xc = B + cp
    order = slot_order(PL, n, m0)
    real = order >= 0
    assert int(real.sum()) == n
    x = np.where(real, (k - mn + B)[np.maximum(order, 0)], xc)   # every register, padding included
    xr = x[real]
    srt = np.sort(k - mn)
    t0 = n // 2 if n & 1 else n // 2 - 1
    t1 = n // 2
    shift = bits - LOG if bits > LOG else 0
    assert shift <= 26, "dead: the shift > 26 rank loop"
    wlo, below = B, 0
    d0 = d1 = None
    visits = []
    for level in range(levels(LOG)):
        span = NB << shift
        # ---- clear_bins, then one atomic per register inside the window
        pad_bin = pad_side = None
        if pad:
            q = (xc - wlo) & M32
            if level == 0:
                pad_bin = (xc >> shift) & (NB - 1)
            elif q < span:
                pad_bin = q >> shift
            else:
                pad_side = "below" if xc < wlo else "above"
        if level == 0:
            h = np.bincount((x >> shift) & (NB - 1), minlength=NB)
        else:
            rel = (x - wlo) & M32
            h = np.bincount(rel[rel < span] >> shift, minlength=NB)
        assert h.size == NB
        if pad_bin is not None:
            h[pad_bin] -= pad
        relr = (xr - wlo) & M32
        assert np.array_equal(h, np.bincount(relr[relr < span] >> shift, minlength=NB)), "net bins = real samples"
        # ---- the one or two locates
        l0 = _locate(h, t0 - below, BPL)
        b0, c0, n0 = l0.ba, l0.bfa, l0.ca
        locs = [l0]
        b1 = b0
        if not t1 - below < c0 + n0:
            locs.append(_locate(h, t1 - below, BPL))
            b1 = locs[-1].ba
        lo0 = wlo + (b0 << shift)
        width = 1 << shift
        in_bucket = pad and ((xc - lo0) & M32) < width
        pad_at = ("none" if not pad else "bucket" if in_bucket else "window" if pad_bin is not None
                  else pad_side if level else "window")
        base = dict(level=level, shift=shift, wlo=wlo - B, below=below, pad_bin=pad_bin, pad_side=pad_side,
                    pad_at=pad_at, locs=tuple(locs), n0=n0, r0=None, r1=None, L0=None, L1=None, cands=None,
                    tie0=None, tie1=None)
        if b0 != b1:
            hi0 = wlo + ((b0 + 1) << shift)
            lo1 = wlo + (b1 << shift)
            assert hi0 <= M32 and lo1 <= M32
            d0 = int(((x - hi0) & M32).max()) + hi0 & M32
            d1 = int(((x - lo1) & M32).min()) + lo1 & M32
            if pad:
                base["pad_at"] = "lt_hi0" if xc < hi0 else "ge_lo1"
                assert xc < hi0 or xc >= lo1
            visits.append(Visit(exit="two_buckets", **base))
            break
        if shift == 0:
            d0 = d1 = wlo + b0
            visits.append(Visit(exit="one_value", **base))
            break
        if n0 <= CAND:
            masked = bool(not full and in_bucket)
            inb = ((x - lo0) & M32) < width
            if masked:
                inb &= real
                name = "compact_masked"
            else:
                name = "compact_keepbin" if kb and level == 0 else "compact_plain"
                if kb and level == 0:   # the kept level-0 bin of every register
                    assert np.array_equal(inb, ((x >> shift) & (NB - 1)) == b0)
            ci = x[inb]                                           # LDS order: register, then lane
            assert ci.size == n0, (ci.size, n0, name)
            assert shift <= 26
            key = (((ci - lo0) << 6) | np.arange(n0)) & M32
            assert int(key.max()) <= M32 and np.unique(key).size == n0
            lanes = np.full(64, M32, np.int64)
            lanes[:n0] = key
            nread = (n0 + 3) // 4 * 4                             # the loop unrolled by 4 reads these lanes
            rank = (lanes[None, :nread] < key[:, None]).sum(axis=1)
            r0, r1 = t0 - below - c0, t1 - below - c0
            L0, L1 = np.flatnonzero(rank == r0), np.flatnonzero(rank == r1)
            assert L0.size == 1 and L1.size == 1
            d0, d1 = int(ci[L0[0]]), int(ci[L1[0]])
            base.update(r0=r0, r1=r1, L0=int(L0[0]), L1=int(L1[0]), cands=tuple(int(c) - B for c in ci),
                        tie0=int((ci == d0).sum()) > 1, tie1=int((ci == d1).sum()) > 1)
            visits.append(Visit(exit=name, **base))
            break
        if n0 <= 2 * CAND:  # what a compaction would have met, for the tests' "65 taken as 64"
            base["cands"] = tuple(int(c) - B for c in x[(((x - lo0) & M32) < width) & real])
        visits.append(Visit(exit="descend", **base))
        below += c0
        wlo += b0 << shift
        shift = shift - LOG if shift > LOG else 0
    assert d0 is not None, "LEVELS visits always reach an exit"
    d0, d1 = d0 - B, d1 - B
    assert (d0, d1) == (int(srt[t0]), int(srt[t1])), (d0, d1, int(srt[t0]), int(srt[t1]))
    return Trace(PL, bool(full), bool(kb), n, m0, NB, LOG, BPL, mn, mx, bits, B != 0, pad, mn + cp,
                 tuple(visits), d0, d1)


# ---------------------------------------------------------------- which lean_core a segment runs
def _smallest_pl(need):
    return next((PL for PL in CLASSES if need <= 64 * PL), None)


def instantiation(family, n, phase=0, aligned16=True, full_n=0):
    """(PL, full, kb) of the lean_core a retained run of n samples runs in, None when the family
    does not take it (another family, a lane class, or the EXACT kernel).

    strided_masked / strided_full: `segment_stats_strided` with a stride that is a multiple of 4
    and the run starting `phase` slots into a 16-byte vector; the launch is the group kernel
    (FULL) when the run is aligned and exactly 64 PL long, else seg_stats_fast_kernel<PL, false>.
    ragged_list / ragged_full: the class of tests/_ragged_model.py under the caller's aligned16
    and the launch's FULL length."""
    if family in ("strided_masked", "strided_full"):
        aligned = phase == 0
        PL = _smallest_pl(n if aligned else n + 3)
        if PL is None:
            return None
        full = aligned and n == 64 * PL
        if full != (family == "strided_full"):
            return None
        return PL, full, PL <= 16
    cls = RM.seg_class(n, aligned16, False, full_n)
    if family == "ragged_full":
        return (n // 64, True, n // 64 <= 16) if cls == "F" else None
    assert family == "ragged_list", family
    return (RM.WAVE_PL[cls], False, RM.WAVE_PL[cls] <= 8) if cls in RM.WAVE_PL else None


def instantiations():
    """Every (family, PL, full, kb) that exists: 6 + 6 + 6 + 4."""
    out = [("strided_masked", PL, False, PL <= 16) for PL in CLASSES]
    out += [("strided_full", PL, True, PL <= 16) for PL in CLASSES]
    out += [("ragged_list", PL, False, PL <= 8) for PL in CLASSES]
    out += [("ragged_full", n // 64, True, n // 64 <= 16) for n in RM.FULL_LENS]
    return out


def reachable(family, full, kb):
    """The (exit, level >= 1) pairs and padding positions an instantiation can reach, and the
    pairs it cannot with the reason.  Padding: FULL has none; a strided masked launch always has
    some (pad = 0 there means aligned and 64 PL long, which is the group kernel's launch); the
    ragged list kernels meet pad = 0 in an aligned run of 64 PL that is not the FULL length."""
    pairs, dead = set(), {}
    for e in EXITS:
        for deep in (False, True):
            why = None
            if e == "compact_masked" and full:
                why = "FULL: no padding, `masked` is false at compile time"
            elif e == "compact_keepbin" and not kb:
                why = "KB false: no kept bins"
            elif e == "compact_keepbin" and deep:
                why = "the kept bins are level 0's (`KEEPBIN && level == 0`)"
            elif e == "compact_plain" and kb and not deep:
                why = "KB: an unmasked level-0 compaction is compact_keepbin"
            if why:
                dead[(e, deep)] = why
            else:
                pairs.add((e, deep))
    pads = {"bucket", "window", "below", "above", "lt_hi0", "ge_lo1"}
    pads = {"none"} if full else pads if family == "strided_masked" else pads | {"none"}
    return pairs, dead, pads
