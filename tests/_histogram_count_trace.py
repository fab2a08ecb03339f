"""A small integer model of the COUNTING of csrc/segment_histogram.hip (`count_reg`, `Kept`) over one
wave's registers in trip order, and of the register order of the wave kernel and of one wave of the
workgroup kernel.  Numpy, no GPU.

tests/test_segment_gate_model_cpu.py uses it to prove, from the keys alone, that a constructed
segment of tests/_segment_gate_cases.py reaches the counting event it was built for.  The model
decides nothing about correctness on the device: the GPU tests compare with np.bincount, and the
model's own final counts are compared with np.bincount as well.

    a register        64 lanes, one slot each: the bucket of the key in that slot, SPARE for a slot
                      outside the retained run (a masked lane, or a clamped re-read)
    wave kernel       trip t, vector u < WV, component c < 4, lane L: slot 1024 t + 256 u + 4 L + c - m0
    workgroup kernel  wave w, thread 64 w + L: slot 4 (4096 t + 1024 u + 64 w + L) + c - m0
    count_reg         p0 / p1 lanes hit the kept buckets; with HIST_REPLACE or more of the others
                      missing, the kept bucket with fewer hits (b0 on a tie) is flushed and replaced
                      by the bucket of the first missing lane
"""
from collections import namedtuple

import numpy as np

from nvidia_resiliency_ext.straggler import histograms
from _segment_gate_model import HIST_REPLACE, HS_THREADS, WV

BINS = histograms.BINS
SPARE, SPARE2 = BINS, BINS + 1

# one register: hits of the kept buckets, misses, and for a replacement the side ("b0" / "b1"),
# the bucket evicted with the count flushed for it, and the bucket adopted
Reg = namedtuple("Reg", "trip p0 p1 miss distinct side evicted flushed adopted")
Trace = namedtuple("Trace", "regs counts spare end")   # end: the Kept state (b0, c0, b1, c1) before flush_kept


def wave_slots(n, m0):
    """[registers, 64] slot numbers of the wave kernel in the order count_reg sees them."""
    nvec = (n + m0 + 3) >> 2
    trips = (nvec + 64 * WV - 1) // (64 * WV)
    t, u, c, lane = np.meshgrid(np.arange(trips), np.arange(WV), np.arange(4), np.arange(64), indexing="ij")
    return (1024 * t + 256 * u + 4 * lane + c - m0).reshape(-1, 64), 4 * WV


def block_slots(n, m0, wave):
    """The same for wave `wave` of the workgroup kernel (a clamped re-read lies past n: masked)."""
    nvec = (n + m0 + 3) >> 2
    tv = HS_THREADS * WV
    trips = (nvec + tv - 1) // tv
    t, u, c, lane = np.meshgrid(np.arange(trips), np.arange(WV), np.arange(4), np.arange(64), indexing="ij")
    return (4 * (tv * t + HS_THREADS * u + 64 * wave + lane) + c - m0).reshape(-1, 64), 4 * WV


def trace(keys, m0, kernel="wave", wave=0):
    """count_reg over every register of one wave; counts: the wave's 240 bins after flush_kept."""
    keys = np.asarray(keys, np.uint32)
    n = int(keys.size)
    assert n >= 1 and 0 <= m0 < 4
    slots, per_trip = wave_slots(n, m0) if kernel == "wave" else block_slots(n, m0, wave)
    live = (slots >= 0) & (slots < n)
    b = np.where(live, histograms.bucket_of(keys)[np.clip(slots, 0, n - 1)], SPARE)
    h = np.zeros(BINS + 2, np.int64)
    b0, c0, b1, c1 = SPARE, 0, SPARE2, 0
    regs = []
    for r in range(b.shape[0]):
        row = b[r]
        h0, h1 = row == b0, row == b1
        p0, p1 = int(h0.sum()), int(h1.sum())
        c0 += p0
        c1 += p1
        rest = ~(h0 | h1)
        miss = int(rest.sum())
        side = evicted = flushed = adopted = None
        if miss:
            np.add.at(h, row[rest], 1)
            if miss >= HIST_REPLACE:
                adopted = int(row[np.argmax(rest)])     # the first missing lane's bucket
                if p0 <= p1:
                    side, evicted, flushed = "b0", b0, c0
                    h[b0] += c0
                    b0, c0 = adopted, 0
                else:
                    side, evicted, flushed = "b1", b1, c1
                    h[b1] += c1
                    b1, c1 = adopted, 0
        assert b0 != b1, (r, b0, b1)                     # Kept's invariant
        regs.append(Reg(r // per_trip, p0, p1, miss, int(np.unique(row).size), side, evicted, flushed, adopted))
    end = (b0, c0, b1, c1)
    h[b0] += c0
    h[b1] += c1
    return Trace(regs, h[:BINS].copy(), int(h[SPARE]), end)


def events(tr):
    """The names of what a trace met (the counting aims of tests/_segment_gate_cases.py)."""
    ev = set()
    repl = [r for r in tr.regs if r.side]
    for r in tr.regs:
        if r.miss == HIST_REPLACE - 1:
            ev.add("miss15_no_replacement")
            assert r.side is None
        if r.miss == HIST_REPLACE:
            ev.add("miss16_replacement")
            assert r.side is not None
        if r.distinct == 64:
            ev.add("distinct64")
    for r in repl:
        ev.add("flush_empty" if r.flushed == 0 else "flush_nonempty")
        if r.p0 == r.p1 and r.p0 > 0:
            ev.add("p_equal")
    sides = "".join("0" if r.side == "b0" else "1" for r in repl)
    if "0101" in sides or "1010" in sides:
        ev.add("alternate")
    gone = set()
    spare_left = False
    for r in repl:
        if r.adopted in gone:
            ev.add("readopt_spare" if r.adopted == SPARE else "readopt")
        gone.add(r.evicted)
        if r.evicted == SPARE:
            ev.add("spare_evicted_nonempty" if r.flushed else "spare_evicted")
            spare_left = True
    if spare_left and ((tr.end[0] == SPARE and tr.end[1]) or (tr.end[2] == SPARE and tr.end[3])):
        ev.add("spare_flushed_at_end")
    last = tr.regs[-1].trip
    if any(r.trip == last and r.adopted == SPARE and r.miss >= HIST_REPLACE for r in repl):
        ev.add("spare_adopted_in_last_trip")
    return ev
