"""Reference and layout model of the record bucketing kernel (csrc/records.hip): numpy, no GPU.

retain() is the contract: per (stream, slot) the push count and the last `cap` ns in push order,
written as a stable grouping by slot.  It knows nothing of the kernel.

launch(), layout(), sources() and walk() restate, by hand, where records_bucket_kernel reads a
record from and where it puts a bucket: control flow and positions only, no arithmetic on samples
(as tests/_quantile_trace.py does for the quantile kernels).  tests/_records_cases.py sizes its
streams from them, tests/test_records_model_cpu.py proves each case's claim on them, and
tests/test_gpu_records_branches.py ties the device to them through the bucket order."""
from collections import namedtuple

import numpy as np

# These follow csrc/records.hip (and NVRX_RECORDS_MAX_LDS csrc/nvrx_internal.h); a constant that
# changes there is changed here by hand, and the cases then say which of them are mis-aimed.
RB_LDS_KB = 160
RB_STAGE_KB = 96
RB_WAVES = 16
RB_REGS_PER_BLOCK = 16384
RB_COLD = 512
RB_TINY = 8
RB_UNROLL = 8
NVRX_RECORDS_MAX_LDS = 144 * 1024

RB_PASS_SLOTS = NVRX_RECORDS_MAX_LDS // 12      # three u32 counters per slot
HEAD_RECORDS = 2 * RB_REGS_PER_BLOCK            # the register head, in records
BATCH_PAIRS = 64 * RB_UNROLL                    # pairs one unrolled iteration of a wave reads

REG, STASH, UNROLL, TAIL, SCALAR = range(5)
SOURCE_NAMES = ("register head", "LDS stash", "unrolled re-read", "re-read tail", "scalar path")


# ------------------------------------------------------------------ the contract
Retained = namedtuple("Retained", "counts kept")


def retain(recs, off, nslots, cap):
    """recs [n, 2] u32 {slot, ns}, off [nstreams + 1].  counts[t * nslots + s]: pushes of slot s in
    stream t; kept[t * nslots + s]: the last `cap` of their ns in push order (cap 0: all of them).
    Records of slots >= nslots are dropped."""
    recs = np.asarray(recs, np.uint32).reshape(-1, 2)
    nstreams = len(off) - 1
    counts = np.zeros(nstreams * nslots, np.int64)
    kept = []
    for t in range(nstreams):
        stream = recs[off[t]:off[t + 1]]
        stream = stream[stream[:, 0] < nslots]
        slot = stream[:, 0].astype(np.int64)
        order = np.argsort(slot, kind="stable")  # by slot, push order inside a slot
        c = np.bincount(slot, minlength=nslots)
        counts[t * nslots:(t + 1) * nslots] = c
        for pushed in np.split(stream[order, 1], np.cumsum(c)[:-1]):
            kept.append(pushed[-cap:] if cap > 0 else pushed)
    return Retained(counts, kept)


def passes(nslots):
    """[(slot_lo, nslots_pass)] of a slot table: one bucketing pass per RB_PASS_SLOTS slots."""
    return [(lo, min(RB_PASS_SLOTS, nslots - lo)) for lo in range(0, nslots, RB_PASS_SLOTS)]


# ------------------------------------------------------------------ records_bucket_pass
Launch = namedtuple("Launch", "stage_cap stash_pairs")


def launch(nslots_pass):
    lds_launch = max(nslots_pass * 12, RB_LDS_KB * 1024 - 256)
    counters = ((3 * nslots_pass + 3) & ~3) * 4
    stage_cap = 0
    if lds_launch > counters:
        stage_cap = min(RB_STAGE_KB * 256, (lds_launch - counters) // 4) & ~3
    fixed = counters + stage_cap * 4
    stash_pairs = 0
    if lds_launch > fixed:
        stash_pairs = ((lds_launch - fixed) // (16 * RB_WAVES)) & ~63
    return Launch(stage_cap, stash_pairs)


# ------------------------------------------------------------------ the scan
Layout = namedtuple("Layout", "tier st padded overflow reduced tiny_end cold_total stage_lim skip")


def layout(counts, cap, nslots_pass, for_stats):
    """Where one stream's buckets of one pass go (positions relative to the stream's base), from
    the pushes per slot.  tier 0: kept everything, <= RB_TINY; 1: kept everything, <= RB_COLD;
    2: the rest.  The tiers follow one another, slot order inside a tier.  for_stats: the launch
    comes from records_stats, which lets the kernel reduce staged tiny buckets itself."""
    counts = np.asarray(counts, np.int64)
    assert counts.size == nslots_pass
    stage_cap = launch(nslots_pass).stage_cap
    keep = np.where((cap > 0) & (counts > cap), cap, counts)
    overflow = keep != counts
    tier = np.where(overflow | (keep > RB_COLD) | (stage_cap == 0), 2, np.where(keep <= RB_TINY, 0, 1))
    padded = (keep + 3) & ~3
    st = np.zeros(nslots_pass, np.int64)
    pos = 0
    ends = []
    for k in range(3):
        for s in np.flatnonzero(tier == k):
            st[s] = pos
            pos += padded[s]
        ends.append(pos)
    tiny_end, cold_total = ends[0], ends[1]
    stage_lim = min(cold_total, stage_cap)
    reduced = (tier == 0) & (keep >= 1) & (st + padded <= stage_lim) & bool(for_stats)
    skip = tiny_end // 4 if for_stats and tiny_end <= stage_lim else 0
    return Layout(tier, st, padded, overflow, reduced, tiny_end, cold_total, stage_lim, skip)


# ------------------------------------------------------------------ pass 2's reads
Wave = namedtuple("Wave", "lo hi wpairs snp iters per_it stash_loop stash_final short_iter")
Sources = namedtuple("Sources", "src waves rp")


def sources(n, r0_odd, nslots_pass):
    """Which of the five sources pass 2 takes each of a stream's n records from.  r0_odd: the
    stream starts at an odd record index, so it is not 16-byte aligned.  Per wave: its chunk
    [lo, hi) of the rest, wpairs, the pairs in its stash, the unrolled iterations every lane makes
    and the stash entries per lane interleaved with each; of lane 0's stash entries, how many the
    loop places and how many the final place_stash, and whether an iteration asked for more stash
    than was left."""
    S = launch(nslots_pass).stash_pairs
    pairs = not r0_odd
    rp = min(n >> 1, RB_REGS_PER_BLOCK) if pairs else 0
    src = np.full(n, -1, np.int8)
    src[:2 * rp] = REG
    n_rest = n - 2 * rp
    per = ((n_rest + RB_WAVES - 1) // RB_WAVES + 1) & ~1
    waves = []
    for w in range(RB_WAVES):
        lo = 2 * rp + min(n_rest, per * w)
        hi = min(n, lo + per)
        wpairs = pairs and (hi - lo) % 2 == 0
        np_ = (hi - lo) >> 1 if wpairs else 0
        snp = min(np_, S)
        iters = (np_ - snp) // BATCH_PAIRS
        entries = (snp + 63) // 64
        per_it = (snp // 64 + iters - 1) // iters if iters > 0 else 0
        in_loop = min(entries, per_it * iters)
        waves.append(Wave(lo, hi, wpairs, snp, iters, per_it, in_loop, entries - in_loop,
                          per_it * iters > entries))
        if not wpairs:
            src[lo:hi] = SCALAR
            continue
        p = np.arange(np_)
        rel = p - snp
        # a lane's unrolled iteration k reads pairs snp + lane + 512 k + 64 u, u < RB_UNROLL, while
        # the last of them is inside the chunk
        first = snp + rel % 64 + BATCH_PAIRS * (rel // BATCH_PAIRS)
        kind = np.where(p < snp, STASH, np.where(first + 64 * (RB_UNROLL - 1) < np_, UNROLL, TAIL))
        src[lo:hi] = np.repeat(kind, 2)
    assert (src >= 0).all()
    return Sources(src, waves, rp)


# ------------------------------------------------------------------ the ordered walk
Group = namedtuple("Group", "slot lanes occ0 drop")
Step = namedtuple("Step", "groups kept invalid lanes")


def walk(slots, nslots_pass, cap, slot_lo=0):
    """Wave 0's walk over a stream in steps of 64 records: per step the ballot groups of the
    overflowed slots (local slot, lanes, occurrences before the step, records the ring drops), in
    leader order, and how many lanes hold records of kept slots and of slots outside the pass."""
    ls = (np.asarray(slots, np.uint32) - np.uint32(slot_lo)).astype(np.int64)  # wraps below slot_lo
    valid = ls < nslots_pass
    cnt = np.bincount(ls[valid], minlength=nslots_pass)
    ovf = (cnt > cap) if cap > 0 else np.zeros(nslots_pass, bool)
    seen = np.zeros(nslots_pass, np.int64)
    steps = []
    for b in range(0, ls.size, 64):
        l, v = ls[b:b + 64], valid[b:b + 64]
        ok = v.copy()
        ok[v] = ovf[l[v]]
        groups = []
        for s in dict.fromkeys(l[ok].tolist()):
            lanes = np.flatnonzero(ok & (l == s))
            groups.append(Group(s, lanes, int(seen[s]), int(cnt[s] - cap)))
            seen[s] += lanes.size
        steps.append(Step(groups, int((v & ~ok).sum()), int((~v).sum()), l.size))
    return steps
