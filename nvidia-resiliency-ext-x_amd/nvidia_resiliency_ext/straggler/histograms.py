"""The fixed buckets of the duration histograms, on the host (numpy only, no native library).

``ops.segment_histogram_*``, ``KernelProfiler.get_histograms``, ``Detector.kernel_histograms``
and ``MatrixReporter.histograms`` count duration keys (``_native.duration_keys``: plain ns below
3.76 s) into ``BINS`` = 240 log-linear buckets with 3 mantissa bits, each at most 12.5 % wide::

    bucket(x) = x                                  x < 8
              = 8*(e-2) + ((x >> (e-3)) & 7)       otherwise, e = x.bit_length() - 1
    edge(b)   = b                                  b < 8      (lower edge, a key)
              = (8 + b%8) << (b//8 - 1)            otherwise; edge(240) = 2**32

``bucket`` is monotone in the duration, ``edge(bucket(x)) <= x < edge(bucket(x) + 1)``, and
``edge(238) == KEY_WIDE``: buckets 238 and 239 hold exactly the durations of 3.76 s and more.
The edges are the same for every kernel, rank and report (they are part of the C ABI), so
counts add: ``merge`` over ranks gives the fleet-wide distribution of a kernel, over reports a
whole run's, and ``quantile_bounds`` brackets any quantile of the merged samples by one bucket.
``tail_threshold`` and ``tail_scores`` are the host twins (Python-integer sums) of the device's
tail scores (``ops.histogram_sum`` / ``histogram_tail_threshold`` / ``histogram_tail_scores``,
``MatrixReporter.tail_scores``, ``Detector.kernel_tail_score``): a per-rank score from the fleet's
summed histograms that sees a rank slow on every n-th call, which its median hides.
``history_scores`` is the host twin of the individual leg (``ops.histogram_history_scores``,
``MatrixReporter.individual_tail_scores``, ``Detector.kernel_individual_tail_score``): a rank's
interval against its own summed history, and the history with the interval folded in.
``tail_attribution`` / ``history_attribution`` are the host twins of the tail score attribution
(``ops.histogram_tail_attribution``, ``MatrixReporter.tail_scores(attribute=)``,
``Detector.kernel_tail_score(attribute=)`` and their individual legs): per rank the kernels with
the largest excess tail time in ns.
``segment_counts`` / ``segment_tail_scores`` are the host twins of the tail scores taken straight
from ragged segments, without the counts (``ops.segment_fleet_histogram_ragged``,
``ops.segment_tail_scores_ragged``, ``MatrixReporter.tail_scores_records``), and
``segment_tail_attribution`` of their attribution (``ops.segment_tail_attribution_ragged``,
``MatrixReporter.tail_scores_records(attribute=)``).
``compact_to_dense`` / ``compact_from_dense`` / ``compact_is_canonical`` /
``compact_history_scores`` / ``segment_compact_history_scores`` are the host side of the compact
history (64 bytes per rank and kernel: at most 12 used buckets, further ones folded downwards;
``ops.segment_history_scores_compact_ragged``,
``MatrixReporter.individual_tail_scores_records(history="compact")``), and
``compact_history_attribution`` / ``segment_compact_history_attribution`` of the attribution
against it (``ops.segment_history_attribution_compact_ragged``,
``MatrixReporter.compact_tail_attribution``).
``history_age`` / ``compact_age`` are the host twins of the aging of the two histories (every count
shifted right, the compact entries that reach zero evicted; ``ops.histogram_history_age``,
``ops.compact_history_age``, ``MatrixReporter.age_tail_history``, ``half_life=``).
``rank_attribution`` is the host twin of the converse of the attributions (``ops.rank_attribution``,
``MatrixReporter.kernel_ranks``): per kernel the ranks with the largest loss in a ``loss_all``.
``score_losses`` / ``score_rank_attribution`` are the host twins of the same question about the
median scores (``ops.score_rank_attribution``, ``MatrixReporter.score_kernel_ranks``): the loss
``NUM*AVG * (1 - base/MED)`` of every element a score takes, and per kernel the ranks with the
largest.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

BINS = 240
KEY_WIDE = 0xE0000000
_KEY_WIDE_F32BITS = 0x4F600000


def bucket_of(keys) -> np.ndarray:
    """Bucket (int64, 0..239) of every u32 duration key."""
    x = np.asarray(keys).astype(np.uint64)
    if x.size and int(x.max()) >= 1 << 32:
        raise ValueError("keys must be u32 duration keys")
    # e - 3 for x >= 8 (0 below): the exponent of x | 8, exact in f64 for a 32-bit integer
    sh = np.frexp((x | np.uint64(8)).astype(np.float64))[1].astype(np.int64) - 4
    return 8 * sh + (x >> sh.astype(np.uint64)).astype(np.int64)


def edges_keys() -> np.ndarray:
    """The 241 bucket edges as duration keys (u64): bucket b is [edges[b], edges[b + 1])."""
    b = np.arange(BINS + 1, dtype=np.uint64)
    hi = (np.uint64(8) + b % np.uint64(8)) << np.maximum(b // np.uint64(8), np.uint64(1)) - np.uint64(1)
    return np.where(b < 8, b, hi)


def _keys_to_us(keys: np.ndarray) -> np.ndarray:
    # key_to_f32(key) / 1000.0f, as every sample is converted (include/nvrx_straggler.h)
    k = keys.astype(np.uint32)
    wide = (k.astype(np.int64) - KEY_WIDE + _KEY_WIDE_F32BITS).astype(np.uint32).view(np.float32)
    return np.where(k < KEY_WIDE, k.astype(np.float32), wide) / np.float32(1000.0)


def edges_us() -> np.ndarray:
    """The 241 bucket edges in microseconds (f32), converted like every sample; the last is +inf."""
    e = edges_keys()
    us = np.empty(BINS + 1, np.float32)
    us[:BINS] = _keys_to_us(e[:BINS])
    us[BINS] = np.inf
    return us


def merge(*counts) -> np.ndarray:
    """Sum of histograms (arrays of equal shape [..., 240]; torch tensors on the host are taken
    too) as int64: counts of the same buckets add, over ranks and over reports."""
    if not counts:
        raise ValueError("merge needs at least one histogram")
    total = None
    for c in counts:
        a = np.asarray(c)
        if a.dtype == np.int32:  # device counts are u32 in an int32 tensor
            a = a.view(np.uint32)
        a = a.astype(np.int64)
        if a.shape[-1:] != (BINS,):
            raise ValueError(f"a histogram has {BINS} bins in its last dimension, got shape {a.shape}")
        total = a if total is None else total + a
    return total


def _check_permille(permille) -> int:
    if isinstance(permille, bool) or int(permille) != permille or not 0 <= permille <= 1000:
        raise ValueError(f"permille must be an int in [0, 1000], got {permille!r}")
    return int(permille)


def weights() -> list:
    """w(b) of the tail scores as Python ints: the lower edge of bucket min(b, 238) in ns (the
    two wide buckets both weigh ``KEY_WIDE``, a true lower bound of their durations)."""
    e = edges_keys().tolist()
    return [e[min(b, BINS - 2)] for b in range(BINS)]


def tail_threshold(fleet, permille: int) -> np.ndarray:
    """Threshold bucket per kernel of a fleet histogram ``fleet`` ([K, 240] counts, e.g.
    ``merge`` over the ranks): int64 [K], the bucket that holds the fleet's sample of 0-based rank
    ``(permille * (N - 1)) // 1000`` (the rank rule of the quantile calls, the bucket
    ``quantile_bounds`` brackets); -1 for a kernel without samples.  Python-integer sums: the
    host twin of ``ops.histogram_tail_threshold``."""
    pm = _check_permille(permille)
    f = merge(fleet) if np.asarray(fleet).dtype != np.uint64 else np.asarray(fleet)
    if f.ndim != 2 or f.shape[1] != BINS:
        raise ValueError(f"fleet must have shape [K, {BINS}]")
    out = np.full(f.shape[0], -1, np.int64)
    for k, row in enumerate(f.tolist()):
        n = sum(row)
        if n == 0:
            continue
        rank, c = (pm * (n - 1)) // 1000, 0
        for b, v in enumerate(row):
            c += v
            if c > rank:
                out[k] = b
                break
    return out


@dataclass
class TailScores:
    """``tail_scores``: per row the tail score and what it was made from."""
    score: np.ndarray             # [R] f64, NaN without weighted samples
    tail_ns: np.ndarray           # [R] u64, time above the fleet's threshold buckets (lower bound)
    total_ns: np.ndarray          # [R] u64
    fleet_share: float            # fleet_tail / fleet_total (NaN for an empty fleet)
    threshold_bucket: np.ndarray  # [K] i64, -1: kernel skipped
    tail_calls: np.ndarray        # [R, K] i64 calls above the threshold bucket
    fleet_tail: int = 0
    fleet_total: int = 0


def tail_scores(counts, permille: int, col_valid=None) -> TailScores:
    """Tail score per row of ``counts`` ([R, K, 240]; device counts as int32 are read as u32),
    the host twin of ``ops.histogram_sum`` -> ``histogram_tail_threshold`` ->
    ``histogram_tail_scores`` with the same definition (include/nvrx_straggler.h): the fleet is
    the sum over rows, T_k its threshold bucket at ``permille`` (kernels with ``col_valid[k] ==
    0`` or no sample are skipped), ``w(b)`` the bucket's lower edge in ns,

        score[r] = (1 - tail_ns[r] / total_ns[r]) / (1 - fleet_tail / fleet_total)

    with ``tail_ns`` the weighted counts above T_k.  About 1 for a healthy row, lower for one whose
    time sits in the fleet's tail; exact integer sums (Python ints, wrapped to 64 bits like the
    device's), three f64 operations.  A slowdown below one bucket (12.5 %) may not cross T_k, and
    ``permille`` must leave more room than the slow row's own share of the fleet's samples."""
    pm = _check_permille(permille)
    c = merge(counts)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    T = tail_threshold(c.sum(0), pm) if R else np.full(K, -1, np.int64)
    if col_valid is not None:
        T = np.where(np.asarray(col_valid).astype(bool), T, -1)
    w, M = weights(), (1 << 64) - 1
    rows = c.tolist()
    tail, total = [0] * R, [0] * R
    calls = np.zeros((R, K), np.int64)
    for k in range(K):
        t = int(T[k])
        if t < 0:
            continue
        for r in range(R):
            h = rows[r][k]
            total[r] += sum(v * w[b] for b, v in enumerate(h) if v)
            tail[r] += sum(h[b] * w[b] for b in range(t + 1, BINS) if h[b])
            calls[r, k] = sum(h[t + 1:]) & 0xFFFFFFFF
    ftail, ftotal = sum(tail) & M, sum(total) & M
    tail, total = [v & M for v in tail], [v & M for v in total]
    nan = float("nan")
    fs = float(ftail) / float(ftotal) if ftotal else nan
    den = 1.0 - fs
    score = [(1.0 - float(tl) / float(tt)) / den if tt and ftotal and den != 0.0 else nan
             for tl, tt in zip(tail, total)]
    return TailScores(np.asarray(score, np.float64).reshape(R), np.asarray(tail, np.uint64).reshape(R),
                      np.asarray(total, np.uint64).reshape(R), fs, T.astype(np.int64), calls,
                      ftail, ftotal)


def segment_counts(keys, seg_off, seg_len, K: int, cap: int = 0) -> np.ndarray:
    """Histograms of ragged segments of duration keys as int64 [R, K, 240]: segment ``r * K + k``
    is ``keys[seg_off[g] : seg_off[g] + seg_len[g]]`` (``seg_len`` None: ``seg_off`` holds one more
    offset), of which the last ``cap`` samples are retained (0: all); a length <= 0 counts
    nothing.  What ``ops.segment_histogram_ragged`` writes into zeroed counts."""
    keys, off = np.asarray(keys), np.asarray(seg_off, np.int64)
    if isinstance(K, bool) or int(K) != K or K < 0:
        raise ValueError(f"K must be a non-negative int, got {K!r}")
    lens = np.diff(off) if seg_len is None else np.asarray(seg_len, np.int64)
    nseg = lens.size
    if (K == 0 and nseg) or (K and nseg % K) or off.size < nseg:
        raise ValueError("the segments must be R * K, with an offset each")
    c = np.zeros((nseg, BINS), np.int64)
    for g in range(nseg):
        n = int(lens[g])
        if n <= 0:
            continue
        e = int(off[g]) + n
        keep = cap if 0 < cap < n else n
        c[g] = np.bincount(bucket_of(keys[e - keep:e]), minlength=BINS)
    return c.reshape(nseg // K if K else 0, K, BINS)


def segment_tail_scores(keys, seg_off, seg_len, K: int, permille: int, cap: int = 0,
                        col_valid=None) -> TailScores:
    """Tail score per row straight from ragged segments of duration keys (``segment_counts``'s
    addressing), the host twin of ``ops.segment_fleet_histogram_ragged`` ->
    ``histogram_tail_threshold`` -> ``segment_tail_scores_ragged`` and of
    ``MatrixReporter.tail_scores_records``: ``tail_scores`` (Python-integer sums, three f64
    operations) over the retained windows' counts."""
    return tail_scores(segment_counts(keys, seg_off, seg_len, K, cap), permille, col_valid)


@dataclass
class HistoryScores:
    """``history_scores``: per row the individual tail score, what it was made from, and the
    history after the call.  With ``score=False`` only ``hist`` is set."""
    hist: np.ndarray                      # [R, S, 240] u32, the history after the call
    score: np.ndarray = None              # [R] f64, NaN without eligible weighted samples
    tail_ns: np.ndarray = None            # [R] u64, current time above the history's thresholds
    total_ns: np.ndarray = None           # [R] u64
    base_tail_ns: np.ndarray = None       # [R] u64, the history's time above its thresholds
    base_total_ns: np.ndarray = None      # [R] u64
    history_share: np.ndarray = None      # [R] f64 base_tail_ns / base_total_ns (NaN: no history)
    stragglers: np.ndarray = None         # [R] bool, score < score_thr (NaN never)
    threshold_bucket: np.ndarray = None   # [R, K] i64, -1: (row, kernel) not eligible
    tail_calls: np.ndarray = None         # [R, K] i64 calls above the threshold bucket


def history_scores(counts, hist, permille: int, *, score: bool = True, update: bool = True,
                   hist_index=None, col_valid=None, skip_rows=None,
                   score_thr: float = 0.75) -> HistoryScores:
    """Individual tail score per row of ``counts`` ([R, K, 240]) against the row's own history
    ``hist`` ([R, S, 240], left unchanged; int32 arrays are read as u32), the host twin of
    ``ops.histogram_history_scores`` with the same definition (include/nvrx_straggler.h).  Column
    k uses slot ``hist_index[k]`` (identity without; negative: none).  A (row, kernel) is scored
    when it has a slot, ``col_valid``, history (N > 0) and current samples; T is the bucket of the
    history's sample of rank ``(permille * (N - 1)) // 1000``, and

        score[r] = (1 - tail_ns[r] / total_ns[r]) / (1 - base_tail_ns[r] / base_total_ns[r])

    in Python integers (wrapped to 64 bits like the device's) and three f64 operations.
    ``update`` returns ``min(H + C, 2**32 - 1)`` as the new history for every column with a slot
    and ``col_valid`` in the rows ``skip_rows`` does not mark; the score always uses the history
    as given.  Emulate ``absorb="healthy"`` with a ``score`` call followed by an ``update`` call
    with ``skip_rows=stragglers``."""
    pm = _check_permille(permille)
    if not (score or update):
        raise ValueError("history_scores: at least one of score and update")
    c, H = merge(counts), merge(hist)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    if H.ndim != 3 or H.shape[0] != R or H.shape[2] != BINS:
        raise ValueError(f"hist must have shape [R, S, {BINS}]")
    S = H.shape[1]
    index = list(range(K)) if hist_index is None else [int(s) for s in np.asarray(hist_index)]
    if len(index) != K or any(s >= S for s in index):
        raise ValueError("hist_index must hold K slots below hist.shape[1]")
    valid = [True] * K if col_valid is None else [bool(v) for v in np.asarray(col_valid)]
    skip = [False] * R if skip_rows is None else [bool(v) for v in np.asarray(skip_rows)]
    cols = [(k, s) for k, s in enumerate(index) if s >= 0 and valid[k]]
    res = HistoryScores(H.astype(np.uint32))
    if score:
        w, M, nan = weights(), (1 << 64) - 1, float("nan")
        sums = np.zeros((4, R), np.uint64)
        T = np.full((R, K), -1, np.int64)
        calls = np.zeros((R, K), np.int64)
        sc, share = [nan] * R, [nan] * R
        for r in range(R):
            tl = tt = bl = bt = 0
            for k, s in cols:
                h, cur = H[r, s].tolist(), c[r, k].tolist()
                n = sum(h)
                if n == 0 or not any(cur):
                    continue
                rank, acc = (pm * (n - 1)) // 1000, 0
                for t, v in enumerate(h):
                    acc += v
                    if acc > rank:
                        break
                T[r, k] = t
                tt += sum(v * w[b] for b, v in enumerate(cur) if v)
                bt += sum(v * w[b] for b, v in enumerate(h) if v)
                tl += sum(cur[b] * w[b] for b in range(t + 1, BINS) if cur[b])
                bl += sum(h[b] * w[b] for b in range(t + 1, BINS) if h[b])
                calls[r, k] = sum(cur[t + 1:]) & 0xFFFFFFFF
            tl, tt, bl, bt = tl & M, tt & M, bl & M, bt & M
            sums[:, r] = (tl, tt, bl, bt)
            if bt:
                share[r] = float(bl) / float(bt)
                den = 1.0 - share[r]
                if tt and den != 0.0:
                    sc[r] = (1.0 - float(tl) / float(tt)) / den
        res.score = np.asarray(sc, np.float64).reshape(R)
        res.tail_ns, res.total_ns, res.base_tail_ns, res.base_total_ns = sums
        res.history_share = np.asarray(share, np.float64).reshape(R)
        res.stragglers = res.score < score_thr
        res.threshold_bucket, res.tail_calls = T, calls
    if update:
        new = H.copy()
        for k, s in cols:
            new[:, s] = np.minimum(H[:, s] + c[:, k], 0xFFFFFFFF)
        new[np.asarray(skip, bool)] = H[np.asarray(skip, bool)]
        res.hist = new.astype(np.uint32)
    return res


def segment_history_scores(keys, seg_off, seg_len, K: int, hist, permille: int, cap: int = 0,
                           **kwargs) -> HistoryScores:
    """Individual tail score per row straight from ragged segments of duration keys
    (``segment_counts``'s addressing) against the rows' own history, the host twin of
    ``ops.segment_history_scores_ragged`` and of ``MatrixReporter.individual_tail_scores_records``:
    ``history_scores`` (its keywords pass through) over the retained windows' counts."""
    return history_scores(segment_counts(keys, seg_off, seg_len, K, cap), hist, permille, **kwargs)


CHIST_ENTRIES = 12  # NVRX_CHIST_ENTRIES
CHIST_BYTES = 64    # NVRX_CHIST_BYTES: u32 count[12], u8 bucket[12], u32 n


def _chist_array(chist) -> np.ndarray:
    c = np.asarray(chist)
    if c.dtype != np.uint8 or c.ndim != 3 or c.shape[2] != CHIST_BYTES:
        raise ValueError(f"chist must be a uint8 array of shape [R, S, {CHIST_BYTES}]")
    return np.ascontiguousarray(c)


def _chist_fields(c: np.ndarray):
    """(count [.., 12] int64, bucket [.., 12] int64, n [..] int64) of compact elements."""
    count = c[..., :4 * CHIST_ENTRIES].view("<u4").astype(np.int64)
    bucket = c[..., 4 * CHIST_ENTRIES:5 * CHIST_ENTRIES].astype(np.int64)
    n = c[..., 5 * CHIST_ENTRIES:].view("<u4")[..., 0].astype(np.int64)
    return count, bucket, n


def compact_is_canonical(chist) -> np.ndarray:
    """Per element of a compact history (uint8 [R, S, 64]) whether it is canonical: n <= 12,
    entries 0..n-1 with strictly ascending bucket < 240 and count >= 1, entries n..11 all zero
    (bool [R, S]; the all-zero element is the empty history)."""
    count, bucket, n = _chist_fields(_chist_array(chist))
    i = np.arange(CHIST_ENTRIES)
    used = i < n[..., None]
    ok = n <= CHIST_ENTRIES
    ok &= np.where(used, (count >= 1) & (bucket < BINS), (count == 0) & (bucket == 0)).all(-1)
    ok &= (~used[..., 1:] | (bucket[..., 1:] > bucket[..., :-1])).all(-1)
    return ok


def _chist_entries(elem: np.ndarray) -> dict:
    """{bucket: count} of one canonical element (uint8 [64])."""
    count, bucket, n = _chist_fields(elem)
    n = int(n)
    return dict(zip(bucket[:n].tolist(), count[:n].tolist()))


def _chist_pack(entries: dict) -> np.ndarray:
    e = np.zeros(CHIST_BYTES, np.uint8)
    b = sorted(entries)
    e[:4 * len(b)] = np.asarray([entries[x] for x in b], "<u4").view(np.uint8)
    e[4 * CHIST_ENTRIES:4 * CHIST_ENTRIES + len(b)] = b
    e[5 * CHIST_ENTRIES:] = np.asarray([len(b)], "<u4").view(np.uint8)
    return e


def _chist_update(entries: dict, c) -> tuple:
    """UPDATE of one element ({bucket: count}) with the interval's counts ``c`` (240 ints): the
    new entries and the number of folded samples (include/nvrx_straggler.h)."""
    seen = [b for b, v in enumerate(c) if v > 0]
    if not seen:
        return dict(entries), 0
    fresh = [b for b in seen if b not in entries]
    kept = sorted(list(entries) + fresh[:CHIST_ENTRIES - len(entries)])
    add = dict.fromkeys(kept, 0)
    folded = 0
    for b in seen:
        below = [s for s in kept if s <= b]
        add[below[-1] if below else kept[0]] += c[b]
        if b not in add:
            folded += c[b]
    return {s: min(entries.get(s, 0) + add[s], 0xFFFFFFFF) for s in kept}, folded


def compact_to_dense(chist) -> np.ndarray:
    """The dense expansion (u32 [R, S, 240]) of a canonical compact history (uint8 [R, S, 64]):
    ``H[bucket[i]] = count[i]`` for the used entries, zero elsewhere."""
    c = _chist_array(chist)
    if not compact_is_canonical(c).all():
        raise ValueError("compact_to_dense: an element is not canonical")
    count, bucket, n = _chist_fields(c)
    H = np.zeros(c.shape[:2] + (BINS,), np.uint32)
    for r, s, i in zip(*np.nonzero(np.arange(CHIST_ENTRIES) < n[..., None])):
        H[r, s, bucket[r, s, i]] = count[r, s, i]
    return H


def compact_from_dense(hist) -> tuple:
    """``(chist uint8 [R, S, 64], folded u64 [R])`` of a dense history ([R, S, 240]; int32 is read
    as u32): by definition the UPDATE of an empty element with those counts -- the 12 lowest used
    buckets are kept, the others folded into the highest kept one, ``folded`` their samples per
    row."""
    H = merge(hist)
    if H.ndim != 3 or H.shape[2] != BINS:
        raise ValueError(f"hist must have shape [R, S, {BINS}]")
    out = np.zeros(H.shape[:2] + (CHIST_BYTES,), np.uint8)
    folded = np.zeros(H.shape[0], np.uint64)
    for r, s in zip(*np.nonzero(H.any(-1))):
        entries, f = _chist_update({}, H[r, s].tolist())
        out[r, s] = _chist_pack(entries)
        folded[r] += np.uint64(f)
    return out, folded


@dataclass
class CompactHistoryScores(HistoryScores):
    """``compact_history_scores``: the fields of ``HistoryScores`` with ``hist`` the compact
    history after the call (uint8 [R, S, 64]), and the samples UPDATE folded."""
    folded: np.ndarray = None             # [R] u64 (None without update)


def compact_history_scores(counts, chist, permille: int, *, score: bool = True, update: bool = True,
                           hist_index=None, col_valid=None, skip_rows=None,
                           score_thr: float = 0.75) -> CompactHistoryScores:
    """``history_scores`` against a compact history ``chist`` (uint8 [R, S, 64], left unchanged;
    the elements of the slots in use must be canonical): the score is ``history_scores``'s against
    the dense expansion of every element; ``update`` admits an interval's new buckets in ascending
    order while an element has free entries and folds every other sample into the nearest kept
    bucket at or below it (the lowest kept one without any), ``folded`` counting them per row.
    Only elements with samples in a row ``skip_rows`` does not mark change.  Python integers: the
    host twin of ``ops.segment_history_scores_compact_ragged``."""
    pm = _check_permille(permille)
    if not (score or update):
        raise ValueError("compact_history_scores: at least one of score and update")
    c, ch = merge(counts), _chist_array(chist)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    if ch.shape[0] != R:
        raise ValueError(f"chist must have shape [R, S, {CHIST_BYTES}]")
    S = ch.shape[1]
    index = list(range(K)) if hist_index is None else [int(s) for s in np.asarray(hist_index)]
    if len(index) != K or any(s >= S for s in index):
        raise ValueError("hist_index must hold K slots below chist.shape[1]")
    valid = [True] * K if col_valid is None else [bool(v) for v in np.asarray(col_valid)]
    skip = [False] * R if skip_rows is None else [bool(v) for v in np.asarray(skip_rows)]
    cols = [(k, s) for k, s in enumerate(index) if s >= 0 and valid[k]]
    slots = sorted({s for _, s in cols})
    if not compact_is_canonical(ch[:, slots]).all():
        raise ValueError("compact_history_scores: an element of a slot in use is not canonical")
    res = CompactHistoryScores(ch.copy())
    if score:
        H = np.zeros((R, S, BINS), np.uint32)
        H[:, slots] = compact_to_dense(ch[:, slots])
        d = history_scores(c, H, pm, update=False, hist_index=hist_index, col_valid=col_valid,
                           score_thr=score_thr)
        for f in ("score", "tail_ns", "total_ns", "base_tail_ns", "base_total_ns", "history_share",
                  "stragglers", "threshold_bucket", "tail_calls"):
            setattr(res, f, getattr(d, f))
    if update:
        folded = [0] * R
        for r in range(R):
            if skip[r]:
                continue
            for k, s in cols:
                if c[r, k].any():
                    entries, f = _chist_update(_chist_entries(ch[r, s]), c[r, k].tolist())
                    res.hist[r, s] = _chist_pack(entries)
                    folded[r] += f
        res.folded = np.asarray([f & _M64 for f in folded], np.uint64).reshape(R)
    return res


def segment_compact_history_scores(keys, seg_off, seg_len, K: int, chist, permille: int,
                                   cap: int = 0, **kwargs) -> CompactHistoryScores:
    """Individual tail score per row straight from ragged segments of duration keys
    (``segment_counts``'s addressing) against the rows' own compact history, the host twin of
    ``ops.segment_history_scores_compact_ragged`` and of
    ``MatrixReporter.individual_tail_scores_records(history="compact")``:
    ``compact_history_scores`` (its keywords pass through) over the retained windows' counts."""
    return compact_history_scores(segment_counts(keys, seg_off, seg_len, K, cap), chist, permille,
                                  **kwargs)


def _age_shift(shift) -> int:
    if isinstance(shift, bool) or int(shift) != shift or not 1 <= shift <= 31:
        raise ValueError(f"shift must be an int in [1, 31], got {shift!r}")
    return int(shift)


def history_age(hist, shift: int) -> np.ndarray:
    """A dense history ([R, S, 240]; int32 is read as u32) aged by ``shift`` (1..31): every count
    becomes ``count >> shift`` (u32, a new array).  The host twin of
    ``ops.histogram_history_age``."""
    s = _age_shift(shift)
    H = merge(hist)
    if H.ndim != 3 or H.shape[2] != BINS:
        raise ValueError(f"hist must have shape [R, S, {BINS}]")
    return (H >> s).astype(np.uint32)  # int64 holding u32 values: exact


def compact_age(chist, shift: int) -> tuple:
    """A canonical compact history (uint8 [R, S, 64], left unchanged) aged by ``shift`` (1..31):
    ``(chist', evicted u64 [R], full u64 [R])``.  Every count of every element becomes ``count >>
    shift``; the entries that reach zero are evicted and the others keep their order at the front
    of the element, everything behind them zero, so the result is canonical and an element that
    loses every entry is the empty history.  ``evicted`` counts the entries freed per row,
    ``full`` the elements per row that still hold 12 entries.  Python integers: the host twin of
    ``ops.compact_history_age``."""
    s = _age_shift(shift)
    c = _chist_array(chist)
    if not compact_is_canonical(c).all():
        raise ValueError("compact_age: an element is not canonical")
    out = c.copy()
    R, S, _ = c.shape
    evicted, full = [0] * R, [0] * R
    for r in range(R):
        for k in range(S):
            old = _chist_entries(c[r, k])
            new = {b: v >> s for b, v in old.items() if v >> s}
            out[r, k] = _chist_pack(new)
            evicted[r] += len(old) - len(new)
            full[r] += len(new) == CHIST_ENTRIES
    return out, np.asarray(evicted, np.uint64).reshape(R), np.asarray(full, np.uint64).reshape(R)


@dataclass
class TailAttribution:
    """``tail_attribution`` / ``history_attribution``: per row the ``top`` kernels with the largest
    excess tail time, largest first (ties: the lower column)."""
    idx: np.ndarray         # [R, top] i32 kernel column, -1 beyond the elements taken
    loss: np.ndarray        # [R, top] f64 ns, tail - total * base_share; NaN where idx is -1
    tail_ns: np.ndarray     # [R, top] u64 the kernel's weighted counts above T
    total_ns: np.ndarray    # [R, top] u64 all its weighted counts
    tail_calls: np.ndarray  # [R, top] u32 its calls above T
    thr_bucket: np.ndarray  # [R, top] i32 T, -1 where idx is -1
    base_share: np.ndarray  # [R, top] f64 btail / btotal of the base; NaN where idx is -1
    loss_all: np.ndarray    # [R, K] f64 every kernel's loss, NaN where not taken


_M64 = (1 << 64) - 1


def _wsums(h, t, w):
    """(weighted sum above bucket t, weighted sum, count above t) of one histogram (a list), as
    the device's wrapped u64 / u32."""
    total = sum(v * w[b] for b, v in enumerate(h) if v)
    tail = sum(h[b] * w[b] for b in range(t + 1, BINS) if h[b])
    return tail & _M64, total & _M64, sum(h[t + 1:]) & 0xFFFFFFFF


def _excess(tail, total, btail, btotal):
    """(share, loss) in f64, every operation rounded separately, the u64 converted first."""
    nan = float("nan")
    if btotal:
        share = float(btail) / float(btotal)
    else:
        share = nan if btail == 0 else float("inf")  # IEEE x / 0
    return share, float(tail) - float(total) * share


def _attribution(R, K, top, element) -> TailAttribution:
    """Rank what ``element(r, k)`` returns -- None, or (loss, tail, total, calls, T, share) -- per
    row: a stable sort by descending loss over the columns in order, NaN losses left out."""
    if isinstance(top, bool) or int(top) != top or not 1 <= top <= 16:
        raise ValueError(f"top must be an int in [1, 16], got {top!r}")
    top = int(top)
    res = TailAttribution(np.full((R, top), -1, np.int32), np.full((R, top), np.nan),
                          np.zeros((R, top), np.uint64), np.zeros((R, top), np.uint64),
                          np.zeros((R, top), np.uint32), np.full((R, top), -1, np.int32),
                          np.full((R, top), np.nan), np.full((R, K), np.nan))
    for r in range(R):
        terms = {}
        for k in range(K):
            e = element(r, k)
            if e is not None and e[0] == e[0]:
                terms[k] = e
                res.loss_all[r, k] = e[0]
        ks = np.fromiter(terms, dtype=np.int64, count=len(terms))
        order = ks[np.argsort(-res.loss_all[r, ks], kind="stable")][:top]
        for j, k in enumerate(order.tolist()):
            loss, tail, total, calls, t, share = terms[k]
            res.idx[r, j], res.loss[r, j], res.thr_bucket[r, j] = k, loss, t
            res.tail_ns[r, j], res.total_ns[r, j] = tail, total
            res.tail_calls[r, j], res.base_share[r, j] = calls, share
    return res


def tail_attribution(counts, permille: int, top: int, col_valid=None, *, fleet=None,
                     thr_index=None) -> TailAttribution:
    """The kernels behind the tail score of each row of ``counts`` ([R, K, 240]): per row the
    ``top`` (1..16) kernels with the largest excess tail time

        loss = tail - total * (fleet_tail_k / fleet_total_k)          (ns, f64)

    where ``tail`` / ``total`` are the row's weighted counts of kernel k above its threshold bucket
    T_k / in all buckets and the fleet's the same sums of the fleet's histogram: the part of the
    row's tail beyond what the fleet's tail share predicts.  A count of tail calls is not a cost;
    this is.  The host twin of ``ops.histogram_tail_base`` -> ``histogram_tail_attribution(kind=
    "relative")`` with the same definition (include/nvrx_straggler.h): Python integers (wrapped to
    64 bits like the device's), three f64 operations, a stable sort.  The fleet is the sum over
    rows, or ``fleet`` ([Kf, 240]) with column k using fleet kernel ``thr_index[k]`` (negative:
    none); ``col_valid`` is over the fleet's kernels.  A kernel without a threshold bucket, without
    samples in the row, or with a NaN loss (a fleet wholly in bucket 0) is left out."""
    pm = _check_permille(permille)
    c = merge(counts)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    if fleet is None:
        F = c.sum(0)
    else:
        F = merge(fleet) if np.asarray(fleet).dtype != np.uint64 else np.asarray(fleet)
    T = tail_threshold(F, pm) if F.shape[0] else np.zeros(0, np.int64)
    if col_valid is not None:
        T = np.where(np.asarray(col_valid).astype(bool), T, -1)
    index = list(range(K)) if thr_index is None else [int(u) for u in np.asarray(thr_index)]
    if len(index) != K or any(u >= F.shape[0] for u in index):
        raise ValueError("thr_index must hold K fleet kernels below fleet.shape[0]")
    w = weights()
    base = {u: _wsums(F[u].tolist(), int(T[u]), w)[:2] for u in set(index) if u >= 0 and T[u] >= 0}
    rows = c.tolist()

    def element(r, k):
        u = index[k]
        if u not in base or not any(rows[r][k]):
            return None
        t = int(T[u])
        tail, total, calls = _wsums(rows[r][k], t, w)
        share, loss = _excess(tail, total, *base[u])
        return loss, tail, total, calls, t, share

    return _attribution(R, K, top, element)


def history_attribution(counts, hist, permille: int, top: int, hist_index=None,
                        col_valid=None) -> TailAttribution:
    """The kernels behind the individual tail score of each row: as ``tail_attribution`` with the
    row's own history ``hist`` ([R, S, 240], read only) as the base, T from the history by the rank
    rule of ``history_scores``, over the (row, kernel) elements eligible there (a slot,
    ``col_valid``, history and current samples).  The host twin of
    ``ops.histogram_tail_attribution(kind="individual")``."""
    pm = _check_permille(permille)
    c, H = merge(counts), merge(hist)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    if H.ndim != 3 or H.shape[0] != R or H.shape[2] != BINS:
        raise ValueError(f"hist must have shape [R, S, {BINS}]")
    index = list(range(K)) if hist_index is None else [int(s) for s in np.asarray(hist_index)]
    if len(index) != K or any(s >= H.shape[1] for s in index):
        raise ValueError("hist_index must hold K slots below hist.shape[1]")
    valid = [True] * K if col_valid is None else [bool(v) for v in np.asarray(col_valid)]
    w = weights()

    def element(r, k):
        s = index[k]
        if s < 0 or not valid[k]:
            return None
        h, cur = H[r, s].tolist(), c[r, k].tolist()
        n = sum(h)
        if n == 0 or not any(cur):
            return None
        rank, acc = (pm * (n - 1)) // 1000, 0
        for t, v in enumerate(h):
            acc += v
            if acc > rank:
                break
        tail, total, calls = _wsums(cur, t, w)
        share, loss = _excess(tail, total, *_wsums(h, t, w)[:2])
        return loss, tail, total, calls, t, share

    return _attribution(R, K, top, element)


def segment_tail_attribution(keys, seg_off, seg_len, K: int, permille: int, top: int, cap: int = 0,
                             col_valid=None, thr_index=None) -> TailAttribution:
    """The kernels behind the tail score of each row straight from ragged segments of duration
    keys (``segment_counts``'s addressing), the host twin of ``ops.segment_fleet_histogram_ragged``
    -> ``histogram_tail_threshold`` -> ``histogram_tail_base`` ->
    ``segment_tail_attribution_ragged`` and of ``MatrixReporter.tail_scores_records(attribute=)``:
    ``tail_attribution`` over the retained windows' counts, the fleet being their sum over rows."""
    return tail_attribution(segment_counts(keys, seg_off, seg_len, K, cap), permille, top, col_valid,
                            thr_index=thr_index)


def segment_history_attribution(keys, seg_off, seg_len, K: int, hist, permille: int, top: int,
                                cap: int = 0, hist_index=None, col_valid=None) -> TailAttribution:
    """The kernels behind the individual tail score of each row straight from ragged segments of
    duration keys (``segment_counts``'s addressing) against the rows' own history ``hist`` (read
    only), the host twin of ``ops.segment_history_attribution_ragged`` and of
    ``MatrixReporter.individual_tail_scores_records(attribute=)``: ``history_attribution`` over
    the retained windows' counts."""
    return history_attribution(segment_counts(keys, seg_off, seg_len, K, cap), hist, permille, top,
                               hist_index, col_valid)


def compact_history_attribution(counts, chist, permille: int, top: int, hist_index=None,
                                col_valid=None) -> TailAttribution:
    """``history_attribution`` against a compact history ``chist`` (uint8 [R, S, 64], read only;
    the elements of the slots in use must be canonical): by definition its result on the dense
    expansion of every element, worked out here from the element's at most 12 entries directly --
    N their counts' sum, T the bucket of the first entry whose running count passes the rank
    ``(permille * (N - 1)) // 1000``, the base sums ``count * weight`` over the entries / those
    above T.  The content of slots no column uses is not looked at.  Python integers: the host
    twin of ``ops.histogram_history_attribution_compact`` (and of
    ``MatrixReporter.compact_tail_attribution(counts=)``) on the counts themselves, and through
    ``segment_compact_history_attribution`` of ``ops.segment_history_attribution_compact_ragged``."""
    pm = _check_permille(permille)
    c, ch = merge(counts), _chist_array(chist)
    if c.ndim != 3 or c.shape[2] != BINS:
        raise ValueError(f"counts must have shape [R, K, {BINS}]")
    R, K, _ = c.shape
    if ch.shape[0] != R:
        raise ValueError(f"chist must have shape [R, S, {CHIST_BYTES}]")
    S = ch.shape[1]
    index = list(range(K)) if hist_index is None else [int(s) for s in np.asarray(hist_index)]
    if len(index) != K or any(s >= S for s in index):
        raise ValueError("hist_index must hold K slots below chist.shape[1]")
    valid = [True] * K if col_valid is None else [bool(v) for v in np.asarray(col_valid)]
    slots = sorted({s for k, s in enumerate(index) if s >= 0 and valid[k]})
    if not compact_is_canonical(ch[:, slots]).all():
        raise ValueError("compact_history_attribution: an element of a slot in use is not canonical")
    count, bucket, used = (x.tolist() for x in _chist_fields(ch))
    w = weights()

    def element(r, k):
        s = index[k]
        if s < 0 or not valid[k]:
            return None
        n = used[r][s]
        cnt, bkt = count[r][s][:n], bucket[r][s][:n]
        N = sum(cnt)
        cur = c[r, k].tolist()
        if N == 0 or not any(cur):
            return None
        rank, acc = (pm * (N - 1)) // 1000, 0
        for v, t in zip(cnt, bkt):
            acc += v
            if acc > rank:
                break
        btotal = sum(v * w[b] for v, b in zip(cnt, bkt)) & _M64
        btail = sum(v * w[b] for v, b in zip(cnt, bkt) if b > t) & _M64
        tail, total, calls = _wsums(cur, t, w)
        share, loss = _excess(tail, total, btail, btotal)
        return loss, tail, total, calls, t, share

    return _attribution(R, K, top, element)


def segment_compact_history_attribution(keys, seg_off, seg_len, K: int, chist, permille: int,
                                        top: int, cap: int = 0, hist_index=None,
                                        col_valid=None) -> TailAttribution:
    """The kernels behind the individual tail score of each row straight from ragged segments of
    duration keys (``segment_counts``'s addressing) against the rows' own compact history ``chist``
    (read only), the host twin of ``ops.segment_history_attribution_compact_ragged`` and of
    ``MatrixReporter.compact_tail_attribution``: ``compact_history_attribution`` over the retained
    windows' counts."""
    return compact_history_attribution(segment_counts(keys, seg_off, seg_len, K, cap), chist,
                                       permille, top, hist_index, col_valid)


@dataclass
class RankAttribution:
    """``rank_attribution``: per column (kernel) the ``top`` rows (ranks) with the largest loss,
    largest first (ties: the lower row)."""
    idx: np.ndarray       # [K, top] i32 row, -1 beyond the elements taken
    loss: np.ndarray      # [K, top] f64 the input's value, bit for bit; NaN where idx is -1
    taken: np.ndarray     # [K] i32 rows taken: valid and not NaN
    positive: np.ndarray  # [K] i32 taken rows with loss > 0


def rank_attribution(loss, top: int, rows=None) -> RankAttribution:
    """The ranks behind a kernel's tail loss: per column of ``loss`` ([R, K] f64, e.g. the
    ``loss_all`` of any attribution above) the ``top`` (1..16) rows with the largest loss.  An
    element is taken iff it is not NaN and its row is on (``rows``: [R], zero = off; None: all
    on).  Per column a stable sort of the rows by descending loss: the comparison is on values, so
    -0.0 and +0.0 tie and the lower row goes first, while the loss returned is the input's element
    (its sign kept).  The host twin of ``ops.rank_attribution`` / ``MatrixReporter.kernel_ranks``
    with the same definition (include/nvrx_straggler.h)."""
    if isinstance(top, bool) or int(top) != top or not 1 <= top <= 16:
        raise ValueError(f"top must be an int in [1, 16], got {top!r}")
    top = int(top)
    x = np.asarray(loss, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("loss must have shape [R, K]")
    R, K = x.shape
    taken = ~np.isnan(x)
    if rows is not None:
        on = np.asarray(rows).astype(bool)
        if on.shape != (R,):
            raise ValueError("rows must have shape [R]")
        taken &= on[:, None]
    res = RankAttribution(np.full((K, top), -1, np.int32), np.full((K, top), np.nan),
                          taken.sum(0).astype(np.int32), (taken & (x > 0.0)).sum(0).astype(np.int32))
    # NaN keys (not taken) sort behind every value, +inf (a loss of -inf) included
    order = np.argsort(np.where(taken, -x, np.nan), axis=0, kind="stable")[:top]
    for j in range(order.shape[0]):
        r, k = order[j], np.arange(K)
        have = j < res.taken
        res.idx[have, j] = r[have]
        res.loss[have, j] = x[r[have], k[have]]
    return res


def score_losses(num, med, avg, kind: str, col_valid=None, ref=None, ref_index=None,
                 ref_missing=None, hist=None, hist_index=None, hist_stride: int = 0, rows=None):
    """Every element's loss behind the median scores, as ``ops.score_attribution`` defines it:
    ``(loss_all, s_all, err)`` with ``loss_all`` [R, K] f64 the loss where the element is taken and
    NaN where it is not, ``s_all`` [R, K] f64 its ``s`` (whatever the arithmetic gives where not
    taken), ``err`` 1 when an eligible MED is 0 (in a row that is on, when ``rows`` is given).
    Per element in f64, one operation per statement: ``m = MED; w = NUM * AVG; s = base / m;
    loss = w * (1 - s)``.  Eligible: ``col_valid`` None or nonzero, ``num > 0``, and for
    ``kind="relative"`` a reference ``ref[ref_index[k]] >= 0`` (-1 and NaN: none) not flagged in
    ``ref_missing``; ``kind="individual"`` takes ``hist[r, hist_index[k]]`` (rows ``hist_stride``
    apart) as it stands.  Taken: eligible, MED != 0 and the loss not NaN."""
    if kind not in ("relative", "individual"):
        raise ValueError(f"kind must be 'relative' or 'individual', got {kind!r}")
    num, med, avg = np.asarray(num), np.asarray(med), np.asarray(avg)
    if med.ndim != 2 or num.shape != med.shape or avg.shape != med.shape:
        raise ValueError("num, med and avg must share one shape [R, K]")
    R, K = med.shape
    cols = np.arange(K)
    elig = num > 0
    if col_valid is not None:
        elig = elig & (np.asarray(col_valid) != 0)[None, :]
    if kind == "relative":
        if ref is None:
            raise ValueError("kind='relative' needs ref")
        ri = cols if ref_index is None else np.asarray(ref_index)
        b32 = np.asarray(ref, np.float32)[ri]
        with np.errstate(invalid="ignore"):
            usable = b32 >= 0  # -1 and NaN: no reference
        if ref_missing is not None:
            usable = usable & (np.asarray(ref_missing)[ri] == 0)
        elig = elig & usable[None, :]
        base = np.broadcast_to(b32.astype(np.float64)[None, :], (R, K))
    else:
        if hist is None:
            raise ValueError("kind='individual' needs hist")
        hi = cols if hist_index is None else np.asarray(hist_index)
        flat = np.asarray(hist).reshape(-1)
        base = flat[(np.arange(R) * (hist_stride or K))[:, None] + hi[None, :]].astype(np.float64)
    with np.errstate(all="ignore"):
        m = med.astype(np.float64)
        w = num.astype(np.float64) * avg.astype(np.float64)
        s = base / m
        d = 1.0 - s
        loss = w * d
    zero = elig & (m == 0.0)
    if rows is not None:
        zero = zero & np.asarray(rows).astype(bool)[:, None]
    take = elig & (m != 0.0) & ~np.isnan(loss)
    return np.where(take, loss, np.nan), s, int(zero.any())


@dataclass
class ScoreRankAttribution:
    """``score_rank_attribution``: ``RankAttribution`` of the score losses plus the winners' s."""
    idx: np.ndarray       # [K, top] i32 row, -1 beyond the elements taken
    loss: np.ndarray      # [K, top] f64 the element's loss; NaN where idx is -1
    score: np.ndarray     # [K, top] f64 the element's s = base / MED; NaN where idx is -1
    taken: np.ndarray     # [K] i32 rows taken
    positive: np.ndarray  # [K] i32 taken rows with loss > 0
    err: int = 0          # 1: an eligible MED of a row that is on was 0


def score_rank_attribution(num, med, avg, top: int, kind: str, rows=None,
                           **base) -> ScoreRankAttribution:
    """The ranks behind a kernel's score loss: ``rank_attribution(loss_all, top, rows)`` over the
    ``loss_all`` of ``score_losses(num, med, avg, kind, **base)``, plus the winners' ``s``.  The
    host twin of ``ops.score_rank_attribution`` / ``MatrixReporter.score_kernel_ranks``."""
    loss_all, s_all, err = score_losses(num, med, avg, kind, rows=rows, **base)
    r = rank_attribution(loss_all, top, rows)
    score = np.full(r.idx.shape, np.nan)
    k, j = np.nonzero(r.idx >= 0)
    score[k, j] = s_all[r.idx[k, j], k]
    return ScoreRankAttribution(r.idx, r.loss, score, r.taken, r.positive, err)


def quantile_bounds(counts, permille: int):
    """``(lo_us, hi_us)`` of the bucket that holds the quantile ``permille`` (an int in
    [0, 1000]) of the n samples counted in ``counts`` ([240]): the sample of 0-based rank
    ``(permille * (n - 1)) // 1000``, the rank rule of the quantile calls, lies in
    ``[lo_us, hi_us)`` (``hi_us`` is +inf for the last bucket).  (NaN, NaN) for n = 0."""
    _check_permille(permille)
    c = merge(counts)
    if c.shape != (BINS,):
        raise ValueError(f"counts must have shape [{BINS}]")
    n = int(c.sum())
    if n == 0:
        return float("nan"), float("nan")
    k = (int(permille) * (n - 1)) // 1000
    b = int(np.searchsorted(np.cumsum(c), k, side="right"))
    us = edges_us()
    return float(us[b]), float(us[b + 1])
