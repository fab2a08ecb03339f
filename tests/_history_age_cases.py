"""The elements of the history-aging tests (CPU twins and GPU kernels): the directed elements
aimed at history_age.hip's compaction -- every count lane evicted or kept, bucket byte 0 used and
unused, the two ends of the entry array -- and a few hundred random canonical elements from a
fixed seed.  ``history(R, S, phase)`` lays them out as a compact history starting at element
``phase`` of the list (cyclically), so that the smallest shapes still meet every directed element;
``aged`` is the host twin's result, computed once per argument set and never written to."""
import functools

import numpy as np

from nvidia_resiliency_ext.straggler import histograms

E = histograms.CHIST_ENTRIES
CB = histograms.CHIST_BYTES
BINS = histograms.BINS
MAXC = 2 ** 32 - 1
BIG = 2 ** 31  # survives every shift up to 31
SHIFTS = (1, 2, 31)

DIRECTED = (
    ("empty", {}),
    ("one_count_1", {50: 1}),                                            # becomes empty
    ("one_count_max", {50: MAXC}),
    ("full_all_survive", {7 * i + 3: BIG + 5 * i for i in range(E)}),
    ("full_alternating", {9 * i + 1: (1 if i % 2 == 0 else BIG + i) for i in range(E)}),
    ("full_alternating_odd", {9 * i + 2: (1 if i % 2 else MAXC - i) for i in range(E)}),
    ("full_last_survives", {11 * i + 4: (MAXC if i == E - 1 else 1) for i in range(E)}),  # 11 -> 0
    ("full_first_survives", {11 * i + 5: (MAXC if i == 0 else 1) for i in range(E)}),
    ("bucket0_survives", {0: BIG + 1, 9: 1, 17: 3}),                     # byte 0 is a used entry
    ("bucket0_evicted", {0: 1, 9: MAXC}),
    ("bucket0_alone", {0: MAXC}),
    ("bucket239", {100: 1, 239: BIG}),
    ("bucket239_evicted", {3: BIG, 239: 1}),
    ("full_ends", {**{0: 2, 239: 3}, **{20 * i: BIG for i in range(1, E - 1)}}),
    ("full_to_empty", {13 * i: 1 for i in range(E)}),
)
NAMES = tuple(n for n, _ in DIRECTED)


def pack(entries) -> np.ndarray:
    """A canonical element (uint8 [64]) from {bucket: count}, written out field by field."""
    e = np.zeros(CB, np.uint8)
    b = sorted(entries)
    assert len(b) <= E and all(0 <= x < BINS and 1 <= entries[x] <= MAXC for x in b)
    e[:4 * len(b)] = np.asarray([entries[x] for x in b], "<u4").view(np.uint8)
    e[4 * E:4 * E + len(b)] = b
    e[5 * E:] = np.asarray([len(b)], "<u4").view(np.uint8)
    return e


def _random(n, seed=20240):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = int(rng.integers(0, E + 1))
        buckets = np.sort(rng.choice(BINS, m, replace=False)).tolist()
        kinds = rng.integers(0, 5, m)
        counts = [int([rng.integers(1, 4), rng.integers(1, 9), rng.integers(1, 1 << 16),
                       rng.integers(1 << 30, 1 << 32), MAXC][k]) for k in kinds]
        out.append(dict(zip(buckets, counts)))
    return out


@functools.lru_cache(maxsize=None)
def elements() -> np.ndarray:
    """uint8 [len(DIRECTED) + 300, 64]: the directed elements, then the random ones."""
    e = np.stack([pack(d) for _, d in DIRECTED] + [pack(d) for d in _random(300)])
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def history(R: int, S: int, phase: int = 0) -> np.ndarray:
    """uint8 [R, S, 64]: elements()[phase], [phase + 1], ... cyclically (read-only)."""
    el = elements()
    h = el[(phase + np.arange(R * S)) % len(el)].reshape(R, S, CB).copy()
    h.setflags(write=False)
    return h


def phases(R: int, S: int):
    """Start elements such that a [R, S] history meets every directed element at least once."""
    return tuple(range(0, len(DIRECTED), R * S))


@functools.lru_cache(maxsize=None)
def aged(R: int, S: int, phase: int, shift: int):
    """``histograms.compact_age`` of ``history(R, S, phase)``: (chist', evicted, full), read-only."""
    out = histograms.compact_age(history(R, S, phase), shift)
    for a in out:
        a.setflags(write=False)
    return out


def direct(h: np.ndarray, shift: int):
    """Aging restated without the twin's helpers, straight on the bytes: (chist', evicted, full)."""
    R, S, _ = h.shape
    out = np.zeros_like(h)
    evicted, full = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    for r in range(R):
        for s in range(S):
            cnt = h[r, s, :4 * E].view("<u4").tolist()
            bkt = h[r, s, 4 * E:5 * E].tolist()
            n = int(h[r, s, 5 * E:].view("<u4")[0])
            kept = [(cnt[i] >> shift, bkt[i]) for i in range(n) if cnt[i] >> shift]
            out[r, s, :4 * len(kept)] = np.asarray([c for c, _ in kept], "<u4").view(np.uint8)
            out[r, s, 4 * E:4 * E + len(kept)] = [b for _, b in kept]
            out[r, s, 5 * E:] = np.asarray([len(kept)], "<u4").view(np.uint8)
            evicted[r] += np.uint64(n - len(kept))
            full[r] += np.uint64(len(kept) == E)
    return out, evicted, full
