"""The shared case list of the tail score attribution tests (CPU: host twins against the plain
reference; GPU: device against host twins), aimed at the branches of
csrc/histogram_attribution.hip: workgroup trips and splits of the loss kernel (16 kernels per
trip), the select kernel's batches (2,048 columns each) and template instantiations (top <= 1 / 4
/ 8 / 16), empty slots, ordering, values at the limits, indexing and validity.

A case is a dict: name, kind ("relative" | "individual"), counts u32 [R, K, 240], pm, top and
  relative:    fleet (u64 [Kf, 240] or None: the sum over rows), thr_index (i32 [K] or None),
               col_valid (u8 [Kf] or None)
  individual:  hist u32 [R, S, 240], hist_index (i32 [K] or None), col_valid (u8 [K] or None)
"""
import numpy as np

BINS = 240
U32 = 0xFFFFFFFF


def synth(rng, R, K, tail_every=3, lo=24, hi=200):
    """Counts with a body in two adjacent buckets per kernel and, in every `tail_every`-th
    (row, kernel), a few calls some buckets higher."""
    c = np.zeros((R, K, BINS), np.uint32)
    body = rng.integers(lo, hi, K)
    r, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    c[r, k, body[k]] = rng.integers(50, 400, (R, K))
    c[r, k, body[k] + 1] = rng.integers(1, 60, (R, K))
    slow = rng.random((R, K)) < 1.0 / tail_every
    c[r[slow], k[slow], body[k[slow]] + rng.integers(3, 12, int(slow.sum()))] = rng.integers(1, 9, int(slow.sum()))
    return c


def _rel(name, counts, pm, top, fleet=None, thr_index=None, col_valid=None):
    return dict(name="rel-" + name, kind="relative", counts=counts, pm=pm, top=top, fleet=fleet,
                thr_index=None if thr_index is None else np.asarray(thr_index, np.int32),
                col_valid=None if col_valid is None else np.asarray(col_valid, np.uint8))


def _ind(name, counts, hist, pm, top, hist_index=None, col_valid=None):
    return dict(name="ind-" + name, kind="individual", counts=counts, hist=hist, pm=pm, top=top,
                hist_index=None if hist_index is None else np.asarray(hist_index, np.int32),
                col_valid=None if col_valid is None else np.asarray(col_valid, np.uint8))


def _history(rng, counts, scale=5):
    """A history like `scale` earlier intervals of the same body, without the slow calls."""
    body = counts.copy()
    top2 = np.sort(body, axis=2)[:, :, -2:-1]
    body[body < top2] = 0
    return (body * scale + rng.integers(0, 3, body.shape).astype(np.uint32) * (body > 0)).astype(np.uint32)


def build():
    rng = np.random.default_rng(20240613)
    cases = []
    # trips, splits, batches and instantiations: (R, K, top)
    shapes = [(1, 1, 1), (3, 15, 4), (64, 16, 5), (1, 17, 8), (3, 33, 16), (64, 33, 4), (64, 1, 16),
              (1, 16, 1), (3, 17, 5), (1, 2048, 8), (2, 2049, 16)]
    for R, K, top in shapes:
        c = synth(rng, R, K)
        cases.append(_rel(f"shape-{R}x{K}-top{top}", c, 950, top))
        cases.append(_ind(f"shape-{R}x{K}-top{top}", c, _history(rng, c), 950, top))

    # ties: columns 2 and 5 identical in every row (and in the base); the lower column first
    c = synth(rng, 3, 8, tail_every=1)
    c[:, 5] = c[:, 2]
    h = _history(rng, c)
    h[:, 5] = h[:, 2]
    cases += [_rel("ties", c, 900, 8), _ind("ties", c, h, 900, 8)]

    # a row whose every loss is negative: no call above the threshold while the base has a tail;
    # and zero losses (share 0 and no tail: +0.0 ties, the column order decides)
    c = synth(rng, 4, 12, tail_every=1)
    quiet = c[0].copy()
    quiet[np.arange(12)[:, None], np.argsort(quiet, axis=1)[:, :-2]] = 0
    c[0] = quiet
    h = c.copy() * 3  # the history has the slow calls: base share > 0
    cases += [_rel("negative-row", c, 900, 16), _ind("negative-row", c, h, 900, 16)]
    z = np.zeros((2, 6, BINS), np.uint32)
    z[:, :, 40] = 100  # one bucket: T = 40, nothing above it anywhere: tail 0, share 0, loss +0.0
    z[1, 3, 44] = 2
    cases += [_rel("zero-loss-ties", z, 990, 4), _ind("zero-loss-ties", z[:1], z[1:], 990, 5)]

    # values at the limits
    c = synth(rng, 2, 6)
    c[:, 1] = 0
    c[:, 1, 0] = 77            # every sample in bucket 0: btotal == 0, a NaN loss, left out
    c[:, 2] = 0
    c[:, 2, 1] = 10            # bucket 1 weighs 1: the smallest total
    c[:, 3, 236:] = [[5, 4, 3, 2], [9, 0, 1, 7]]   # the wide buckets 238 / 239
    c[0, 4, 100:104] = [U32, U32 - 1, 3, U32]      # u64 sums beyond 2^53: the conversion rounds
    c[1, 4, 100:104] = [U32, 1, U32, U32 - 7]
    c[:, 5, 237] = U32                             # products near 2^64: sums wrap mod 2^64
    c[:, 5, 239] = U32
    h = c[::-1].copy()
    h[:, 1] = c[:, 1]
    cases += [_rel("limits", c, 500, 8), _ind("limits", c, h, 500, 8),
              _rel("limits-pm0", c, 0, 4), _ind("limits-pm1000", c, h, 1000, 4)]

    # indexing and validity, relative: a fleet of 9 kernels, the rank's 7 columns a permuted
    # subset with negative entries; fleet kernel 4 has no samples and kernel 6 is not valid
    fleet = synth(rng, 40, 9, tail_every=2).astype(np.uint64).sum(0)
    fleet[4] = 0
    index = [7, -1, 0, 4, 6, 2, -3]
    c = np.zeros((3, 7, BINS), np.uint32)
    own = synth(rng, 3, 9, tail_every=2)
    for k, u in enumerate(index):
        c[:, k] = own[:, max(u, 0)]
    c[2] = 0  # an empty row of counts
    valid = [1, 1, 1, 1, 1, 1, 0, 1, 1]
    cases.append(_rel("thr-index", c, 950, 5, fleet=fleet, thr_index=index, col_valid=valid))
    cases.append(_rel("col-valid", synth(rng, 3, 9), 950, 4, col_valid=valid))

    # individual: slots permuted in a stride of 11 > K = 7 with negative entries, col_valid zeros,
    # an empty row of counts, a slot without history
    c = synth(rng, 3, 7, tail_every=2)
    slots = [9, 2, -1, 10, 0, -5, 4]
    h = np.zeros((3, 11, BINS), np.uint32)
    hk = _history(rng, c)
    for k, s in enumerate(slots):
        if s >= 0:
            h[:, s] = hk[:, k]
    h[:, 10] = 0   # column 3 has a slot and no history
    c[1] = 0
    cases.append(_ind("hist-index", c, h, 950, 8, hist_index=slots, col_valid=[1, 0, 1, 1, 1, 1, 1]))
    cases.append(_ind("no-history", synth(rng, 2, 5), np.zeros((2, 5, BINS), np.uint32), 950, 4))
    return cases


CASES = build()
IDS = [c["name"] for c in CASES]
