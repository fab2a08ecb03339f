"""Inputs of the history tail-score tests (CPU twin and GPU kernel share them): seeded random
(counts, history) pairs and the hand-made cells.  numpy only builds the arrays; the expected
values come from ``_history_tail_ref``."""
import numpy as np

import _history_tail_ref as HREF

BINS = 240
TOP = 0x80000000
FULL = 0xFFFFFFFF

# kernels of the hand-made row, by name
HAND = ("n1", "l0b0", "l0b1", "l0b2", "l0b3", "l59b0", "l59b1", "l59b2", "l59b3", "only239",
        "topbit", "no_current", "no_history", "invalid")
HAND_T = dict(l0b0=0, l0b1=1, l0b2=2, l0b3=3, l59b0=236, l59b1=237, l59b2=238, l59b3=239)


def random_case(R, K, seed, stride=None):
    """u32 counts [R, K, 240] and history [R, stride or K, 240]: clustered kernels whose history is
    a few intervals of the same shape, a tail on every 5th row's current counts, spread kernels,
    kernels without history / without current samples, and an all-zero row."""
    rng = np.random.default_rng(seed)
    S = stride or K
    c = np.zeros((R, K, BINS), np.uint32)
    h = np.zeros((R, S, BINS), np.uint32)
    for k in range(K):
        base = int(rng.integers(8, 228))
        if k % 4 == 1:  # spread
            c[:, k] = rng.integers(0, 2000, size=(R, BINS)) * (rng.random((R, BINS)) < 0.3)
            h[:, k] = rng.integers(0, 9000, size=(R, BINS)) * (rng.random((R, BINS)) < 0.3)
        else:           # clustered
            for j in range(int(rng.integers(2, 4))):
                c[:, k, base + j] = rng.integers(1, 400, size=R)
                h[:, k, base + j] = rng.integers(1, 1600, size=R)
            if k % 4 == 2:
                c[::5, k, base + 6] = rng.integers(1, 40, size=len(range(0, R, 5)))
        if k % 7 == 3:
            h[:, k] = 0          # a kernel first seen now
        if k % 7 == 5:
            c[:, k] = 0          # a kernel that did not run in this interval
    if K >= 2:  # counts the int32 view shows negative; one sum that saturates
        c[0, 1, 77], h[0, 1, 77], c[R - 1, 1, 78], h[R // 2, 1, 90] = TOP, TOP + 5, FULL, TOP + 1
    if R >= 3:
        c[1], h[1] = 0, 0        # a rank without samples or history
    return c, h


def hand_case():
    """One row of hand-made kernels (HAND) and one all-zero row; pm = 500 puts T on HAND_T."""
    K = len(HAND)
    c = np.zeros((2, K, BINS), np.uint32)
    h = np.zeros((2, K, BINS), np.uint32)
    col = {n: i for i, n in enumerate(HAND)}
    k = col["n1"]
    h[0, k, 100] = 1
    c[0, k, 99], c[0, k, 100], c[0, k, 101] = 3, 4, 5
    for n, t in HAND_T.items():
        k = col[n]
        h[0, k, t] = 100
        if t > 0:
            h[0, k, t - 1] = 10
        if t < BINS - 1:
            h[0, k, t + 1] = 10
        c[0, k, max(t - 1, 0)] += 7
        c[0, k, t] += 20
        c[0, k, min(t + 1, BINS - 1)] += 3
        c[0, k, min(t + 2, BINS - 1)] += 2
    k = col["only239"]
    h[0, k, 239], c[0, k, 239], c[0, k, 238] = 9, 4, 2
    k = col["topbit"]
    h[0, k, 120], h[0, k, 130], h[0, k, 131] = TOP, FULL, 7
    c[0, k, 120], c[0, k, 130], c[0, k, 131], c[0, k, 132] = FULL, 1, TOP + 1, TOP
    k = col["no_current"]
    h[0, k, 50], h[0, k, 51] = 30, 40
    k = col["no_history"]
    c[0, k, 60], c[0, k, 61] = 11, 12
    k = col["invalid"]
    h[0, k, 70], c[0, k, 70], c[0, k, 75] = 20, 10, 10
    valid = [int(n != "invalid") for n in HAND]
    return c, h, valid


def lists(a):
    return np.ascontiguousarray(a).view(np.uint32).tolist()


def reference(c, h, pm, mode=HREF.SCORE | HREF.UPDATE, **kw):
    """(rows, new history as a u32 array) of the plain-integer reference."""
    rows, new = HREF.history_scores(lists(c), lists(h), pm, mode, **kw)
    return rows, np.asarray(new, dtype=np.uint32).reshape(h.shape)
