"""CPU: the record bucketing reference and layout model (tests/_records_model.py) and the claims of
the constructed streams (tests/_records_cases.py).  No GPU: a case whose claim fails here is
mis-aimed -- it no longer takes the branch it was built for -- whatever the kernel does with it."""
import numpy as np
import pytest

import _records_cases as C
import _records_model as M
import oracle as O


@pytest.mark.parametrize("cap", [0, 1, 3, 64])
def test_retain_is_the_reference_ring(cap):
    # per slot: the pushes through the oracle's ring (CircularBuffer.h restated), in ring order
    rng = np.random.default_rng(cap)
    nslots = 11
    lens = [0, 1, 500, 37]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    slot = rng.integers(0, nslots + 3, off[-1]).astype(np.uint32)  # three invalid slots
    slot[::97] = 0xFFFFFFFF
    ns = rng.integers(1, 1 << 24, off[-1]).astype(np.uint32)      # exact in float32
    r = M.retain(np.stack([slot, ns], 1), off, nslots, cap)
    assert len(r.kept) == r.counts.size == len(lens) * nslots
    for t in range(len(lens)):
        sl, v = slot[off[t]:off[t + 1]], ns[off[t]:off[t + 1]]
        for s in range(nslots):
            pushed = v[sl == s]
            g = t * nslots + s
            assert r.counts[g] == pushed.size
            want = O.ring_linearize(pushed.astype(np.float32), cap if cap else max(1, pushed.size))
            assert np.array_equal(r.kept[g].astype(np.float32), want), (t, s)


def test_launch_sizes():
    # small slot tables leave the stage its full size and 192 pairs of stash per wave; a full
    # pass has neither; in between the stash goes first, then the stage shrinks
    assert M.RB_PASS_SLOTS == 12288 and M.HEAD_RECORDS == 32768
    assert M.launch(37) == M.Launch(M.RB_STAGE_KB * 256, 192)
    assert M.launch(C.SOURCES_NSLOTS[1]) == M.Launch(M.RB_STAGE_KB * 256, 0)
    assert M.launch(C.STAGE_NSLOTS) == M.Launch(22896, 0)
    full = M.launch(M.RB_PASS_SLOTS)
    assert full.stash_pairs == 0 and 0 < full.stage_cap < M.RB_STAGE_KB * 256
    for n in (1, 37, 4100, 6000, 12288):
        L = M.launch(n)
        used = ((3 * n + 3) & ~3) * 4 + 4 * L.stage_cap + 16 * M.RB_WAVES * L.stash_pairs
        assert used <= M.RB_LDS_KB * 1024 - 256 and L.stage_cap % 4 == 0 and L.stash_pairs % 64 == 0


def test_sources_cover_every_record_once():
    for n in (0, 1, 129, M.HEAD_RECORDS + 10, M.HEAD_RECORDS + 40_001):
        for odd in (False, True):
            so = M.sources(n, odd, 37)
            covered = np.zeros(n, int)
            covered[:2 * so.rp] += 1
            for w in so.waves:
                covered[w.lo:w.hi] += 1
                assert w.stash_loop + w.stash_final == (w.snp + 63) // 64
            assert (covered == 1).all()


@pytest.mark.parametrize("i", range(len(C.BUILDERS)), ids=C.IDS)
def test_case_takes_its_branch(i):
    case = C.build(i)
    ns = case.recs[:, 1]
    assert np.array_equal(ns, np.arange(ns.size, dtype=np.uint32) + C.NS0)  # distinct
    case.claim(case)


def test_a_mis_aimed_case_fails_its_claim(monkeypatch):
    # the claims move with the constants: other constants, and the cases say they are mis-aimed
    case = C.sources_case(37)
    monkeypatch.setattr(M, "RB_UNROLL", 4)
    monkeypatch.setattr(M, "BATCH_PAIRS", 64 * 4)
    with pytest.raises(AssertionError):
        case.claim(case)
    monkeypatch.undo()
    stage = C.stage_case()
    monkeypatch.setattr(M, "RB_STAGE_KB", 64)
    with pytest.raises(AssertionError):
        stage.claim(stage)
    monkeypatch.undo()
    tiers = C.tiers_case(9)
    monkeypatch.setattr(M, "RB_TINY", 16)
    with pytest.raises(AssertionError):
        tiers.claim(tiers)
