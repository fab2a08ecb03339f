"""Record streams built to order for the branches of records_bucket_kernel (numpy, no GPU).

Every case is one launch: `recs` / `off` / `nslots` / `cap`, and `claim`, a function that
raises AssertionError unless the model (tests/_records_model.py) shows the case taking the branch
it was built for.  Sizes come from the model's constants, so after a constant changes the claim
says that a case is mis-aimed instead of the case quietly testing something else.  Every record's
ns is its index in the launch plus NS0: a lost, duplicated or misplaced record shows in the
content of a bucket.  tests/test_records_model_cpu.py runs the claims; tests/test_gpu_records_branches.py
runs the streams on the GPU against retain()."""
import functools
from collections import namedtuple

import numpy as np

import _records_model as M

NS0 = 1000
Case = namedtuple("Case", "name recs off nslots cap claim names")


def invalid_slots(nslots):
    return [nslots, nslots + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]


def _finish(name, streams, nslots, cap, claim, names=None):
    """streams: one array of slots per stream, push order."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    slots = np.concatenate([np.asarray(s, np.uint32) for s in streams]) if off[-1] else np.zeros(0, np.uint32)
    recs = np.stack([slots, np.arange(slots.size, dtype=np.uint32) + NS0], axis=1)
    return Case(name, np.ascontiguousarray(recs), off, nslots, cap, claim,
                names or [str(t) for t in range(len(streams))])


def stream_slots(case, t):
    return case.recs[case.off[t]:case.off[t + 1], 0]


def pass_counts(case, t, slot_lo, m):
    """pushes per slot of stream t inside one pass's slot range"""
    ls = (stream_slots(case, t) - np.uint32(slot_lo)).astype(np.int64)
    return np.bincount(ls[ls < m], minlength=m)


def _shuffled(rng, counts, first_slot=0):
    s = np.repeat(np.arange(first_slot, first_slot + len(counts), dtype=np.uint32), counts)
    rng.shuffle(s)
    return s


def _parity(streams, names, body, name, odd):
    """append `body` so that it starts at an even (odd) record index, after a one-record filler
    stream where the running offset has the other parity"""
    if (sum(len(s) for s in streams) % 2 == 1) != odd:
        streams.append(np.zeros(1, np.uint32))
        names.append("filler")
    streams.append(body)
    names.append(name + ("@odd" if odd else "@even"))


# ------------------------------------------------------------------ (a) sources
SOURCES_NSLOTS = (37, 4100)  # the second: no room for a stash beside the counters and the stage


def source_lengths(nslots):
    S = M.launch(nslots).stash_pairs
    H, W, B = M.HEAD_RECORDS, M.RB_WAVES, M.BATCH_PAIRS
    full = H + 2 * W * S
    return {"n0": 0, "n1": 1, "n2": 2, "n127": 127, "n128": 128, "n129": 129, "one_row": 2 * 64 * W,
            "head-1": H - 1, "head": H, "head+1": H + 1,
            "stash_full": full, "stash_full-2": full - 2, "stash_full+2": full + 2,
            "iters0": H + W * (2 * (S + B) - 2), "iters1": H + W * 2 * (S + B),
            "stash_runs_out": H + W * 2 * (S + 2 * B), "stash_idle_iter": H + W * 2 * (S + 4 * B),
            "empty_chunks": H + 10}


def _claim_source(name, n, nslots):
    """the aligned variant of one length"""
    S = M.launch(nslots).stash_pairs
    B = M.BATCH_PAIRS
    so = M.sources(n, False, nslots)
    w, src = so.waves, so.src
    count = lambda k: int((src == k).sum())  # noqa: E731
    if S == 0:
        assert count(M.STASH) == 0 and all(x.snp == 0 for x in w)
        if name.startswith("stash_"):  # aimed at the stash: here only lengths like the others
            return
    if name in ("n0", "n1", "n2", "n127", "n128", "n129", "one_row", "head-1", "head", "head+1"):
        assert count(M.REG) == min(n & ~1, M.HEAD_RECORDS) and count(M.SCALAR) == n - count(M.REG) <= 1
    elif name == "stash_full":
        assert all(x.snp == S and x.hi - x.lo == 2 * S and x.iters == 0 for x in w)
        assert count(M.STASH) == n - M.HEAD_RECORDS and all(x.stash_final == S // 64 for x in w)
    elif name == "stash_full-2":
        assert w[-1].snp == S - 1 and all(x.snp == S for x in w[:-1]) and count(M.TAIL) == 0
    elif name == "stash_full+2":
        assert all(x.snp == S and x.hi - x.lo == 2 * S + 2 for x in w[:-1]) and count(M.TAIL) == 2 * (M.RB_WAVES - 1)
        assert 0 < w[-1].snp < S
    elif name == "iters0":
        assert all(x.iters == 0 and x.snp == S and x.stash_final == S // 64 for x in w)
        # one pair short of a batch for lane 63: the other lanes run the loop once, with no stash
        # interleaved (per_it 0), lane 63 reads the tail
        assert all(x.per_it == 0 for x in w) and count(M.TAIL) == M.RB_WAVES * 2 * (B // 64 - 1)
        assert count(M.UNROLL) == M.RB_WAVES * 2 * 63 * M.RB_UNROLL
    elif name == "iters1":
        assert all(x.iters == 1 and x.per_it == S // 64 and x.stash_final == 0 and not x.short_iter for x in w)
        assert count(M.UNROLL) == M.RB_WAVES * 2 * B and count(M.TAIL) == 0
    elif name == "stash_runs_out":  # the last iteration asks for more stash than is left
        assert all(x.short_iter and x.per_it * (x.iters - 1) < S // 64 for x in w)
        assert all(x.iters == 2 for x in w)
    elif name == "stash_idle_iter":  # the last iteration finds the stash empty
        assert all(x.iters == 4 and x.per_it * (x.iters - 1) >= S // 64 for x in w)
    elif name == "empty_chunks":
        assert any(x.hi == x.lo for x in w) and any(x.hi > x.lo for x in w)
    else:
        raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def sources_case(nslots):
    rng = np.random.default_rng(nslots)
    lengths = source_lengths(nslots)
    streams, names = [], []
    for name, n in lengths.items():
        for odd in (False, True):
            _parity(streams, names, rng.integers(0, nslots, n).astype(np.uint32), name, odd)

    def claim(case):
        S = M.launch(nslots).stash_pairs
        assert (S == 0) == (nslots == SOURCES_NSLOTS[1])
        seen = set()
        for t, nm in enumerate(case.names):
            if nm == "filler":
                continue
            name, at = nm.split("@")
            n = int(case.off[t + 1] - case.off[t])
            assert n == lengths[name] and (case.off[t] % 2 == 1) == (at == "odd")
            if at == "odd":  # not 16-byte aligned: every record by the scalar path
                so = M.sources(n, True, nslots)
                assert so.rp == 0 and (so.src == M.SCALAR).all()
            else:
                _claim_source(name, n, nslots)
            seen |= set(np.unique(M.sources(n, at == "odd", nslots).src).tolist())
        assert seen == ({M.REG, M.UNROLL, M.TAIL, M.SCALAR} | ({M.STASH} if S else set()))

    return _finish(f"sources_{nslots}", streams, nslots, 0, claim, names)


# ------------------------------------------------------------------ (b) tiers
TIER_CAPS = (1, 7, 8, 9, 512, 513, 0)


def tier_counts(cap):
    return [0, 1, 4, 5, 8, 9, 12, 511, 512, 513] + ([cap, cap + 1, cap - 1] if cap > 0 else [])


@functools.lru_cache(maxsize=None)
def tiers_case(cap):
    counts = tier_counts(cap)
    nslots = len(counts)

    def claim(case):
        assert pass_counts(case, 0, 0, nslots).tolist() == counts
        L = M.layout(counts, cap, nslots, False)
        tier = dict(zip(counts[:10], L.tier[:10].tolist()))
        free = lambda c: cap == 0 or cap >= c  # noqa: E731  a ring of c records does not overflow
        assert tier[0] == 0
        assert tier[8] == (0 if free(8) else 2) and tier[9] == (1 if free(9) else 2)
        assert tier[512] == (1 if free(512) else 2) and tier[513] == 2
        assert L.overflow[9] == (not free(513))  # 513 records
        if cap > 0:
            at_cap, over, under = 10, 11, 12
            assert not L.overflow[at_cap] and L.overflow[over] and not L.overflow[under]
            assert L.tier[over] == 2
            assert L.tier[at_cap] == {1: 0, 7: 0, 8: 0, 9: 1, 512: 1, 513: 2}[cap]
        # the tiers follow one another
        order = np.lexsort((np.arange(nslots), L.tier))
        assert (np.diff(L.st[order]) >= 0).all()

    return _finish(f"tiers_cap{cap}", [_shuffled(np.random.default_rng(cap), counts)], nslots, cap, claim)


# ------------------------------------------------------------------ (c) the stage limit
STAGE_NSLOTS = 6000
STAGE_CAP = 8192
STAGE_NAMES = ("tiny_ends_at_limit", "tiny_starts_at_limit", "tiny_straddles", "cold_straddles",
               "tiny_end_is_limit", "tiny_past_limit")


@functools.lru_cache(maxsize=None)
def stage_case():
    nslots = STAGE_NSLOTS
    lim = M.launch(nslots).stage_cap
    rng = np.random.default_rng(lim)
    z = lambda: np.zeros(nslots, np.int64)  # noqa: E731
    c = {}
    c["tiny_ends_at_limit"] = z() + 5                       # padded 8
    if lim % 8:
        c["tiny_ends_at_limit"][0] = 3
    c["tiny_starts_at_limit"] = z() + 2                     # padded 4
    c["tiny_straddles"] = z() + 7
    if lim % 8 == 0:
        c["tiny_straddles"][0] = 1                          # st = 4 + 8 k
    c["cold_straddles"] = z()
    c["cold_straddles"][:50] = 3
    c["cold_straddles"][50:150] = 500 - np.arange(100) % 3
    c["tiny_end_is_limit"] = z()
    c["tiny_end_is_limit"][:lim // 4] = 4
    c["tiny_end_is_limit"][lim // 4:lim // 4 + 40] = 100
    c["tiny_past_limit"] = rng.integers(0, 9, nslots)
    streams = [_shuffled(rng, c[k]) for k in STAGE_NAMES]

    def claim(case):
        assert lim < M.RB_STAGE_KB * 256
        L = {}
        for t, k in enumerate(STAGE_NAMES):
            assert np.array_equal(pass_counts(case, t, 0, nslots), c[k])
            L[k] = M.layout(c[k], STAGE_CAP, nslots, True)
            assert not L[k].overflow.any()
        x = L["tiny_ends_at_limit"]
        assert x.stage_lim == lim and ((x.tier == 0) & (x.st + x.padded == lim) & x.reduced).any()
        x = L["tiny_starts_at_limit"]
        assert x.stage_lim == lim and ((x.tier == 0) & (x.st == lim) & (x.padded > 0) & ~x.reduced).any()
        x = L["tiny_straddles"]
        assert ((x.tier == 0) & (x.padded == 8) & (x.st + 4 == x.stage_lim) & ~x.reduced).any()
        x = L["cold_straddles"]
        assert ((x.tier == 1) & (x.st < x.stage_lim) & (x.st + x.padded > x.stage_lim)).any()
        assert x.stage_lim == lim and 0 < x.skip == x.tiny_end // 4 < lim // 4
        x = L["tiny_end_is_limit"]
        assert x.tiny_end == x.stage_lim == lim < x.cold_total and x.skip == lim // 4
        x = L["tiny_past_limit"]
        assert x.tiny_end > x.stage_lim == lim and x.skip == 0 and x.reduced.any()
        assert ((x.tier == 0) & (x.padded > 0) & ~x.reduced).any() and (x.tier == 1).sum() == 0

    return _finish("stage_limit", streams, nslots, STAGE_CAP, claim, list(STAGE_NAMES))


# ------------------------------------------------------------------ (d) the ordered walk
WALK_NSLOTS = 200     # 0..63 overflow, 64..199 are pushed once per stream (kept at any cap)
WALK_CAPS = (3, 1)
WALK_NAMES = ("same_slot", "distinct64", "drop_inside_group", "partial_last_step", "mixed_step")


@functools.lru_cache(maxsize=None)
def walk_case(cap):
    nslots = WALK_NSLOTS
    rng = np.random.default_rng(64)
    bad = invalid_slots(nslots)

    def kept_slots():
        return iter(rng.permutation(np.arange(64, nslots)).tolist())

    def take(it, k):
        return [next(it) for _ in range(k)]

    s = {}
    k = kept_slots()
    s["same_slot"] = take(k, 64) + [0] * 64
    k = kept_slots()
    s["distinct64"] = take(k, 64) + [x for _ in range(4) for x in rng.permutation(64).tolist()]
    k = kept_slots()
    step0 = [0] * 20 + take(k, 44)
    rng.shuffle(step0)
    step1 = take(k, 5) + [x for _ in range(10) for x in (0, next(k))]
    s["drop_inside_group"] = step0 + step1
    k = kept_slots()
    s["partial_last_step"] = take(k, 64) + [1] * 10 + take(k, 20) + [1] * 7
    k = kept_slots()
    s["mixed_step"] = take(k, 64) + [x for i in range(16) for x in (2, next(k), bad[i % 5], 3)]
    streams = [np.array(s[n], np.uint32) for n in WALK_NAMES]

    def claim(case):
        W = {n: M.walk(stream_slots(case, t), nslots, cap) for t, n in enumerate(WALK_NAMES)}
        assert any(len(st.groups) == 1 and st.groups[0].lanes.size == 64 for st in W["same_slot"])
        assert any(len(st.groups) == 64 for st in W["distinct64"])
        st = W["drop_inside_group"][1]  # step 1, from lane 5 on, every other lane
        g = st.groups[0]
        assert g.lanes[0] == 5 and (np.diff(g.lanes) == 2).all()
        assert g.occ0 < g.drop < g.occ0 + g.lanes.size
        st = W["partial_last_step"][-1]
        assert 0 < st.lanes < 64 and st.groups and st.kept > 0
        assert any(len(st.groups) >= 2 and st.kept > 0 and st.invalid >= 5 for st in W["mixed_step"])
        if cap == 1:
            assert all(g.drop == 63 for st in W["same_slot"] for g in st.groups)

    return _finish(f"walk_cap{cap}", streams, nslots, cap, claim, list(WALK_NAMES))


# ------------------------------------------------------------------ (e) invalid slots
INVALID_NSLOTS = (37, 2 * M.RB_PASS_SLOTS + 5)
_PICKS = (3, 70, 201, 334, -1)  # which records of a source carry the five invalid slots


def _invalid_length():
    S = M.launch(5).stash_pairs  # also launch(37): both leave the stash its full size
    return M.HEAD_RECORDS + M.RB_WAVES * 2 * (S + M.BATCH_PAIRS + 100)


def _invalid_positions(n, models):
    pos = []
    for nslots_pass in models:
        src = M.sources(n, False, nslots_pass).src
        for k in (M.REG, M.STASH, M.UNROLL, M.TAIL):
            idx = np.flatnonzero(src == k)
            if idx.size:
                pos.append(idx[list(_PICKS)])
    return np.unique(np.concatenate(pos).reshape(-1, 5), axis=0)  # rows of five positions


@functools.lru_cache(maxsize=None)
def invalid_case(nslots):
    single = nslots <= M.RB_PASS_SLOTS
    cap = 100 if single else 3
    n = _invalid_length()
    rng = np.random.default_rng(nslots)
    ranges = M.passes(nslots)
    models = sorted({m for _, m in ranges})
    if single:  # five heavy slots overflow, the others keep everything
        body = np.where(rng.random(n) < 0.97, rng.integers(0, 5, n), rng.integers(5, nslots, n))
    else:       # the first and last slot of every pass overflow; so do some of the others
        edges = np.array([e for lo, m in ranges for e in (lo, lo + m - 1)])
        body = np.where(rng.random(n) < 0.2, edges[rng.integers(0, edges.size, n)], rng.integers(0, nslots, n))
    body = body.astype(np.uint32)
    rows = _invalid_positions(n, models)
    for row in rows:
        body[row] = invalid_slots(nslots)
    streams, names = [], []
    _parity(streams, names, body, "main", False)
    _parity(streams, names, body.copy(), "main", True)

    def claim(case):
        assert M.launch(37).stash_pairs == M.launch(5).stash_pairs > 0
        assert names == ["main@even", "filler", "main@odd"] and case.off[2] % 2 == 1
        sl = stream_slots(case, 0)
        assert np.array_equal(sl, stream_slots(case, 2))
        assert sorted(set(sl[sl >= nslots].tolist())) == sorted(invalid_slots(nslots))
        for lo, m in ranges:
            so = M.sources(n, False, m)
            want = {M.REG, M.UNROLL, M.TAIL} | ({M.STASH} if M.launch(m).stash_pairs else set())
            for v in invalid_slots(nslots):  # every invalid value from every source of this pass
                assert set(so.src[sl == v].tolist()) == want, (lo, v)
            assert (M.sources(n, True, m).src == M.SCALAR).all()
            # records on either side of the pass's range, and inside it
            assert (sl < lo).any() == (lo > 0) and (sl[sl < nslots] >= lo + m).any() == (lo + m < nslots)
            cnt = pass_counts(case, 0, lo, m)
            assert cnt[0] > cap and (single or cnt[m - 1] > cap) and (cnt[(cnt > 0)] <= cap).any()
            # in the walk: steps that hold overflowed and invalid records together, and (the
            # five-slot last pass of the large table has next to no kept records) kept ones too
            W = M.walk(sl, m, cap, lo)
            steps = {int(i) // 64 for i in np.flatnonzero(sl >= nslots)}
            assert sum(1 for b in steps if W[b].groups) >= 5
            assert m == 5 or sum(1 for b in steps if W[b].groups and W[b].kept) >= 5
        assert any(M.launch(m).stash_pairs for m in models) and len(ranges) == (1 if single else 3)

    return _finish(f"invalid_{nslots}", streams, nslots, cap, claim, names)


# ------------------------------------------------------------------ (f) passes
PASS_NSLOTS = (1, 63, 64, 65, 1024, 1025, 12287, 12288, 12289)
PASS_CAP = 3


@functools.lru_cache(maxsize=None)
def passes_case(nslots):
    rng = np.random.default_rng(nslots)
    ranges = M.passes(nslots)
    streams = []
    for _ in range(2):
        counts = rng.integers(0, 5, nslots)
        for lo, m in ranges:
            counts[lo] = counts[lo + m - 1] = 7
        streams.append(_shuffled(rng, counts))

    def claim(case):
        assert len(ranges) == (2 if nslots > 12288 else 1) and ranges[-1][1] == (1 if nslots == 12289 else nslots)
        for t in range(2):
            for lo, m in ranges:
                L = M.layout(pass_counts(case, t, lo, m), PASS_CAP, m, False)
                assert L.overflow[0] and L.overflow[m - 1]
                assert m < 63 or ((L.tier == 0) & (L.padded > 0)).any()

    return _finish(f"passes_{nslots}", streams, nslots, PASS_CAP, claim)


# ------------------------------------------------------------------ every case
BUILDERS = ([("sources", sources_case, n) for n in SOURCES_NSLOTS] +
            [("tiers", tiers_case, c) for c in TIER_CAPS] +
            [("stage", lambda _: stage_case(), 0)] +
            [("walk", walk_case, c) for c in WALK_CAPS] +
            [("invalid", invalid_case, n) for n in INVALID_NSLOTS] +
            [("passes", passes_case, n) for n in PASS_NSLOTS])
IDS = [f"{kind}-{arg}" for kind, _, arg in BUILDERS]


def build(i):
    _, fn, arg = BUILDERS[i]
    return fn(arg)
