"""CPU: the dispatch model of the ragged statistics (tests/_ragged_model.py) and the case list of
tests/test_gpu_ragged_classes.py (tests/_ragged_cases.py).  No GPU.

Closure is the statement whose violation leaves output rows unwritten: whatever class the
classifier gives a segment from its own retained length, the host launches that class's kernel
from the hint and cap alone."""
import numpy as np
import pytest

import _ragged_cases as C
import _ragged_model as M
from _moments_cases import sent_to_exact

PARAMS = pytest.mark.parametrize("aligned16,exact", C.PARAMS, ids=[C.tag(a, e) for a, e in C.PARAMS])
BIG_HINT = 1 << 20


@PARAMS
def test_closure(aligned16, exact):
    top = max(8200, M.all_gate_keeps(aligned16, exact)[-1])
    # below[k]: the classes of every n in 1..k when no n is the FULL length (grown one n at a time)
    below = [frozenset()]
    for n in range(1, top + 1):
        below.append(below[-1] | {M.seg_class(n, aligned16, exact, 0)})
    gate_keeps = set(M.all_gate_keeps(aligned16, exact))
    assert gate_keeps <= set(range(1, top + 1))
    for keep in range(1, top + 1):  # every keep in 1..8200 and every gate keep
        # every n in 1..keep: the FULL length of a launch is its keep, so it changes the class of
        # n == keep alone
        fn = M.full_len(keep, aligned16, exact)
        classes = below[keep - 1] | {M.seg_class(keep, aligned16, exact, fn)}
        if keep <= 300 or keep in gate_keeps:  # the same, plainly
            assert classes == {M.seg_class(n, aligned16, exact, fn) for n in range(1, keep + 1)}
        tight = M.launched(keep, 0, aligned16, exact)
        assert classes <= tight, (keep, sorted(classes - tight))
        # the same keep through cap under a large hint: the classifier sees min(len, cap), the
        # host keep_of(hint, cap)
        assert M.keep_of(BIG_HINT, keep) == keep and M.launched(BIG_HINT, keep, aligned16, exact) == tight
        # loose hints (max_len > true longest = keep): no segment has the hint's FULL length
        for hint in {keep + 1, keep + 3, 2 * keep, 1024, 2048, 4096, 8192, 8193, 20000, 70000}:
            if hint > keep:
                loose = M.launched(hint, 0, aligned16, exact)
                assert below[keep] <= loose, (keep, hint, sorted(below[keep] - loose))


@PARAMS
def test_closure_breaks_when_a_gate_moves(aligned16, exact, monkeypatch):
    # the self-check of the suite: the lane gate `keep > n / 2` flipped to `keep > n` leaves the
    # segments of (n / 2, n] in a class nothing launches -- the closure above must see it
    real = M.launched

    def flipped(max_len, cap, a, e):
        keep = M.keep_of(max_len, cap)
        return frozenset(c for c in real(max_len, cap, a, e) if c not in M.LANE[1:] or keep > M.LANE_N[c])

    monkeypatch.setattr(M, "launched", flipped)
    with pytest.raises(AssertionError):
        test_closure(aligned16, exact)


def test_classes_and_gates():
    assert [M.seg_class(n, False, False, 0) for n in (1, 8, 9, 16, 17, 128, 129, 253, 254, 8189, 8190)] == \
        ["T8", "T8", "T16", "T16", "T32", "T128", "W4", "W4", "W8", "W128", "X"]
    assert [M.seg_class(n, True, False, 1024) for n in (256, 257, 1023, 1024, 1025, 8192, 8193)] == \
        ["W4", "W8", "W16", "F", "W32", "W128", "X"]
    assert M.seg_class(1024, True, False, 0) == "W16" and M.seg_class(1024, False, False, 1024) == "F"
    assert M.seg_class(129, True, True, 0) == "X" and M.seg_class(128, True, True, 0) == "T128"
    assert M.full_len(2048, True, False) == 2048
    assert not M.full_len(2048, False, False) and not M.full_len(2048, True, True) and not M.full_len(2047, True, False)
    assert M.keep_of(10, 0) == 10 and M.keep_of(10, 7) == 7 and M.keep_of(5, 7) == 5 and M.keep_of(10, -1) == 10
    # the gates the scan finds: what the host code states, not typed into the model's scan
    g = M.gate_keeps(True, False)
    assert g["T16"] == [(8, 9)] and g["T128"] == [(64, 65)] and g["W4"] == [(128, 129)]
    assert g["W8"] == [(256, 257)] and g["W128"] == [(4096, 4097)] and g["X"] == [(8192, 8193)]
    assert g["F"] == [(1023, 1024), (1025, 1024), (2047, 2048), (2049, 2048), (4095, 4096), (4097, 4096),
                      (8191, 8192), (8193, 8192)]
    g = M.gate_keeps(False, False)
    assert g["W8"] == [(253, 254)] and g["X"] == [(8189, 8190)] and "F" not in g
    g = M.gate_keeps(False, True)
    assert g["X"] == [(128, 129)] and set(g) == {"T16", "T32", "T64", "T128", "X"}
    assert M.reachable(True, False) == frozenset(M.CLASSES)
    assert M.reachable(False, False) == frozenset(M.CLASSES) - {"F"}
    assert M.reachable(True, True) == M.reachable(False, True) == frozenset(M.LANE + ("X",))


def test_exact_variant_edges():
    want = {129: ("lds1024", None), 1024: ("lds1024", None), 1025: ("lds8192", None),
            8192: ("lds8192", None), 8193: ("lds32768", None), 32768: ("lds32768", None),
            32769: ("global", 65536), 65536: ("global", 65536), 65537: ("global", 131072)}
    assert set(want) == set(C.EXACT_EDGES)
    for keep, v in want.items():
        assert tuple(M.exact_variant(keep)) == v, keep
    assert M.exact_global_np2(1) == 8192 and M.exact_global_np2(8193) == 16384
    assert M.exact_global_np2(M.MAX_SEGMENT) == M.MAX_SEGMENT


def test_expect_exact_bits_agrees_with_sent_to_exact():
    # sent_to_exact is the rule of a launch beyond the lane classes (the strided tests use it at
    # any length); expect_exact_bits adds the lane classes of the ragged path and EXACT mode
    for aligned16 in (False, True):
        for keep in range(1, 9001):
            want = sent_to_exact(keep, aligned16) or keep <= 128
            assert M.expect_exact_bits(keep, aligned16, False) == want, (keep, aligned16)
            assert M.expect_exact_bits(keep, aligned16, True)
            if keep <= 128:
                assert not sent_to_exact(keep, aligned16)


def test_classifier_blocks():
    assert M.classifier_blocks(1) == (1, 1) and M.classifier_blocks(1024) == (1, 1024)
    assert M.classifier_blocks(1025) == (2, 513)
    nb, chunk = M.classifier_blocks(C.NSEGS[-1])
    assert nb == 66 and nb > 64 and (nb - 1) * chunk < C.NSEGS[-1] <= nb * chunk
    assert M.classifier_blocks(5 << 20) == (1024, 5120)


def test_cases_are_aimed():
    """Every case honours the contract and sits where its name says."""
    for c in C.all_cases():
        assert populated_is_launched(c), c.name
    for a, e in C.PARAMS:
        for keep in M.all_gate_keeps(a, e):
            c = C.gate_case(keep, a, e)
            k = C.kept(c)
            assert c.max_len == keep == k.max() and (k == keep - 1).any() == (keep > 1)
            assert (k == 0).any() and (k < 0).any()
        tight, loose = C.loose_cases(a, e)
        assert np.array_equal(tight.lens, loose.lens) and tight.lens.max() == 5 == tight.max_len
        assert loose.max_len == 20000
    # partition: the deliberately placed classes are in their block and nowhere else
    for nseg in C.NSEGS[1:]:
        nblocks, chunk = M.classifier_blocks(nseg)
        where = C.partition_blocks(nseg)
        for config, (a, e, cap, hint, special) in C.PARTITION.items():
            c = C.partition_case(nseg, config)
            k = C.kept(c)
            fn = M.full_len(M.keep_of(hint, cap), a, e)
            cls = np.array([M.seg_class(int(n), a, e, fn) if n > 0 else "-" for n in k])
            block = np.arange(nseg) // chunk
            homes = {}
            for w, groups in special.items():
                for name, *_ in groups:
                    homes.setdefault(name, set()).add(where[w])
            for name, blocks in homes.items():
                assert set(block[cls == name]) == blocks, (c.name, name)
            if nblocks > 2:  # lane classes absent from whole blocks, present in others
                for name in ("T16", "T32", "T64", "T128"):
                    seen = set(block[cls == name])
                    assert seen and seen != set(range(nblocks)), (c.name, name)
                assert (k == 0).any() and (k < 0).any()
    nb = M.classifier_blocks(C.NSEGS[-1])[0]
    assert C.partition_blocks(C.NSEGS[-1]) == {"first": 0, "last": nb - 1, "high": 64}
    for c, only in zip(C.one_class_cases(), ("T8", "W4", "X")):
        assert C.populated(c) == {only} and (c.lens > 0).all()


def populated_is_launched(case):
    return C.populated(case) <= C.case_launched(case)


def test_coverage():
    report = C.coverage()
    assert C.format_coverage(report)
    # an incomplete list is noticed: without the cap launches nothing populates FULL next to an
    # open X gate ... without (b) the global EXACT kernel never runs
    with pytest.raises(AssertionError):
        C.coverage([c for c in C.all_cases() if c.group != "b"])
    with pytest.raises(AssertionError):
        C.coverage([c for c in C.all_cases() if not c.name.startswith("gate-")])
