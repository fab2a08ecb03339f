"""GPU: Detector.kernel_tail_score, the collective tail score of the per-process drop-in.  2- and
3-rank gloo worlds on one GPU (fresh processes, each under its own time limit): the ranks hold
overlapping but different kernel sets, one rank has an injected tail; every rank's TailScore
equals the definition in plain Python integers (``_tail_ref``) over all ranks' pushed records,
and the report that follows is the report of a run that never made the call."""
import pytest

import _tail_ref as REF
import _tail_workers as W
from _mp import run_world

pytestmark = pytest.mark.gpu

ZERO = [0] * REF.BINS


def reference(ws):
    per = [W.pushed(r, ws) for r in range(ws)]
    union = sorted(set().union(*(set(p) for p in per)))
    counts = [[REF.hist_of(p[n]) if n in p else ZERO for n in union] for p in per]
    _, _, sums, rows = REF.full(counts, W.PM, W.THRESHOLD)
    return union, sums, rows


def check_rank(ts, rank, union, sums, rows):
    row = rows[rank]
    assert ts["tail_ns"] == row["tail_ns"] and ts["total_ns"] == row["total_ns"]
    assert REF.bits(ts["score"]) == REF.bits(row["score"])
    assert REF.bits(ts["fleet_share"]) == REF.bits(float(sums[0]) / float(sums[1]))
    assert ts["is_straggler"] == row["strag"]
    want = sorted(((n, c) for n, c in zip(union, row["calls"]) if c), key=lambda e: (-e[1], e[0]))
    assert ts["top"] == want[:3]


@pytest.mark.parametrize("ws", [2, 3])
def test_every_rank_equals_the_reference(ws):
    union, sums, rows = reference(ws)
    got = run_world(ws, "_tail_workers", "tail_score_rank", timeout=120)
    assert sorted(union) == sorted(W.NAMES) and all(len(W.rank_names(r, ws)) == 5 for r in range(ws))
    for rank in range(ws):
        check_rank(got[rank]["ts"], rank, union, sums, rows)
        assert got[rank]["after"] == {}  # generate_report reset the interval
    assert [got[r]["ts"]["is_straggler"] for r in range(ws)] == [r == W.SLOW_RANK for r in range(ws)]
    if ws == 2:
        # the report after the call is the report of a run that does not make it
        plain = run_world(ws, "_tail_workers", "tail_score_rank", timeout=120, tail=False)
        for rank in range(ws):
            assert plain[rank]["ts"] is None
            for key in ("kern", "rel", "ind"):
                assert got[rank][key] == plain[rank][key], (rank, key)
            # the median-based score does not flag the rank the tail score flags
            assert all(v >= W.THRESHOLD for v in got[rank]["rel"].values())


def test_world_of_one_without_a_process_group():
    union, sums, rows = reference(1)
    got = W.run_solo(timeout=120)
    check_rank(got["ts"], 0, union, sums, rows)
    assert got["ts"]["score"] == 1.0 and not got["ts"]["is_straggler"]  # the fleet is the rank
    assert len(got["ts"]["top"]) == 3 and sorted(got["kern"]) == sorted(W.NAMES)
