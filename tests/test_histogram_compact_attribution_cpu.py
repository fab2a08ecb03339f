"""CPU: ``histograms.compact_history_attribution`` -- the host twin of
nvrx_histogram_history_attribution_compact -- against the definition, on every case of
``_histogram_compact_cases.cases()`` with ``top`` cycling through 1, 4, 8, 16 (and the
supplementary case of ``_histogram_compact_attr_cases``): it equals
``histograms.history_attribution`` on the dense expansion of the history, every field byte for
byte.  The cases together must hold what an attribution can get wrong -- a row with fewer taken
elements than ``top``, a negative loss, a NaN loss left out because the history weighs nothing, a
tie between two columns -- or the table proves less than it claims."""
import numpy as np
import pytest

import _histogram_compact_attr_cases as A

CASES = A.cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_twin_equals_the_dense_twin_on_the_expansion(c):
    got, want = A.twin(c.name), A.oracle(c.name)
    top = A.top_of(c.name)
    assert got.idx.shape == (c.R, top) and got.loss_all.shape == (c.R, c.K)
    for f in A.FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype, f
        assert g.tobytes() == w.tobytes(), f


def test_top_cycles_and_the_table_is_whole():
    assert [A.top_of(c.name) for c in CASES[:5]] == [1, 4, 8, 16, 1]
    assert A.table_size() == len(CASES) - 1 and CASES[-1].name == "weightless_history"


def test_the_cases_hold_what_an_attribution_can_get_wrong():
    fewer = negative = nan_left_out = tie = 0
    for c in CASES:
        res, top = A.twin(c.name), A.top_of(c.name)
        taken = ~np.isnan(res.loss_all)
        short = taken.sum(1) < top
        fewer += int(short.any())
        for r in np.flatnonzero(short):  # the empty slots of such a row
            n = int(taken[r].sum())
            assert (res.idx[r, n:] == -1).all() and np.isnan(res.loss[r, n:]).all()
        negative += int((res.loss_all < 0).any())
        for r in range(min(c.R, 3)):
            v = res.loss_all[r][taken[r]]
            tie += int(len(set(v.tolist())) < v.size)
            for k in range(c.K):
                if c.counts[r, k].any() and A.base_total(c, r, k) == 0 and \
                        A.dense_of(c)[r, k if c.hist_index is None else c.hist_index[k]].any():
                    assert np.isnan(res.loss_all[r, k]) and k not in res.idx[r].tolist()
                    nan_left_out += 1
    assert fewer and negative and nan_left_out and tie, (fewer, negative, nan_left_out, tie)
