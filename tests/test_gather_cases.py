"""tests/gather_cases.py has the shape it is meant to have: counted with oracle/kmer_oracle alone, no GPU.  The planted
input's filtered pair list holds 63, 64, 65, one, several hundred and no survivors in items of the pipelined intersection,
and something in the first and in the last item."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import gather_cases as GC                                                   # noqa: E402
from coarse_run import _reference                                           # noqa: E402


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def test_planted_items(K):
    texts, flags = GC.planted()
    p_in, p_out = CC.pillars(flags)
    _, cands, _ = _reference(K, "gather_planted_pair", [texts[p_in], texts[p_out]], [True, False], CC.LDR)
    hist = GC.item_histogram(cands)
    want = GC.expected_items()
    for item, n in want.items():
        assert hist[item] == n, (item, n, hist[item])
    assert np.delete(hist, list(want)).sum() == 0            # (nothing but the plants survives)
    assert {0, 1, 63, 64, 65} <= set(hist.tolist()) and hist.max() >= 300
    assert hist[0] > 0 and hist[-1] > 0


@pytest.mark.parametrize("case", ["dense", "skew"])
def test_the_borrowed_cases_fill_their_items(K, case):
    """dense: thousands of survivors in the items of one top byte beside items with a handful; skew: entries in most items"""
    texts, flags = CC.dense("AAAA", 4000) if case == "dense" else CC.skew()
    p_in, p_out = CC.pillars(flags)
    _, cands, _ = _reference(K, f"gather_{case}_pair", [texts[p_in], texts[p_out]], [True, False], CC.LDR)
    hist = GC.item_histogram(cands, 9 if case == "dense" else 10)
    if case == "dense":
        assert hist.max() > 300 and np.median(hist) < 63
    else:
        assert (hist > 0).sum() > len(hist) // 4
