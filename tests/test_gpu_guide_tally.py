"""kr_guide_hits_tally on the GPU (csrc/k_guide_hits.inc: k_ghit_tally): the device's counts per (guide, mismatches) equal
the counts of the fetched hits over seeded cases of guide_hit_cases.py; the hit list is only read -- the fetch and the
windows give the same bytes before and after --; a dense text whose every hit is one guide's gives the closed-form count; a
text without a hit gives zeros; the state and capacity errors."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hit_cases as GC                                               # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("g12_none", 3, False), ("g20_tttv", 2, False), ("g20_tttv", 2, True), ("g28_h", 1, False), ("g40_long", 0, False)]


def _texts(guides):
    G = len(guides[0]) if len(guides) else 1
    return np.frombuffer("".join(guides).encode("ascii"), dtype=np.uint8).reshape(-1, G)


def _counts(hits, nguides):
    return np.bincount(4 * hits["guide"].astype(np.int64) + hits["mismatches"], minlength=4 * nguides).reshape(nguides, 4)


@pytest.mark.parametrize("name, M, need", CASES, ids=[f"{n}-M{m}{'-need_pam' if p else ''}" for n, m, p in CASES])
def test_the_tally_counts_the_fetched_hits(name, M, need):
    from krisp_amd import _native
    c = GC.case(name, M)
    want = GC.reference(name, M, False, need)
    n = len(c["guides"])
    with _native.Engine() as eng:
        eng.set_params_locate(0, c["G"], 0, False, max_bases=GC.N_TEXT)
        eng.upload(0, c["text"])
        eng.guide_hits_table(_texts(c["guides"]), M, c["pam5"], c["pam3"], need)
        hits = eng.guide_hits(0)
        rows = eng.guide_hit_windows(c["G"])
        tally = eng.guide_hits_tally()
        again = eng.guide_hits_tally()
        # the list is only read
        out = np.empty(max(len(hits), 1), dtype=_native.GUIDE_HIT_RAW)
        assert eng.lib.kr_guide_hits_fetch(eng.ctx, out.ctypes.data_as(ctypes.c_void_p), len(hits)) == len(hits)
        assert out[:len(hits)].tobytes() == hits.tobytes()
        assert eng.guide_hit_windows(c["G"]).tobytes() == rows.tobytes()
        # a scan without a fetch, as guide_tallies runs it
        assert eng.guide_hits_scan(0) == len(hits)
        third = eng.guide_hits_tally()
    print(name, "M", M, "need_pam", need, "hits", len(hits), "guides", n, "tally", tally.sum(axis=0).tolist())
    assert len(hits) == len(want) > 0
    assert tally.dtype == np.uint32 and tally.shape == (n, 4)
    assert np.array_equal(tally, _counts(hits, n)) and int(tally.sum()) == len(hits)
    assert np.array_equal(tally, _counts(want, n))
    assert not tally[:, M + 1:].any()
    assert tally.tobytes() == again.tobytes() == third.tobytes()


@pytest.mark.parametrize("period", [1, 2])
def test_one_guide_takes_every_hit(period):
    """runs of thousands of equal neighbours: the adds are combined, the count is exact; a second guide without a hit"""
    from krisp_amd import _native
    G = 20
    text, guide, plus, minus = GC.dense(G, period)
    quiet = "ACGGTCATTGCAGGATCCAA"
    with _native.Engine() as eng:
        eng.set_params_locate(0, G, 0, False, max_bases=len(text))
        eng.upload(0, text)
        for M in (0, 3):
            eng.guide_hits_table(_texts([quiet, guide]), M)
            assert eng.guide_hits_scan(0) == plus + minus
            tally = eng.guide_hits_tally()
            print("period", period, "M", M, "tally", tally.tolist())
            assert tally.tolist() == [[0, 0, 0, 0], [plus + minus, 0, 0, 0]]
        # no hit at all: zeros
        eng.guide_hits_table(_texts([quiet]), 1)
        assert eng.guide_hits_scan(0) == 0
        assert eng.guide_hits_tally().tolist() == [[0, 0, 0, 0]]


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    CAP, STATE = -3, -4
    guide = "ACGTTGCAAGCTTGACCTGA"
    text = (b"TTTC" + guide.encode() + b"CAGT") * 3
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    out = np.full(16, 77, dtype=np.uint32)
    with _native.Engine() as eng:
        tally = lambda cap: eng.lib.kr_guide_hits_tally(eng.ctx, ptr(out), cap)          # noqa: E731
        assert tally(16) == STATE                                              # no locate context
        eng.set_params_locate(0, 20, 0, False, max_bases=1000)
        assert tally(16) == STATE                                              # no table, no scan
        eng.upload(0, text)
        eng.guide_hits_table(_texts([guide, guide[::-1]]), 1)
        assert tally(16) == STATE and b"kr_guide_hits_scan first" in eng.lib.kr_last_error(eng.ctx)
        assert eng.guide_hits_scan(0) == 3
        assert tally(7) == CAP and (out == 77).all()
        assert tally(8) == 8 and out[:8].tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and (out[8:] == 77).all()
        # a new table: the hits are another table's
        eng.guide_hits_table(_texts([guide]), 1)
        assert tally(16) == STATE
        assert eng.guide_hits_scan(0) == 3 and tally(4) == 4 and out[:4].tolist() == [3, 0, 0, 0]
        # no guides: nothing to count, any buffer will do
        eng.guide_hits_table(np.empty((0, 20), dtype=np.uint8), 1)
        assert eng.guide_hits_scan(0) == 0 and tally(0) == 0
        assert eng.guide_hits_tally().shape == (0, 4)
