"""kr_primers_tally on the GPU (csrc/k_primers.inc: k_prim_tally): the device's counts per pair equal np.bincount of the
fetched products over the seeded texts of primer_cases.py, for every length set and M = 0 .. 3; the list's bytes are the
same before and after; a dense periodic text where one pair takes every product, so that the combined adds run; an empty
list; the library's refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primer_cases as PC                                                  # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_CAPACITY, KR_ERR_STATE = -3, -4      # include/krisp_hip.h


def _fetch(eng, n):
    """the n products the latest scan left on the device, as kr_primers_fetch orders them"""
    from krisp_amd import _native
    out = np.empty(max(n, 1), dtype=_native.PRODUCT_HIT)
    assert int(eng.lib.kr_primers_fetch(eng.ctx, _native._ptr(out), n)) == n
    return out[:n]


def _bincount(hits, npairs):
    """the fetched products counted on the host: [npairs, 8], column m = left_mm + right_mm, column 7 = clean ends"""
    want = np.zeros((npairs, 8), dtype=np.int64)
    pair = hits["pair"].astype(np.int64)
    mm = hits["left_mm"].astype(np.int64) + hits["right_mm"]
    assert len(hits) == 0 or (int(pair.max()) < npairs and int(mm.max()) <= 6)
    want[:, :7] = np.bincount(pair * 7 + mm, minlength=7 * npairs).reshape(npairs, 7)
    clean = (hits["left_end_mm"] == 0) & (hits["right_end_mm"] == 0)
    want[:, 7] = np.bincount(pair[clean], minlength=npairs)
    return want


@pytest.mark.parametrize("name", list(PC.LENGTH_SETS))
def test_the_tally_equals_the_bincount_of_the_fetched_products(name):
    """M = 0 .. 3: the counters against the fetched list, the list's bytes before and after the tally, a second tally"""
    from krisp_amd import _native
    for M in range(4):
        text, left, right, pairs, _ = PC.case(name, M)
        with _native.Engine() as eng:
            eng.set_params_locate(30, 40, 30, False, max_bases=len(text))
            eng.upload(0, np.frombuffer(text, dtype=np.uint8))
            eng.primers_table(left + right, len(left), pairs, M, PC.MAX_PRODUCT)
            n = eng.primers_scan(0)
            before = _fetch(eng, n)
            got = eng.primers_tally()
            again = eng.primers_tally()
            after = _fetch(eng, n)
        want = _bincount(before, len(pairs))
        print(name, "M", M, "products", n, "clean", int(want[:, 7].sum()), "by mismatches", want[:, :7].sum(axis=0).tolist())
        assert n == len(before) >= 16 and before.tobytes() == after.tobytes()
        assert got.shape == (len(pairs), 8) and got.dtype == np.uint32
        assert (got == want).all(), np.argwhere(got != want)[:5].tolist()
        assert got.tobytes() == again.tobytes()
        assert int(want[:, :7].sum()) == n and 0 < int(want[:, 7].sum()) <= n
        assert M == 0 or (want[:, 1:2 * M + 1].sum() > 0 and want[:, 7].sum() < n)     # (mismatches and unclean ends occur)
        assert not want[:, 2 * M + 1:7].any()


def test_a_repeat_sends_every_product_to_one_pair():
    """a text of period 16 whose every window is a site of left 0 or right 0: thousands of neighbouring products of pair 0 --
    whole wavefronts of one key, which the kernel adds once -- beside a pair that has none and a text that no pair names"""
    from krisp_amd import _native
    unit = b"ACGGTCATTGCAAGTC"
    text = unit * 600
    a, b = unit[:12], unit[4:16]                    # left 0 at every 16 k, right 0 at every 16 k + 4
    other = b"TTTTTGGGGGAAAAACCCCC"
    with _native.Engine() as eng:
        eng.set_params_locate(30, 40, 30, False, max_bases=len(text))
        eng.upload(0, np.frombuffer(text, dtype=np.uint8))
        eng.primers_table([a, other, b, other[::-1]], 2, [(0, 0), (1, 1), (1, 0)], 0, 400)
        n = eng.primers_scan(0)
        hits = _fetch(eng, n)
        got = eng.primers_tally()
    want = _bincount(hits, 3)
    print("products", n, "tally", got.tolist())
    assert n == len(hits) > 64 * 100 and (hits["pair"] == 0).all()
    assert (got == want).all() and got[0, 0] == n == got[0, 7] and not got[1:].any()


def test_an_empty_list_no_pair_and_the_refusals():
    from krisp_amd import _native
    a, b = b"ACGTACGTAC", b"GGATCCATTGCA"
    out = np.full(16, 7, dtype=np.uint32)

    def tally(cap):
        return int(eng.lib.kr_primers_tally(eng.ctx, _native._ptr(out), cap))

    with _native.Engine() as eng:
        eng.set_params_locate(10, 4, 10, False, max_bases=1000)
        eng.upload(0, np.frombuffer(b"ACGT" * 100, dtype=np.uint8))
        assert tally(16) == KR_ERR_STATE
        with pytest.raises(Exception, match="kr_primers_scan first"):
            eng.primers_tally()
        eng.primers_table([a, b], 1, [(0, 0)], 1, 100)
        assert tally(16) == KR_ERR_STATE                        # (a table, no scan yet)
        assert eng.primers_scan(0) == 0                         # GGATCCATTGCA is nowhere: an empty list
        assert tally(7) == KR_ERR_CAPACITY and tally(8) == 8
        assert not out[:8].any() and (out[8:] == 7).all()       # (zeros, nothing beyond the 8 counters)
        assert eng.primers_tally().tolist() == [[0] * 8]
        # a table without a pair: no counters
        eng.primers_table([a, b], 1, np.empty((0, 2), dtype=np.uint32), 1, 100)
        assert tally(16) == KR_ERR_STATE
        assert eng.primers_scan(0) == 0 and tally(0) == 0 and eng.primers_tally().shape == (0, 8)
        # products, and a short buffer
        eng.primers_table([a, a], 1, [(0, 0)], 0, 100)
        assert tally(16) == KR_ERR_STATE                        # (the new table's list is not scanned yet)
        n = eng.primers_scan(0)
        assert n > 0 and tally(7) == KR_ERR_CAPACITY
        out[:] = 7
        assert tally(16) == 8 and int(out[0]) == n == int(out[7]) and not out[1:7].any() and (out[8:] == 7).all()
