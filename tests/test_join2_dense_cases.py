"""tests/join2_dense_cases.py without a GPU: with oracle/kmer_oracle alone, the item of every case holds exactly the planted
keys -- n of the anchor, n (or 3 n) of the other genome, no stray window of either strand --, every one of them is live under
the numpy restatement of the screen, and all planted prefixes are candidates."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as cc                                                   # noqa: E402
import join2_cases as J                                                     # noqa: E402
import join2_dense_cases as JD                                              # noqa: E402

GEO = J.PLANT_GEO
SLOTS = 4 * GEO["T"]


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _item(keys):
    return keys[J.item_of(keys, GEO) == np.uint64(JD.HEAD)]


def _held(K, name, texts, flags, plants, per_b, out_mask, per_a=1, in_mask=1 << J.A_):
    c = J.census(K, name, texts, flags)
    ka, kb = (_item(k) for k in c["keys"])
    want = np.sort(np.array(plants["all"], dtype=np.uint64))
    n = len(want)
    assert len(np.unique(want)) == n
    # exactly the planted keys: per_a * n of the anchor, per_b * n of the other genome, nothing else of either strand
    assert len(ka) == per_a * n and np.array_equal(np.unique(ka & cc.PMASK), want)
    assert np.all(np.unique(ka & cc.PMASK, return_counts=True)[1] == per_a)
    shown = 0
    for b in np.unique((ka >> np.uint64(cc.DIAG_SHIFT)) & np.uint64(3)):
        shown |= 1 << int(b)
    assert shown == in_mask
    assert len(kb) == per_b * n and np.array_equal(np.unique(kb & cc.PMASK), want)
    assert np.all(np.unique(kb & cc.PMASK, return_counts=True)[1] == per_b)
    assert len(c["keys"][0]) < len(c["keys"][1])                            # genome 0 is the anchor
    # every key of the item is live
    assert J.live_share(ka, kb, GEO) == 1.0
    # all planted prefixes are candidates, and the item holds no other
    cands = c["cands"]
    inside = cands[J.item_of(cands["prefix"], GEO) == np.uint64(JD.HEAD)]
    assert np.array_equal(inside["prefix"], want)
    assert np.all(inside["in_mask"] == in_mask) and np.all(inside["out_mask"] == out_mask)
    return len(ka), len(kb)


def test_the_item_lies_where_the_cases_say():
    assert GEO["mlog"] == 0 and GEO["rb"] == 54 and JD.T == GEO["T"] == 512
    assert JD.HEAD not in J.HEADS.values()
    assert JD.SIZES == (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1089)
    # element e of thread t is key 2 (t + (e >> 1) T) + (e & 1): with n keys, all live, wave 0 sees min(64, ceil((n - e) / 2))
    # live lanes in key slot e < 2 -- fills of 1 (n = 1, 2), 32 + 31 (63), 32 + 32 = 64: one drain, nothing left (64),
    # 33 + 32 = 65: a drain at exactly 64 and one left (65), two drains (128), a second wave (129)
    live = lambda n, e: min(64, max(0, (n - e + 1) // 2))                   # noqa: E731
    assert [live(n, 0) + live(n, 1) for n in (1, 2, 63, 64, 65, 127, 128)] == [1, 2, 63, 64, 65, 127, 128]


@pytest.mark.parametrize("n", JD.SIZES)
def test_all_live(K, n):
    texts, flags, plants = JD.all_live(n)
    assert len(plants["all"]) == n
    assert _held(K, f"all live {n}", texts, flags, plants, 1, 1 << J.G_) == (n, n)
    assert n <= SLOTS


@pytest.mark.parametrize("count", JD.LONG)
def test_all_live_long(K, count):
    texts, flags, plants = JD.all_live_long(count)
    na, nb = _held(K, f"all live long {count}", texts, flags, plants, 3, 0b1110)
    assert (na, nb) == (count, 3 * count)
    # 500: one batch of the other genome, key slots 2 and 3 on top of drained ones; 700: more than a batch, walked twice
    assert (nb > SLOTS) == (count == JD.LONG[1])


def test_all_live_two_bases(K):
    texts, flags, plants = JD.all_live_two_bases()
    na, nb = _held(K, "all live two bases", texts, flags, plants, 1, 1 << J.G_, per_a=2, in_mask=0b0011)
    assert (na, nb) == (2 * JD.TWO_BASES, JD.TWO_BASES)
    # the anchor's keys reach key slots 2 and 3 of its batch (positions 2 T and up) and stay inside it; the distinct prefixes
    # load the exact table to little more than a half
    assert 2 * JD.T + 64 < na <= SLOTS and len(plants["all"]) * 16 < (1 << J.J2_TAB_LOG) * 9
