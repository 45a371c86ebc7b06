"""tests/join2_cases.py without a GPU: with oracle/kmer_oracle and the numpy restatement of the screen, each case really
forces the branch of k_join2 it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as cc                                                   # noqa: E402
import join2_cases as J                                                     # noqa: E402

GEO = J.PLANT_GEO
SLOTS = 4 * GEO["T"]


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _bases(keys, prefix):
    """the set of diagnostic bases (four bits) and the number of keys a genome holds under a prefix"""
    k = keys[(keys & cc.PMASK) == np.uint64(prefix)]
    s = 0
    for b in (k >> np.uint64(cc.DIAG_SHIFT)) & np.uint64(3):
        s |= 1 << int(b)
    return s, len(k)


def _slot_state(keys_a, keys_b, prefix):
    """(a, b) of the screen slot of `prefix` in its item"""
    it, sl = int(J.item_of(prefix, GEO)), int(J.slot_of(J.item_key(prefix, GEO)))
    out = []
    for keys in (keys_a, keys_b):
        k = keys[J.item_of(keys, GEO) == np.uint64(it)]
        k = k[J.slot_of(J.item_key(k, GEO)) == sl]
        s = 0
        for b in (k >> np.uint64(cc.DIAG_SHIFT)) & np.uint64(3):
            s |= 1 << int(b)
        out.append(s)
    return tuple(out)


def _count(keys, head):
    return int((J.item_of(keys, GEO) == np.uint64(head)).sum())


def test_geometry_takes_the_route():
    assert GEO["tagk"] and GEO["p0"] == 10 and GEO["mlog"] == 0 and GEO["b"] == 10 and GEO["w"] == 44 and GEO["T"] == 512
    u = J.geometry(J.UNIFORM_LEN + J.RECORDS - 1, 2 * J.UNIFORM_LEN, J.UNIFORM_LDR)
    assert u["tagk"] and u["p0"] == 12 and u["mlog"] == 0
    # (25, 1, 2) at 300 kbp -- the coarse tests' shape -- does not: too few items for 32-bit heads
    assert not J.geometry(300_003, 600_000, J.LDR)["tagk"]


@pytest.mark.parametrize("anchor", [0, 1])
def test_trap(K, anchor):
    texts, flags, plants = J.trap(anchor)
    assert len(texts[anchor]) < len(texts[1 - anchor])
    c = J.census(K, f"trap {anchor}", texts, flags)
    ka, kb = c["keys"]
    want = {"overlap": (0b0011, 2, 0b0010, 1), "two_out": (0b0001, 1, 0b0110, 2), "dup": (0b0001, 2, 0b0010, 1),
            "shared": (0b0001, 1, 0b0001, 1)}
    for kind, ps in plants.items():
        for p in ps:
            assert _bases(ka, p) + _bases(kb, p) == want[kind], kind
            sa, sb = _slot_state(ka, kb, p)
            if kind != "shared":
                assert J.live(sa, sb), kind          # (a per-key rule would pass only the overlap trap's a: the slot sends all on)
            assert bool(np.isin(np.uint64(p), c["cands"]["prefix"])) == (kind in ("two_out", "dup"))


def test_screen_collide(K):
    texts, flags, plants = J.screen_collide()
    c = J.census(K, "screen collide", texts, flags)
    ka, kb = c["keys"]
    for kind, pairs in plants.items():
        for p, q in pairs:
            assert p != q and int(J.item_of(p, GEO)) == int(J.item_of(q, GEO))
            assert int(J.slot_of(J.item_key(p, GEO))) == int(J.slot_of(J.item_key(q, GEO)))
            sa, sb = _slot_state(ka, kb, p)
            assert J.live(sa, sb), kind                                     # live through the collision ...
            assert not J.live(*[s for s, _ in (_bases(ka, p), _bases(kb, p))])      # ... P alone would be dead
            assert not np.isin(np.uint64(p), c["cands"]["prefix"])
            assert bool(np.isin(np.uint64(q), c["cands"]["prefix"])) == (kind == "cand_and_shared")
            assert (_bases(ka, q)[1] > 0, _bases(kb, q)[1] > 0) == {"cand_and_shared": (True, True), "only_a": (True, False),
                                                                    "only_b": (False, True)}[kind]


def test_table_collide(K):
    texts, flags, plants = J.table_collide()
    c = J.census(K, "table collide", texts, flags)
    for kind, pairs in plants.items():
        for p, q in pairs:
            ip, iq = int(J.item_key(p, GEO)), int(J.item_key(q, GEO))
            assert ip != iq and int(J.item_of(p, GEO)) == int(J.item_of(q, GEO))
            assert int(J.tab_hash(ip)) == int(J.tab_hash(iq))
            if kind == "low_equal":
                assert ip & 0xFFFFFFFF == iq & 0xFFFFFFFF and ip >> 32 != iq >> 32
            else:
                assert ip >> 32 == iq >> 32 and ip & 0xFFFFFFFF != iq & 0xFFFFFFFF
            assert np.isin(np.array([p, q], dtype=np.uint64), c["cands"]["prefix"]).all()


def test_edges(K):
    texts, flags, plants = J.edges()
    c = J.census(K, "edges", texts, flags)
    ka, kb = c["keys"]
    assert len(ka) < len(kb)
    assert _count(ka, J.HEADS["a_empty"]) == 0 and 0 < _count(kb, J.HEADS["a_empty"]) <= SLOTS
    assert _count(kb, J.HEADS["b_empty"]) == 0 and 0 < _count(ka, J.HEADS["b_empty"]) <= SLOTS
    assert 0 < _count(ka, J.HEADS["multi"]) <= 16 and _count(kb, J.HEADS["multi"]) > SLOTS
    assert _count(ka, J.HEADS["single"]) == 1 and _count(kb, J.HEADS["single"]) == 1
    # the item behind the single key starts at an odd key number in one genome at least
    starts = [int(np.searchsorted(J.item_of(k, GEO), np.uint64(J.HEADS["single"] + 1))) for k in (ka, kb)]
    odd = [s & 1 for s in starts]
    assert any(odd) or any(int(np.searchsorted(J.item_of(k, GEO), np.uint64(h))) & 1 for k in (ka, kb) for h in J.HEADS.values())
    assert int(J.item_of(plants["last"][0], GEO)) == (1 << GEO["b"]) - 1
    for p in plants["multi"][:J.MULTI_A] + plants["single"] + plants["last"]:
        assert np.isin(np.uint64(p), c["cands"]["prefix"])
    # no item's anchor run exceeds the slots: nothing here goes through the redo
    assert np.bincount(J.item_of(ka, GEO).astype(np.int64)).max() <= SLOTS


@pytest.mark.parametrize("count", [J.ALL_CAND, J.FULL])
def test_many_survivors(K, count):
    texts, flags, plants = J.many_survivors(count)
    c = J.census(K, f"survivors {count}", texts, flags)
    ka, kb = c["keys"]
    head = J.HEADS["all_cand" if count == J.ALL_CAND else "full"]
    na = _count(ka, head)
    assert count * 0.95 < na <= SLOTS
    inside = c["cands"]["prefix"][J.item_of(c["cands"]["prefix"], GEO) == np.uint64(head)]
    assert len(inside) > count * 0.95
    # the live anchor prefixes of the item against the exact table
    distinct = len(np.unique(ka[J.item_of(ka, GEO) == np.uint64(head)] & cc.PMASK))
    assert (distinct > (1 << J.J2_TAB_LOG)) == (count == J.FULL)


def test_dense(K):
    texts, flags, plants = J.dense()
    c = J.census(K, "dense", texts, flags)
    assert _count(c["keys"][0], J.HEADS["dense"]) > SLOTS
    assert np.isin(np.array(plants["dense"], dtype=np.uint64), c["cands"]["prefix"]).sum() > J.DENSE_BLOCKS * 0.9


def test_uniform_live_share(K):
    """the screen sends a small share of the keys on: the true candidates' keys and the slots' collisions"""
    texts, flags, _ = J.uniform(71, False, 0)
    c = J.census(K, "uniform False 0", texts, flags, J.UNIFORM_LDR)
    geo = J.geometry(max(len(t) for t in texts), len(c["keys"][0]), J.UNIFORM_LDR)
    assert geo["tagk"]
    share = J.live_share(c["keys"][0], c["keys"][1], geo)
    assert 0.0 < share < 0.5
