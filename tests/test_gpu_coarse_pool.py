"""The pool of placed pass-1 targets for coarse genomes (KR_OPT_COARSE_POOL): a genome that kr_genome_partition
takes for the second time gets, behind that call's kr_intersect, a buffer the placement search chose, and writes its pass 1
there from its next partition on; a genome that leaves the coarse state gives the buffer back.

The rule, as in test_gpu_coarse.py: candidates in order, records in kr_fetch order and counts are BIT-IDENTICAL between
KR_OPT_COARSE_POOL = 1 and = 0 and equal to oracle/kmer_oracle.c (coarse_run.py).  4 x 300 kbp uniform genomes, 2 in / 2 out;
KR_PLACE_MIN_BYTES=0 lets the search run on their 4.8 MB buffers, KR_PLACE_TRIES=2 asks for it.  What the pool did is read
from Engine.debug_coarse_pool(): total = free + held at every point.  Seconds per test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coarse_run import _oracle, _reference, _same                           # noqa: E402

pytestmark = pytest.mark.gpu

LEN = 300_000
LDR = (25, 1, 2)


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


@pytest.fixture(scope="module")
def D():
    from krisp_amd import distributed
    return distributed


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("KR_PLACE_MIN_BYTES", "0")
    monkeypatch.setenv("KR_PLACE_TRIES", "2")
    for name in ("KR_COARSE_POOL", "KR_COARSE_REST", "KR_LANES"):
        monkeypatch.delenv(name, raising=False)


def _family(config, n_in, n_out):
    from krisp_amd import synth
    fam = synth.family(config, n_in, n_out, LEN, records=4, snp_every=2000)
    return [t for _, _, t in fam], [f for _, f, _ in fam]


def _pool(e):
    p = e.debug_coarse_pool()
    assert p["total"] == p["free"] + p["held"], p
    return p


class Session:
    """one engine over `texts`; step(ids) = distributed.sharded_step + what the rule compares, and the pool's state behind it"""

    def __init__(self, N, D, texts, flags, pool, lanes=None, coarse_rest=1, budget=0, upload=None):
        self.N, self.D, self.texts, self.flags = N, D, texts, flags
        self.e = N.Engine(hbm_budget=budget)
        self.e.set_option(N.OPT_COARSE_POOL, pool)
        self.e.set_option(N.OPT_COARSE_REST, coarse_rest)
        if lanes is not None:
            self.e.set_option(N.OPT_LANES, lanes)
        self.e.set_params(*LDR, max_bases=max(len(t) for t in texts))
        for g in (range(len(texts)) if upload is None else upload):
            self.e.upload(g, texts[g])
        self.out = {"cands": [], "recs": [], "counts": [], "keys": {}}
        self.pools = []

    def step(self, ids=None):
        ids = list(range(len(self.texts))) if ids is None else ids
        n, nrec = self.D.sharded_step(self.e, ids, [self.flags[g] for g in ids], 1)
        self.out["cands"].append(self.e.cands().copy())
        self.out["recs"].append(self.e.fetch_records(nrec).copy())
        assert n == len(self.out["cands"][-1])
        self.pools.append(_pool(self.e))
        return self.pools[-1]

    def close(self, ids=None):
        ids = list(range(len(self.texts))) if ids is None else ids
        self.out["counts"] = [self.e.count(g) for g in ids]
        self.e.close()
        return self.out


def _both(N, D, script, texts, flags, **kw):
    """`script(session)` with the pool on and off -> the run with the pool on"""
    res = []
    for pool in (1, 0):
        s = Session(N, D, texts, flags, pool, **kw)
        try:
            script(s)
        finally:
            res.append((s.close(), s.pools))
    (on, pools_on), (off, pools_off) = res
    _same(on, off)
    for p in pools_off:
        assert (p["total"], p["partitions"], p["searches"], p["on"]) == (0, 0, 0, 0), p
    return on, pools_on


@pytest.mark.parametrize("lanes", [None, 1, 3])
def test_four_steps_fill_the_pool_behind_the_second(N, K, D, lanes):
    texts, flags = _family(31, 2, 2)

    def script(s):
        for _ in range(4):
            s.step()

    on, pools = _both(N, D, script, texts, flags, lanes=lanes)
    _oracle(on, _reference(K, "fam31_2_2", texts, flags, LDR))
    assert len(on["cands"][0]) > 20
    p1, p2, p3, p4 = pools
    assert (p1["total"], p1["partitions"], p1["searches"]) == (0, 0, 0), p1
    # behind the second step's intersection: one search for both genomes; nobody holds a buffer yet
    assert (p2["total"], p2["free"], p2["held"], p2["partitions"], p2["searches"]) == (2, 2, 0, 0, 1), p2
    assert (p3["total"], p3["free"], p3["held"], p3["partitions"], p3["searches"]) == (2, 0, 2, 2, 1), p3
    assert (p4["total"], p4["free"], p4["held"], p4["partitions"], p4["searches"]) == (2, 0, 2, 4, 1), p4
    assert 0 < p3["held_ms"][0] <= p3["held_ms"][1]


def test_fetching_keys_promotes_and_frees_the_buffer(N, K, D):
    texts, flags = _family(31, 2, 2)
    ref = _reference(K, "fam31_2_2", texts, flags, LDR)
    seen = {}

    def script(s):
        for _ in range(3):
            s.step()
        if s.e.debug_coarse_pool()["on"]:
            assert _pool(s.e)["held"] == 2
        s.out["keys"][3] = s.e.keys(3)                       # (a reader of a coarse genome's keys sorts it fine)
        seen[s.e.debug_coarse_pool()["on"]] = (_pool(s.e), s.e.debug_lazy()["coarse_promoted"])
        s.step()

    on, pools = _both(N, D, script, texts, flags)
    _oracle(on, ref)
    after_keys, promoted = seen[1]
    assert promoted == 1 and seen[0][1] == 1
    assert (after_keys["total"], after_keys["free"], after_keys["held"]) == (2, 1, 1), after_keys
    assert (pools[3]["held"], pools[3]["free"], pools[3]["partitions"] - pools[2]["partitions"]) == (2, 0, 2), pools[3]


def test_upload_again_and_free_give_the_buffers_back(N, K, D):
    texts, flags = _family(31, 2, 2)
    ref = _reference(K, "fam31_2_2", texts, flags, LDR)
    seen = {}

    def script(s):
        for _ in range(3):
            s.step()
        log = [_pool(s.e)]
        s.e.upload(1, texts[1])
        log.append(_pool(s.e))
        s.e.free(3)
        log.append(_pool(s.e))
        s.e.upload(3, texts[3])
        log.append(_pool(s.e))
        seen[s.e.debug_coarse_pool()["on"]] = log
        s.step()

    on, pools = _both(N, D, script, texts, flags)
    _oracle(on, ref)
    held = [(p["total"], p["free"], p["held"]) for p in seen[1]]
    assert held == [(2, 0, 2), (2, 1, 1), (2, 2, 0), (2, 2, 0)], held
    # the buffers are taken from the free list again: no second search
    assert (pools[3]["held"], pools[3]["free"], pools[3]["searches"]) == (2, 0, 1), pools[3]
    assert pools[3]["partitions"] - pools[2]["partitions"] == 2


def test_six_genomes_after_four(N, K, D):
    """genomes 4 and 5 join behind three steps of the others: they write their own key arrays until their second partition"""
    texts, flags = _family(31, 3, 3)
    order = [0, 1, 3, 4, 2, 5]                               # (2 in / 2 out first; ids 4 and 5 are the ones that join)
    texts, flags = [texts[g] for g in order], [flags[g] for g in order]
    four = [0, 1, 2, 3]
    ref4 = _reference(K, "fam31_3_3_first_four", texts[:4], flags[:4], LDR)
    ref6 = _reference(K, "fam31_3_3_reordered", texts, flags, LDR)

    def script(s):
        for _ in range(3):
            s.step(four)
        s.e.upload(4, texts[4])
        s.e.upload(5, texts[5])
        for _ in range(3):
            s.step()

    on, pools = _both(N, D, script, texts, flags, upload=four)
    first = {key: (v[:3] if isinstance(v, list) and key != "counts" else v) for key, v in on.items()}
    later = {key: (v[3:] if isinstance(v, list) and key != "counts" else v) for key, v in on.items()}
    first["counts"] = [on["counts"][g] for g in four]
    _oracle(first, ref4)
    _oracle(later, ref6)
    got = [(p["total"], p["free"], p["held"], p["partitions"], p["searches"]) for p in pools]
    assert got == [(0, 0, 0, 0, 0), (2, 2, 0, 0, 1), (2, 0, 2, 2, 1),
                   (2, 0, 2, 4, 1),          # the new genomes' first partition: their own arrays, no search
                   (4, 2, 2, 6, 2),          # their second: the pool grows by two behind the intersection
                   (4, 0, 4, 10, 2)], got


def test_a_context_with_an_hbm_budget_never_searches(N, K, D, monkeypatch):
    """(nobody asked for placement: KR_PLACE_TRIES unset, three lanes so that the context counts as one that sorts many
    genomes) -- without a budget the pool fills, with one it stays empty"""
    monkeypatch.delenv("KR_PLACE_TRIES")
    texts, flags = _family(31, 2, 2)
    ref = _reference(K, "fam31_2_2", texts, flags, LDR)
    totals = {}
    for budget in (0, 8 << 30):
        s = Session(N, D, texts, flags, 1, lanes=3, budget=budget)
        try:
            for _ in range(4):
                s.step()
        finally:
            out = s.close()
        _oracle(out, ref)
        totals[budget] = [(p["total"], p["partitions"], p["searches"]) for p in s.pools]
    assert totals[0][-1] == (2, 4, 1), totals
    assert totals[8 << 30] == [(0, 0, 0)] * 4, totals


def test_coarse_rest_off_never_touches_the_pool(N, K, D):
    texts, flags = _family(31, 2, 2)
    s = Session(N, D, texts, flags, 1, coarse_rest=0)
    try:
        for _ in range(3):
            s.step()
    finally:
        out = s.close()
    _oracle(out, _reference(K, "fam31_2_2", texts, flags, LDR))
    assert all((p["total"], p["partitions"], p["searches"]) == (0, 0, 0) for p in s.pools), s.pools
