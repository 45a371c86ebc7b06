"""k_gather_items: the dense, ordered candidate list from the per-item runs of the pipelined intersection, a
workgroup per 64 items whose threads walk the workgroup's outputs.

Two sorted genomes (one ingroup, one outgroup) with the filter on, over inputs whose items hold 0, 1, 63, 64, 65 and several
hundred to thousands of survivors: `dense` and `skew` of coarse_cases.py and the planted input of gather_cases.py (the first
and the last item non-empty; tests/test_gather_cases.py counts the shapes with the oracle alone).  One case in key-space
slices (KR_SLICE_BASES=1: the relative -> absolute prefix step), one without the filter, one n-way call whose list is sparse.
The rule of every case: candidates (prefix, in_mask, out_mask) in order and the records equal oracle/kmer_oracle.c and are
BIT-IDENTICAL to a run with KR_ISECT_KERNEL = 1 (one workgroup per chunk: k_gather_cands, no items).  Seconds per case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import gather_cases as GC                                                   # noqa: E402
from coarse_run import _reference                                           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _run(N, texts, flags, kernel, apply_filter=True):
    ids = list(range(len(texts)))
    with N.Engine() as e:
        e.set_option(N.OPT_COARSE_REST, 0)
        e.set_option(N.OPT_ISECT_KERNEL, kernel)
        e.set_params(*CC.LDR, max_bases=max(len(t) for t in texts))
        for g, t in zip(ids, texts):
            e.upload(g, t)
            e.sort(g)
        n = e.intersect(ids, flags, apply_filter=apply_filter)
        cands = e.cands().copy()
        assert n == len(cands)
        recs = e.collect(ids).copy()
        info, isect = e.debug_info(), e.debug_isect()
    return cands, recs, info, isect


def _case(N, K, name, texts, flags, apply_filter=True, slices=1):
    _, want, wrec = _reference(K, name, texts, flags, CC.LDR, apply_filter=apply_filter)
    got, recs, info, isect = _run(N, texts, flags, 0, apply_filter)
    assert info["nslices"] == slices
    assert isect["threads"] >= 256                      # (the pipelined kernel ran: its items are what k_gather_items reads)
    assert len(got) == len(want)
    for f in ("prefix", "in_mask", "out_mask"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(np.sort(recs, order=["key", "genome"]), wrec)
    chunks, crecs, _, _ = _run(N, texts, flags, 1, apply_filter)
    assert np.array_equal(got, chunks), "candidates differ between KR_ISECT_KERNEL = 0 and 1"
    assert np.array_equal(recs, crecs), "records (in kr_fetch order) differ between KR_ISECT_KERNEL = 0 and 1"
    return got, info, isect


def _pair(texts, flags):
    p_in, p_out = CC.pillars(flags)
    return [texts[p_in], texts[p_out]], [True, False]


def test_planted_counts_per_item(N, K):
    texts, flags = _pair(*GC.planted())
    got, info, isect = _case(N, K, "gather_planted_pair", texts, flags)
    # the items the run had are the items the input was planted for
    assert info["b"] - isect["buckets_per_item_log2"] == GC.ITEM_BITS
    hist = GC.item_histogram(got)
    assert {0, 1, 63, 64, 65} <= set(hist.tolist()) and hist.max() >= 300 and hist[0] > 0 and hist[-1] > 0


def test_planted_in_key_space_slices(N, K, monkeypatch):
    monkeypatch.setenv("KR_SLICE_BASES", "1")
    texts, flags = _pair(*GC.planted())
    _case(N, K, "gather_planted_pair", texts, flags, slices=4)


@pytest.mark.parametrize("case", ["dense", "skew"])
def test_borrowed_cases(N, K, case):
    texts, flags = _pair(*(CC.dense("AAAA", 4000) if case == "dense" else CC.skew()))
    got, _, _ = _case(N, K, f"gather_{case}_pair", texts, flags)
    assert len(got) > 3000


def test_without_the_filter(N, K):
    texts, flags = _pair(*CC.dense("TTTT", 4000))
    got, _, _ = _case(N, K, "gather_dense_T_pair_nofilter", texts, flags, apply_filter=False)
    assert len(got) > 100_000                           # (every shared prefix)


def test_sparse_list_of_four_genomes(N, K):
    """the n-way call over four sorted genomes: a few hundred candidates in 512 items, most workgroups leave at once"""
    from krisp_amd import synth
    fam = synth.family(31, 2, 2, 300_000, records=4, snp_every=2000)
    texts, flags = [t for _, _, t in fam], [f for _, f, _ in fam]
    got, info, isect = _case(N, K, "fam31_2_2", texts, flags)
    hist = GC.item_histogram(got, info["b"] - isect["buckets_per_item_log2"])
    assert 0 < len(got) < 1000 and (hist == 0).sum() > len(hist) // 2
