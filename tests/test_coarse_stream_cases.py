"""The census of tests/coarse_stream_cases.py without a GPU: with oracle/kmer_oracle alone, each case has the shape that
tests/test_gpu_coarse_stream.py relies on -- keys per top byte, hits per unit, which genome lacks which prefix.  The probe has
no counters of its own, so that a branch ran is shown by counting what the kernel cannot avoid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import coarse_stream_cases as SC                                            # noqa: E402


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _in_byte(keys, t):
    return int(np.count_nonzero((keys >> np.uint64(56)) == np.uint64(t)))


def _chunks(n):
    return -(-int(n) // CC.CO_CHUNK)


@pytest.mark.parametrize("ncoarse", SC.MULTI)
def test_multi_genomes_differ_in_one_table(K, ncoarse):
    texts, flags, plants = SC.multi(ncoarse)
    c = CC.census(K, f"multi_{ncoarse}", texts, flags)
    coarse = CC.coarse(flags)
    assert len(coarse) == ncoarse and {flags[g] for g in coarse} == {True, False}
    mini = coarse[-1]
    Cp = c["C"]["prefix"]
    with_cands = [t for t in range(256) if _in_byte(Cp, t)]
    assert len(with_cands) > 200
    # different chunk counts per genome in top byte 0, and more candidates there than KR_COARSE_TCAP = 50: rounds x genomes x chunks
    chunks0 = [_chunks(CC.buckets(c["keys"][g])[0]) for g in coarse]
    assert len(set(chunks0)) == ncoarse and max(chunks0) >= 4 and chunks0[-1] == 1, chunks0
    assert _in_byte(Cp, 0) > 2 * 50
    # the mini genome: shorter than one iteration, and no key in most top bytes that have candidates
    assert len(c["keys"][mini]) == 2 * SC.MULTI_PLANTS < SC.ITER
    bm = CC.buckets(c["keys"][mini])
    assert sum(1 for t in with_cands if bm[t] == 0) > 150
    assert all(bm[SC.head_byte(h)] == SC.MULTI_PLANTS // 4 for h in ("AAAA", "AGTA", "GGAT", "TTTT"))
    # the plants are candidates every genome holds; what the family shares beyond them the mini genome lacks
    assert CC.held(Cp, SC.prefixes(plants)).all()
    assert np.array_equal(np.sort(c["cands"]["prefix"]), np.sort(SC.prefixes(plants)))
    assert len(Cp) > 10 * len(plants)
    # hit lists of different lengths: the longest alone overflows a list that holds the second longest
    nh = sorted(len(c["hits"][g]) for g in coarse)
    assert nh[-1] > nh[-2] > nh[0] == len(plants)
    assert 0 < c["row"] <= CC.COL_CAPM
    print(f"multi {ncoarse}: |C| = {len(Cp)} chunks in byte 0 {chunks0} hits {nh}")


def test_edges_buckets_are_exact(K):
    texts, flags, plants = SC.edges()
    c = CC.census(K, "edges", texts, flags)
    assert CC.coarse(flags) == [1, 3]
    keys = c["keys"][1]
    bucket = CC.buckets(keys)
    base = np.concatenate([[0], np.cumsum(bucket)])
    Cp = c["C"]["prefix"]
    want = {SC.head_byte(h): n for h, n in SC.EDGES}
    assert sorted(want.values()) == [1, SC.ITER - 1, SC.ITER, SC.ITER + 1, 2 * SC.ITER + 1]
    for t, n in want.items():
        assert bucket[t] == n, (t, bucket[t], n)
        assert _in_byte(Cp, t) >= SC.EDGES_PLANTS                    # (a unit exists)
        assert n <= CC.CO_CHUNK                                      # (one unit: its successor is genome 3's)
        assert CC.buckets(c["keys"][3])[t] > 0
        assert _in_byte(c["hits"][1], t) == SC.EDGES_PLANTS
    # every other key of genome 1 is the other strand's: top bytes 0x40 .. 0x7F
    others = [t for t in range(256) if bucket[t] and t not in want]
    assert others and all(0x40 <= t < 0x80 for t in others)
    assert {int(base[t]) & 1 for t in want} == {0, 1}                # an odd and an even base
    # top byte 255 ends the key array with an exact multiple of the iteration: no load may exist behind it
    assert bucket[255] % SC.ITER == 0 and bucket[255] > 0 and base[256] == len(keys)
    assert np.array_equal(np.sort(c["cands"]["prefix"]), np.sort(SC.prefixes(plants)))


@pytest.mark.parametrize("hits", SC.QUEUE)
def test_queue_unit_holds_the_hits(K, hits):
    texts, flags, plants = SC.queue(hits)
    c = CC.census(K, f"queue_{hits}", texts, flags)
    t = SC.head_byte(SC.QUEUE_HEAD)
    assert CC.buckets(c["keys"][1])[t] == hits <= CC.CO_CHUNK         # one unit, nothing in it but the hits
    assert _in_byte(c["hits"][1], t) == hits
    assert hits <= _in_byte(c["C"]["prefix"], t) <= CC.CO_TCAP       # one round: every hit meets its candidate in one table
    assert _in_byte(c["hits"][3], t) >= hits
    assert hits > CC.CO_HB                                           # (and the unit's hits overrun the hit buffer)
    assert np.array_equal(np.sort(c["cands"]["prefix"]), np.sort(SC.prefixes(plants)))
    assert c["row"] <= CC.COL_CAPM


def test_spread_outcomes_differ_between_the_genomes_of_a_call(K):
    texts, flags, plants = SC.spread()
    c = CC.census(K, "spread", texts, flags)
    Cp = c["C"]["prefix"]
    kept = SC.spread_kept(K)
    for kind, ps in plants.items():
        assert len(ps) == CC.SIDES_EACH
        assert CC.held(Cp, [p for p, _ in ps]).all()
        assert {g for _, g in ps} == {g for g in CC.coarse(flags) if flags[g] == (kind != "out_shows_in")}
    for p, g in plants["lacks"]:
        mate = [h for h in CC.coarse(flags) if flags[h] == flags[g] and h != g][0]
        assert not CC.held(c["keys"][g] & CC.PMASK, [p]).any() and CC.held(c["keys"][mate] & CC.PMASK, [p]).all()
    assert not any(kept["lacks"])
    # the deviating genome alone shows the other base: its side-mate and the pillar show their side's
    for kind in ("in_shows_out", "in_shows_third", "out_shows_in"):
        for p, g in plants[kind]:
            mate = [h for h in CC.coarse(flags) if flags[h] == flags[g] and h != g][0]
            bases = lambda h: set(((c["keys"][h][(c["keys"][h] & CC.PMASK) == np.uint64(p)]) >> np.uint64(CC.DIAG_SHIFT)) & np.uint64(3))
            assert len(bases(g)) == 1 and len(bases(mate)) == 1 and bases(g) != bases(mate)
    assert any(any(v) for v in kept.values()) and not all(all(v) for v in kept.values())
    print("spread:", kept)
