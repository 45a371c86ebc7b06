"""The census of tests/coarse_cases.py without a GPU: with oracle/kmer_oracle alone, each case has the shape that makes
k_coarse_probe take the branch the case is named for.  tests/test_gpu_coarse_shapes.py relies on these counts:
the probe has no counters of its own, so that a branch ran is shown by counting what the kernel cannot avoid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _in_byte(prefixes, t):
    return int(np.count_nonzero((prefixes >> np.uint64(56)) == np.uint64(t)))


def test_skew_crowds_two_buckets(K):
    texts, flags = CC.skew()
    assert all(len(t) <= 600_000 + CC.RECORDS for t in texts)
    c = CC.census(K, "skew", texts, flags)
    parities, units = set(), 0
    for g in CC.coarse(flags):
        bucket = CC.buckets(c["keys"][g])
        base = np.concatenate([[0], np.cumsum(bucket)])
        crowded = [t for t in range(256) if bucket[t] > 2 * CC.CO_CHUNK]             # three chunks or more
        assert crowded
        for t in crowded:
            assert bucket[t] % CC.CO_CHUNK != 0                                      # (the last chunk is partial)
            assert _in_byte(c["C"]["prefix"], t) >= 100
            parities.add(int(base[t]) & 1)
        units = sum(-(-int(bucket[t]) // CC.CO_CHUNK) for t in range(256) if _in_byte(c["C"]["prefix"], t))
        assert units >= sum(1 for t in range(256) if _in_byte(c["C"]["prefix"], t)) + 2 * len(crowded)
    # a unit starts at the bucket's base + a multiple of CO_CHUNK: its first 16-byte load is aligned for an even base and
    # reads one key of the bucket in front for an odd one
    assert parities == {0, 1}
    assert c["row"] <= CC.COL_CAPM and len(c["cands"]) > 100
    print("skew: |C| =", len(c["C"]), "final", len(c["cands"]), "units", units, "row", c["row"])


@pytest.mark.parametrize("head,blocks", CC.DENSE)
def test_dense_fills_one_bucket_with_hits(K, head, blocks):
    texts, flags = CC.dense(head, blocks)
    c = CC.census(K, f"dense_{head}_{blocks}", texts, flags)
    t = {"AAAA": 0, "TTTT": 255}[head]
    nc = _in_byte(c["C"]["prefix"], t)
    for g in CC.coarse(flags):
        bucket = int(CC.buckets(c["keys"][g])[t])
        hits = _in_byte(c["hits"][g], t)
        print(f"dense {head} {blocks}: genome {g} bucket {bucket} hits {hits} candidates in the byte {nc} row {c['row']}")
        if blocks == 4000:
            # at most 8192 - 1025 keys of the bucket are no hits: whatever order pass 1 leaves, the first iteration (8192 keys)
            # holds more than CO_QCAP keys that pass the prefilter, and the unit more than CO_HB hits
            assert bucket >= CC.CO_ITER and bucket <= CC.CO_CHUNK
            assert bucket - hits <= CC.CO_ITER - (CC.CO_QCAP + 1)
            assert CC.CO_QCAP == CC.CO_HB
        else:
            assert nc > CC.CO_TCAP and bucket > CC.CO_ITER                          # (two rounds, two iterations)
        assert hits < nc                                                             # (a candidate this genome lacks)
    assert 0 < c["row"] <= CC.COL_CAPM


@pytest.mark.parametrize("copies", CC.ROWS)
def test_rows_hold_the_copies(K, copies):
    texts, flags = CC.rows(copies)
    c = CC.census(K, f"rows_{copies}", texts, flags)
    assert c["row"] == copies
    top = c["recs"][c["recs"]["count"] == copies]
    assert set(top["genome"]) == set(CC.coarse(flags))
    # every genome's records of the final list are the same whatever the copies: only the multiplicities differ
    if copies != CC.ROWS[0]:
        first = CC.census(K, f"rows_{CC.ROWS[0]}", *CC.rows(CC.ROWS[0]))
        assert np.array_equal(first["cands"], c["cands"])
        assert np.array_equal(first["recs"]["key"], c["recs"]["key"])


def test_collide_pairs_share_hash_and_top_byte(K):
    texts, flags, plants = CC.collide()
    c = CC.census(K, "collide", texts, flags)
    final, C = c["cands"]["prefix"], c["C"]["prefix"]
    for kind, pairs in plants.items():
        assert len(pairs) >= 8
        p = np.array([a for a, _ in pairs], dtype=np.uint64)
        q = np.array([b for _, b in pairs], dtype=np.uint64)
        assert np.all(p != q) and np.all((p & ~CC.PMASK) == 0) and np.all((q & ~CC.PMASK) == 0)
        assert np.array_equal(CC.co_hash(p), CC.co_hash(q))                         # same first slot, tag and prefilter bit
        assert np.array_equal(p >> np.uint64(56), q >> np.uint64(56))                # same table
        assert CC.held(C, p).all()
        if kind == "both":
            assert CC.held(C, q).all() and CC.held(final, p).all() and CC.held(final, q).all()
        else:
            assert not CC.held(C, q).any()
            for g in CC.coarse(flags):                                               # (the probe meets P' among the genome's keys)
                assert CC.held(c["keys"][g] & CC.PMASK, q).all()
        if kind == "lacked":
            assert not CC.held(final, p).any()
        if kind == "alone":
            assert CC.held(final, p).all()
            got = c["cands"][np.isin(final, p)]
            assert np.all(got["in_mask"] == 1) and np.all(got["out_mask"] == 2)      # (A in, C out: nothing of P')
    assert not CC.held(c["recs"]["key"] & CC.PMASK, [q for _, q in plants["alone"]]).any()
    assert c["row"] <= CC.COL_CAPM


def test_co_hash_by_hand():
    # (hi ^ lo * 0x9E3779B1) * 0x85EBCA6B in 32 bits
    assert int(CC.co_hash(0)) == 0
    assert int(CC.co_hash(1 << 32)) == 0x85EBCA6B
    assert int(CC.co_hash(0x400)) == ((0x400 * 0x9E3779B1 & 0xFFFFFFFF) * 0x85EBCA6B) & 0xFFFFFFFF
    assert int(CC.co_hash(0xFFFFFFFF_FFFFFC00)) == (((0xFFFFFFFF ^ (0xFFFFFC00 * 0x9E3779B1 & 0xFFFFFFFF)) * 0x85EBCA6B) & 0xFFFFFFFF)


def test_window_and_key_agree_with_the_oracle(K):
    rng = np.random.default_rng(5)
    for _ in range(8):
        key = (int(rng.integers(0, 1 << 56, dtype=np.uint64)) << 8)
        w = CC.window(key)
        assert CC.key_of(w) == key
        left, diag, right = K.key_to_columns(key, *CC.LDR)
        assert "".join("ACGT"[b] for b in w) == left + diag + right
        text = np.frombuffer(("".join("ACGT"[b] for b in w)).encode(), dtype=np.uint8)
        assert key in [int(k) for k in K.sorted_keys(text.tobytes(), *CC.LDR)]


@pytest.mark.parametrize("n", CC.MANY)
def test_many_genomes_keep_candidates(K, n):
    texts, flags = CC.many(n)
    assert len(texts) == n <= 25 and sum(flags) == n // 2 and flags[0] and not flags[-1]
    assert len(CC.coarse(flags)) == n - 2
    c = CC.census(K, f"many_{n}", texts, flags)
    assert len(c["cands"]) > 0 and c["row"] <= CC.COL_CAPM
    print(f"many {n}: final {len(c['cands'])}")


def test_sides_are_candidates_of_the_pillars(K):
    texts, flags, plants = CC.sides()
    c = CC.census(K, "sides", texts, flags)
    for kind in CC.SIDES_KINDS:
        assert len(plants[kind]) >= 4
        assert CC.held(c["C"]["prefix"], plants[kind]).all(), kind
    kept = CC.sides_kept(K)
    print("sides, kept by the oracle:", kept)
    # recorded, not prescribed -- but the kinds must not all end alike, or the case tells nothing
    flat = [k for v in kept.values() for k in v]
    assert any(flat) and not all(flat)
    assert c["row"] <= CC.COL_CAPM
