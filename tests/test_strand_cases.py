"""The census of tests/strand_cases.py without a GPU: with oracle/kmer_oracle alone, each case forces the branch of the
one-strand form (krisp_amd/csrc/co_strand.inc) it is named for.  tests/test_gpu_coarse_strand.py relies on this:
which reading finds a record is shown here by where the record's window stands in the coarse genome's text."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import strand_cases as S                                                    # noqa: E402


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def test_restated_keys_agree_with_the_oracle(K):
    """forward_keys + the reverse complement's keys = the oracle's keys, at every geometry the device tests run"""
    rng = np.random.default_rng(9)
    for L, R in [(25, 2), (20, 6), (20, 0), (20, 1), (20, 3), (20, 4)]:
        k = L + 1 + R
        text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=400)].copy()
        text[100] = ord("N")
        text[250] = 10
        fk, dig = S.forward_keys(text, L, R)
        rev = []
        for i in range(len(text) - k + 1):
            w = text[i:i + k]
            if all(ch in b"ACGT" for ch in w.tobytes()):
                codes = np.array([b"ACGT".index(ch) for ch in w.tobytes()], dtype=np.uint8)
                assert S.digit_of(codes, R) in dig
                rev.append(S.key_of(S.rc(codes), L, R))
        both = np.sort(np.concatenate([fk, np.array(rev, dtype=np.uint64)]))
        assert np.array_equal(both, K.sorted_keys(text.tobytes(), L, 1, R))


def test_classes_by_hand():
    L, R = 25, 2
    rng = np.random.default_rng(3)
    for _ in range(50):
        w = rng.integers(0, 4, size=L + 1 + R, dtype=np.uint8)
        d = S.digit_of(w, R)
        assert d == (int(w[0]) << 6 | int(w[1]) << 4 | int(w[3]) << 2 | int(w[4]))
        assert S.class_fwd(S.prefix_of(w, L, R), L, R) == d
        assert S.class_rev(S.prefix_of(S.rc(w), L, R), L, R) == d


def _holds(keys, key):
    return int(np.count_nonzero(keys == np.uint64(key)))


def test_planted_windows_force_their_readings(K):
    texts, flags, plants = S.planted()
    L, D, R = S.PLANT_LDR
    k = L + D + R
    assert all(len(t) == S.PLANT_LEN + CC.RECORDS - 1 for t in texts)
    c = S.census(K, "planted", texts, flags, S.PLANT_LDR)
    Cp, final = c["C"]["prefix"], c["cands"]["prefix"]
    fwd = {g: S.forward_keys(texts[g], L, R)[0] for g in (S.CIN, S.COUT)}
    for kind in S.KINDS:
        wi, wo = plants[kind]
        P = S.prefix_of(wi, L, R)
        assert P == S.prefix_of(wo, L, R) and wi[L] != wo[L]
        assert CC.held(Cp, [P]).all() and CC.held(final, [P]).all(), kind
        for g, w in ((S.CIN, wi), (S.COUT, wo)):
            key = S.key_of(w, L, R)
            as_fwd = _holds(fwd[g], key)                                 # windows whose FORWARD record is the key
            as_rev = _holds(fwd[g], S.key_of(S.rc(w), L, R))             # windows whose REVERSE record is the key
            total = _holds(c["keys"][g], key)
            assert total == as_fwd + as_rev
            if kind in ("fwd", "nrun", "recend_a", "recend_b"):
                assert (as_fwd, as_rev) == (1, 0), (kind, g)
            elif kind == "rev" or kind.startswith("base"):
                assert (as_fwd, as_rev) == (0, 1), (kind, g)
            elif kind == "both":
                assert (as_fwd, as_rev) == (1, 1), (kind, g)
            elif kind == "palin" and g == S.CIN:
                assert np.array_equal(w, S.rc(w)) and (as_fwd, as_rev) == (1, 1) and total == 2      # one window, both records
        if kind.startswith("base"):
            assert int(wi[L]) == int(kind[-1])                           # (the base the ingroup's reverse record shows)
    got = c["cands"][np.isin(final, [S.prefix_of(plants[f"base{b}"][0], L, R) for b in range(4)])]
    assert sorted(got["in_mask"]) == [1, 2, 4, 8]
    # N runs: the windows around the planted one are no keys of the coarse genomes
    wi, _ = plants["nrun"]
    p = bytes(texts[S.CIN]).find(bytes(b"ACGT"[b] for b in wi))
    assert p > 0 and texts[S.CIN][p - 1] == ord("N") and texts[S.CIN][p + k] == ord("N")
    assert texts[S.PIN][p - 1] != ord("N")
    # record ends
    rl = (S.PLANT_LEN + CC.RECORDS - 1) // CC.RECORDS
    for kind, at in (("recend_a", rl - k), ("recend_b", rl + 1)):
        w = plants[kind][0]
        assert bytes(texts[S.CIN][at:at + k]) == bytes(b"ACGT"[b] for b in w), kind
    assert texts[S.CIN][rl] == 10
    # one window, two candidates
    V, U = plants["two"]
    P1, P2 = S.prefix_of(V, L, R), S.prefix_of(U, L, R)
    assert P1 != P2 and CC.held(final, [P1, P2]).all()
    assert _holds(fwd[S.CIN], S.key_of(V, L, R)) == 1 and _holds(fwd[S.CIN], S.key_of(U, L, R)) == 0
    assert _holds(c["keys"][S.CIN], S.key_of(V, L, R)) == 1 and _holds(c["keys"][S.CIN], S.key_of(U, L, R)) == 1
    assert int(np.max(c["recs"]["count"])) <= CC.COL_CAPM
    print("planted: |C| =", len(Cp), "final", len(final), "longest hit list", max(len(h) for h in c["hits"].values()))


def test_sparse_has_digits_of_one_reading(K):
    """digits whose candidates are all of one reading, in buckets that hold keys: no round of the other reading there"""
    texts, flags = S.sparse()
    L, _, R = S.PLANT_LDR
    c = S.census(K, "sparse", texts, flags, S.PLANT_LDR)
    assert len(c["C"]) == len(c["cands"]) == 2 * S.SPARSE_SITES
    f, r = S.classes(c["C"], S.PLANT_LDR)
    for g in (S.CIN, S.COUT):
        have = np.bincount(S.forward_keys(texts[g], L, R)[1], minlength=256) > 0
        assert np.any((f > 0) & (r == 0) & have) and np.any((f == 0) & (r > 0) & have)
    assert f.sum() == r.sum() == len(c["C"])
    # what the device's round counter shows at the default table size: one round per class with candidates
    print("sparse: forward rounds", np.count_nonzero(f), "reverse rounds", np.count_nonzero(r))


def test_gfree_has_digits_without_keys(K):
    texts, flags = S.gfree()
    L, _, R = S.PLANT_LDR
    assert not any(b"G" in bytes(t) for t in texts)
    c = S.census(K, "gfree", texts, flags, S.PLANT_LDR)
    f, r = S.classes(c["C"], S.PLANT_LDR)
    lost = 0
    for g in (S.CIN, S.COUT):
        keys, dig = S.forward_keys(texts[g], L, R)
        have = np.bincount(dig, minlength=256) > 0
        assert np.count_nonzero(have) == 81                              # (the digits over A, C, T)
        assert np.any((f > 0) & ~have) and np.any((r > 0) & ~have)
        # candidates in forward classes without keys that the genome does hold -- through reverse records
        pm = np.uint64(S.pmask(L, R))
        pre = c["hits"][g] & pm
        cls = np.array([S.class_fwd(p, L, R) for p in np.unique(pre)])
        lost += int(np.count_nonzero(~have[cls]))
    assert lost > 50 and len(c["cands"]) > 50
    print("gfree: |C| =", len(c["C"]), "final", len(c["cands"]), "held through classes without keys", lost)


@pytest.mark.parametrize("R", (6,) + S.OTHER_R)
def test_uniform_keeps_candidates(K, R):
    texts, flags = S.uniform()
    ldr = (20, 1, R)
    c = S.census(K, f"uniform_{R}", texts, flags, ldr)
    f, r = S.classes(c["C"], ldr)
    assert len(c["cands"]) > 20 and f.sum() == r.sum() == len(c["C"])
    assert int(np.max(c["recs"]["count"])) <= CC.COL_CAPM
    print(f"uniform R {R}: |C| = {len(c['C'])} final {len(c['cands'])} classes with candidates {np.count_nonzero(f)} / {np.count_nonzero(r)}")
