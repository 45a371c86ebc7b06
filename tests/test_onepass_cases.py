"""The census of tests/onepass_cases.py without a GPU: with oracle/kmer_oracle alone, each case forces the branch of "one test,
one pass" (krisp_amd/csrc/co_pass.inc) it is named for.  tests/test_gpu_coarse_onepass.py relies on this."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import onepass_cases as OP                                                  # noqa: E402
import strand_cases as S                                                    # noqa: E402

L, R = OP.L, OP.R


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


def _m():
    """M, base by base: the key's bits without window position L (the key's last base) and window position R"""
    m = 0
    for j in range(L + R + 1):
        if j != R and j != L + R:
            m |= 3 << (62 - 2 * j)
    return m


def _holds(keys, key):
    return int(np.count_nonzero(keys == np.uint64(key)))


def test_siblings_share_key_and_m(K):
    texts, flags, plants = OP.siblings()
    c = S.census(K, "op_siblings", texts, flags, OP.LDR)
    final = c["cands"]["prefix"]
    M = _m()
    fwd = {g: S.forward_keys(texts[g], L, R)[0] for g in (OP.CIN, OP.COUT)}
    for kind, n, as_rc in (("fwd4", 4, False), ("rev3", 3, True), ("fwd3", 3, False)):
        group = plants[kind]
        assert len(group) == n
        pre = [S.prefix_of(wi, L, R) for wi, _ in group]
        assert len(set(pre)) == n and CC.held(final, pre).all(), kind
        # the candidates differ at window position R only
        assert len({p & ~(3 << (62 - 2 * R)) for p in pre}) == 1
        # what the coarse genomes hold: forward windows with ONE key & M, each under exactly one entry of the group
        for g, side in ((OP.CIN, 0), (OP.COUT, 1)):
            held = [S.key_of(S.rc(ws[side]) if as_rc else ws[side], L, R) for ws in group]
            assert all(_holds(fwd[g], k) == 1 for k in held), (kind, g)
            assert len({k & M for k in held}) == 1
            if as_rc:
                # ... windows that differ at THEIR position L only: the reverse entries' patterns differ there only
                assert len({k & ~(3 << (62 - 2 * (L + R))) for k in held}) == 1 and len(set(held)) == n
    # the windows that share key & M with a group and lie under no candidate
    for lone, kind, as_rc in ((plants["lone"], "rev3", True), (plants["lone_f"], "fwd3", False)):
        key = S.key_of(S.rc(lone) if as_rc else lone, L, R)
        mate = S.key_of(S.rc(plants[kind][0][0]) if as_rc else plants[kind][0][0], L, R)
        assert _holds(fwd[OP.CIN], key) == 1 and key & M == mate & M and key != mate
        assert not CC.held(c["C"]["prefix"], [S.prefix_of(lone, L, R)]).any()
        assert _holds(c["hits"][OP.CIN], S.key_of(lone, L, R)) == 0
    print("siblings: |C| =", len(c["C"]), "final", len(final))


def test_uneven_digits(K):
    texts, flags, plan = OP.uneven()
    c = S.census(K, "op_uneven", texts, flags, OP.LDR)
    f, r = S.classes(c["C"], OP.LDR)
    nsites = sum(nf + nr for nf, nr in plan.values())
    assert len(c["C"]) == len(c["cands"]) == 2 * nsites             # (a site's two candidates: strand_cases.sparse)
    for d, (nf, nr) in plan.items():
        assert (int(f[d]), int(r[d])) == (nf, nr), (hex(d), f[d], r[d])
    assert f[OP.UNEVEN_F] > 0 and r[OP.UNEVEN_F] == 0 and f[OP.UNEVEN_R] == 0 and r[OP.UNEVEN_R] > 0
    for g in (OP.CIN, OP.COUT):
        have = np.bincount(S.forward_keys(texts[g], L, R)[1], minlength=256) > 0
        assert have.all()
    for tcap, (d, nf, nr) in OP.UNEVEN_X.items():
        assert (-(-nf // tcap), -(-nr // tcap)) == (3, 1)
        rf, rr, np1 = OP.passes(c, texts, flags, tcap, 1)
        assert OP.passes(c, texts, flags, tcap, 0)[2] == rf + rr and np1 < rf + rr
    # both readings hit: records of the coarse genomes that are forward records of their text, and records that are not
    fk = S.forward_keys(texts[OP.CIN], L, R)[0]
    mine = c["recs"][c["recs"]["genome"] == OP.CIN]["key"]
    assert 0 < np.count_nonzero(np.isin(mine, fk)) < len(mine)


def test_full_table_and_a_second_pass(K):
    texts, flags = OP.full()
    c = S.census(K, "op_full", texts, flags, OP.LDR)
    f, r = S.classes(c["C"], OP.LDR)
    d = OP.FULL_DIGIT
    assert OP.TCAP < f[d] <= 2 * OP.TCAP and OP.TCAP < r[d] <= 2 * OP.TCAP, (f[d], r[d])
    # the first pass of the digit: 6144 forward and 6144 reverse entries in 16 384 slots; the second: the rest of both
    assert (-(-int(f[d]) // OP.TCAP), -(-int(r[d]) // OP.TCAP)) == (2, 2)
    rf, rr, np1 = OP.passes(c, texts, flags)
    assert np1 < rf + rr == OP.passes(c, texts, flags, one_pass=0)[2]
    assert len(c["cands"]) > OP.TCAP and int(np.max(c["recs"]["count"])) <= CC.COL_CAPM
    print("full: classes of digit 0:", f[d], r[d], "final", len(c["cands"]))


@pytest.mark.parametrize("hits", OP.QUEUE)
def test_queue_holds_hits_of_both_readings(K, hits):
    texts, flags, plants = OP.queue(hits)
    c = S.census(K, f"op_queue_{hits}", texts, flags, OP.LDR)
    keys, dig = S.forward_keys(texts[OP.CIN], L, R)
    assert len(keys) == hits and (dig == OP.QUEUE_DIGIT).all()       # one unit of `hits` keys
    pre = np.array([S.prefix_of(wi, L, R) for wi, _ in plants], dtype=np.uint64)
    assert len(np.unique(pre)) == hits and CC.held(c["cands"]["prefix"], pre).all()
    pm = np.uint64(S.pmask(L, R))
    as_fwd = np.isin(keys & pm, pre)
    assert np.count_nonzero(as_fwd) == (hits + 1) // 2               # the even plants; the odd ones are met by the reverse reading
    rev = np.array([S.key_of(S.rc(OP.window_of(k)), L, R) for k in keys[~as_fwd]], dtype=np.uint64)
    assert np.isin(rev & pm, pre).all()
    f, r = S.classes(c["C"], OP.LDR)
    assert f[OP.QUEUE_DIGIT] >= hits and r[OP.QUEUE_DIGIT] >= hits and f[OP.QUEUE_DIGIT] + r[OP.QUEUE_DIGIT] <= 2 * OP.TCAP
