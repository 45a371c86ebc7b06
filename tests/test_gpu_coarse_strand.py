"""The one-strand form of the coarse route (KR_OPT_COARSE_ONE_STRAND): a coarse genome's pass 1 writes the forward
record of every window only, in buckets by a digit both of the window's records share, and k_coarse_probe asks each key both
ways (krisp_amd/csrc/co_strand.inc).  The cases are strand_cases.py's, whose census test_strand_cases.py takes on the host.

The rule of every test: the candidates (prefix, in_mask, out_mask) in order, kr_collect's records sorted by (key, genome) and
count(g) are equal to oracle/kmer_oracle.c and BIT-IDENTICAL to the same engine with the option at 0; and the option's counters
(debug_coarse_strand) say which route ran: partitions that wrote one strand, calls that probed them, forward / reverse rounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import strand_cases as S                                                    # noqa: E402

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


@pytest.fixture(scope="module")
def D():
    from krisp_amd import distributed
    return distributed


def _knobs(monkeypatch, grid=None, tcap=None, hitcap=None):
    for name, v in (("KR_COARSE_GRID", grid), ("KR_COARSE_TCAP", tcap), ("KR_COARSE_HITCAP", hitcap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    monkeypatch.delenv("KR_COARSE_ONE_STRAND", raising=False)


def _run(N, D, texts, flags, ldr, one, steps=1, lanes=None, keys_of=(), apply_filter=True, by_hand=None):
    """one engine with KR_OPT_COARSE_ONE_STRAND = `one`: `steps` sharded steps (or by_hand(e): partition / sort in its own
    way, then intersect + collect here) -> everything compared"""
    out = dict(cands=[], recs=[])
    ids = list(range(len(texts)))
    with N.Engine() as e:
        e.set_option(N.OPT_COARSE_ONE_STRAND, one)
        if lanes is not None:
            e.set_option(N.OPT_LANES, lanes)
        e.set_params(*ldr, max_bases=max(len(t) for t in texts))
        for g, t in zip(ids, texts):
            e.upload(g, t)
        assert e.debug_info()["b"] > 8
        for _ in range(steps):
            if by_hand is None:
                n, nrec = D.sharded_step(e, ids, flags, 1, apply_filter=apply_filter)
                recs = e.fetch_records(nrec)
            else:
                by_hand(e)
                n = e.intersect(ids, flags, apply_filter=apply_filter)
                recs = e.collect(ids)
            out["cands"].append(e.cands().copy())
            out["recs"].append(np.sort(recs, order=["key", "genome"]))
            assert n == len(out["cands"][-1])
        out["strand"] = e.debug_coarse_strand()
        out["counts"] = [e.count(g) for g in ids]
        out["lazy"] = e.debug_lazy()
        out["keys"] = {g: e.keys(g) for g in keys_of}
        out["lazy_after_keys"] = e.debug_lazy()
    return out


def _check(on, off, c):
    """the two settings against each other and against the oracle's census"""
    assert len(on["cands"]) == len(off["cands"])
    for x, y in zip(on["cands"] + on["recs"], off["cands"] + off["recs"]):
        assert np.array_equal(x, y), "KR_OPT_COARSE_ONE_STRAND = 1 and 0 differ"
    assert on["counts"] == off["counts"] == [len(k) for k in c["keys"]]
    for x in on["cands"]:
        assert len(x) == len(c["cands"])
        for f in ("prefix", "in_mask", "out_mask"):
            assert np.array_equal(x[f], c["cands"][f]), f
    for r in on["recs"]:
        assert np.array_equal(r, c["recs"])
    for g, k in on["keys"].items():
        assert np.array_equal(k, c["keys"][g]) and np.array_equal(off["keys"][g], c["keys"][g])
    assert (off["strand"]["partitions"], off["strand"]["calls"], off["strand"]["on"]) == (0, 0, 0)


def _rounds(c, texts, flags, ldr, tcap=CC.CO_TCAP):
    """the forward and reverse rounds of one call, from the census: per digit in which a coarse genome has a key, the tables
    its candidates of each reading take"""
    L, _, R = ldr
    f, r = S.classes(c["C"], ldr)
    have = np.zeros(256, dtype=bool)
    for g in CC.coarse(flags):
        have |= np.bincount(S.forward_keys(texts[g], L, R)[1], minlength=256) > 0
    return int(np.sum(-(-f[have] // tcap))), int(np.sum(-(-r[have] // tcap)))


def _ab(N, D, K, name, texts, flags, ldr, steps=1, tcap=CC.CO_TCAP, promoted=0, **kw):
    """-> the run with the option on, held to the other and to the oracle; the route and its rounds asserted"""
    c = S.census(K, name, texts, flags, ldr)
    on = _run(N, D, texts, flags, ldr, 1, steps=steps, **kw)
    off = _run(N, D, texts, flags, ldr, 0, steps=steps, **kw)
    _check(on, off, c)
    ncoarse = len(CC.coarse(flags))
    st = on["strand"]
    assert st["on"] == 1 and st["partitions"] == ncoarse * steps, st
    assert on["lazy"]["coarse_promoted"] == off["lazy"]["coarse_promoted"] == promoted, on["lazy"]
    if promoted == 0:
        rf, rr = _rounds(c, texts, flags, ldr, tcap)
        assert (st["calls"], st["last_forward"], st["last_reverse"]) == (steps, rf, rr), (st, rf, rr)
        assert (st["rounds_forward"], st["rounds_reverse"]) == (steps * rf, steps * rr)
        assert rf > 0 and rr > 0
        assert on["lazy"]["coarse"] == off["lazy"]["coarse"] == ncoarse * steps
    return on, c


# ----------------------------------------------------------------------------
# uniform families
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("R", (6,) + S.OTHER_R)
def test_uniform(N, D, K, monkeypatch, R):
    """300 kbp at (20, 1, R): R = 6 and 4 take the plain top byte for the digit, R = 0, 1, 3 a digit around position R"""
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    on, c = _ab(N, D, K, f"uniform_{R}", texts, flags, (20, 1, R), keys_of=(1,) if R == 6 else ())
    if R == 6:
        # fetching the keys of a one-strand genome sorted it fine, both strands
        assert on["lazy_after_keys"]["coarse_promoted"] == 1


@pytest.mark.parametrize("lanes", [1, 3])
def test_three_steps(N, D, K, monkeypatch, lanes):
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    on, _ = _ab(N, D, K, "uniform_6", texts, flags, S.UNIFORM_LDR, steps=3, lanes=lanes)
    for x, r in zip(on["cands"][1:], on["recs"][1:]):
        assert np.array_equal(x, on["cands"][0]) and np.array_equal(r, on["recs"][0])


# ----------------------------------------------------------------------------
# planted windows
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [None, 1, 3, 7])
def test_planted(N, D, K, monkeypatch, grid):
    """every kind of strand_cases.planted(): the candidate stays, and the coarse genomes' records under it are the oracle's --
    found by the forward reading, by the reverse reading, by both, twice for the palindrome, next to N and record ends"""
    _knobs(monkeypatch, grid=grid)
    texts, flags, plants = S.planted()
    on, c = _ab(N, D, K, "planted", texts, flags, S.PLANT_LDR)
    L, _, R = S.PLANT_LDR
    got = on["cands"][0]["prefix"]
    want = [S.prefix_of(plants[k][0], L, R) for k in S.KINDS] + [S.prefix_of(w, L, R) for w in plants["two"]]
    assert CC.held(got, want).all()
    recs = on["recs"][0]
    mine = recs[recs["genome"] == S.CIN]
    for kind, n in (("fwd", 1), ("rev", 1), ("both", 2), ("palin", 2)):
        assert int(mine[mine["key"] == np.uint64(S.key_of(plants[kind][0], L, R))]["count"][0]) == n, kind


@pytest.mark.parametrize("tcap", [1, 10, 50])
def test_planted_small_tables(N, D, K, monkeypatch, tcap):
    """KR_COARSE_TCAP = 1: every candidate a round of its own, several rounds of each reading in every digit; 10: classes of
    about 14 candidates take a full table and a rest; 50: one table per class, the table still changes in the middle of a
    digit -- from its forward to its reverse round.  The round counts are held to the census in every case (_ab)"""
    _knobs(monkeypatch, tcap=tcap, grid=3 if tcap != 1 else None)
    texts, flags, _ = S.planted()
    c = S.census(K, "planted", texts, flags, S.PLANT_LDR)
    f, r = S.classes(c["C"], S.PLANT_LDR)
    if tcap == 10:
        assert np.count_nonzero(f > tcap) > 100 and np.count_nonzero(r > tcap) > 100
    assert np.count_nonzero((f > 0) & (r > 0)) > 200
    _ab(N, D, K, "planted", texts, flags, S.PLANT_LDR, tcap=tcap)


@pytest.mark.parametrize("below", [0, 1])
def test_hit_list_at_its_capacity(N, D, K, monkeypatch, below):
    """KR_COARSE_HITCAP = the longest hit list: it fits; one below: the call promotes and the result stands"""
    texts, flags, _ = S.planted()
    c = S.census(K, "planted", texts, flags, S.PLANT_LDR)
    _knobs(monkeypatch, hitcap=max(len(h) for h in c["hits"].values()) - below)
    _ab(N, D, K, "planted", texts, flags, S.PLANT_LDR, promoted=2 * below)


def test_sparse_digits_of_one_reading(N, D, K, monkeypatch):
    _knobs(monkeypatch)
    texts, flags = S.sparse()
    on, c = _ab(N, D, K, "sparse", texts, flags, S.PLANT_LDR)
    assert len(on["cands"][0]) == 2 * S.SPARSE_SITES


@pytest.mark.parametrize("grid", [None, 3])
def test_gfree_digits_without_keys(N, D, K, monkeypatch, grid):
    _knobs(monkeypatch, grid=grid)
    texts, flags = S.gfree()
    _ab(N, D, K, "gfree", texts, flags, S.PLANT_LDR)


# ----------------------------------------------------------------------------
# routes not taken
# ----------------------------------------------------------------------------
def _plain(N, D, K, name, texts, flags, ldr, partitions, promoted, **kw):
    c = S.census(K, name, texts, flags, ldr) if kw.get("apply_filter", True) else None
    on = _run(N, D, texts, flags, ldr, 1, **kw)
    off = _run(N, D, texts, flags, ldr, 0, **kw)
    for x, y in zip(on["cands"] + on["recs"], off["cands"] + off["recs"]):
        assert np.array_equal(x, y)
    assert on["counts"] == off["counts"]
    if c is not None:
        _check(on, off, c)
    st = on["strand"]
    assert (st["partitions"], st["calls"]) == (partitions, 0), st
    assert on["lazy"]["coarse_promoted"] == promoted, on["lazy"]
    return on


def test_two_diagnostic_columns_partition_both_strands(N, D, K, monkeypatch):
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    hand = lambda e: [(e.partition if g in (1, 3) else e.sort)(g) for g in range(4)]       # noqa: E731
    _plain(N, D, K, "uniform_25_2_2", texts, flags, (25, 2, 2), 0, 2, by_hand=hand)


def test_without_filter_promotes(N, D, K, monkeypatch):
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    hand = lambda e: [(e.partition if g in (1, 3) else e.sort)(g) for g in range(4)]       # noqa: E731
    on = _plain(N, D, K, "uniform_nofilter", texts, flags, S.UNIFORM_LDR, 2, 2, by_hand=hand, apply_filter=False)
    keys = [K.sorted_keys(t.tobytes(), *S.UNIFORM_LDR) for t in texts]
    assert on["counts"] == [len(k) for k in keys]
    assert np.array_equal(on["cands"][0]["prefix"], K.intersect(keys, flags, *S.UNIFORM_LDR, apply_filter=False)["prefix"])


def test_single_strand_context_sorts(N, monkeypatch):
    """forward-only keys: kr_genome_partition is the full sort, nothing is written in the one-strand form"""
    _knobs(monkeypatch)
    texts, _ = S.uniform()
    got = []
    for one in (1, 0):
        with N.Engine() as e:
            e.set_option(N.OPT_COARSE_ONE_STRAND, one)
            e.set_params(*S.UNIFORM_LDR, max_bases=len(texts[1]))
            e.set_strands(N.STRANDS_FORWARD)
            e.upload(1, texts[1])
            e.partition(1)
            got.append(e.keys(1))
            st, lazy = e.debug_coarse_strand(), e.debug_lazy()
            assert (st["partitions"], st["calls"], lazy["coarse_promoted"]) == (0, 0, 0)
    fk = np.sort(S.forward_keys(texts[1], S.UNIFORM_LDR[0], S.UNIFORM_LDR[2])[0])
    assert np.array_equal(got[0], fk) and np.array_equal(got[1], fk)


@pytest.mark.parametrize("first", [1, 0])
def test_genomes_of_both_forms_in_one_call_promote(N, D, K, monkeypatch, first):
    """genome 1 partitioned under one setting, genome 3 under the other: the call sorts both fine"""
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    c = S.census(K, "uniform_6", texts, flags, S.UNIFORM_LDR)

    def hand(e):
        e.set_option(N.OPT_COARSE_ONE_STRAND, first)
        e.sort(0)
        e.partition(1)
        e.sort(2)
        e.set_option(N.OPT_COARSE_ONE_STRAND, 1 - first)
        e.partition(3)

    on = _run(N, D, texts, flags, S.UNIFORM_LDR, 1, by_hand=hand)
    for f in ("prefix", "in_mask", "out_mask"):
        assert np.array_equal(on["cands"][0][f], c["cands"][f])
    assert np.array_equal(on["recs"][0], c["recs"]) and on["counts"] == [len(k) for k in c["keys"]]
    assert (on["strand"]["partitions"], on["strand"]["calls"]) == (1, 0)
    assert (on["lazy"]["coarse"], on["lazy"]["coarse_promoted"]) == (0, 2)
