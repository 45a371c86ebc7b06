"""One test per key, one pass per pair of rounds (DESIGN §10b "One test, one pass", KR_OPT_COARSE_ONE_PASS): k_coarse_probe<1>
tests each key of a one-strand genome once for both readings and streams a bucket past the forward AND the reverse candidates of
its digit in one pass (krisp_amd/csrc/co_pass.inc).  The cases are onepass_cases.py's and strand_cases.py's, whose census
test_onepass_cases.py / test_strand_cases.py take on the host.

The rule of every test: the candidates (prefix, in_mask, out_mask) in order, kr_collect's records sorted by (key, genome) and
count(g) are equal to oracle/kmer_oracle.c and BIT-IDENTICAL to the same engine with KR_OPT_COARSE_ONE_PASS = 0 and with
KR_OPT_COARSE_ONE_STRAND = 0; the forward / reverse rounds and the passes of the call (debug_coarse_strand) are the census's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cases as CC                                                   # noqa: E402
import coarse_stream_cases as SC                                            # noqa: E402
import onepass_cases as OP                                                  # noqa: E402
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


def _knobs(monkeypatch, grid=None, tcap=None):
    for name, v in (("KR_COARSE_GRID", grid), ("KR_COARSE_TCAP", tcap), ("KR_COARSE_HITCAP", None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    monkeypatch.delenv("KR_COARSE_ONE_STRAND", raising=False)
    monkeypatch.delenv("KR_COARSE_ONE_PASS", raising=False)


def _run(N, D, texts, flags, ldr, one_strand, one_pass, steps=1, lanes=None):
    out = dict(cands=[], recs=[], passes=[])
    ids = list(range(len(texts)))
    with N.Engine() as e:
        e.set_option(N.OPT_COARSE_ONE_STRAND, one_strand)
        e.set_option(N.OPT_COARSE_ONE_PASS, one_pass)
        if lanes is not None:
            e.set_option(N.OPT_LANES, lanes)
        e.set_params(*ldr, max_bases=max(len(t) for t in texts))
        for g, t in zip(ids, texts):
            e.upload(g, t)
        assert e.debug_info()["b"] > 8
        for _ in range(steps):
            n, nrec = D.sharded_step(e, ids, flags, 1, apply_filter=True)
            out["cands"].append(e.cands().copy())
            out["recs"].append(np.sort(e.fetch_records(nrec), order=["key", "genome"]))
            out["passes"].append(e.debug_coarse_strand()["last_passes"])
            assert n == len(out["cands"][-1])
        out["strand"] = e.debug_coarse_strand()
        out["counts"] = [e.count(g) for g in ids]
        out["lazy"] = e.debug_lazy()
    return out


def _abc(N, D, c, texts, flags, ldr, steps=1, tcap=CC.CO_TCAP, lanes=None):
    """-> the run with both options on, held to the run with the pass option off, to the run with the strand option off and to
    the oracle's census c; the rounds and the passes of every call held to the census"""
    on = _run(N, D, texts, flags, ldr, 1, 1, steps, lanes)
    seq = _run(N, D, texts, flags, ldr, 1, 0, steps, lanes)
    two = _run(N, D, texts, flags, ldr, 0, 1, steps, lanes)
    for other, what in ((seq, "KR_OPT_COARSE_ONE_PASS = 0"), (two, "KR_OPT_COARSE_ONE_STRAND = 0")):
        assert len(other["cands"]) == steps
        for x, y in zip(on["cands"] + on["recs"], other["cands"] + other["recs"]):
            assert np.array_equal(x, y), what
        assert on["counts"] == other["counts"]
    assert on["counts"] == [len(k) for k in c["keys"]]
    for x, r in zip(on["cands"], on["recs"]):
        assert len(x) == len(c["cands"])
        for f in ("prefix", "in_mask", "out_mask"):
            assert np.array_equal(x[f], c["cands"][f]), f
        assert np.array_equal(r, c["recs"])
    ncoarse = len(CC.coarse(flags))
    for run, one_pass in ((on, 1), (seq, 0)):
        rf, rr, npass = OP.passes(c, texts, flags, tcap, one_pass) if ldr == OP.LDR else _passes(c, texts, flags, ldr, tcap, one_pass)
        st = run["strand"]
        assert (st["on"], st["partitions"], st["calls"]) == (1, ncoarse * steps, steps), st
        assert (st["last_forward"], st["last_reverse"]) == (rf, rr) and run["passes"] == [npass] * steps, (st, rf, rr, npass)
        assert (st["rounds_forward"], st["rounds_reverse"]) == (steps * rf, steps * rr)
        assert run["lazy"]["coarse_promoted"] == 0 and run["lazy"]["coarse"] == ncoarse * steps
    assert (two["strand"]["partitions"], two["strand"]["calls"], two["strand"]["on"]) == (0, 0, 0)
    assert two["lazy"]["coarse_promoted"] == 0 and two["lazy"]["coarse"] == ncoarse * steps
    return on, seq


def _passes(c, texts, flags, ldr, tcap, one_pass):
    L, _, R = ldr
    f, r = S.classes(c["C"], ldr)
    have = np.zeros(256, dtype=bool)
    for g in CC.coarse(flags):
        have |= np.bincount(S.forward_keys(texts[g], L, R)[1], minlength=256) > 0
    rf, rr = -(-f[have] // tcap), -(-r[have] // tcap)
    return int(rf.sum()), int(rr.sum()), int(np.maximum(rf, rr).sum() if one_pass else (rf + rr).sum())


# ----------------------------------------------------------------------------
# one window under a forward and a reverse entry of one pass; the palindrome; each base as the reverse record's
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3, 7])
def test_planted(N, D, K, monkeypatch, grid):
    _knobs(monkeypatch, grid=grid)
    texts, flags, plants = S.planted()
    c = S.census(K, "planted", texts, flags, S.PLANT_LDR)
    on, seq = _abc(N, D, c, texts, flags, S.PLANT_LDR)
    L, _, R = S.PLANT_LDR
    V, U = plants["two"]
    # the window of "two" lies under P1's forward entry and P2's reverse entry, both classes in ITS digit: one pass
    assert S.class_fwd(S.prefix_of(V, L, R), L, R) == S.class_rev(S.prefix_of(U, L, R), L, R) == S.digit_of(V, R)
    mine = on["recs"][0][on["recs"][0]["genome"] == S.CIN]
    for kind, n in (("fwd", 1), ("rev", 1), ("both", 2), ("palin", 2)):
        assert int(mine[mine["key"] == np.uint64(S.key_of(plants[kind][0], L, R))]["count"][0]) == n, kind
    assert on["passes"][0] < seq["passes"][0]


def test_siblings_walk_to_the_empty_slot(N, D, K, monkeypatch):
    _knobs(monkeypatch)
    texts, flags, plants = OP.siblings()
    c = S.census(K, "op_siblings", texts, flags, OP.LDR)
    on, _ = _abc(N, D, c, texts, flags, OP.LDR)
    got = on["cands"][0]["prefix"]
    for kind in ("fwd4", "rev3", "fwd3"):
        assert CC.held(got, [S.prefix_of(wi, OP.L, OP.R) for wi, _ in plants[kind]]).all(), kind
    recs = on["recs"][0]
    for lone in (plants["lone"], plants["lone_f"]):
        assert not np.any(recs["key"] == np.uint64(S.key_of(lone, OP.L, OP.R)))


@pytest.mark.parametrize("tcap", [1, 10, 50])
def test_uneven_rounds(N, D, K, monkeypatch, tcap):
    """a digit with forward candidates only, one with reverse candidates only, and at every table size a digit with three forward
    rounds and one reverse round: passes that hold one reading"""
    _knobs(monkeypatch, tcap=tcap, grid=3 if tcap != 1 else None)
    texts, flags, _ = OP.uneven()
    c = S.census(K, "op_uneven", texts, flags, OP.LDR)
    on, seq = _abc(N, D, c, texts, flags, OP.LDR, tcap=tcap)
    assert on["passes"][0] < seq["passes"][0]


def test_full_table(N, D, K, monkeypatch):
    """12 288 entries in the 16 384 slots of digit 0's first pass, the rest in a second; the unit overruns the queue"""
    _knobs(monkeypatch)
    texts, flags = OP.full()
    c = S.census(K, "op_full", texts, flags, OP.LDR)
    on, seq = _abc(N, D, c, texts, flags, OP.LDR)
    assert on["passes"][0] < seq["passes"][0]


@pytest.mark.parametrize("hits", OP.QUEUE)
def test_queue(N, D, K, monkeypatch, hits):
    """a unit of the queue's capacity - 1, = and + 1 passing keys, half of them hits of the reverse reading: the last overruns
    the queue, and the unit is looked up in place, both ways"""
    _knobs(monkeypatch)
    texts, flags, _ = OP.queue(hits)
    c = S.census(K, f"op_queue_{hits}", texts, flags, OP.LDR)
    on, _ = _abc(N, D, c, texts, flags, OP.LDR)
    assert len(on["cands"][0]) >= hits


@pytest.mark.parametrize("lanes", [1, 3])
def test_three_steps(N, D, K, monkeypatch, lanes):
    _knobs(monkeypatch)
    texts, flags = S.uniform()
    c = S.census(K, "uniform_6", texts, flags, S.UNIFORM_LDR)
    on, _ = _abc(N, D, c, texts, flags, S.UNIFORM_LDR, steps=3, lanes=lanes)
    for x, r in zip(on["cands"][1:], on["recs"][1:]):
        assert np.array_equal(x, on["cands"][0]) and np.array_equal(r, on["recs"][0])


# ----------------------------------------------------------------------------
# the two-strand form: the batched phase 1 and the two-bit prefilter
# ----------------------------------------------------------------------------
def _two_strand(N, D, K, name, texts, flags):
    c = CC.census(K, name, texts, flags)
    two = _run(N, D, texts, flags, CC.LDR, 0, 1)
    assert (two["strand"]["partitions"], two["strand"]["calls"]) == (0, 0)
    ncoarse = len(CC.coarse(flags))
    assert two["lazy"]["coarse_promoted"] == 0 and two["lazy"]["coarse"] == ncoarse
    x = two["cands"][0]
    assert len(x) == len(c["cands"])
    for f in ("prefix", "in_mask", "out_mask"):
        assert np.array_equal(x[f], c["cands"][f]), f
    assert np.array_equal(two["recs"][0], c["recs"]) and two["counts"] == [len(k) for k in c["keys"]]


@pytest.mark.parametrize("head,blocks", CC.DENSE)
def test_two_strand_dense(N, D, K, monkeypatch, head, blocks):
    _knobs(monkeypatch)
    texts, flags = CC.dense(head, blocks)
    _two_strand(N, D, K, f"dense_{head}_{blocks}", texts, flags)


@pytest.mark.parametrize("grid", [None, 3])
def test_two_strand_multi_and_edges(N, D, K, monkeypatch, grid):
    _knobs(monkeypatch, grid=grid)
    texts, flags, _ = SC.multi(3)
    _two_strand(N, D, K, "multi_3", texts, flags)
    texts, flags, _ = SC.edges()
    _two_strand(N, D, K, "edges", texts, flags)
