"""--guide-candidates without a GPU: the planted lane set holds what it was planted for; pick_guides against
plain loops on random tallies; shortlist_texts; the columns and the order of both writers."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import _native
from krisp_amd import krisp_fasta as KF
from krisp_amd import reports

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_shortlist_cases as SC                                         # noqa: E402
import guide_shortlist_reference as ref                                    # noqa: E402
from guides_reference import rc                                            # noqa: E402


# ----------------------------------------------------------------------------
# the planted set
# ----------------------------------------------------------------------------
def test_the_lane_set_holds_what_it_was_planted_for():
    s, o = SC.SETS[SC.LANES], SC.options(SC.LANES)
    L, D, _ = s["geo"]
    seen = {}
    for label, (rows, lo, hi), want in SC.lane_regions():
        n, ln = ref.lanes(rows, lo, hi, L, D, o["g"], 8, o["pam5"], o["pam3"], o["gc"][0], o["gc"][1], o["min_mismatches"])
        assert n == want, (label, n, want)
        seen[label] = (n, ln)
        first = ref.shortlist(rows, lo, hi, L, D, o["g"], 3, o["pam5"], o["pam3"], o["gc"][0], o["gc"][1], o["min_mismatches"])
        if label == "nine in one lane":
            assert [(r["start"], r["min_mismatches"], r["sum_mismatches"]) for r in first] == [(68, 6, 12), (164, 4, 9), (228, 4, 8)]
    # all of a region's candidates in one lane, nine of them or more; every count around the N of the tests
    for label in ("nine in one lane", "nine in one lane, no outgroup row", "bounds that keep all nine"):
        assert seen[label][0] == 9 and len(set(seen[label][1])) == 1, label
    assert len(set(seen["bounds cut the footprint"][1])) == 1
    assert len(set(seen["seventeen in two lanes"][1])) == 2
    assert {seen[f"exactly {n}"][0] for n in (8, 7, 2, 1, 0)} == {8, 7, 2, 1, 0}


# ----------------------------------------------------------------------------
# pick_guides
# ----------------------------------------------------------------------------
def _random_shortlist(rng, n, top):
    short = np.zeros((n, top), dtype=_native.GUIDE_RECORD)
    filled = rng.integers(0, top + 1, n)
    filled[:3] = (0, top, 1)                                     # a region without a candidate, a full one, one of one
    for i in range(n):
        short["candidates"][i] = filled[i] + rng.integers(0, 3)
        for j in range(filled[i]):
            short[i, j] = (1, rng.integers(0, 2), rng.integers(0, 50), rng.integers(0, 20), rng.integers(0, 99), rng.integers(0, 20),
                           short["candidates"][i, j], 0)
    return short, filled


@pytest.mark.parametrize("M", [0, 1, 2, 3])
@pytest.mark.parametrize("top", [1, 2, 8])
def test_the_pick_equals_plain_loops(M, top):
    """few distinct counts, so ties at every level; counts above 2^32; the columns above M hold garbage that must not count"""
    rng = np.random.default_rng(100 * M + top)
    n, ntexts = 400, 12
    short, filled = _random_shortlist(rng, n, top)
    tallies = rng.choice(np.array([0, 0, 1, 2, (1 << 32) + 1, (1 << 40) + 7, (1 << 63) + 5], dtype=np.uint64), (ntexts, 4))
    tallies[:, M + 1:] = rng.integers(0, 1 << 62, (ntexts, 3 - M), dtype=np.uint64)
    index = np.full((n, top), -1, dtype=np.int64)
    for i in range(n):
        index[i, :filled[i]] = rng.integers(0, ntexts, filled[i])     # (texts shared by ranks and regions)
    before = (short.copy(), index.copy(), tallies.copy())
    picked, ranks, picked_tallies = reports.pick_guides(short, index, tallies, M)
    assert all(np.array_equal(a, b) for a, b in zip(before, (short, index, tallies)))            # (the arguments are only read)
    assert picked.dtype == _native.GUIDE_RECORD and picked.shape == (n,) and ranks.shape == (n,)
    assert picked_tallies.dtype == np.uint64 and picked_tallies.shape == (n, 4)
    tied = 0
    for i in range(n):
        slots = [None if index[i, j] < 0 else [int(x) for x in tallies[index[i, j]]] for j in range(top)]
        rank, tally = ref.pick(slots, M)
        assert int(ranks[i]) == rank, (i, slots, int(ranks[i]), rank)
        assert picked[i].tobytes() == short[i, rank].tobytes()
        assert tuple(int(x) for x in picked_tallies[i]) == tuple(tally) + (0,) * (3 - M)
        keys = [tuple(t[:M + 1]) for t in slots if t is not None]
        tied += len(keys) > len(set(keys))
    assert int(picked["found"][0]) == 0 and int(ranks[0]) == 0 and not picked_tallies[0].any()
    assert top == 1 or tied > 5
    if top == 1:
        assert not ranks.any()


def test_the_pick_of_no_region():
    short = np.zeros((0, 4), dtype=_native.GUIDE_RECORD)
    picked, ranks, tallies = reports.pick_guides(short, np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4), dtype=np.uint64), 2)
    assert len(picked) == len(ranks) == len(tallies) == 0


# ----------------------------------------------------------------------------
# shortlist_texts
# ----------------------------------------------------------------------------
def test_the_texts_of_a_shortlist():
    g = 12
    word = "ACGGTCATTGCA"                    # (no palindrome)
    other = "GGATCCAAGTCA"
    t0 = "TT" + word + "CC" + rc(word) + "AAAA"          # the text on '+' at 2 and on '-' at 16
    t1 = rc(word) + "G" + other + "ACGTACG"              # the same text on '-' at 0, another on '+' at 13
    assert len(t0) == len(t1) == 32
    templates = np.frombuffer((t0 + t1 + t0).encode(), dtype=np.uint8).reshape(3, 32)
    short = np.zeros((3, 3), dtype=_native.GUIDE_RECORD)
    for (i, j), (strand, start) in {(0, 0): (0, 2), (0, 1): (1, 16), (1, 0): (1, 0), (1, 1): (0, 13), (1, 2): (1, 13)}.items():
        short[i, j]["found"], short[i, j]["strand"], short[i, j]["start"] = 1, strand, start
    short["candidates"] = 7
    texts, index = reports.shortlist_texts(templates, short, g)
    want = sorted({word.encode(), other.encode(), rc(other).encode()})
    assert texts == want                                             # (listed once, ordered by their bytes)
    assert index.dtype == np.int64 and index.shape == (3, 3)
    w, o, r = (want.index(x.encode()) for x in (word, other, rc(other)))
    assert index.tolist() == [[w, w, -1], [w, o, r], [-1, -1, -1]]
    # guide_texts gives the same text for the same record
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2)):
        one, _ = reports.guide_texts(templates[i:i + 1], short[i:i + 1, j], g)
        assert one == [texts[index[i, j]]]
    none, index = reports.shortlist_texts(templates, np.zeros((3, 2), dtype=_native.GUIDE_RECORD), g)
    assert none == [] and (index == -1).all() and index.shape == (3, 2)
    # no region at all, as a run that finds none gives it
    none, index = reports.shortlist_texts(np.empty((0, 1), dtype=np.uint8), np.zeros((0, 4), dtype=_native.GUIDE_RECORD), g)
    assert none == [] and index.shape == (0, 4)


# ----------------------------------------------------------------------------
# the writers
# ----------------------------------------------------------------------------
def _written():
    g = 12
    t = ["TTTC" + "ACGGTCATTGCA" + "GGATCCAAGTCAGAAA", "TTTC" + "GGATCCAAGTCA" + "ACGGTCATTGCAGAAA", "A" * 32]
    templates = np.frombuffer("".join(t).encode(), dtype=np.uint8).reshape(3, 32)
    short = np.zeros((3, 3), dtype=_native.GUIDE_RECORD)
    short[0, 0] = (1, 0, 4, 5, 9, 6, 2, 0)
    short[0, 1] = (1, 1, 16, 4, 8, 6, 2, 0)
    short[0, 2]["candidates"] = 2
    short[1, 0] = (1, 0, 4, 3, 3, 6, 1, 0)
    short[1, 1]["candidates"] = short[1, 2]["candidates"] = 1
    texts, index = reports.shortlist_texts(templates, short, g)
    tallies = np.zeros((len(texts), 4), dtype=np.uint64)
    tallies[index[0, 0]] = (1, 0, (1 << 33) + 2, 99)
    tallies[index[0, 1]] = (0, 7, 1, 98)
    tallies[index[1, 0]] = (0, 0, 3, 97)
    return g, t, templates, short, index, tallies


def test_write_guides_with_and_without_the_pick(tmp_path):
    g, t, templates, short, index, tallies = _written()
    M = 2
    picked, ranks, picked_tallies = reports.pick_guides(short, index, tallies, M)
    assert ranks.tolist() == [1, 0, 0]
    plain, with_pick = str(tmp_path / "plain.tsv"), str(tmp_path / "pick.tsv")
    reports.write_guides(plain, templates, picked, g, 4, 0, regions=[5, 6, 7])
    reports.write_guides(with_pick, templates, picked, g, 4, 0, regions=[5, 6, 7], ranks=ranks, shortlisted=(index >= 0).sum(axis=1),
                         outgroup_hits=picked_tallies[:, :M + 1])
    a, b = open(plain).read().split("\n"), open(with_pick).read().split("\n")
    assert a[0] == KF.GUIDE_HEADER and b[0] == KF.GUIDE_HEADER + "\trank\tshortlisted\toutgroup_hits"
    assert len(a) == len(b) == 4 and a[-1] == b[-1] == ""
    assert a[1] == "5\t-\t16\t28\tTTTC\t\t" + rc(t[0][16:28]) + "\t50.000\t4\t8\t2"
    assert b[1] == a[1] + "\t2\t2\t0,7,1" and b[2] == a[2] + "\t1\t1\t0,0,3"
    with pytest.raises(ValueError):
        reports.write_guides(with_pick, templates, picked, g, 4, 0, ranks=ranks)


def test_write_guide_candidates(tmp_path):
    g, t, templates, short, index, tallies = _written()
    M = 2
    picked, ranks, _ = reports.pick_guides(short, index, tallies, M)
    path, one = str(tmp_path / "c.tsv"), str(tmp_path / "one.tsv")
    reports.write_guide_candidates(path, templates, short, index, tallies, ranks, g, M, 4, 0, regions=[5, 6, 7])
    lines = open(path).read().split("\n")
    assert lines[0] == KF.GUIDE_HEADER + "\trank\tshortlisted\toutgroup_hits\tpicked" and lines[-1] == "" and len(lines) == 5
    # a candidate's first eleven columns are write_guides' for its record
    for ln, (i, j) in zip(lines[1:4], ((0, 0), (0, 1), (1, 0))):
        reports.write_guides(one, templates[i:i + 1], short[i:i + 1, j], g, 4, 0, regions=[5 + i])
        assert ln.split("\t")[:11] == open(one).read().split("\n")[1].split("\t")
    assert [ln.split("\t")[11:] for ln in lines[1:4]] == [["1", "2", f"1,0,{(1 << 33) + 2}", "0"], ["2", "2", "0,7,1", "1"],
                                                         ["1", "1", "0,0,3", "1"]]
    # with M = 0 only t0 is written and compared
    _, ranks0, _ = reports.pick_guides(short, index, tallies, 0)
    reports.write_guide_candidates(path, templates, short, index, tallies, ranks0, g, 0, 4, 0)
    assert [ln.split("\t")[13] for ln in open(path).read().split("\n")[1:4]] == ["1", "0", "0"]


def test_the_refusals_of_the_option():
    why = reports.guide_candidates_refusal
    assert why(True, None, ["o"], False) is None and why(False, None, [], False) is None
    assert why(True, None, ["o"], True) == "--out_guide_candidates needs --guide-candidates"
    assert "needs --out_guides" in why(False, 4, ["o"], False)
    for n in (0, 9, -1):
        assert "between 1 and 8" in why(True, n, ["o"], False)
    assert "needs an --outgroup file" in why(True, 4, [], False)
    for n in range(1, 9):
        assert why(True, n, ["o"], True) is None
    assert reports.GUIDE_MAX_CANDIDATES == 8
