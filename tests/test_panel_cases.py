"""The candidate sets of the panel pass (panel_cases.py) keep what the device test relies on, by the reference alone
(panel_reference.py), without a GPU: a change of the generator that loses a fate, the full panel, the short one, a late
member's drops or a planted verdict fails here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_cases as PC                                                    # noqa: E402
import panel_reference as ref                                               # noqa: E402


def _fates(name):
    return PC.expected(name)[1]


def test_every_fate_occurs_in_at_least_three_sets():
    for fate in (0, 1, 2, 3):
        sets = [n for n in PC.SETS if any(f == fate for f, _ in _fates(n))]
        print("fate", fate, "in", len(sets), "sets")
        assert len(sets) >= 3, (fate, sets)


def test_a_panel_fills_and_a_panel_ends_short():
    full = [n for n in PC.SETS if len(PC.expected(n)[0]) == PC.case(n)["size"]]
    short = [n for n in PC.SETS if len(PC.expected(n)[0]) < PC.case(n)["size"]]
    assert full and short, (full, short)
    # N = 1; N = 64 reached with candidates left alive; N above what survives; one locus, one member
    assert PC.case("size_1")["size"] == 1 and len(PC.expected("size_1")[0]) == 1
    assert PC.case("size_64_filled")["size"] == 64 and len(PC.expected("size_64_filled")[0]) == 64
    assert any(f == 0 for f, _ in _fates("size_64_filled"))
    members, fates = PC.expected("size_above_survivors")
    assert 1 < len(members) < 64 and all(f != 0 for f, _ in fates)
    members, fates = PC.expected("one_locus")
    assert len(members) == 1 and sorted(fates) == [(1, 1)] + [(2, 1)] * 19


def test_a_later_member_drops_for_either_cause():
    for fate in (2, 3):
        sets = [n for n in PC.SETS if any(f == fate and by >= 2 for f, by in _fates(n))]
        assert sets, fate


@pytest.mark.parametrize("name", [n for n in PC.SETS if "plant" in PC.SETS[n]()])
def test_the_planted_verdicts(name):
    """a plant with a fate ends with it; the 15-mer and the window broken by an N end alive or as a member"""
    fates = _fates(name)
    for position, want in PC.case(name)["plant"]:
        if want is None:
            assert fates[position][0] in (0, 1), (name, position, fates[position])
        else:
            assert fates[position] == want, (name, position, fates[position])


def test_the_plants_are_what_their_names_say():
    t = PC.case("locus_fifteen")["templates"]
    assert t[0][12:27] in t[1] and not ref.same_locus(t[0], t[1])
    t = PC.case("locus_broken_n")["templates"]
    assert t[0][12:28] == t[1][12:28] and "N" in t[0][12:28] and not ref.same_locus(t[0], t[1])
    for name, mine, theirs in (("locus_first_window", 0, 24), ("locus_last_window", 24, 0)):
        t = PC.case(name)["templates"]
        shared = ref.windows(t[0]) & ref.windows(t[1])
        assert shared == {t[1][mine:mine + 16]} == {t[0][theirs:theirs + 16]}, name
    t = PC.case("locus_reverse_only")["templates"]
    assert not ref.windows(t[0]) & ref.windows(t[1]) and ref.same_locus(t[0], t[1])
    t = PC.case("locus_poly")["templates"]
    assert t[0] == "A" * 40 and t[1] == "T" * 40
    # W = 15: equal templates, never the same locus; W = 16: one window
    c = PC.case("w15")
    assert c["templates"][0] == c["templates"][1] and all(f != 2 for f, _ in _fates("w15"))
    assert all(len(ref.windows(x)) == 1 for x in PC.case("w16")["templates"])
    assert len(PC.case("w2047")["templates"][0]) == 2047
    lengths = {n for p in PC.case("primers_10_and_60")["pairs"] for n in (p[1], p[3])}
    assert {10, 60} <= lengths and (0, 60, 70, 60) in PC.case("primers_10_and_60")["pairs"]
    assert [len(PC.case(n)["templates"]) for n in ("random_1", "random_2", "random_65", "random_300", "pooled_5000")] == [1, 2, 65, 300, 5000]
    # the clash plants: the planted duplex lies above max_sec, and the candidate of clash_by2 passes member 1
    c = PC.case("clash_by2")
    o = [ref.primers(t, p) for t, p in zip(c["templates"], c["pairs"])]
    assert max(ref.cross_figure(o[2], o[0])) <= c["max_sec"] < ref.cross_figure(o[2], o[1])[1]
    c = PC.case("clash_and_locus")
    o = [ref.primers(t, p) for t, p in zip(c["templates"], c["pairs"])]
    assert ref.cross_figure(o[1], o[0])[1] > c["max_sec"] and ref.same_locus(c["templates"][0], c["templates"][1])


def test_end_never_exceeds_any():
    for name in ("random_65", "clash_end3", "primers_10_and_60"):
        c = PC.case(name)
        o = [ref.primers(t, p) for t, p in zip(c["templates"], c["pairs"])]
        for x in o[1:8]:
            a, e = ref.cross_figure(x, o[0])
            assert e <= a
