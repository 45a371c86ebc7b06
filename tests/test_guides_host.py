"""--out_guides without a GPU: the reference (guides_reference.py) pinned to regions whose answers are worked out by hand
here, the generator's plants (guide_cases.py) against their intended outcomes, guide_rows, the motif masks, every refusal,
write_guides' columns and the parser's dependent options."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import amplicon, primers
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_cases                                                         # noqa: E402
import guides_reference as ref                                             # noqa: E402

RECORD = np.dtype([(f, "<u4") for f in ref.FIELDS + ("pad",)])


def _records(recs):
    out = np.zeros(len(recs), dtype=RECORD)
    for i, r in enumerate(recs):
        for f in ref.FIELDS:
            out[f][i] = r[f]
    return out


# ----------------------------------------------------------------------------
# the reference, by hand
# ----------------------------------------------------------------------------
def test_three_windows_counted_by_hand():
    """K = 14, g = 12, no motifs, L = 5, D = 4 (the centre is 14): the windows 0, 1, 2 lie 2, 0, 2 off it.  The outgroup row
    differs from the template at columns 0 and 13: mm = 1, 0, 1.  Every window has 6 of 12 G or C."""
    T, O = "ACGTACGTACGTAC", "CCGTACGTACGTAA"
    kw = dict(lo=0, hi=14, L=5, D=4, g=12)
    # at least 1: the windows 0 and 2 on both strands; all tie in d, s and the centre: '+', then the smaller p
    assert ref.guide([T, O], min_mismatches=1, **kw) == dict(found=1, strand=0, start=0, min_mismatches=1, sum_mismatches=1, gc=6,
                                                             candidates=4)
    # at least 0: six candidates, d = 1 still beats the centred window's d = 0
    assert ref.guide([T, O], min_mismatches=0, **kw) == dict(found=1, strand=0, start=0, min_mismatches=1, sum_mismatches=1, gc=6,
                                                             candidates=6)
    assert ref.guide([T, O], min_mismatches=2, **kw) == dict.fromkeys(ref.FIELDS, 0)
    # a second row that differs at columns 12 and 13: window 2 has mm = (1, 2), window 0 (1, 0) -> d = 0 there
    assert ref.guide([T, O, "ACGTACGTACGTCA"], min_mismatches=1, **kw) == dict(found=1, strand=0, start=2, min_mismatches=1,
                                                                               sum_mismatches=3, gc=6, candidates=2)
    # no outgroup rows: d = g, s = 0, the centred window
    assert ref.guide([T], min_mismatches=1, **kw) == dict(found=1, strand=0, start=1, min_mismatches=12, sum_mismatches=0, gc=6,
                                                          candidates=6)
    # bounds [1, 14): the windows 1 and 2; [1, 13): window 1 alone; [2, 13): none
    assert ref.guide([T], **dict(kw, lo=1))["candidates"] == 4
    assert ref.guide([T], **dict(kw, lo=1, hi=13)) == dict(found=1, strand=0, start=1, min_mismatches=12, sum_mismatches=0, gc=6,
                                                           candidates=2)
    assert ref.guide([T], **dict(kw, lo=2, hi=13))["found"] == 0
    # GC bounds in whole percent against 6 of 12
    assert ref.guide([T], gc_lo=50, gc_hi=50, **kw)["candidates"] == 6
    assert ref.guide([T], gc_lo=51, gc_hi=70, **kw)["found"] == 0 and ref.guide([T], gc_lo=30, gc_hi=49, **kw)["found"] == 0


HAND_T = "GCATCGATGCATGGAAACGC"


def test_a_guide_on_the_minus_strand_by_hand():
    """TTTV, g = 12, K = 20: the template holds GAAA at 13 .. 16 and no TTT: the one candidate is the window [1, 13) read on
    '-', whose 5' neighbours read rc(GAAA) = TTTC.  The window CATCGATGCATG has 6 G or C."""
    kw = dict(lo=0, hi=20, L=8, D=4, g=12, pam5="TTTV")
    want = dict(found=1, strand=1, start=1, min_mismatches=12, sum_mismatches=0, gc=6, candidates=1)
    assert ref.guide([HAND_T], **kw) == want
    assert ref.guide([HAND_T], **dict(kw, hi=17)) == want and ref.guide([HAND_T], **dict(kw, hi=16))["found"] == 0
    assert ref.guide([HAND_T], **dict(kw, lo=1)) == want and ref.guide([HAND_T], **dict(kw, lo=2))["found"] == 0
    # V excludes T: with A at 12 and 13 the window [1, 13) has AAAA behind it, which reads TTTT (and TAAA at 11 .. 14 would
    # serve a window at -1 only)
    assert ref.guide([HAND_T[:12] + "AA" + HAND_T[14:]], **kw)["found"] == 0
    # as a 3' motif on '-' the columns in front of the window are read: rc(GC) = GC at [0, 2) for the window [2, 14)
    assert ref.guide([HAND_T], **dict(kw, pam5="", pam3="GC", gc_lo=0, gc_hi=100))["candidates"] >= 1
    got = ref.candidates([HAND_T], 0, 20, 8, 4, 12, "", "GC", 0, 100, 1)
    assert (12, 0, abs(2 * 2 + 12 - 20), 1, 2, 6) in got
    # an outgroup row: differences at 3 and 7, an N at 5 that never counts
    o = HAND_T[:3] + "A" + HAND_T[4] + "N" + HAND_T[6] + "C" + HAND_T[8:]
    assert ref.guide([HAND_T, o], **kw) == dict(want, min_mismatches=2, sum_mismatches=2)
    assert ref.rc("GAAA") == "TTTC" and ref.rc("CATCGATGCATG") == "CATGCATCGATG"


def test_a_run_of_five_and_a_letter_that_is_no_base_by_hand():
    kw = dict(lo=0, hi=14, L=5, D=4, g=12)
    assert ref.guide(["ACGTCCCCCGTACG"], **kw)["found"] == 0                # CCCCC lies in every window
    assert ref.guide(["CCCCCGTACGTACG"], **kw) == dict(found=1, strand=0, start=1, min_mismatches=12, sum_mismatches=0, gc=8,
                                                       candidates=4)         # ... in window 0 alone
    assert ref.guide(["ACGTACGTACGTAN"], **kw)["candidates"] == 4           # N at 13: the windows 0 and 1
    assert ref.guide(["ACGTACNTACGTAC"], **kw)["found"] == 0
    # the N lies beside the window but under the motif: N matches every base, the template's letter must still be one
    assert ref.guide(["NCGTACGTACGTAC"], pam5="N", **kw)["candidates"] == 2         # '+' at 2, '-' at 1 (window 0 holds the N)
    assert ref.guide(["ACGTACGTACGTAC"], pam5="N", **kw)["candidates"] == 4


# ----------------------------------------------------------------------------
# the generator did its work
# ----------------------------------------------------------------------------
def test_every_plant_produces_its_intended_outcome():
    s = guide_cases.SETS[guide_cases.PLANTED]
    plants = guide_cases.planted_regions()
    labels = [p[0] for p in plants]
    for want in ["no outgroup rows"] + [f"{n} outgroup rows" for n in (1, 3, 64, 65, 130)] + \
            ["outgroup N", "outgroup R", "template IUPAC in the protospacer", "template IUPAC in the PAM only", "PAM at column -1",
             "PAM at column K", "bounds of one window", "bounds one short on the right", "bounds one short on the left", "lo = hi",
             "minus strand only", "d decides", "d ties, s decides", "d and s tie, the centre decides",
             "d, s and the centre tie, the strand decides", "all but p tie", "GC alone fails", "a run of five alone fails",
             "d one below the least"]:
        assert want in labels, want
    L, D, _ = s["geo"]
    for label, (rows, lo, hi), expect in plants:
        got = ref.guide(rows, lo, hi, L, D, s["g"], s["pam5"], s["pam3"], s["gc"][0], s["gc"][1], s["min_mismatches"])
        assert {k: got[k] for k in expect} == expect, (label, got)
        assert len(rows) - 1 == int(label.split()[0]) if label.endswith("outgroup rows") and label[0].isdigit() else True
    # the plants that fail for one reason only pass without it
    by = {p[0]: p[1] for p in plants}
    kw = dict(L=L, D=D, g=s["g"], pam5=s["pam5"], pam3=s["pam3"])
    rows, lo, hi = by["GC alone fails"]
    assert ref.guide(rows, lo, hi, gc_lo=28, gc_hi=70, min_mismatches=2, **kw)["found"] == 1
    rows, lo, hi = by["d one below the least"]
    assert ref.guide(rows, lo, hi, gc_lo=30, gc_hi=70, min_mismatches=1, **kw) == dict(found=1, strand=0, start=40, min_mismatches=1,
                                                                                       sum_mismatches=3, gc=ref.guide(
                                                                                           rows[:1], lo, hi, **kw)["gc"], candidates=1)
    rows, lo, hi = by["template IUPAC in the PAM only"]
    assert rows[0][36:40] == "TTTV" and ref.guide(rows, lo, hi, **dict(kw, pam5=""))["found"] == 1


@pytest.mark.parametrize("name", list(guide_cases.SETS))
def test_every_set_has_regions_with_and_without_a_guide(name):
    s = guide_cases.SETS[name]
    L, D, R = s["geo"]
    regs = guide_cases.regions(name)
    recs = ref.guides(regs, L, D, **guide_cases.options(name))
    assert len(regs) == s["n"] + (len(guide_cases.planted_regions()) if name == guide_cases.PLANTED else 0)
    assert all(len(row) == L + D + R for rows, _, _ in regs for row in rows)
    found = sum(r["found"] for r in recs)
    if s["n"] == 1:
        assert found == 1 and L + D + R == 2047
        return
    assert 0 < found < len(regs)
    if s["g"] < L + D + R:
        assert any(r["strand"] for r in recs) and any(r["found"] and not r["strand"] for r in recs)
    assert {len(rows) - 1 for rows, _, _ in regs} >= {0, 1, 3, 64, 65, 130}
    assert any(lo == hi for _, lo, hi in regs) and any(0 < hi - lo < L + D + R for _, lo, hi in regs)


# ----------------------------------------------------------------------------
# the host layer
# ----------------------------------------------------------------------------
def test_the_motif_masks():
    assert KF.motif_masks("") == []
    assert KF.motif_masks("TTTV") == [8, 8, 8, 7] and KF.motif_masks("h") == [11] and KF.motif_masks("U") == [8]
    for letter, bases in ref.IUPAC.items():
        assert KF.motif_masks(letter) == [sum(1 << "ACGT".index(b) for b in bases)], letter
    assert set(KF.IUPAC_MASK) == set(ref.IUPAC)
    for bad in ("X", "TT-V", "TT V", "1"):
        with pytest.raises(ValueError, match="IUPAC"):
            KF.motif_masks(bad)


def _groups():
    left, right = "ACGATCAGTCAT", "GATTACAGGCAT"
    g0 = [amplicon.Amplicon(left, "ACGT", right, ["a"]), amplicon.Amplicon(left, "ACGA", right, ["b"]),
          amplicon.Amplicon(left, "TCGT", right, ["a", "x"]), amplicon.Amplicon(left.lower(), "UCGU", right, ["x", "y"])]
    g1 = [amplicon.Amplicon(left, "GCGC", right, ["a", "b", "x"])]
    g2 = [amplicon.Amplicon(left, "CCCC", right, ["a", "b"]), amplicon.Amplicon(left, "CCCA", right, ["y"])]
    return [g0, g1, g2], left, right


def test_guide_rows_on_groups_with_mixed_labels_and_without_an_outgroup():
    groups, left, right = _groups()
    rows, off, L, D, R = KF.guide_rows(groups, ["a", "b"])
    text = [bytes(r).decode() for r in rows]
    assert (L, D, R) == (12, 4, 12) and off.tolist() == [0, 3, 4, 6] and off.dtype == np.uint64 and rows.dtype == np.uint8
    # group 0: the consensus of the two Amplicons whose labels are all ingroup (T / A -> W), then the two others -- one
    # shared with an ingroup genome -- upper case with T for U; group 1: one Amplicon, its own template whatever its labels
    assert text == [left + "ACGW" + right, left + "TCGT" + right, left + "TCGT" + right, left + "GCGC" + right,
                    left + "CCCC" + right, left + "CCCA" + right]
    assert text[0] == primers.design_template(groups[0], frozenset("ab"))
    # a run without --outgroup: every Amplicon is in the template, no outgroup rows
    rows, off, _, _, _ = KF.guide_rows(groups, None)
    assert off.tolist() == [0, 1, 2, 3] and bytes(rows[2]).decode() == left + "CCCM" + right
    assert bytes(rows[0]).decode() == primers.design_template(groups[0], None)
    # templates handed in are taken as they are
    t = KF.design_templates(groups, ["a", "b"])
    again = KF.guide_rows(groups, ["a", "b"], templates=t)
    assert again[0].tobytes() == KF.guide_rows(groups, ["a", "b"])[0].tobytes() and again[1].tolist() == [0, 3, 4, 6]
    rows, off, _, _, _ = KF.guide_rows([], ["a"])
    assert len(rows) == 0 and off.tolist() == [0]
    # ... and the reference on them: group 2's window differs from its one outgroup row in the last diagnostic column
    rows, off, L, D, R = KF.guide_rows(groups, ["a", "b"])
    regs = [([bytes(r).decode() for r in rows[int(off[i]):int(off[i + 1])]], 0, 28) for i in range(3)]
    recs = ref.guides(regs, L, D, 28)
    assert [r["found"] for r in recs] == [0, 1, 1]                            # (group 0's template holds a W)
    assert recs[1]["min_mismatches"] == 28 and recs[2]["min_mismatches"] == 1 and recs[2]["sum_mismatches"] == 1


REFUSALS = [
    (["--primer3"], "cannot be combined with --primer3"),
    (["--guide-size", "11"], "between 12 and 40"),
    (["--guide-size", "41"], "between 12 and 40"),
    (["--pam5", "TTTX"], "no letter of the IUPAC code"),
    (["--pam3", "T-"], "no letter of the IUPAC code"),
    (["--pam5", "NNNNNTTTV"], "at most 8 letters"),
    (["--pam3", "HNNNNNNNN"], "at most 8 letters"),
    (["--guide-gc", "60", "40"], "upper bound lies below"),
    (["--guide-min-mismatches", "-1"], "between 0 and --guide-size"),
    (["--guide-min-mismatches", "29"], "between 0 and --guide-size"),
    (["--guide-size", "20", "--guide-min-mismatches", "21"], "between 0 and --guide-size"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_every_refusal_exits_2_with_its_message(extra, message, capsys):
    """before a genome is read: the files named do not exist"""
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_ingroup.fasta", "--outgroup", "no_such_outgroup.fasta", "-c", "30", "-d", "40", "--out_guides", "g.tsv"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "ERROR: " in err and message in err


def test_a_guide_longer_than_the_amplicon_is_refused(capsys):
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_ingroup.fasta", "-c", "10", "-d", "4", "--out_guides", "g.tsv", "--guide-size", "25"])
    assert e.value.code == 2 and "must not exceed the amplicon length 24" in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--guide-size", "20"], ["--pam5", "TTTV"], ["--pam3", "H"], ["--guide-gc", "30", "70"],
                                   ["--guide-min-mismatches", "2"]])
def test_the_dependent_options_need_out_guides(extra, capsys):
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_ingroup.fasta", "-c", "30", "-d", "40"] + extra)
    assert e.value.code == 2 and f"ERROR: {extra[0]} needs --out_guides" in capsys.readouterr().err


def test_the_parser_and_its_defaults():
    p = KF.build_parser()
    a = p.parse_args(["x.fasta", "-c", "30", "-d", "40"])
    assert (a.out_guides, a.guide_size, a.pam5, a.pam3, a.guide_gc, a.guide_min_mismatches) == (None,) * 6
    a = p.parse_args(["x.fasta", "-c", "30", "-d", "40", "--out_guides", "g.tsv", "--guide-size", "20", "--pam5", "TTTV", "--pam3", "H",
                      "--guide-gc", "35", "65", "--guide-min-mismatches", "3"])
    assert (a.out_guides, a.guide_size, a.pam5, a.pam3, a.guide_gc, a.guide_min_mismatches) == ("g.tsv", 20, "TTTV", "H", [35, 65], 3)
    import inspect
    sig = inspect.signature(KF.design_guides).parameters
    assert (sig["guide_size"].default, sig["pam5"].default, sig["pam3"].default, sig["gc"].default,
            sig["min_mismatches"].default) == (28, "", "", (30, 70), 1)


def test_the_functions_refuse_as_the_command_line_does():
    assert KF.guides_refusal(100, 28, "TTTV", "", (30, 70), 1) is None
    assert KF.guides_refusal(100, 28, "", "h", (30, 30), 0) is None and KF.guides_refusal(28, 28, "", "", (0, 100), 28) is None
    assert "amplicon length" in KF.guides_refusal(27, 28, "", "", (30, 70), 1)
    with pytest.raises(ValueError, match="between 12 and 40"):
        KF.design_guides([], None, guide_size=11)
    with pytest.raises(ValueError, match="IUPAC"):
        KF.design_guides([], None, pam5="TTTZ")
    assert len(KF.design_guides([], None)) == 0                               # (no region: no device is asked for)


def test_write_guides_columns(tmp_path):
    """the hand-made '-' guide above, a '+' guide with both motifs, a region without a guide; the region numbers given"""
    kw = dict(lo=0, hi=20, L=8, D=4, g=12, pam5="TTTV")
    minus = ref.guide([HAND_T], **kw)
    plus_t = "GTTTC" + "CATCGATGCATG" + "TAC"
    plus = ref.guide([plus_t, plus_t[:7] + "G" + plus_t[8:]], **dict(kw, pam3="H"))
    assert plus == dict(found=1, strand=0, start=5, min_mismatches=1, sum_mismatches=1, gc=6, candidates=1)
    rows = np.frombuffer((HAND_T + "A" * 20 + plus_t).encode(), dtype=np.uint8).reshape(3, 20)
    recs = _records([minus, dict.fromkeys(ref.FIELDS, 0), plus])
    p = str(tmp_path / "g.tsv")
    KF.write_guides(p, rows, recs, 12, 4, 0)
    assert open(p).read() == KF.GUIDE_HEADER + "\n" + "0\t-\t1\t13\tTTTC\t\tCATGCATCGATG\t50.000\t12\t0\t1\n" + \
        "2\t+\t5\t17\tTTTC\t\tCATCGATGCATG\t50.000\t1\t1\t1\n"
    KF.write_guides(p, rows, recs, 12, 4, 1, regions=[7, 8, 9])
    lines = open(p).read().split("\n")
    assert lines[0].split("\t") == ["region", "strand", "start", "end", "pam5", "pam3", "protospacer", "gc_percent", "min_mismatches",
                                    "sum_mismatches", "candidates"]
    assert lines[2] == "9\t+\t5\t17\tTTTC\tT\tCATCGATGCATG\t50.000\t1\t1\t1" and lines[1].startswith("7\t-\t1\t13\tTTTC\tC\t")
    assert lines[3] == "" and len(lines) == 4
    KF.write_guides(p, rows[:0], recs[:0], 12)
    assert open(p).read() == KF.GUIDE_HEADER + "\n"
