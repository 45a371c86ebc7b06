"""The definition of --design-primers on hand-made templates with written-out answers, through the brute-force
reference (design_reference.py) that the GPU test holds the device to; the integer Tm against a float64 restatement; the
command line's refusals.  No GPU."""
import math
import os
import random
import sys

import pytest

from krisp_amd import krisp_fasta as KF
from krisp_amd import primers, thermo as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_reference as ref                                             # noqa: E402

LOOSE = dict(tm=(-200, 200), gc=(0, 100), amp_size=(1, 2000), primer_size=(10, 12), max_sec_tm=200, gc_clamp=0, max_end_gc=5)


def test_the_constants_are_the_rounded_logarithms():
    assert T.SALT_DS == -1102 and T.SALT_DS == round(368 * math.log(0.05))
    assert T.CONC_DS == round(1987 * math.log(50e-9 / 4)) and -36160 < T.CONC_DS < -36157
    assert T.CONC_SELF_DS == round(1987 * math.log(50e-9)) and -33406 < T.CONC_SELF_DS < -33402
    # a step and its reverse complement are one entry: the Tm of an oligo is the Tm of its reverse complement
    for a in range(4):
        for b in range(4):
            assert T.NN_DH[4 * a + b] == T.NN_DH[4 * (3 - b) + (3 - a)] and T.NN_DS[4 * a + b] == T.NN_DS[4 * (3 - b) + (3 - a)]
    assert T.mk(40) == 313150 and T.celsius(313150) == "40.000" and T.celsius(0) == "-273.150" and T.milli(-5) == "-0.005"
    assert T.gc_percent(1, 3) == "33.333" and T.gc_percent(2, 3) == "66.667" and T.gc_percent(10, 20) == "50.000"


def test_a_tm_computed_by_hand():
    """ACACACACAC: five AC steps and four CA steps, terminals A and C
    dH = 5 (-8400) + 4 (-8500) + 2300 + 100 = -73600
    dS = 5 (-22400) + 4 (-22700) + 4100 - 2800 + 9 SALT + CONC = -201500 + 9 SALT + CONC"""
    x = "ACACACACAC"
    ds = -201500 + 9 * T.SALT_DS + T.CONC_DS
    assert ref.primer_tm(x) == (-73600 * 10 ** 6) // ds == 73600 * 10 ** 6 // -ds
    assert 297000 < ref.primer_tm(x) < 297600                   # about 24.2 degrees Celsius
    assert ref.primer_tm(ref.rc(x)) == ref.primer_tm(x)


def test_a_palindromic_primer_takes_the_symmetry_terms():
    """AACGCGCGTT is its own reverse complement: steps AA AC CG GC CG GC CG GT TT, terminals A and T
    dH = -84000 + 4600 = -79400;  dS = -219600 + 8200 + 9 SALT + CONC_SELF - 1400"""
    x = "AACGCGCGTT"
    assert ref.rc(x) == x
    ds = -219600 + 8200 + 9 * T.SALT_DS + T.CONC_SELF_DS + T.SYM_DS
    assert ref.primer_tm(x) == (-79400 * 10 ** 6) // ds
    assert ref.primer_tm(x) != ref.duplex_tm(x)                 # (a run of a duplex figure takes neither term)
    assert ref.duplex_tm(x) == (-79400 * 10 ** 6) // (-219600 + 8200 + 9 * T.SALT_DS + T.CONC_DS)


def test_each_single_filter_in_turn():
    o = T.options(**dict(LOOSE, primer_size=(20, 20), gc=(40, 60), tm=(45, 65), gc_clamp=1, max_end_gc=3))
    good = "ACGATCAGTCATGACTTGAC"                               # 9 of 20 G or C, ends ..TTGAC: clamp C, 2 G or C at the end
    tm, gc = ref.single_ok(good, o)
    assert gc == 9 and o["tm_lo"] <= tm <= o["tm_hi"]
    assert ref.single_ok(good, dict(o, tm_lo=tm + 1)) is None and ref.single_ok(good, dict(o, tm_hi=tm - 1)) is None
    assert ref.single_ok(good, dict(o, tm_lo=tm, tm_hi=tm)) == (tm, 9)
    assert ref.single_ok(good, dict(o, gc_lo=46)) is None and ref.single_ok(good, dict(o, gc_lo=45)) == (tm, 9)
    assert ref.single_ok(good, dict(o, gc_hi=44)) is None and ref.single_ok(good, dict(o, gc_hi=45)) == (tm, 9)
    assert ref.single_ok("ACGATCAGTCATGAAAAAGC", o) is None      # five A in a row
    assert ref.single_ok("ACGATCAGTCATGAAAAGGC", dict(o, tm_lo=0)) is not None      # four are allowed
    assert ref.single_ok(good[:-1] + "A", dict(o, tm_lo=0)) is None                 # gc_clamp 1: the 3' base is A
    assert ref.single_ok(good[:-1] + "A", dict(o, tm_lo=0, gc_clamp=0)) is not None
    assert ref.single_ok(good, dict(o, gc_clamp=2)) is None                         # ..AC
    assert ref.single_ok(good, dict(o, max_end_gc=1)) is None and ref.single_ok(good, dict(o, max_end_gc=2)) == (tm, 9)
    assert ref.single_ok(good[:7] + "N" + good[8:], o) is None


def test_the_duplex_figure_on_a_case_counted_by_hand():
    """x = AAAAAAAAGC, y = AAAAAAAAGC: only G-C pairs can form; x[8..9] = GC pairs with y[8..9] = GC antiparallel
    (x[8] G - y[9] C, x[9] C - y[8] G): one run of two, holding both 3' ends.  Its Tm: step GC, terminals G and C."""
    x = "AAAAAAAAGC"
    want = ((-9800 + 200) * 10 ** 6) // (-24400 - 5600 + T.SALT_DS + T.CONC_DS)
    assert ref.duplex_figure(x, x) == (want, want)
    # the same run away from both 3' ends: any only
    assert ref.duplex_figure("AAAAGCAAAA", "AAAAGCAAAA") == (want, 0)
    # no run of two pairs at all
    assert ref.duplex_figure("AAAAAAAAAA", "CCCCCCCCCC") == (0, 0)
    # the run is read on x: x = ..GGA, y = ..TCC -> x's GGA pairs y's TCC, step GG and GA, terminals G and A
    w2 = ((-8000 - 8200 + 100 + 2300) * 10 ** 6) // (-19900 - 22200 - 2800 + 4100 + 2 * T.SALT_DS + T.CONC_DS)
    assert ref.duplex_figure("CCCCCCCGGA", "CCCCCCCTCC") == (w2, w2)


def _tmpl(left, right, D=4):
    return left + "ACGT" * (D // 4) + ref.rc(right), len(left), D, len(right)


def test_a_pair_excluded_only_by_pair_end():
    """the left primer ends in GGAGG, the right primer in CCTCC: their 3' ends pair over five bases; alone neither folds
    on itself by more than two pairs.  With --max_sec_tm between the self figures and pair_end there is no pair; above
    pair_end the pair is the answer and reports that figure."""
    left, right = "ATATATTGGAGG", "TATTATACCTCC"
    t, L, D, R = _tmpl(left, right)
    o = T.options(**dict(LOOSE, primer_size=(12, 12)))
    cl, cr = ref.candidates(t, L, D, R, o)
    a, b = cl[(0, 12)], cr[(L + D, 12)]
    assert a["seq"] == left and b["seq"] == right
    pa, pe = ref.duplex_figure(left, right)
    assert pa == pe == ref.duplex_tm("GGAGG")
    assert max(a["self_any"], a["self_end"], b["self_any"], b["self_end"]) < pe
    below = pe // 1000 - 273 - 1                                 # whole degrees Celsius under pair_end ...
    assert T.mk(below) < pe and T.mk(below) >= max(a["self_any"], b["self_any"])      # ... and above every self figure
    assert ref.design([t], L, D, R, **dict(LOOSE, primer_size=(12, 12), max_sec_tm=below))["found"][0] == 0
    r = ref.design([t], L, D, R, **dict(LOOSE, primer_size=(12, 12), max_sec_tm=below + 2))[0]
    assert r["found"] == 1 and (r["left_start"], r["left_len"], r["right_start"], r["right_len"]) == (0, 12, 16, 12)
    assert r["pair_any"] == pe and r["pair_end"] == pe and r["product_size"] == 28


def test_a_tie_goes_to_the_smallest_tuple():
    """the left flank holds the same ten bases twice: the two left primers have one Tm, one length, one penalty, and with
    one right primer the two pairs tie; the answer is the one with the smaller left_start.  (Only the last of the ten
    is G or C: with --gc_clamp 1 no window in between is a candidate.)"""
    p, q = "ATTATAATAC", "TGACCATGAG"
    t, L, D, R = p + p + "ACGT" + ref.rc(q), 20, 4, 10
    opts = dict(LOOSE, primer_size=(10, 10), gc_clamp=1)
    _, _, rows = ref.passing_pairs(t, L, D, R, T.options(**opts))
    best = min(r[0] for r in rows)
    tied = sorted(r[1:5] for r in rows if r[0] == best)
    assert tied == [(0, 10, 24, 10), (10, 10, 24, 10)] and len(rows) == 2
    r = ref.design([t], L, D, R, **opts)[0]
    assert (r["left_start"], r["left_len"], r["right_start"], r["right_len"]) == tied[0] == (0, 10, 24, 10)
    assert r["product_size"] == 34 and r["pair_penalty"] == best


def test_a_region_with_no_pair_and_the_letters_that_are_no_bases():
    assert ref.design(["A" * 28], 12, 4, 12, **LOOSE)["found"][0] == 0
    assert not ref.design(["A" * 28], 12, 4, 12, **LOOSE).tobytes().strip(b"\0")
    # an IUPAC letter removes exactly the candidates that cover it
    t = "ACGATCAGTCATGACTTGACGATC" + "ACGT" + "GATTACAGGCATCGATCGGA"
    L, D, R = 24, 4, 20
    o = T.options(**LOOSE)
    every = {(s, n) for n in (10, 11, 12) for s in range(L - n + 1)}
    left, _ = ref.candidates(t, L, D, R, o, self_check=False)
    assert set(left) == every
    left_r, right_r = ref.candidates(t[:7] + "R" + t[8:], L, D, R, o, self_check=False)
    assert set(left_r) == {(s, n) for s, n in every if not s <= 7 < s + n} and len(left_r) < len(every)
    assert set(right_r) == set(ref.candidates(t, L, D, R, o, self_check=False)[1])


def test_the_integer_tm_agrees_with_float64():
    """Tm = dH / dS in float64 with the unrounded salt and concentration terms: the integer figure lies within 1 mK (the
    floor) plus what the rounding of the two constants can move it, Tm (n / 2) / |dS|"""
    rng = random.Random(5)
    worst = 0.0
    for _ in range(2000):
        n = rng.randrange(10, 61)
        x = "".join(rng.choice("ACGT") for _ in range(n))
        pal = x == ref.rc(x)
        dh = sum(T.NN_DH[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(x, x[1:]))
        ds = float(sum(T.NN_DS[4 * T.BASES.index(a) + T.BASES.index(b)] for a, b in zip(x, x[1:])))
        for b in (x[0], x[-1]):
            dh += T.TERM_DH[T.BASES.index(b)]
            ds += T.TERM_DS[T.BASES.index(b)]
        ds += 368.0 * math.log(0.05) * (n - 1) + 1987.0 * math.log(50e-9 if pal else 50e-9 / 4) + (T.SYM_DS if pal else 0)
        tm = 1e6 * dh / ds
        bound = 1 + tm * (n / 2) / abs(ds) + 1e-6
        worst = max(worst, abs(ref.primer_tm(x) - tm) / bound)
        assert abs(ref.primer_tm(x) - tm) <= bound, (x, ref.primer_tm(x), tm, bound)
    print("largest share of the bound used:", worst)


def test_the_renderer_prints_from_the_integers():
    t = "ACGATCAGTCATGACTTGACGATC" + "ACGT" + "GATTACAGGCATCGATCGGA"
    r = ref.design([t], 24, 4, 20, **LOOSE)[0]
    assert r["found"] == 1
    f = primers.design_fields(t, r)
    assert f["left_sequence"] == t[r["left_start"]:r["left_start"] + r["left_len"]]
    assert f["right_sequence"] == ref.rc(t[r["right_start"]:r["right_start"] + r["right_len"]])
    assert f["left_tm"] == T.celsius(int(r["left_tm"])) and f["pair_penalty"] == T.milli(int(r["pair_penalty"]))
    assert f["PRIMER_RIGHT_0"] == (int(r["right_start"]) + int(r["right_len"]) - 1, int(r["right_len"]))
    marks = primers.annotate([t], f, True)[1]
    assert marks.index("└") == r["left_start"] and marks.rindex("┘") == r["right_start"] + r["right_len"] - 1
    assert "Forward" in primers.design_stats_text(f) and "Pair statistics" in primers.design_stats_text(f)


def test_a_column_of_t_and_u_designs_as_t_and_stops_the_renderer_as_without_the_option(capsys):
    from krisp_amd import amplicon
    left, diag, right = "ACGATCAGTCATGACTTGACGATC", "ACGT", "GATTACAGGCATCGATCGGA"
    dna = [amplicon.Amplicon(left, diag, right, ["a"]), amplicon.Amplicon(left, "ACGA", right, ["b"])]
    mixed = [amplicon.Amplicon(left, diag, right, ["a"]), amplicon.Amplicon(left.replace("T", "U"), diag, right, ["b"])]
    assert primers.design_template(mixed, None) == left + diag + right
    assert primers.design_template(dna, frozenset(["a"])) == left + diag + right
    rows, L, D, R = KF.design_templates([dna, mixed], ["a", "b"])
    assert (L, D, R) == (24, 4, 20) and bytes(rows[1]).decode() == left + diag + right
    recs = ref.design([bytes(r) for r in rows], L, D, R, **LOOSE)
    assert recs["found"].tolist() == [1, 1]
    csv, align = primers.render_designed([dna, mixed], ["a", "b"], recs)
    plain_csv, plain_align = amplicon.render([dna, mixed], ["a", "b"])
    # both renderers stop at the second group and keep the blocks of 1000 written before it: none
    assert csv.count("\n") == plain_csv.count("\n") == 1 and align == plain_align == ""
    assert capsys.readouterr().err.count("stops at group 2") == 2
    csv, align = primers.render_designed([dna, dna], ["a", "b"], recs)
    assert csv.count("\n") == 3 and align.count("Forward") == 4


REFUSALS = [
    (["--primer3"], "cannot be combined with --primer3"),
    (["--out_locations", "x.tsv"], "--out_locations cannot be combined with --design-primers"),
    (["--out_near", "x.tsv"], "--out_near cannot be combined with --design-primers"),
    (["--out_products", "x.tsv"], "--out_products cannot be combined with --design-primers"),
    (["--primer_size", "25", "61"], "--primer_size within 10 .. 60"),
    (["--primer_size", "9", "20"], "--primer_size within 10 .. 60"),
    (["--primer_size", "30", "25"], "--primer_size: the upper bound 25 lies below the lower bound 30"),
    (["--tm", "60", "50"], "--tm: the upper bound"),
    (["--gc", "60", "50"], "--gc: the upper bound"),
    (["--amp_size", "200", "100"], "--amp_size: the upper bound"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_every_refusal_exits_2_with_its_message(extra, message, capsys):
    """before a genome is read: the files named do not exist"""
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_ingroup.fasta", "--outgroup", "no_such_outgroup.fasta", "-c", "30", "-d", "40", "--design-primers"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "ERROR: " in err and message in err


def test_the_function_refuses_as_the_command_line_does():
    with pytest.raises(ValueError, match="within 10 .. 60"):
        KF.design_primers([], None, primer_size=(5, 20))
    with pytest.raises(ValueError, match="--gc_clamp"):
        KF.design_primers([], None, gc_clamp=40)
