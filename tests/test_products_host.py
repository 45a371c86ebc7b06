"""--out_products on the host: the brute-force definition (products_reference.py) against hand-made texts whose answer is
written out here, the refusals of the command line and of predict_products, the parser, the TSV's text."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import amplicon
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from products_reference import ref_products, ref_sites        # noqa: E402

A = b"ACGTTGCAAC"
B = b"GGATCCTTAG"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(b):
    return b[::-1].translate(_COMP)


def sub(text, col, letter):
    assert text[col:col + 1] != letter
    return text[:col] + letter + text[col + 1:]


def u8(*texts):
    return np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(len(texts), -1)


def products(text, M, max_product=1000, omit=False, left=(A,), right=(B,), pairs=((0, 0),)):
    lf, rt = u8(*left), u8(*right)
    return [tuple(int(x) for x in r) for r in
            ref_products(text, omit, lf, rt, lf.shape[1], rt.shape[1], pairs, M, max_product).tolist()]


def sites(text, M, omit=False, left=(A,), right=(B,)):
    lf, rt = u8(*left), u8(*right)
    return [tuple(int(x) for x in r) for r in ref_sites(text, omit, lf, rt, lf.shape[1], rt.shape[1], M).tolist()]


# rows are (pos, length, strand, pair, left_mm, right_mm, left_end_mm, right_end_mm)
def test_an_insertion_in_the_diagnostic_stretch_is_a_longer_product():
    """the design's amplicon has 4 diagnostic bases (length 24); a genome with 5 or 9 there still amplifies"""
    for gap in (4, 5, 9, 0):
        text = b"TTT" + A + b"C" * gap + B + b"TTT"
        assert products(text, 0) == [(3, 20 + gap, 0, 0, 0, 0, 0, 0)], gap
        assert sites(text, 0) == [(3, 0, 0, 0), (13 + gap, 2, 0, 0)]
        # the other strand of the same text: rc(B) ... rc(A), the entries 3 and 1
        assert products(rc(text), 0) == [(3, 20 + gap, 1, 0, 0, 0, 0, 0)], gap
        assert sites(rc(text), 0) == [(3, 3, 0, 0), (13 + gap, 1, 0, 0)]


def test_mismatches_in_the_three_prime_five_and_outside_them_on_both_strands():
    a_end, a_out = sub(A, 8, b"G"), sub(A, 1, b"T")            # the 3' five of the left flank: its last columns 5 .. 9
    b_end, b_out = sub(B, 2, b"C"), sub(B, 8, b"C")            # ... of the right flank: its first columns 0 .. 4
    fwd = b"TT" + a_end + b"CC" + b_out
    rev = b"TT" + rc(a_out + b"CC" + b_end)
    text = fwd + b"\n" + rev
    assert products(text, 1) == [(2, 22, 0, 0, 1, 1, 1, 0), (27, 22, 1, 0, 1, 1, 0, 1)]
    assert products(text, 0) == []
    # the sites: A' at 2, B'' at 14; rc(B') at 27 (entry 3: its 3' five are its LAST columns), rc(A'') at 39 (entry 1: FIRST)
    assert sites(text, 1) == [(2, 0, 1, 1), (14, 2, 1, 0), (27, 3, 1, 1), (39, 1, 1, 0)]
    # two mismatches in one flank, both counted, one of them at the end
    two = sub(sub(A, 0, b"T"), 9, b"A")
    assert products(b"G" + two + B, 2) == [(1, 20, 0, 0, 2, 0, 1, 0)]
    assert products(b"G" + two + B, 1) == []
    # column 4 of the left flank and column 5 of the right one lie just outside the five
    assert products(sub(A, 4, b"A") + sub(B, 5, b"A"), 1) == [(0, 20, 0, 0, 1, 1, 0, 0)]
    assert products(sub(A, 5, b"A") + sub(B, 4, b"A"), 1) == [(0, 20, 0, 0, 1, 1, 1, 1)]


def test_a_record_separator_cuts_a_pair_and_what_lies_between_the_sites_is_not_looked_at():
    assert products(A + b"CC\nCC" + B, 1) == []
    assert sites(A + b"CC\nCC" + B, 0) == [(0, 0, 0, 0), (15, 2, 0, 0)]
    assert products(A + b"CNNnC" + B, 1) == [(0, 25, 0, 0, 0, 0, 0, 0)]
    assert products(A + b"CacgC" + B, 1, omit=True) == [(0, 25, 0, 0, 0, 0, 0, 0)]
    # an N inside a site is no mismatch: the window is no window
    assert products(sub(A, 4, b"N") + b"CC" + B, 3) == []
    assert products(A + b"CC" + sub(B, 0, b"n"), 3) == []
    # lower case is upper case unless soft-masked bases are omitted
    assert products(A.lower() + b"CC" + B, 0) == [(0, 22, 0, 0, 0, 0, 0, 0)]
    assert products(A.lower() + b"CC" + B, 0, omit=True) == []
    assert products(A + b"CC" + sub(B, 3, b"t"), 0, omit=True) == []
    # the same pair in two records: one product each, positions in the joined text
    two = b"T" + A + b"C" + B + b"\n" + A + b"GG" + B
    assert products(two, 0) == [(1, 21, 0, 0, 0, 0, 0, 0), (23, 22, 0, 0, 0, 0, 0, 0)]


def test_overlapping_sites_are_refused_and_abutting_ones_kept():
    b2 = b"CAACGGATCC"                                          # begins with the left flank's last four letters
    text = b"TT" + A[:6] + b2 + b"TT"
    assert sites(text, 0, right=(b2,)) == [(2, 0, 0, 0), (8, 2, 0, 0)]
    assert products(text, 0, right=(b2,)) == []
    assert products(b"TT" + A + b2 + b"TT", 0, right=(b2,)) == [(2, 20, 0, 0, 0, 0, 0, 0)]


def test_max_product_is_inclusive():
    text = b"G" + A + b"CCCCC" + B + b"G"
    assert products(text, 0, max_product=25) == [(1, 25, 0, 0, 0, 0, 0, 0)]
    assert products(text, 0, max_product=24) == []
    assert products(rc(text), 0, max_product=25) == [(1, 25, 1, 0, 0, 0, 0, 0)]
    assert products(rc(text), 0, max_product=24) == []


def test_flanks_of_unequal_length_regions_that_share_a_text_and_the_rows_order():
    a12 = b"ACGTTGCAACTG"
    b_other = b"CCTAGGTTAA"
    left, right = (a12, b"TTGACCAGTGCA"), (B, b_other)
    pairs = ((0, 0), (0, 1), (1, 1))                            # regions 0 and 1 share the left text
    text = b"G" + a12 + b"TT" + B + b"T" + b_other + b"\n" + rc(a12 + b"C" + b_other)
    # record 0: a12 at 1, B at 15 (length 24, pair 0), b_other at 26 (length 35, pair 1); record 1 from 37: rc(b_other) at
    # 37, rc(a12) at 48: length 23 on '-', pair 1
    assert products(text, 0, left=left, right=right, pairs=pairs) == [
        (1, 24, 0, 0, 0, 0, 0, 0), (1, 35, 0, 1, 0, 0, 0, 0), (37, 23, 1, 1, 0, 0, 0, 0)]
    assert products(text, 0, left=left, right=right, pairs=pairs, max_product=34) == [
        (1, 24, 0, 0, 0, 0, 0, 0), (37, 23, 1, 1, 0, 0, 0, 0)]
    # a pair that is no region makes no product: (1, 0) is not listed
    assert products(left[1] + B, 0, left=left, right=right, pairs=pairs) == []
    # one position, one length, both strands: '+' first -- a palindromic arrangement A .. rc(A) with B = rc(A)
    pal = A + b"CC" + rc(A)
    assert products(pal, 0, right=(rc(A),)) == [(0, 22, 0, 0, 0, 0, 0, 0), (0, 22, 1, 0, 0, 0, 0, 0)]


def test_products_refusal_and_predict_products_refuse_alike():
    assert KF.products_refusal(30, 30, 100, 1, 1000) is None
    assert KF.products_refusal(12, 12, 28, 3, 24) is None       # packed, flanks long enough
    assert KF.products_refusal(10, 16, 40, 0, 26) is None
    assert "at least 10 bases" in KF.products_refusal(25, 2, 28, 1, 1000)
    assert "at least 10 bases" in KF.products_refusal(9, 30, 60, 1, 1000)
    assert "between 0 and 3" in KF.products_refusal(30, 30, 100, 4, 1000)
    assert "between 0 and 3" in KF.products_refusal(30, 30, 100, -1, 1000)
    assert "at least the two flanks together, 60" in KF.products_refusal(30, 30, 100, 1, 59)
    assert KF.products_refusal(30, 30, 100, 1, 60) is None
    for L, R, k, M, mp in ((25, 2, 28, 1, 1000), (30, 30, 100, 4, 1000), (30, 30, 100, 1, 59)):
        with pytest.raises(ValueError):
            KF.predict_products([], ["a.fa"], [], L, R, k, mismatches=M, max_product=mp)
    assert (KF.PRODUCT_END, KF.PRODUCT_MIN_PRIMER) == (5, 10)


def test_the_parser_takes_the_three_options():
    args = KF.build_parser().parse_args(["a.fa", "-c", "30", "-a", "100", "--out_products", "p.tsv", "--primer-mismatches", "2",
                                         "--max-product", "500"])
    assert (args.out_products, args.primer_mismatches, args.max_product) == ("p.tsv", 2, 500)
    args = KF.build_parser().parse_args(["a.fa", "-c", "30", "-a", "100"])
    assert (args.out_products, args.primer_mismatches, args.max_product) == (None, None, None)


REFUSALS = [
    (["-c", "30", "-a", "100", "--out_products", "p.tsv", "--primer3"], "--out_products cannot be combined with --primer3"),
    (["-c", "30", "-a", "100", "--primer-mismatches", "1"], "--primer-mismatches needs --out_products"),
    (["-c", "30", "-a", "100", "--max-product", "500"], "--max-product needs --out_products"),
    (["-c", "30", "-a", "100", "--out_products", "p.tsv", "--primer-mismatches", "4"], "between 0 and 3"),
    (["-c", "30", "-a", "100", "--out_products", "p.tsv", "--primer-mismatches", "-1"], "between 0 and 3"),
    (["-c", "30", "-a", "100", "--out_products", "p.tsv", "--max-product", "59"], "at least the two flanks together"),
    (["--conserved-left", "25", "--conserved-right", "2", "-a", "28", "--out_products", "p.tsv"], "at least 10 bases"),
    (["-c", "9", "-a", "40", "--out_products", "p.tsv"], "at least 10 bases"),
]


@pytest.mark.parametrize("argv,message", REFUSALS)
def test_refusals_exit_2_before_any_genome_is_read(argv, message, capsys, monkeypatch):
    for name in ("find_regions", "find_regions_multi_device", "find_regions_distributed", "predict_products"):
        monkeypatch.setattr(KF, name, lambda *a, **k: pytest.fail("no run may start"))
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fa"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and err.count("\n") == 1


GROUPS = [[amplicon.Amplicon("A" * 12, "CCCC", "G" * 12, ["in0"])]]


def test_main_passes_the_options_on_and_calls_nothing_without_the_flag(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (GROUPS, {"kmers": 0, "device_s": 0.0}))
    seen = []

    def fake(groups, ing, out, L, R, k, mismatches=None, max_product=None, omit_soft=False, device=0):
        seen.append((groups, list(ing), list(out), L, R, k, mismatches, max_product, omit_soft))
        return np.empty(0, dtype=KF.PRODUCT)

    monkeypatch.setattr(KF, "predict_products", fake)
    p = tmp_path / "p.tsv"
    assert KF.main(["a.fa", "b.fa", "--outgroup", "c.fa", "-c", "12", "-a", "28", "--out_products", str(p)]) == 0
    assert seen == [(GROUPS, ["a.fa", "b.fa"], ["c.fa"], 12, 12, 28, 1, 1000, False)]
    assert p.read_text() == KF.PRODUCT_HEADER + "\n"
    assert KF.main(["a.fa", "-c", "12", "-a", "28", "--omit-soft", "--out_products", str(p), "--primer-mismatches", "0",
                    "--max-product", "24"]) == 0
    assert seen[1][6:] == (0, 24, True)
    monkeypatch.setattr(KF, "predict_products", lambda *a, **k: pytest.fail("not asked for"))
    assert KF.main(["a.fa", "-c", "12", "-a", "28"]) == 0
    capsys.readouterr()


def test_write_products_text(tmp_path):
    rows = np.empty(2, dtype=KF.PRODUCT)
    rows[0] = (0, "x/in0.fa", "chr1", 0, 5, 105, "+", 100, 0, 1, 0, 1)
    rows[1] = (3, "x/out0.fa.gz", "", 2, 0, 61, "-", 61, 2, 0, 1, 0)
    p = tmp_path / "p.tsv"
    KF.write_products(str(p), rows)
    assert KF.PRODUCT_HEADER == ("region\tfile\trecord\trecord_index\tstart\tend\tstrand\tlength\tleft_mismatches\t"
                                 "right_mismatches\tleft_end_mismatches\tright_end_mismatches")
    assert p.read_text() == (KF.PRODUCT_HEADER + "\n"
                             "0\tx/in0.fa\tchr1\t0\t5\t105\t+\t100\t0\t1\t0\t1\n"
                             "3\tx/out0.fa.gz\t\t2\t0\t61\t-\t61\t2\t0\t1\t0\n")
