"""--out_primer_products without a GPU: the brute-force definition (primers_reference.py) pinned to hand-made texts and to
products_reference.py where the lengths are uniform; the generator of test_gpu_primers.py held to what it says it plants,
from the reference's lists alone; the command line's refusals; primer_products' table and row expansion; the file."""
import os
import random
import sys

import numpy as np
import pytest

from krisp_amd import _native, amplicon, primers, reports
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primer_cases as PC                                                  # noqa: E402
import products_reference as flank_ref                                     # noqa: E402
from primers_reference import ref_products, ref_sites                      # noqa: E402

A = b"ACGTTGCAAC"                   # a left text of 10
B = b"GGATCCATTGCA"                 # a right text of 12
B10 = B[:10]


def _t(rows):
    return [tuple(r) for r in rows.tolist()]


# ----------------------------------------------------------------------------
# the reference on texts made by hand
# ----------------------------------------------------------------------------
def test_a_product_on_either_strand_with_each_entry_of_its_own_length():
    text = b"TT" + A + b"CCC" + B + b"T"
    assert _t(ref_sites(text, False, [A, B], 1, 0)) == [(2, 0, 0, 0), (15, 2, 0, 0)]
    assert _t(ref_products(text, False, [A, B], 1, [(0, 0)], 0, 100)) == [(2, 25, 0, 0, 0, 0, 0, 0)]
    back = PC.rc(text)
    assert _t(ref_sites(back, False, [A, B], 1, 0)) == [(1, 3, 0, 0), (16, 1, 0, 0)]
    assert _t(ref_products(back, False, [A, B], 1, [(0, 0)], 0, 100)) == [(1, 25, 1, 0, 0, 0, 0, 0)]


def test_end_mismatches_are_counted_in_the_primers_own_five_columns():
    def sub(t, c):
        return t[:c] + (b"A" if t[c:c + 1] != b"A" else b"C") + t[c + 1:]
    for ca, cb, want in ((9, 0, (1, 1, 1, 1)), (5, 4, (1, 1, 1, 1)), (4, 5, (1, 1, 0, 0)), (0, 11, (1, 1, 0, 0))):
        text = b"TT" + sub(A, ca) + b"CCC" + sub(B, cb) + b"T"
        assert _t(ref_products(text, False, [A, B], 1, [(0, 0)], 1, 100)) == [(2, 25, 0, 0) + want]
        assert _t(ref_products(PC.rc(text), False, [A, B], 1, [(0, 0)], 1, 100)) == [(1, 25, 1, 0) + want]
        assert len(ref_products(text, False, [A, B], 1, [(0, 0)], 0, 100)) == 0


def test_a_prefix_and_its_longer_text_are_sites_at_one_position_and_max_product_takes_each_length():
    text = b"TT" + A + b"CCC" + B + b"T"
    texts = [A, B, B10]
    assert _t(ref_sites(text, False, texts, 1, 0)) == [(2, 0, 0, 0), (15, 2, 0, 0), (15, 4, 0, 0)]
    pairs = [(0, 0), (0, 1)]
    assert _t(ref_products(text, False, texts, 1, pairs, 0, 25)) == [(2, 23, 0, 1, 0, 0, 0, 0), (2, 25, 0, 0, 0, 0, 0, 0)]
    assert _t(ref_products(text, False, texts, 1, pairs, 0, 24)) == [(2, 23, 0, 1, 0, 0, 0, 0)]
    assert _t(ref_products(text, False, texts, 1, pairs, 0, 22)) == []


def test_a_bad_byte_in_the_tail_ends_the_long_text_only():
    for bad in (b"N", b"n", b"\n"):
        text = b"TT" + A + b"CCC" + B10 + bad + B[11:] + b"T"
        # (a bad byte is no mismatch: one substitution allowed, the long text is still no site)
        assert _t(ref_sites(text, False, [A, B, B10], 1, 1)) == [(2, 0, 0, 0), (15, 4, 0, 0)]
    text = b"TT" + A + b"CCC" + B10 + b"ca" + b"T"
    assert [s[1] for s in _t(ref_sites(text, False, [A, B, B10], 1, 0))] == [0, 2, 4]
    assert [s[1] for s in _t(ref_sites(text, True, [A, B, B10], 1, 0))] == [0, 4]
    # the text's end: the window of 12 does not exist
    assert _t(ref_sites(b"TT" + B[:11], False, [A, B, B10], 1, 0)) == [(2, 4, 0, 0)]


def test_abutting_sites_pair_overlapping_ones_do_not_and_a_separator_cuts():
    assert _t(ref_products(A + B, False, [A, B], 1, [(0, 0)], 0, 22)) == [(0, 22, 0, 0, 0, 0, 0, 0)]
    a = A[:-1] + B[:1]
    assert len(ref_sites(a + B[1:], False, [a, B], 1, 0)) == 2
    assert len(ref_products(a + B[1:], False, [a, B], 1, [(0, 0)], 0, 100)) == 0
    assert len(ref_products(A + b"CC\nC" + B, False, [A, B], 1, [(0, 0)], 0, 100)) == 0
    assert len(ref_products(b"\n" + A + b"CCnC" + B + b"\n", False, [A, B], 1, [(0, 0)], 0, 100)) == 1


def test_with_uniform_lengths_it_is_the_flank_definition():
    rng = random.Random(7)
    for Le, Re in ((10, 10), (12, 30)):
        left = [bytes(rng.choice(b"ACGT") for _ in range(Le)) for _ in range(3)]
        right = [bytes(rng.choice(b"ACGT") for _ in range(Re)) for _ in range(3)]
        text = bytearray(rng.choice(b"ACGTacgtN\n") for _ in range(3000))
        for i in range(12):
            amp = left[i % 3] + bytes(rng.choice(b"ACGT") for _ in range(5 * i)) + right[(i // 2) % 3]
            text[200 * i + 50:200 * i + 50 + len(amp)] = PC.rc(amp) if i & 1 else amp
        pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (2, 0)]
        lf = np.frombuffer(b"".join(left), dtype=np.uint8).reshape(3, Le)
        rt = np.frombuffer(b"".join(right), dtype=np.uint8).reshape(3, Re)
        for M in (0, 2):
            for omit in (False, True):
                got = ref_sites(bytes(text), omit, left + right, 3, M)
                assert _t(got) == _t(flank_ref.ref_sites(bytes(text), omit, lf, rt, Le, Re, M)) and len(got) >= 12
                got = ref_products(bytes(text), omit, left + right, 3, pairs, M, 120)
                assert _t(got) == _t(flank_ref.ref_products(bytes(text), omit, lf, rt, Le, Re, pairs, M, 120)) and len(got) >= 4


# ----------------------------------------------------------------------------
# the generator, held to the reference alone
# ----------------------------------------------------------------------------
def generator_did_its_work(sites, products, name, M, omit):
    """conditions, not measurements: every length of the set has a site, every special case of primer_cases occurs or is
    absent as stated, every strand has a product without a mismatch and (M > 0) with one in each text and one at a 3' end,
    at least 10 of the 12 pairs have products, products straddle the tile edges"""
    text, left, right, pairs, marks = PC.case(name, M)
    elen = PC.entry_lengths(left, right)
    site = {(s[0], s[1]): (s[2], s[3]) for s in sites}
    prod = {r[:4]: r[4:] for r in products}
    assert len(site) == len(sites) and len(prod) == len(products)
    assert {elen[e] for _, e in site} == set(elen), (name, M)
    mixed = len(set(elen)) > 1
    assert mixed == (name != "16")
    for key in ("tail_sep", "tail_n", "tail_mismatches", "head_and_tail", "prefix", "max_product_pair", "tail_end"):
        assert (key in marks) == mixed, key
    for key in ("sep_around", "n_between", "lower_between", "abut"):
        assert prod[marks[key]] == (0, 0, 0, 0), key
    assert marks["n_inside"] not in site
    assert (marks["lower_whole"] in prod) == (not omit)
    p, w, e1, s2, e2 = marks["overlap"]
    assert (p, e1) in site and (s2, e2) in site and s2 == p + elen[e1] - 1
    assert not any(r[0] == p and r[2] == 0 and r[3] == 2 for r in products)
    assert marks["abut"][1] == elen[4] + elen[20]
    for key, col in (("end_opening", 2), ("end_closing", 3)):
        assert prod[marks[key]] == ((0, 0, 0, 0) if M == 0 else tuple(int(c in (col, col - 2)) for c in range(4))), key
    if mixed:
        for key in ("tail_sep", "tail_n"):
            p, long_e, short_e = marks[key]
            assert (p, long_e) not in site and site[(p, short_e)] == (0, 0), key
        p, e, mm = marks["tail_mismatches"]
        assert site[(p, e)][0] == mm == M
        assert marks["head_and_tail"] not in site and marks["tail_end"] not in site
        p, e_long, e_short = marks["prefix"]
        assert site[(p, e_long)] == site[(p, e_short)] == (0, 0) and elen[e_long] > elen[e_short]
        p, fits, pair_short, too_long, pair_long = marks["max_product_pair"]
        assert fits <= PC.MAX_PRODUCT == too_long - 1
        assert (p, fits, 0, pair_short) in prod and not any(r[0] == p and r[3] == pair_long for r in products)
        s2 = p + too_long - elen[16]
        assert (s2, 16) in site and (s2, 18) in site
    assert marks["last_window"] in site and marks["last_window"][0] + min(elen) == len(text)
    assert len(marks["edges"]) == 3
    for edge, pos, length, strand, pair in marks["edges"]:
        assert prod[(pos, length, strand, pair)] == (0, 0, 0, 0) and pos < edge < pos + length
        assert site[(edge - 1, 0)] == (0, 0) and elen[0] == max(elen)
    for strand in (0, 1):
        rows = [r for r in products if r[2] == strand]
        assert any(r[4] == 0 and r[5] == 0 for r in rows), (M, strand)
        if M:
            assert any(r[4] > 0 for r in rows) and any(r[5] > 0 for r in rows), (M, strand)
            assert any(r[6] > 0 or r[7] > 0 for r in rows), (M, strand)
    assert len({r[3] for r in products}) >= 10 and len(products) >= 16


@pytest.mark.parametrize("name", list(PC.LENGTH_SETS))
def test_the_generator_plants_what_it_says(name):
    assert len(PC.PAIRS) == 12 and len(set(PC.PAIRS)) == 12 and {(0, 0), (0, 1)} <= set(PC.PAIRS)
    for M in range(4):
        text, left, right, pairs, marks = PC.case(name, M)
        llen, rlen = PC.LENGTH_SETS[name]
        assert len(text) == 3 * PC.TILE + 900 and ([len(t) for t in left], [len(t) for t in right]) == (llen, rlen)
        assert set(llen) != set(rlen) or name != "10,11,37,60" or sorted(llen) != sorted(rlen)
        for omit in (False, True):
            sites, products = PC.reference(name, M, omit)
            print(name, "M", M, "omit", omit, "sites", len(sites), "products", len(products))
            generator_did_its_work(sites, products, name, M, omit)


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
DP = ["-c", "30", "-a", "100", "--design-primers", "--out_primer_products", "p.tsv"]
REFUSALS = [
    (["-c", "30", "-a", "100", "--out_primer_products", "p.tsv"], "--out_primer_products needs --design-primers"),
    (["-c", "30", "-a", "100", "--out_primer_products", "p.tsv", "--out_products", "q.tsv"],
     "--out_primer_products needs --design-primers"),
    (["-c", "30", "-a", "100", "--primer-mismatches", "1"], "--primer-mismatches needs --out_products or --out_primer_products"),
    (["-c", "30", "-a", "100", "--max-product", "500"], "--max-product needs --out_products or --out_primer_products"),
    (["-c", "30", "-a", "100", "--design-primers", "--max-product", "500"], "--max-product needs --out_products"),
    (DP + ["--primer-mismatches", "4"], "between 0 and 3"),
    (DP + ["--primer-mismatches", "-1"], "between 0 and 3"),
    (DP + ["--max-product", "149"], "--max-product must be at least the upper bound of --amp_size, 150"),
    (DP + ["--amp_size", "70", "100", "--max-product", "99"], "upper bound of --amp_size, 100"),
    (DP + ["--amp_size", "70", "1200"], "upper bound of --amp_size, 1200"),
    (DP + ["--out_products", "q.tsv"], "--out_products cannot be combined with --design-primers"),
    (DP + ["--primer3"], "cannot be combined with --primer3"),
]


@pytest.mark.parametrize("argv,message", REFUSALS)
def test_refusals_exit_2_before_any_genome_is_read(argv, message, capsys, monkeypatch):
    for name in ("find_regions", "find_regions_multi_device", "find_regions_distributed", "design_primers", "primer_products"):
        monkeypatch.setattr(KF, name, lambda *a, **k: pytest.fail("no run may start"))
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fa"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and err.count("\n") == 1


def test_the_function_refuses_as_the_command_line_does():
    assert KF.primer_products_refusal((70, 150), 1, 150) is None
    assert KF.primer_products_refusal((70, 150), 3, 1000) is None
    assert "2^31" in KF.primer_products_refusal((70, 150), 1, 1 << 31)
    for M, mp in ((4, 1000), (-1, 1000), (1, 1 << 31)):
        with pytest.raises(ValueError):
            KF.primer_products([], [], None, ["a.fa"], [], 30, 30, 100, mismatches=M, max_product=mp)
    with pytest.raises(ValueError, match="1 records for 0 groups"):
        KF.primer_products([], np.zeros(1, dtype=_native.DESIGN_RECORD), None, ["a.fa"], [], 30, 30, 100)
    assert len(KF.primer_products([], [], None, ["no_such_file.fa"], [], 30, 30, 100)) == 0


LEFT, DIAG, RIGHT = "ACGATCAGTCATGACTTGACGATC", "ACGT", "GATTACAGGCATCGATCGGA"
OTHER = "TTGATCAGTCATGACTTGACGAAA"


def _groups_and_records():
    """three regions: 0 and 2 get the same pair of texts (from different starts), 1 gets none"""
    groups = [[amplicon.Amplicon(LEFT, DIAG, RIGHT, ["in0"])], [amplicon.Amplicon(OTHER, DIAG, RIGHT, ["in0"])],
              [amplicon.Amplicon("G" + LEFT[:-1], "CCGT", RIGHT[1:] + "T", ["in0"])]]
    rec = np.zeros(3, dtype=_native.DESIGN_RECORD)
    rec[0]["found"], rec[0]["left_start"], rec[0]["left_len"], rec[0]["right_start"], rec[0]["right_len"] = 1, 2, 12, 30, 15
    rec[2]["found"], rec[2]["left_start"], rec[2]["left_len"], rec[2]["right_start"], rec[2]["right_len"] = 1, 3, 12, 29, 15
    rec["product_size"] = [43, 0, 41]
    return groups, rec


def test_primer_pairs_lists_equal_texts_and_equal_pairs_once():
    groups, rec = _groups_and_records()
    rows, L, D, R = KF.design_templates(groups, None)
    left, right, pairs, regions = KF.primer_pairs(rows, rec)
    assert left == [LEFT[2:14].encode()] and right == [RIGHT[2:17].encode()]
    assert pairs.tolist() == [[0, 0]] and regions == [[0, 1]]
    rec[2]["left_start"] = 4
    left, right, pairs, regions = KF.primer_pairs(rows, rec)
    assert left == sorted([LEFT[2:14].encode(), LEFT[3:15].encode()]) and len(right) == 1
    assert sorted(map(tuple, pairs.tolist())) == [(0, 0), (1, 0)] and sorted(regions) == [[0], [1]]


def test_the_rows_of_a_shared_pair_are_expanded_per_region(monkeypatch):
    groups, rec = _groups_and_records()
    seen = []

    class Eng:
        def primers_table(self, texts, nleft, pairs, mismatches, max_product):
            seen.append((list(texts), nleft, np.asarray(pairs).tolist(), mismatches, max_product))

        def primer_products(self, gid):
            hits = np.zeros(2, dtype=_native.PRODUCT_HIT)
            hits["pos"], hits["length"], hits["strand"], hits["left_mm"], hits["right_end_mm"] = [7, 130], [43, 50], [0, 1], [0, 1], [0, 1]
            return hits

    def scan(files, Le, De, Re, k, omit_soft, device, table):
        eng = Eng()
        table(eng)
        for fi, path in enumerate(files):
            yield eng, fi, path, False, lambda: (np.array([99], dtype=np.int64), ["chr1", "chr2"])

    monkeypatch.setattr(reports, "_scan_genomes", scan)
    rows = KF.primer_products(groups, rec, None, ["a.fa", "b.fa"], [], 24, 20, 48, mismatches=2, max_product=400)
    assert seen == [([LEFT[2:14].encode(), RIGHT[2:17].encode()], 1, [[0, 0]], 2, 400)]
    assert rows.dtype == KF.PRODUCT
    got = [tuple(r) for r in rows[["region", "file", "record", "record_index", "start", "end", "strand", "length", "left_mismatches",
                                  "right_end_mismatches"]].tolist()]
    per_file = lambda f: [(f, "chr1", 0, 7, 50, "+", 43, 0, 0), (f, "chr2", 1, 30, 80, "-", 50, 1, 1)]    # noqa: E731
    assert got == [(r,) + x for r in (0, 1) for f in ("a.fa", "b.fa") for x in per_file(f)]
    with pytest.raises(ValueError, match="at least a pair's two primers together, 27"):
        KF.primer_products(groups, rec, None, ["a.fa"], [], 24, 20, 48, max_product=26)


def test_main_passes_the_options_on_and_calls_nothing_without_the_flag(tmp_path, monkeypatch, capsys):
    groups, rec = _groups_and_records()
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (groups, {"kmers": 0, "device_s": 0.0}))
    monkeypatch.setattr(KF, "design_primers", lambda *a, **k: rec)
    monkeypatch.setattr(primers, "render_designed", lambda *a, **k: ("csv\n", ""))
    seen = []

    def fake(g, records, ingroup, ing, out, L, R, k, mismatches=None, max_product=None, omit_soft=False, device=0):
        seen.append((g, records, ingroup, list(ing), list(out), L, R, k, mismatches, max_product, omit_soft))
        return np.empty(0, dtype=KF.PRODUCT)

    monkeypatch.setattr(KF, "primer_products", fake)
    p = tmp_path / "p.tsv"
    base = ["a.fa", "b.fa", "--outgroup", "c.fa", "-c", "12", "-a", "28", "--design-primers"]
    assert KF.main(base + ["--out_primer_products", str(p)]) == 0
    assert seen[0][2:] == (["a", "b"], ["a.fa", "b.fa"], ["c.fa"], 12, 12, 28, 1, 1000, False) and seen[0][1] is rec
    assert p.read_text() == KF.PRODUCT_HEADER + "\n"
    assert KF.main(base + ["--omit-soft", "--out_primer_products", str(p), "--primer-mismatches", "0", "--max-product", "150"]) == 0
    assert seen[1][8:] == (0, 150, True)
    monkeypatch.setattr(KF, "primer_products", lambda *a, **k: pytest.fail("not asked for"))
    assert KF.main(base) == 0
    assert capsys.readouterr().out == "csv\n" * 3


def test_write_products_round_trip(tmp_path):
    rows = np.empty(2, dtype=KF.PRODUCT)
    rows[0] = (0, "x/in0.fa", "chr1", 0, 5, 105, "+", 100, 0, 1, 0, 1)
    rows[1] = (3, "x/out0.fa.gz", "", 2, 0, 61, "-", 61, 2, 0, 1, 0)
    p = tmp_path / "p.tsv"
    KF.write_products(str(p), rows)
    lines = p.read_text().split("\n")
    assert lines[0] == KF.PRODUCT_HEADER and lines[-1] == "" and len(lines) == 4
    names = KF.PRODUCT_HEADER.split("\t")
    assert names == list(KF.PRODUCT.names)
    for ln, row in zip(lines[1:-1], rows):
        assert ln.split("\t") == [str(row[n]) for n in names]
