"""--out_assay_hits without a GPU: the brute-force reference (assay_reference.py) against hand-made lists whose
answers are written out here; the links the host builds; the orientation rule; the refusals of the command line and of the
function."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from assay_reference import ref_assay_hits                                  # noqa: E402
from guide_hits_reference import HIT                                        # noqa: E402
from primers_reference import PRODUCT                                       # noqa: E402

G = 20
LENGTHS = [(18, 24), (10, 12)]      # pair 0: a left text of 18 and a right text of 24 letters; pair 1: 10 and 12


def _products(rows):
    """(pos, length, strand, pair) -> PRODUCT, mismatch figures 0"""
    out = np.zeros(len(rows), dtype=PRODUCT)
    for i, (pos, length, strand, pair) in enumerate(rows):
        out[i]["pos"], out[i]["length"], out[i]["strand"], out[i]["pair"] = pos, length, strand, pair
    return out


def _hits(rows):
    """(pos, strand, guide) -> HIT, pam = 3"""
    out = np.zeros(len(rows), dtype=HIT)
    for i, (pos, strand, guide) in enumerate(rows):
        out[i]["pos"], out[i]["strand"], out[i]["guide"], out[i]["pam"] = pos, strand, guide, 3
    return out


def _keys(rows):
    return [(int(r["pos"]), int(r["pair"]), int(r["hit_pos"]), int(r["hit_strand"]), int(r["guide"])) for r in rows]


# ----------------------------------------------------------------------------
# the reference against hand-made lists
# ----------------------------------------------------------------------------
def test_the_ends_of_the_interior():
    """a '+' product of pair 0 at 1000 of 100 bases: its interior is [1018, 1076)"""
    P = _products([(1000, 100, 0, 0)])
    links = [(0, 7)]
    # flush with the lower end and with the upper end (1076 - 20 = 1056): both count
    got = ref_assay_hits(P, _hits([(1018, 0, 7), (1056, 1, 7)]), LENGTHS, links, G)
    assert _keys(got) == [(1000, 0, 1018, 0, 7), (1000, 0, 1056, 1, 7)]
    # one base outside either end: neither counts
    assert len(ref_assay_hits(P, _hits([(1017, 0, 7), (1057, 0, 7)]), LENGTHS, links, G)) == 0
    # wholly inside a site, across a site's edge, before and behind the product
    assert len(ref_assay_hits(P, _hits([(1000, 0, 7), (1010, 0, 7), (1070, 0, 7), (1080, 0, 7), (900, 0, 7), (1100, 0, 7)]), LENGTHS,
                              links, G)) == 0


def test_the_first_site_is_the_right_texts_on_the_minus_strand():
    """a '-' product of pair 0 at 1000 of 100 bases: rc(right) of 24 opens it, rc(left) of 18 closes it: [1024, 1082)"""
    P = _products([(1000, 100, 1, 0)])
    got = ref_assay_hits(P, _hits([(1018, 0, 7), (1023, 0, 7), (1024, 0, 7), (1062, 0, 7), (1063, 0, 7)]), LENGTHS, [(0, 7)], G)
    assert _keys(got) == [(1000, 0, 1024, 0, 7), (1000, 0, 1062, 0, 7)]


def test_a_hit_under_another_regions_link_does_not_count():
    P = _products([(1000, 100, 0, 0), (1000, 100, 0, 1)])
    H = _hits([(1030, 0, 7), (1030, 0, 8), (1030, 1, 9)])
    # pair 0 is linked with guide 7, pair 1 (interior [1010, 1088)) with guide 8; guide 9 with neither
    got = ref_assay_hits(P, H, LENGTHS, [(0, 7), (1, 8)], G)
    assert _keys(got) == [(1000, 0, 1030, 0, 7), (1000, 1, 1030, 0, 8)]
    assert len(ref_assay_hits(P, H, LENGTHS, [], G)) == 0
    # two products share the hit when both are linked with its guide
    got = ref_assay_hits(P, H, LENGTHS, [(0, 7), (1, 7)], G)
    assert _keys(got) == [(1000, 0, 1030, 0, 7), (1000, 1, 1030, 0, 7)]


def test_an_interior_of_exactly_G_bases_and_one_of_G_minus_1():
    H = _hits([(p, 0, 7) for p in range(1000, 1070)])
    # 18 + 20 + 24 = 62: the one window at 1018
    got = ref_assay_hits(_products([(1000, 62, 0, 0)]), H, LENGTHS, [(0, 7)], G)
    assert _keys(got) == [(1000, 0, 1018, 0, 7)]
    # 61: the interior [1018, 1037) holds no window of 20
    assert len(ref_assay_hits(_products([(1000, 61, 0, 0)]), H, LENGTHS, [(0, 7)], G)) == 0
    # the two sites abut: an empty interior
    assert len(ref_assay_hits(_products([(1000, 42, 0, 0)]), H, LENGTHS, [(0, 7)], G)) == 0


def test_the_record_check_and_the_carried_fields():
    P = _products([(1000, 100, 0, 0)])
    P[0]["left_mm"], P[0]["right_mm"], P[0]["left_end_mm"], P[0]["right_end_mm"] = 1, 2, 1, 0
    H = _hits([(1030, 1, 7)])
    H[0]["mismatches"], H[0]["columns"], H[0]["pam"] = 2, 0b101, 1
    got = ref_assay_hits(P, H, LENGTHS, [(0, 7)], G, seps=[500, 2000])
    assert got.tolist() == [(1000, 100, 0, 0, 1030, 1, 7, 1, 2, 1, 0, 2, 0b101, 1)]
    # (a separator between the product's start and the hit: the lists of one text never hold such a pair; the check stands)
    assert len(ref_assay_hits(P, H, LENGTHS, [(0, 7)], G, seps=[1025])) == 0
    assert len(ref_assay_hits(P, H, LENGTHS, [(0, 7)], G, seps=[1040])) == 0


# ----------------------------------------------------------------------------
# the links and the orientation
# ----------------------------------------------------------------------------
def test_assay_links():
    # pair 0: regions 0 and 3 (a shared pair); pair 1: region 1; pair 2: region 2 (no guide); pair 3: region 4
    # text 0: regions 0, 3; text 1: regions 1 and 4 (a shared protospacer); text 2: region 9 (no pair)
    links, regions = KF.assay_links([[0, 3], [1], [2], [4]], [[0, 3], [1, 4], [9]])
    assert links.dtype == np.uint32 and links.tolist() == [[0, 0], [1, 1], [3, 1]]
    assert regions == [[0, 3], [1], [4]]
    # a shared pair whose regions picked different guides: a link each
    links, regions = KF.assay_links([[0, 1]], [[1], [0]])
    assert links.tolist() == [[0, 0], [0, 1]] and regions == [[1], [0]]
    links, regions = KF.assay_links([], [[0]])
    assert links.shape == (0, 2) and regions == []
    keys = (links[:, 0].astype(np.int64) << 32) | links[:, 1]
    assert (np.diff(keys) > 0).all()


@pytest.mark.parametrize("s_d,s_p,s_h,want", [
    (0, 0, 0, "design"), (0, 0, 1, "reverse"), (0, 1, 0, "reverse"), (0, 1, 1, "design"),
    (1, 0, 0, "reverse"), (1, 0, 1, "design"), (1, 1, 0, "design"), (1, 1, 1, "reverse")])
def test_the_orientation_rule(s_d, s_p, s_h, want):
    assert KF.assay_orientation(s_d, s_p, s_h) == want


# ----------------------------------------------------------------------------
# the refusals
# ----------------------------------------------------------------------------
BASE = ["-c", "30", "-a", "100"]
ALL = BASE + ["--design-primers", "--out_guides", "g.tsv", "--out_assay_hits", "a.tsv"]
REFUSALS = [
    (BASE + ["--out_assay_hits", "a.tsv"], "--out_assay_hits needs --design-primers"),
    (BASE + ["--out_guides", "g.tsv", "--out_assay_hits", "a.tsv"], "--out_assay_hits needs --design-primers"),
    (BASE + ["--design-primers", "--out_assay_hits", "a.tsv"], "--out_assay_hits needs --out_guides"),
    (ALL + ["--primer-mismatches", "4"], "--primer-mismatches must lie between 0 and 3"),
    (ALL + ["--max-product", "149"], "--max-product must be at least the upper bound of --amp_size, 150"),
    (ALL + ["--guide-hit-mismatches", "4"], "--guide-hit-mismatches must lie between 0 and 3"),
    (ALL + ["--guide-hits-need-pam"], "--guide-hits-need-pam needs a motif"),
    (ALL + ["--guide-hit-bulges", "1"], "--guide-hit-bulges needs --out_guide_hits"),
    (BASE + ["--primer-mismatches", "1"], "--primer-mismatches needs --out_products or --out_primer_products or --out_assay_hits"),
    (BASE + ["--max-product", "500"], "--max-product needs --out_products or --out_primer_products or --out_assay_hits"),
    (BASE + ["--guide-hit-mismatches", "1"], "--guide-hit-mismatches needs --out_guide_hits or --out_assay_hits"),
    (BASE + ["--guide-hits-need-pam"], "--guide-hits-need-pam needs --out_guide_hits or --out_assay_hits"),
]


@pytest.mark.parametrize("argv,message", REFUSALS)
def test_refusals_exit_2_before_any_genome_is_read(argv, message, capsys, monkeypatch):
    for name in ("find_regions", "find_regions_multi_device", "find_regions_distributed", "design_primers", "design_guides",
                 "assay_hits"):
        monkeypatch.setattr(KF, name, lambda *a, **k: pytest.fail("no run may start"))
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fa"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and err.count("\n") == 1


def test_the_four_figures_are_taken_with_the_option_alone(monkeypatch):
    """--primer-mismatches, --max-product, --guide-hit-mismatches and --guide-hits-need-pam pass the checks with
    --out_assay_hits and neither of the two files: the run starts"""
    class Started(Exception):
        pass

    def start(*a, **k):
        raise Started()

    monkeypatch.setattr(KF, "find_regions", start)
    with pytest.raises(Started):
        KF.main(["no_such_file.fa"] + ALL + ["--primer-mismatches", "2", "--max-product", "400", "--guide-hit-mismatches", "1",
                                             "--pam3", "H", "--guide-hits-need-pam"])


def test_the_function_refuses_as_the_command_line_does():
    ok = (True, True, (70, 150), 1, 1000, 28, 2, "", "H", False)
    assert KF.assay_hits_refusal(*ok) is None
    assert "--design-primers" in KF.assay_hits_refusal(False, True, *ok[2:])
    assert "--out_guides" in KF.assay_hits_refusal(True, False, *ok[2:])
    assert KF.assay_hits_refusal(True, True, (70, 150), 1, 149, 28, 2, "", "H", False) == KF.primer_products_refusal((70, 150), 1, 149)
    assert KF.assay_hits_refusal(True, True, (70, 150), 1, 1000, 41, 2, "", "H", False) == KF.guide_hits_refusal(41, 2, "", "H", False)
    a, b, g = b"ACGTACGTACGT", b"GGATCCATTGCA", b"ACGATCAGTCATGACTTGAC"
    for kw in (dict(primer_mismatches=4), dict(guide_mismatches=4), dict(max_product=1 << 31), dict(need_pam=True)):
        with pytest.raises(ValueError):
            KF.assay_hits([a], [b], [(0, 0)], [[0]], [g], [[0]], [0], ["no_such_file.fa"], [], 20, **kw)
    with pytest.raises(ValueError, match="a pair's two primers together, 24"):
        KF.assay_hits([a], [b], [(0, 0)], [[0]], [g], [[0]], [0], ["no_such_file.fa"], [], 20, max_product=23)
    with pytest.raises(ValueError, match="--guide-size = 20"):
        KF.assay_hits([a], [b], [(0, 0)], [[0]], [g[:19]], [[0]], [0], ["no_such_file.fa"], [], 20)
    # no link: nothing to search for, no file is read
    rows = KF.assay_hits([a], [b], [(0, 0)], [[0]], [g], [[1]], [0, 0], ["no_such_file.fa"], [], 20)
    assert len(rows) == 0 and rows.dtype == KF.ASSAY_HIT


def test_the_file_has_its_header_and_a_line_per_row(tmp_path):
    rows = np.zeros(1, dtype=KF.ASSAY_HIT)
    rows[0] = (3, "a.fa", "chr1", 0, 100, 200, "+", 100, 0, 1, 0, 0, 130, 150, "-", 2, "1,5", 1, 0, "reverse", "ACGT")
    path = str(tmp_path / "a.tsv")
    KF.write_assay_hits(path, rows)
    lines = open(path).read().split("\n")
    assert lines[0] == KF.ASSAY_HIT_HEADER and len(KF.ASSAY_HIT_HEADER.split("\t")) == 21
    assert lines[1] == "3\ta.fa\tchr1\t0\t100\t200\t+\t100\t0\t1\t0\t0\t130\t150\t-\t2\t1,5\t1\t0\treverse\tACGT" and lines[2:] == [""]
