"""The guide-hit search without a GPU: the reference (guide_hits_reference.py) on texts counted by hand; every
plant of guide_hit_cases.py in the reference's lists; the census of what the cases cover; the reference's cost; guide_texts;
the writer's columns."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_hit_cases as GC                                                # noqa: E402
import guide_hits_reference as ref                                          # noqa: E402

RECORD = np.dtype([("found", "<u4"), ("strand", "<u4"), ("start", "<u4"), ("min_mismatches", "<u4"), ("sum_mismatches", "<u4"),
                   ("gc", "<u4"), ("candidates", "<u4"), ("pad", "<u4")])


def _tuples(hits):
    return [tuple(int(h[f]) for f in ref.FIELDS) for h in hits]


# ----------------------------------------------------------------------------
# the reference by hand
# ----------------------------------------------------------------------------
GUIDE = "ACGTTGCATGCA"              # rc: TGCATGCAACGT


def test_a_hit_on_each_strand_counted_by_hand():
    #       0    5                 17      23               35
    text = "TTTC" + "G" + GUIDE + "CATAA" + "A" + "TGCATGCAACGT" + "GAAAT"
    assert text[5:17] == GUIDE and text[23:35] == ref.rc(GUIDE)
    # no motifs: both bits set
    assert _tuples(ref.ref_hits(text.encode(), False, [GUIDE], 0)) == [(5, 0, 0, 0, 0, 3), (23, 1, 0, 0, 0, 3)]
    # TTTV / H: '+' reads TTCG before the window (no TTTV) and C behind it (H); '-' reads rc(GAAA) = TTTC (TTTV) and
    # rc(A) = T behind it (H)
    assert _tuples(ref.ref_hits(text.encode(), False, [GUIDE], 0, "TTTV", "H")) == [(5, 0, 0, 0, 0, 2), (23, 1, 0, 0, 0, 3)]
    assert _tuples(ref.ref_hits(text.encode(), False, [GUIDE], 0, "TTTV", "H", need_pam=True)) == [(23, 1, 0, 0, 0, 3)]
    # the '+' window one byte later: TTTC lies before it
    shifted = text[:4] + text[5:]
    assert _tuples(ref.ref_hits(shifted.encode(), False, [GUIDE], 0, "TTTV", "H"))[0] == (4, 0, 0, 0, 0, 3)


def test_the_mask_is_in_the_guides_orientation():
    # '+': guide columns 0 and 11 substituted -> bits 0 and 11; '-': the window's FIRST column substituted is guide column 11
    plus = "C" + GUIDE[1:11] + "C"
    minus = "A" + ref.rc(GUIDE)[1:]
    text = "GG" + plus + "GGGG" + minus + "GG"
    hits = _tuples(ref.ref_hits(text.encode(), False, [GUIDE], 2))
    assert hits == [(2, 0, 0, 2, (1 << 0) | (1 << 11), 3), (18, 1, 0, 1, 1 << 11, 3)]
    assert _tuples(ref.ref_hits(text.encode(), False, [GUIDE], 1)) == [(18, 1, 0, 1, 1 << 11, 3)]
    assert ref.ref_windows(text.encode(), ref.ref_hits(text.encode(), False, [GUIDE], 2), 12) == [plus, ref.rc(minus)]


def test_bad_bytes_letters_and_the_texts_ends_by_hand():
    g = GUIDE
    # a separator, N and -- under omit -- lower case inside the window: no window; lower case without omit reads as upper
    for bad in ("\n", "N", "n"):
        assert len(ref.ref_hits((g[:5] + bad + g[6:]).encode(), False, [g], 3)) == 0
    low = g[:5] + g[5].lower() + g[6:]
    assert _tuples(ref.ref_hits(low.encode(), False, [g], 0)) == [(0, 0, 0, 0, 0, 3)] and len(ref.ref_hits(low.encode(), True, [g], 3)) == 0
    # an IUPAC letter in the window is a mismatch, in a neighbour it matches nothing; U uploaded as it is is such a letter
    assert _tuples(ref.ref_hits((g[:5] + "R" + g[6:]).encode(), False, [g], 1)) == [(0, 0, 0, 1, 1 << 5, 3)]
    assert len(ref.ref_hits((g[:5] + "R" + g[6:]).encode(), False, [g], 0)) == 0
    assert _tuples(ref.ref_hits(("R" + g + "C").encode(), False, [g], 0, "N", "H")) == [(1, 0, 0, 0, 0, 2)]
    assert _tuples(ref.ref_hits(("A" + g + "U").encode(), False, [g], 0, "N", "H")) == [(1, 0, 0, 0, 0, 1)]
    # the text's start and end, a separator, N, and lower case under omit cut a motif
    assert _tuples(ref.ref_hits(g.encode(), False, [g], 0, "N", "N")) == [(0, 0, 0, 0, 0, 0)]
    assert _tuples(ref.ref_hits(g.encode(), False, [g], 0, "", "N")) == [(0, 0, 0, 0, 0, 1)]
    assert _tuples(ref.ref_hits(("\n" + g + "N").encode(), False, [g], 0, "N", "N")) == [(1, 0, 0, 0, 0, 0)]
    assert _tuples(ref.ref_hits(("a" + g + "c").encode(), False, [g], 0, "N", "N")) == [(1, 0, 0, 0, 0, 3)]
    assert _tuples(ref.ref_hits(("a" + g + "C").encode(), True, [g], 0, "N", "N")) == [(1, 0, 0, 0, 0, 2)]
    # a palindrome is a hit on both strands; equal texts stay separate guides; a text shorter than G has no window
    pal = "ACGTACGTACGT"
    assert pal == ref.rc(pal)
    assert _tuples(ref.ref_hits(pal.encode(), False, [g, pal, pal], 0)) == [(0, 0, 1, 0, 0, 3), (0, 0, 2, 0, 0, 3), (0, 1, 1, 0, 0, 3),
                                                                          (0, 1, 2, 0, 0, 3)]
    assert len(ref.ref_hits(g[:11].encode(), False, [g], 3)) == 0 and len(ref.ref_hits(b"", False, [g], 3)) == 0
    assert len(ref.ref_hits(g.encode(), False, [], 3)) == 0


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def test_a_reference_call_stays_within_its_cost():
    worst = 0
    for name in GC.SETS:
        c = GC.case(name, 0)
        assert len(c["text"]) == GC.N_TEXT and 3 * GC.TILE < GC.N_TEXT < 4 * GC.TILE
        worst = max(worst, ref.comparisons(len(c["text"]), c["guides"]))
    for G in GC.GS:
        text, guide, _, _ = GC.dense(G, 1)
        worst = max(worst, ref.comparisons(len(text), [guide]))
    print("the dearest reference call:", worst, "byte comparisons")
    assert worst <= GC.MAX_COMPARISONS


@pytest.mark.parametrize("name", list(GC.SETS))
def test_every_plant_is_in_the_references_list(name):
    s = GC.SETS[name]
    for M in GC.MS:
        c = GC.case(name, M)
        assert len(c["guides"]) == s["nguides"] and all(len(g) == s["G"] for g in c["guides"])
        kinds = [p["kind"] for p in c["plants"]]
        assert len(set(kinds)) == len(kinds)
        for omit in (False, True):
            hits = GC.reference(name, M, omit)
            GC.check_plants(c["plants"], hits, omit)
            keys = list(zip(hits["pos"].tolist(), hits["strand"].tolist(), hits["guide"].tolist()))
            assert keys == sorted(set(keys))
            filtered = GC.reference(name, M, omit, True)
            assert _tuples(filtered) == [t for t in _tuples(hits) if t[5] == 3]
        for text, plants in GC.short_texts(name, M):
            assert len(text) <= s["G"] + 20
            for omit in (False, True):
                GC.check_plants(plants, ref.ref_hits(text, omit, c["guides"], M, c["pam5"], c["pam3"]), omit)
        assert sorted(len(t) for t, _ in GC.short_texts(name, M))[:3] == [0, 1, s["G"] - 1]
    if s["nguides"] > 1:
        gs = GC.guides(name)
        assert gs[GC.palindrome_index(name)] == ref.rc(gs[GC.palindrome_index(name)]) and gs[-1] == gs[-2]
        assert len(set(gs)) == len(gs) - 1
    if s["nguides"] >= 40:
        # 36 guides share the first G / 2 columns: a whole seed piece for M >= 1
        assert len({g[:s["G"] // 2] for g in GC.guides(name)[:36]}) == 1 and GC.pieces(s["G"], 1)[1] == s["G"] // 2


@pytest.mark.parametrize("G", GC.GS)
def test_the_dense_texts_have_their_closed_form_counts(G):
    for period in (1, 2):
        text, guide, plus, minus = GC.dense(G, period)
        for M in (0, 3):
            hits = ref.ref_hits(text, False, [guide], M)
            assert (int((hits["strand"] == 0).sum()), int((hits["strand"] == 1).sum())) == (plus, minus)
            assert not hits["mismatches"].any() and (hits["pam"] == 3).all()
            assert not ((hits["pos"] >= GC.TILE) & (hits["pos"] < 2 * GC.TILE)).any()          # a tile without a hit
            assert ((hits["pos"] >= 3 * GC.TILE).any() and (hits["pos"] < GC.TILE).any())
        assert plus > 8000 and minus > 8000


def test_the_census():
    """every (G, M, motif set, omit) occurs; per motif and strand there are hits with and without it; a hit crosses each
    interior tile edge; every edge offset occurs on both strands; both ends of the mask are set on both strands"""
    combos, edge_plants = set(), set()
    with_bit, crossing, mask_ends = set(), set(), set()
    for name, s in GC.SETS.items():
        G = s["G"]
        for M in GC.MS:
            c = GC.case(name, M)
            for p in c["plants"]:
                if p["kind"].startswith("edge"):
                    pos, strand = p["rows"][0][:2]
                    edge_plants.add((round(pos / GC.TILE), pos - round(pos / GC.TILE) * GC.TILE, strand))
            for omit in (False, True):
                combos.add((G, M, s["motifs"], omit))
                hits = GC.reference(name, M, omit)
                assert len(hits) >= 10
                for side, motif in enumerate((c["pam5"], c["pam3"])):
                    if motif:
                        for strand in (0, 1):
                            for bit in set(((hits["pam"][hits["strand"] == strand] >> side) & 1).tolist()):
                                with_bit.add((s["motifs"], side, strand, bit))
                for e in (1, 2, 3):
                    if ((hits["pos"] < e * GC.TILE) & (hits["pos"] + G > e * GC.TILE)).any():
                        crossing.add(e)
                for strand in (0, 1):
                    cols = hits["columns"][hits["strand"] == strand]
                    if (cols & np.uint64(1)).any():
                        mask_ends.add((G, strand, 0))
                    if ((cols >> np.uint64(G - 1)) & np.uint64(1)).any():
                        mask_ends.add((G, strand, G - 1))
    assert combos == {(G, M, m, o) for G in GC.GS for M in GC.MS for m in GC.MOTIFS for o in (False, True)}
    assert edge_plants == {(e, d, sd) for e in (1, 2, 3) for d in (-1, 0, 1) for sd in (0, 1)}
    assert with_bit == {(m, side, sd, bit) for m, (p5, p3) in GC.MOTIFS.items() for side, x in enumerate((p5, p3)) if x
                        for sd in (0, 1) for bit in (0, 1)}
    assert crossing == {1, 2, 3}
    assert mask_ends == {(G, sd, c) for G in GC.GS for sd in (0, 1) for c in (0, G - 1)}
    assert sorted({s["nguides"] for s in GC.SETS.values()}) == [1, 8, 40]


# ----------------------------------------------------------------------------
# guide_texts, the writer
# ----------------------------------------------------------------------------
def _records(rows):
    out = np.zeros(len(rows), dtype=RECORD)
    for i, (found, strand, start) in enumerate(rows):
        out["found"][i], out["strand"][i], out["start"][i] = found, strand, start
    return out


def test_guide_texts_on_shared_and_distinct_guides():
    proto = "CATCGATGCATG"
    t0 = "GTTTC" + proto + "TAC"                       # '+' at 5
    t1 = "AA" + ref.rc(proto) + "GGGGGG"                # '-' at 2: the same protospacer
    t2 = "ACGTACGATTACAGGCATTC"                         # '+' at 0: another one
    t3 = "T" * 20                                       # no guide
    rows = np.frombuffer((t0 + t1 + t2 + t3).encode(), dtype=np.uint8).reshape(4, 20)
    recs = _records([(1, 0, 5), (1, 1, 2), (1, 0, 0), (0, 0, 0)])
    texts, regions = KF.guide_texts(rows, recs, 12)
    assert texts == [b"ACGTACGATTAC", proto.encode()] and regions == [[2], [0, 1]]
    # the numbering of --design-primers: a region is named by its rank among the regions with a pair
    texts, regions = KF.guide_texts(rows, recs, 12, regions=[0, 0, 1, 2])
    assert regions == [[1], [0, 0]]
    texts, regions = KF.guide_texts(rows[[3, 1, 3, 2]], recs[[3, 1, 3, 2]], 12, regions=np.array([-1, 0, 0, 1]))
    assert texts == [b"ACGTACGATTAC", proto.encode()] and regions == [[1], [0]]
    assert KF.guide_texts(rows[:0], recs[:0], 12) == ([], []) and KF.guide_texts(rows[3:], recs[3:], 12) == ([], [])


def test_write_guide_hits_columns(tmp_path):
    rows = np.zeros(3, dtype=KF.GUIDE_HIT)
    rows[0] = (0, "a.fasta", "chr1", 0, 5, 33, "+", 0, "-", 1, 1, "A" * 28)
    rows[1] = (0, "a.fasta", "chr1 second", 1, 7, 35, "-", 2, "1,28", 0, 1, "C" + "A" * 26 + "C")
    rows[2] = (3, "b.fasta.gz", "r", 0, 0, 28, "+", 1, "14", 1, 0, "U" * 28)
    p = str(tmp_path / "h.tsv")
    KF.write_guide_hits(p, rows)
    lines = open(p).read().split("\n")
    assert lines[0] == KF.GUIDE_HIT_HEADER
    assert lines[0].split("\t") == ["region", "file", "record", "record_index", "start", "end", "strand", "mismatches",
                                    "mismatch_columns", "pam5_match", "pam3_match", "sequence"]
    assert lines[1] == "0\ta.fasta\tchr1\t0\t5\t33\t+\t0\t-\t1\t1\t" + "A" * 28
    assert lines[2] == "0\ta.fasta\tchr1 second\t1\t7\t35\t-\t2\t1,28\t0\t1\tC" + "A" * 26 + "C"
    assert lines[3] == "3\tb.fasta.gz\tr\t0\t0\t28\t+\t1\t14\t1\t0\t" + "U" * 28 and lines[4:] == [""]
    KF.write_guide_hits(p, rows[:0])
    assert open(p).read() == KF.GUIDE_HIT_HEADER + "\n"
    assert KF._mask_columns(0) == "-" and KF._mask_columns((1 << 39) | 1) == "1,40" and KF._mask_columns(0b1010) == "2,4"
