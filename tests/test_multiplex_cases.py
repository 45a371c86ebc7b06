"""The census of multiplex_cases.py, with the reference (multiplex_reference.py) alone: every plant is a row of the
brute-force list or an absent row as intended, every kind, M, T and length set occurs, sites cross each interior tile edge,
products cross an edge of the join's blocks, an opening site is site number 255 of its block, both values of the tally's
`clean` occur -- so test_gpu_multiplex.py compares the device against lists that hold what the generator set out to plant.
And the reference is pinned to primers_reference.py: for the table read as disjoint members (2 m, 2 m + 1) the (mL, mR)
products are that reference's '+' products of pair m and the (mR, mL) products its '-' products, field for field."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiplex_cases as MC                                               # noqa: E402
from multiplex_reference import rc, ref_products, ref_sites, ref_tally    # noqa: E402


def _rows(prods):
    return {p[:4] for p in prods}


@pytest.mark.parametrize("name,T,M", MC.CASES)
def test_every_plant_is_a_row_or_an_absent_row_as_intended(name, T, M):
    text, texts, marks = MC.case(name, T, M)
    for omit in (False, True):
        sites, prods = MC.reference(name, T, M, omit)
        rows, full, at = _rows(prods), set(prods), {s[:2] for s in sites}
        assert len(sites) > 0 and len(prods) > 0
        for key, m in marks.items():
            if not (isinstance(m, tuple) and isinstance(m[0], str)):
                continue
            want = m[0] == "row" or (m[0] == "row unless omit" and not omit)
            assert (tuple(m[1:5]) in rows) == want, (key, m, omit)
            if len(m) > 5:                                              # the end mismatches of either side
                assert any(p[:4] == tuple(m[1:5]) and p[6:] == tuple(m[5:]) for p in prods), (key, m)
        for pos, w, a, b, ma, mb, end_a, end_b in marks["spread"]:
            row = (pos, w, a, b, ma, mb, ma if end_a else 0, mb if end_b else 0)
            assert (row in full) == (ma <= M and mb <= M), (row, omit)
        for key in ("diverging_sites", "overlap_sites", "palindrome_sites"):
            for s in marks.get(key, ()):
                assert s in at, (key, s)
        for key in ("tail_sep", "tail_n"):
            if key in marks:
                p, long_entry, short_entry = marks[key]
                assert (p, long_entry) not in at and (p, short_entry) in at, key
        if "tail_lower" in marks:
            assert (marks["tail_lower"] in at) == (not omit)
        for edge, row, site in marks["edges"]:
            assert row[1:] in rows and site in at and site[0] < edge < site[0] + len(texts[site[1] // 2])
            assert row[1] < edge < row[1] + row[2]
        assert marks["last_window"] in at and marks["last_window"][0] + min(map(len, texts)) == len(text)


@pytest.mark.parametrize("name,T,M", [c for c in MC.CASES if "block_255" in MC.case(*c)[2]])
def test_products_cross_the_edges_of_the_join_blocks(name, T, M):
    text, texts, marks = MC.case(name, T, M)
    for omit in (False, True):
        sites, prods = MC.reference(name, T, M, omit)
        pos = [s[0] for s in sites]
        _, p, w, a, b = marks["block_255"]
        # the probe's opening site stands alone at its position: its number in the list is the device's too
        assert pos.count(p) == 1 and sites[pos.index(p)][1] == 2 * a
        assert pos.index(p) % MC.BLOCK == MC.BLOCK - 1
        assert (p, w, a, b) in _rows(prods) and pos.index(p + w - len(texts[b])) // MC.BLOCK == pos.index(p) // MC.BLOCK + 1
        # the row of abutting products: some product's opening site lies in one block for certain, its closing site in the next
        at, n = marks["crowd"]
        import bisect
        crossing = 0
        for s1, length, fa, fb in _rows(prods):
            if at <= s1 < at + n * (len(texts[a]) + len(texts[b]) + 2):
                s2 = s1 + length - len(texts[fb])
                last_of_s1 = bisect.bisect_right(pos, s1) - 1           # the greatest number a site at s1 can have
                first_of_s2 = bisect.bisect_left(pos, s2)               # the least a site at s2 can have
                crossing += last_of_s1 // MC.BLOCK < first_of_s2 // MC.BLOCK
        assert crossing > 0


def test_every_kind_distance_table_size_and_length_set_occurs():
    seen_kinds, clean = {}, {}
    for name, T, M in MC.CASES:
        _, prods = MC.reference(name, T, M, False)
        for p in prods:
            seen_kinds.setdefault((T, MC.kind(p[2], p[3])), 0)
            seen_kinds[(T, MC.kind(p[2], p[3]))] += 1
            clean.setdefault(M, set()).add(p[6] == 0 and p[7] == 0)
        tally = ref_tally(prods, T)
        assert sum(c for row in tally for cell in row for c in cell) == len(prods)
    assert {c[0] for c in MC.CASES} == set(MC.LENGTH_SETS)
    assert {c[1] for c in MC.CASES} == {1, 2, 16, 128} and {c[2] for c in MC.CASES} == {0, 1, 2, 3}
    for T in (16, 128):
        assert all(seen_kinds.get((T, k), 0) > 0 for k in ("pair", "single", "cross")), seen_kinds
    assert seen_kinds[(2, "pair")] > 0 and seen_kinds[(2, "single")] > 0 and seen_kinds[(1, "single")] > 0
    # both readings of a planted combination: (a, b) and (b, a)
    for name, T, M in MC.CASES:
        rows = {p[2:4] for p in MC.reference(name, T, M, False)[1]}
        for a, b in MC.case(name, T, M)[2]["combos"]:
            if T <= 16:
                assert (a, b) in rows and (b, a) in rows, (name, T, M, a, b)
    assert clean[0] == {True} and all(clean[M] == {True, False} for M in (1, 2, 3))


@pytest.mark.parametrize("name,T,M", [("16", 16, 1), ("10-14", 16, 2), ("10,60", 2, 1), ("18-24", 16, 3)])
def test_the_member_products_are_the_primer_references(name, T, M):
    from primers_reference import ref_products as prim_products
    text, texts, _ = MC.case(name, T, M)
    left, right = texts[0::2], [rc(t) for t in texts[1::2]]      # (a right text: the template's text under the right primer)
    pairs = [(m, m) for m in range(T // 2)]
    for omit in (False, True):
        _, prods = MC.reference(name, T, M, omit)
        want = prim_products(text, omit, left + right, len(left), pairs, M, MC.MAX_PRODUCT).tolist()
        plus = sorted((p[0], p[1], p[2] // 2, p[4], p[5], p[6], p[7]) for p in prods if p[2] % 2 == 0 and p[3] == p[2] + 1)
        minus = sorted((p[0], p[1], p[3] // 2, p[5], p[4], p[7], p[6]) for p in prods if p[3] % 2 == 0 and p[2] == p[3] + 1)
        # primers_reference: (pos, length, strand, pair, left_mm, right_mm, left_end_mm, right_end_mm)
        assert plus == sorted((w[0], w[1], w[3], w[4], w[5], w[6], w[7]) for w in want if w[2] == 0) and len(plus) > 0
        assert minus == sorted((w[0], w[1], w[3], w[4], w[5], w[6], w[7]) for w in want if w[2] == 1) and len(minus) > 0


def test_the_reference_on_texts_made_by_hand():
    a, b = b"ACGTTGCAAGGC", b"TTGACCATGGAT"
    text = a + b"CC" + rc(b) + b"\n" + a + rc(b)[:5] + b"\n" + rc(b) + b"GG" + a + b"N" + a + rc(a)
    sites = ref_sites(text, False, [a, b], 0)
    assert sites == [(0, 0, 0, 0), (14, 3, 0, 0), (27, 0, 0, 0), (45, 3, 0, 0), (59, 0, 0, 0), (72, 0, 0, 0), (84, 1, 0, 0)]
    assert ref_products(text, False, [a, b], 0, 100) == [
        (0, 26, 0, 1, 0, 0, 0, 0), (59, 37, 0, 0, 0, 0, 0, 0), (72, 24, 0, 0, 0, 0, 0, 0)]     # (an N between two sites is no bar)
    assert ref_products(text, False, [a, b], 0, 25) == [(72, 24, 0, 0, 0, 0, 0, 0)]
    # one substitution in the last five columns of a as written, one in the first five of rc(b): the 3' ends of both
    t2 = a[:-2] + b"T" + a[-1:] + rc(b)[:1] + b"A" + rc(b)[2:]
    assert ref_products(t2, False, [a, b], 1, 100) == [(0, 24, 0, 1, 1, 1, 1, 1)]
    assert ref_products(t2.lower(), True, [a, b], 1, 100) == [] and len(ref_products(t2.lower(), False, [a, b], 1, 100)) == 1
