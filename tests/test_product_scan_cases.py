"""The census of product_scan_cases.cases, the generator test_gpu_product_scan_properties.py draws its random cases from: with
the brute-force references alone (products_reference.py, primers_reference.py) it asserts what the default seeds cover, so
that an edit of the generator cannot hollow out the GPU comparison unnoticed, and that the references list what the
generator planted.  Nothing here needs a GPU.  KR_PRODSCAN_SEEDS sets the number of seeds (default: every length set with
every M once)."""
import functools
import os
import sys
from bisect import bisect_left, bisect_right

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import product_scan_cases as PS                                            # noqa: E402

TILE = PS.TILE
BLOCK = 256                         # sites of a join block (LOC_T)
N_SEEDS = int(os.environ.get("KR_PRODSCAN_SEEDS", str(PS.SEEDS)))
KINDS = ("flank", "primer")


@functools.lru_cache(maxsize=None)
def census(kind):
    """every case of the pass with its reference lists -> [(case, sites, products)]: computed once"""
    out = []
    for seed in range(N_SEEDS):
        c = PS.cases(seed)[kind]
        sites, prods = PS.reference(c, c["text"])
        out.append((c, sites, prods))
    return out


def closing_length(c, row):
    i, j = c["pairs"][row[3]]
    return len(c["left"][i]) if row[2] else len(c["right"][j])


def test_the_default_seeds_cover_every_length_set_with_every_M():
    assert PS.SEEDS == 4 * len(PS.PRIMER_SETS) >= 4 * len(PS.FLANK_SETS)
    assert PS.FLANK_SETS[-1] == (256, 256)
    for kind in KINDS:
        seen = {(c["set"], c["M"]) for c, _, _ in census(kind)}
        sets = {s for s, _ in seen}
        assert len(sets) == (len(PS.FLANK_SETS) if kind == "flank" else len(PS.PRIMER_SETS)), sets
        assert all((s, M) in seen for s in sets for M in range(4))
        assert {c["omit"] for c, _, _ in census(kind)} == {False, True}


def test_nothing_is_compared_against_an_empty_list():
    for kind in KINDS:
        for M in range(4):
            rows = [r for c, _, p in census(kind) if c["M"] == M for r in p]
            for strand in (0, 1):
                assert any(r[2] == strand and r[4] == 0 and r[5] == 0 for r in rows), (kind, M, strand)
                if M:
                    assert any(r[2] == strand and r[4] + r[5] > 0 for r in rows), (kind, M, strand)
        rows = [r for _, _, p in census(kind) for r in p]
        assert any(r[6] > 0 for r in rows) and any(r[7] > 0 for r in rows), kind       # end mismatches on both sides
        assert sum(len(s) > 0 for _, s, _ in census(kind)) >= N_SEEDS - 3
        assert sum(len(p) > 0 for _, _, p in census(kind)) >= N_SEEDS - 3


def test_the_references_list_what_was_planted():
    for kind in KINDS:
        listed = absent = 0
        for c, sites, prods in census(kind):
            have = {r[:6] for r in prods}
            for pl in c["plants"]:
                row = (pl["pos"], pl["length"], pl["strand"], pl["pair"], pl["ml"], pl["mr"])
                if pl["expect"]:
                    assert row in have, (kind, c["seed"], pl)
                    listed += 1
                elif pl["ml"] > c["M"] or pl["mr"] > c["M"] or pl["length"] > c["max_product"]:
                    assert row not in have, (kind, c["seed"], pl)
                    absent += 1
        print(kind, "plants listed", listed, "absent", absent)
        assert listed >= 6 * N_SEEDS and absent >= 3 * N_SEEDS


def test_sites_straddle_every_interior_tile_edge_in_each_class_and_orientation():
    """over the cases together: one site at most lies across an edge of one text, so a case has one kind there; the seeds'
    union holds every (edge, length class, orientation)"""
    for kind in KINDS:
        seen = set()
        for c, sites, _ in census(kind):
            lens = PS.entry_lengths(c)
            nl2 = 2 * len(c["left"])
            for pos, e, _, _ in sites:
                edge = (pos + lens[e] - 1) // TILE
                if edge != pos // TILE:
                    cls = (e >= nl2) if kind == "flank" else (lens[e] > c["smin"])
                    seen.add((edge, cls, e & 1))
        want = {(edge, cls, o) for edge in (1, 2) for cls in (False, True) for o in (0, 1)}
        assert want <= seen, (kind, sorted(want - seen))


def test_products_whose_sites_lie_in_different_tiles_and_join_blocks():
    for kind in KINDS:
        tiles = blocks = many = 0
        for c, sites, prods in census(kind):
            pos = [s[0] for s in sites]                         # (ascending: kr_*_sites lists the sites in position order)
            many += len(sites) > BLOCK
            for r in prods:
                s1, s2 = r[0], r[0] + r[1] - closing_length(c, r)
                tiles += s1 // TILE != s2 // TILE
                # whatever the order of the sites of one position: the opening site's block lies before the closing site's
                blocks += (bisect_right(pos, s1) - 1) // BLOCK < bisect_left(pos, s2) // BLOCK
        print(kind, "products across tiles", tiles, "across join blocks", blocks, "cases over a block of sites", many)
        assert tiles >= 3 and blocks >= 10 and many >= 3


def test_sites_at_window_0_and_at_the_last_window():
    for kind in KINDS:
        first = last = 0
        for c, sites, _ in census(kind):
            lens = PS.entry_lengths(c)
            first += any(s[0] == 0 for s in sites)
            last += any(s[0] == len(c["text"]) - lens[s[1]] for s in sites)
        assert first >= 3 and last >= 3, (kind, first, last)


def test_the_exact_max_product_row_and_the_absent_row_one_longer():
    for kind in KINDS:
        exact = over = 0
        for c, sites, prods in census(kind):
            exact += any(r[1] == c["max_product"] for r in prods)
            assert all(r[1] <= c["max_product"] for r in prods)
            at = {(s[0], s[1]) for s in sites}
            nl2 = 2 * len(c["left"])
            for pl in c["plants"]:
                if pl["length"] == c["max_product"] + 1 and pl["ml"] <= c["M"] and pl["mr"] <= c["M"]:
                    i, j = c["pairs"][pl["pair"]]
                    e1, e2 = (2 * i, nl2 + 2 * j) if pl["strand"] == 0 else (nl2 + 2 * j + 1, 2 * i + 1)
                    n2 = len(c["left"][i]) if pl["strand"] else len(c["right"][j])
                    # both sites are there: the length alone keeps the row out
                    over += (pl["pos"], e1) in at and (pl["pos"] + pl["length"] - n2, e2) in at
        assert exact >= 5 and over >= 5, (kind, exact, over)


def test_tails_ended_by_each_kind_of_bad_byte():
    seen = {}
    for c, sites, _ in census("primer"):
        text, smin = c["text"], c["smin"]
        at = {(s[0], s[1]) for s in sites}
        texts = c["left"] + c["right"]
        for t in c["tails"]:
            p, e, col = t["pos"], t["entry"], t["col"]
            x = texts[e >> 1] if e % 2 == 0 else PS.rc(texts[e >> 1])
            w = text[p:p + len(x)]
            up = np.where((w >= 97) & (w <= 122), w - 32, w)
            bad = (w == 10) | (w == ord("N")) | (w == ord("n")) | ((w >= 97) & c["omit"])
            # the seeded columns are valid and equal, the columns before `col` hold no bad byte and no mismatch: the
            # comparison reaches the bad byte
            assert not bad[:col].any() and (up[:col] == np.frombuffer(x, dtype=np.uint8)[:col]).all() and col >= smin
            if t["kind"] == "end":
                assert p + col == len(text)
            else:
                assert w[col] == {"\n": 10, "N": ord("N"), "lower": np.frombuffer(x, dtype=np.uint8)[col] | 0x20}[t["kind"]]
            ended = t["kind"] != "lower" or c["omit"]
            assert ((p, e) in at) != ended, (c["seed"], t)
            seen[(t["kind"], ended)] = seen.get((t["kind"], ended), 0) + 1
    print(seen)
    for what in (("\n", True), ("N", True), ("lower", True), ("lower", False), ("end", True)):
        assert seen.get(what, 0) >= 2, (what, seen)


def test_tables_separators_and_alphabets():
    for kind in KINDS:
        cs = [c for c, _, _ in census(kind)]
        sizes = {len(c["right"]) for c in cs}
        assert {1, 4, 300, 3000} <= sizes and any(4 < s <= 30 for s in sizes), sizes
        assert len({c["alphabet"] for c in cs if len(c["text"]) > 1000}) == len(PS.ALPHABETS) == 7
        crowded = [(c, p) for c, _, p in census(kind) if int((c["text"] == 10).sum()) >= 2000]
        assert crowded and all(len(p) > 0 for _, p in crowded)
        # pairs of every kind: shared lefts and rights, a left text that is a right text, a palindrome
        assert any(c["left"][1] == c["right"][1] for c in cs if len(c["right"]) >= 4)
        assert any(c["left"][2] == PS.rc(c["left"][2]) for c in cs if len(c["right"]) >= 4)
        assert any((0, 1) in c["pairs"] and (1, 0) in c["pairs"] for c in cs)
    # the primer pass: 1 to 40 texts under one seed; a table whose shortest text no pair names, and an opening site from
    # which no closing site is in reach (first > last in prim_walk)
    shared = sorted(len(c["shared"]) for c, _, _ in census("primer") if c["shared"])
    assert shared and shared[0] <= 3 and shared[-1] >= 8, shared
    unreachable = 0
    for c, sites, _ in census("primer"):
        lens = PS.entry_lengths(c)
        named = {len(c["left"][i]) for i, _ in c["pairs"]} | {len(c["right"][j]) for _, j in c["pairs"]}
        if c["smin"] < min(named):
            nl2 = 2 * len(c["left"])
            unreachable += sum(1 for s in sites if ((s[1] < nl2) != bool(s[1] & 1)) and lens[s[1]] + c["smin"] > c["max_product"])
    assert unreachable >= 2, unreachable
