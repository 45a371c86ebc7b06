"""The case set of assay_cases.py, held to what it is built for -- from the brute-force lists alone (assay_reference.py and
the two passes' references), no GPU: test_gpu_assay.py compares the device's lists with these, so none of them may be
empty where the join is meant to work, and every way in which a candidate is NOT an assay hit has to occur."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assay_cases as AC                                                    # noqa: E402
from assay_reference import interior, record_of                            # noqa: E402

NEED_ROWS = [n for n in AC.NAMES if n not in ("products_no_hit", "hits_no_product")]


def _counts(name):
    prods, hits, rows = AC.reference(name)
    return len(prods), len(hits), len(rows)


@pytest.mark.parametrize("name", NEED_ROWS)
def test_every_case_has_an_assay_hit(name):
    np_, nh, nr = _counts(name)
    print(name, "products", np_, "hits", nh, "assay hits", nr)
    assert np_ > 0 and nh > 0 and nr > 0


def test_the_text_is_a_tile_and_a_tail_and_loci_lie_across_the_edge():
    for name in AC.NAMES:
        assert AC.TILE < len(AC.case(name)["text"]) == AC.N_TEXT < 2 * AC.TILE
    for name in ("spread_m1_m2", "blocks_520"):
        _, _, rows = AC.reference(name)
        G = AC.case(name)["G"]
        assert any(r["pos"] < AC.TILE < r["pos"] + r["length"] for r in rows), name     # (a product across the edge)
        if name == "spread_m1_m2":
            assert any(r["hit_pos"] < AC.TILE < r["hit_pos"] + G for r in rows)         # (... with the guide on it)
        assert any(r["pos"] > AC.TILE for r in rows), name      # (the tail has rows of its own)


def test_all_four_strand_combinations_occur():
    seen = set()
    for name in AC.NAMES:
        _, _, rows = AC.reference(name)
        seen |= set(zip(rows["strand"].tolist(), rows["hit_strand"].tolist()))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_products_with_two_hits_hits_in_two_products_and_a_link_with_two_regions():
    two_hits = shared = False
    for name in AC.NAMES:
        _, _, rows = AC.reference(name)
        prod_keys = list(zip(rows["pos"].tolist(), rows["length"].tolist(), rows["strand"].tolist(), rows["pair"].tolist()))
        hit_keys = list(zip(rows["hit_pos"].tolist(), rows["hit_strand"].tolist(), rows["guide"].tolist()))
        two_hits |= any(prod_keys.count(k) >= 2 for k in set(prod_keys))
        shared |= any(hit_keys.count(k) >= 2 for k in set(hit_keys))
    assert two_hits and shared
    c = AC.case("spread_m1_m2")
    assert any(len(r) == 2 for r in c["link_regions"])
    # ... and its link has rows
    i = [len(r) for r in c["link_regions"]].index(2)
    _, _, rows = AC.reference("spread_m1_m2")
    assert any((int(r["pair"]), int(r["guide"])) == tuple(c["links"][i]) for r in rows)
    # a region with a pair and no guide makes no link
    assert all(p != 3 for p, _ in c["links"]) and (3, None) in c["regions"]


def test_every_reason_to_leave_a_candidate_out_occurs():
    """over the set: a hit of the product's link that lies before the product, behind it, reaches into a site, lies beyond
    a separator on another record; a hit inside the interior whose guide is no link of the pair"""
    seen = set()
    for name in AC.NAMES:
        c = AC.case(name)
        prods, hits, _ = AC.reference(name)
        linked, G, seps = set(map(tuple, c["links"])), c["G"], AC.separators(c)
        for P in prods:
            lo, hi = interior(P, AC.lengths(c))
            p0, p1 = int(P["pos"]), int(P["pos"]) + int(P["length"])
            for H in hits:
                hp = int(H["pos"])
                if hp + G <= p0 - 100 or hp >= p1 + 100:
                    continue
                inside = lo <= hp and hp + G <= hi
                if (int(P["pair"]), int(H["guide"])) not in linked:
                    if inside:
                        seen.add("no link")
                    continue
                if inside:
                    continue
                if record_of(seps, hp) != record_of(seps, p0):
                    seen.add("other record")
                elif hp + G <= p0:
                    seen.add("before the product")
                elif hp >= p1:
                    seen.add("behind the product")
                elif hp < lo:
                    seen.add("into the first site")
                else:
                    seen.add("into the second site")
    print(sorted(seen))
    assert seen == {"no link", "other record", "before the product", "behind the product", "into the first site", "into the second site"}


def test_the_block_seams():
    assert _counts("one_product") == (1, 1, 1)
    assert _counts("blocks_257") == (257, 257, 257)
    np_, nh, nr = _counts("blocks_520")
    assert np_ == nh == nr == 520 and np_ > 2 * 256


def test_products_without_a_hit_and_hits_without_a_product():
    np_, nh, nr = _counts("products_no_hit")
    assert np_ >= 40 and nh == 0 and nr == 0
    np_, nh, nr = _counts("hits_no_product")
    assert np_ == 0 and nh >= 40 and nr == 0


def test_the_last_hit_lies_in_the_last_product_and_a_product_lies_behind_every_hit():
    c = AC.case("last_hit_in_last_product")
    prods, hits, rows = AC.reference("last_hit_in_last_product")
    last_hit, last_prod = hits[-1], prods[-1]
    assert int(last_hit["pos"]) == int(hits["pos"].max()) and int(last_prod["pos"]) == int(prods["pos"].max())
    lo, hi = interior(last_prod, AC.lengths(c))
    assert lo <= int(last_hit["pos"]) and int(last_hit["pos"]) + c["G"] <= hi
    assert int(rows[-1]["hit_pos"]) == int(last_hit["pos"]) and int(rows[-1]["pos"]) == int(last_prod["pos"])
    assert len(prods) > 1 and len(hits) > len(rows)        # (hits outside every product too)
    c = AC.case("product_behind_every_hit")
    prods, hits, rows = AC.reference("product_behind_every_hit")
    assert any(interior(P, AC.lengths(c))[0] > int(hits["pos"].max()) for P in prods) and len(rows) > 0
