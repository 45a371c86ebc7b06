"""The census of panel_clean_cases.py, without a GPU: what the sets must hold so that test_gpu_panel_clean.py, which compares
the device with the reference set by set, cannot pass on sets that ask nothing.  Fates 4 and 5 in several sets, a cross by a
later member, every planted verdict, no `single` and no `cross` product among the reference's members (DESIGN §26's
theorem), and -- for the sets that plant one -- such a product among the members of the plain selection."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_clean_cases as CC                                             # noqa: E402
import panel_clean_reference as ref                                        # noqa: E402
import panel_reference                                                     # noqa: E402
from multiplex_reference import ref_products                               # noqa: E402

NAMES = list(CC.SETS)


def kinds_among(c, positions):
    """the kinds of the products of the multiplex pass over the oligos of the members at `positions`"""
    oligos = []
    for p in positions:
        oligos += list(panel_reference.primers(c["templates"][p], c["pairs"][p]))
    texts = sorted({x.encode() for x in oligos})
    own = [[i for i, x in enumerate(oligos) if x.encode() == t] for t in texts]
    kinds = set()
    if not texts:
        return kinds
    for f in c["files"]:
        for row in ref_products(f, c["omit"], texts, c["M"], c["max_product"]):
            for i in own[row[2]]:
                for j in own[row[3]]:
                    kinds.add("single" if i == j else "pair" if i // 2 == j // 2 else "cross")
    return kinds


def test_the_sets_are_what_the_issue_asks_for():
    counts = sorted({len(CC.case(n)["templates"]) for n in NAMES})
    assert {1, 2, 65, 300} <= set(counts)
    for n in NAMES:
        c = CC.case(n)
        sizes = [len(f) for f in c["files"]]
        big = len(c["templates"]) > 16
        assert max(sizes) <= (CC.N_SHORT + 200 if big or n == "file_boundary" else CC.N_TEXT), (n, sizes)
        assert c["max_product"] >= 2 * max(max(p[1], p[3]) for p in c["pairs"])
    assert CC.N_TEXT == 50052 and CC.N_TEXT > 3 * CC.TILE


def test_fates_4_and_5_occur_in_several_sets_and_a_later_member_drops_a_cross():
    with4 = [n for n in NAMES if any(f[0] == 4 for f in CC.expected(n)[1])]
    with5 = [n for n in NAMES if any(f[0] == 5 for f in CC.expected(n)[1])]
    by2 = [n for n in NAMES if any(f[0] == 4 and f[1] >= 2 for f in CC.expected(n)[1])]
    print("fate 4:", with4, "\nfate 5:", with5, "\nby >= 2:", by2)
    assert len(with4) >= 3 and len(with5) >= 3 and len(by2) >= 1
    for n in ("random_65", "random_300", "shared_300"):                       # the large sets hold every fate but 3 at least
        fates = {f[0] for f in CC.expected(n)[1]}
        assert {1, 4, 5} <= fates, (n, fates)
    assert not CC.expected("all_self")[0] and CC.expected("all_self")[2] == [5]
    members, _, _ = CC.expected("size_above_survivors")
    assert len(members) < CC.case("size_above_survivors")["size"]
    assert CC.expected("self_first")[0][0]["position"] == 1                   # pick[0] != 0


@pytest.mark.parametrize("name", NAMES)
def test_planted_verdicts_and_the_drops_add_up(name):
    c = CC.case(name)
    members, fates, drops = CC.expected(name)
    for cand, want in c["plant"]:
        assert fates[cand] == want, (name, cand, fates[cand], want)
    assert len(drops) == 1 + len(members)
    assert drops[0] == sum(1 for f in fates if f[0] == 5)
    for j in range(len(members)):
        assert drops[1 + j] == sum(1 for f in fates if f == (4, j + 1))
        assert members[j]["dropped"] == [sum(1 for f in fates if f == (k, j + 1)) for k in (2, 3)]
    assert [m["position"] for m in members] == [i for i, f in enumerate(fates) if f[0] == 1]
    assert len(members) == c["size"] or not any(f[0] == 0 for f in fates)
    print(name, "members", len(members), "drops", drops, "fates", sorted({f[0] for f in fates}))


@pytest.mark.parametrize("name", NAMES)
def test_no_single_and_no_cross_product_among_the_members(name):
    c = CC.case(name)
    members, _, _ = CC.expected(name)
    assert kinds_among(c, [m["position"] for m in members]) <= {"pair"}


@pytest.mark.parametrize("name", [n for n in NAMES if CC.case(n)["planted_cross"]])
def test_the_plain_selection_of_a_set_with_a_planted_cross_has_one(name):
    c = CC.case(name)
    members, _ = panel_reference.select(c["templates"], c["pairs"], c["size"], c["max_sec"])
    assert kinds_among(c, [m["position"] for m in members]) & {"cross", "single"}


def test_an_empty_store_gives_the_plain_selection():
    for name in ("random_65", "clash_and_cross", "locus_and_cross"):
        c = CC.case(name)
        got = ref.select(c["templates"], c["pairs"], c["size"], c["max_sec"], [], c["omit"], c["M"], c["max_product"])
        want = panel_reference.select(c["templates"], c["pairs"], c["size"], c["max_sec"])
        assert got[:2] == want and got[2] == [0] * (1 + len(want[0]))
