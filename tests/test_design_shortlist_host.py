"""The host side of --primer-candidates without a GPU (krisp_amd/reports.py): pick_pairs against the plain loops of
design_shortlist_reference.py on random tallies, shortlist_pairs' table, the writer, and the shape facts of design_cases.py
that test_gpu_design_shortlist.py relies on for the list's edges."""
import os
import random
import sys
from collections import Counter

import numpy as np
import pytest

from krisp_amd import reports
from krisp_amd._native import DESIGN_RECORD, DESIGN_RECORD_HP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_cases                                                        # noqa: E402
import design_shortlist_reference as SR                                    # noqa: E402


def _random_shortlist(rng, n, top, dtype=DESIGN_RECORD):
    """n regions with 0 .. top filled slots each (the filled slots first, as the device writes them), ranks told apart by
    their penalty; -> (shortlist, index into `pairs` tallies, number of pairs)"""
    shortlist = np.zeros((n, top), dtype=dtype)
    index = np.full((n, top), -1, dtype=np.int64)
    npairs = max(1, n * top // 2)                   # (slots share pairs)
    for i in range(n):
        for j in range(min(top, rng.choice([0, 0, 1, 2, top - 1, top, top]))):
            shortlist[i, j]["found"] = 1
            shortlist[i, j]["pair_penalty"] = 1000 * i + j
            index[i, j] = rng.randrange(npairs)
    return shortlist, index, npairs


@pytest.mark.parametrize("M", [0, 1, 2, 3])
@pytest.mark.parametrize("top", [1, 2, 8])
def test_pick_pairs_equals_the_plain_loops(M, top):
    """random tallies drawn from few values, so that ties in every prefix of (clean, t0, ..., t2M) occur; counts above 2^32;
    garbage in the columns above 2 M, which the pick must not read; regions without a pair; empty slots"""
    rng = random.Random(100 * M + top)
    n = 300
    shortlist, index, npairs = _random_shortlist(rng, n, top)
    values = [0, 0, 1, 2, (1 << 32) + 5, (1 << 33), (1 << 40) + 1]
    # a pool of 12 tallies, each its forerunner with one column redrawn: whole tallies and every prefix of them tie
    cols = list(range(2 * M + 1)) + [7]
    pool = [{m: rng.choice(values) for m in cols}]
    for _ in range(11):
        pool.append({**pool[-1], rng.choice(cols): rng.choice(values)})
    tallies = np.zeros((npairs, 8), dtype=np.uint64)
    for p in range(npairs):
        for m, v in rng.choice(pool).items():
            tallies[p, m] = v
        for m in range(2 * M + 1, 7):
            tallies[p, m] = rng.randrange(1 << 50)              # garbage
    records, ranks, picked = reports.pick_pairs(shortlist, index, tallies, M)
    want = SR.pick_all(shortlist["found"], index, tallies, M)
    assert ranks.tolist() == want
    assert records.dtype == shortlist.dtype and records.tobytes() == shortlist[np.arange(n), want].tobytes()
    assert picked.shape == (n, 2 * M + 2) and picked.dtype == np.uint64
    for i in range(n):
        if index[i, 0] < 0:
            assert int(records[i]["found"]) == 0 and ranks[i] == 0 and not picked[i].any()
        else:
            assert tuple(picked[i].tolist()) == SR.tally_key(tallies[index[i, want[i]]], M)
    if top > 1:
        filled = (index >= 0).sum(axis=1)
        assert (ranks > 0).any() and ((ranks == 0) & (filled > 1)).any() and (filled == 0).any() and (filled == top).any()
        # a tie goes to the lower rank: some region's picked tally is shared by a later slot
        keys = [[SR.tally_key(tallies[index[i, j]], M) for j in range(int(filled[i]))] for i in range(n)]
        assert any(k.count(k[r]) > 1 and k.index(k[r]) == r for k, r in zip(keys, want) if k)


def test_pick_pairs_keeps_the_hairpin_figures_and_takes_no_region():
    shortlist = np.zeros((2, 3), dtype=DESIGN_RECORD_HP)
    shortlist["found"][0, :2] = 1
    shortlist["left_hairpin"][0] = [11, 22, 0]
    index = np.array([[0, 1, -1], [-1, -1, -1]])
    tallies = np.array([[3, 0, 0, 0, 0, 0, 0, 1], [9, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint64)
    records, ranks, picked = reports.pick_pairs(shortlist, index, tallies, 0)
    assert ranks.tolist() == [1, 0] and records["left_hairpin"].tolist() == [22, 0] and picked.tolist() == [[0, 9], [0, 0]]
    none = reports.pick_pairs(np.zeros((0, 4), dtype=DESIGN_RECORD), np.zeros((0, 4), dtype=np.int64), np.zeros((0, 8), dtype=np.uint64), 1)
    assert [len(x) for x in none] == [0, 0, 0] and none[2].shape == (0, 4)


def _slot(rec, ls, ln, rs, rn):
    rec["found"], rec["left_start"], rec["left_len"], rec["right_start"], rec["right_len"] = 1, ls, ln, rs, rn
    rec["product_size"] = rs + rn - ls


def test_shortlist_pairs_lists_equal_texts_and_pairs_once():
    rng = random.Random(7)
    W = 70
    t0 = "".join(rng.choices("ACGT", k=W))
    t1 = t0[:30] + "".join(rng.choices("ACGT", k=10)) + t0[40:]     # the neighbouring region: the same flanks
    t2 = "".join(rng.choices("ACGT", k=W))
    t3 = "".join(rng.choices("ACGT", k=W))
    templates = np.frombuffer((t0 + t1 + t2 + t3).encode(), dtype=np.uint8).reshape(4, W)
    shortlist = np.zeros((4, 3), dtype=DESIGN_RECORD)
    _slot(shortlist[0, 0], 2, 12, 50, 14)
    _slot(shortlist[0, 1], 2, 12, 51, 13)           # shares its left primer with rank 1
    _slot(shortlist[0, 2], 2, 13, 50, 14)           # a left text that its prefix sorts before
    _slot(shortlist[1, 0], 2, 12, 50, 14)           # region 0's pair of rank 1 once more
    _slot(shortlist[1, 1], 5, 10, 50, 14)
    _slot(shortlist[3, 0], 0, 60, 10, 60)           # (region 2 has no pair; the longest texts, overlapping)
    left, right, pairs, index = reports.shortlist_pairs(templates, shortlist)
    want_left = sorted({t0[2:14].encode(), t0[2:15].encode(), t0[5:15].encode(), t3[0:60].encode()})
    want_right = sorted({t0[50:64].encode(), t0[51:64].encode(), t3[10:70].encode()})
    assert left == want_left and right == want_right
    assert pairs.dtype == np.uint32 and pairs.tolist() == [list(p) for p in sorted(set(map(tuple, pairs.tolist())))] and len(pairs) == 5
    assert index.dtype == np.int64 and index.shape == (4, 3)
    assert index[0, 0] == index[1, 0] and len(set(index[index >= 0].tolist())) == 5
    assert (index < 0).tolist() == [[False] * 3, [False, False, True], [True] * 3, [False, True, True]]
    for i in range(4):
        for j in range(3):
            if index[i, j] >= 0:
                r, (a, b) = shortlist[i, j], pairs[index[i, j]]
                row = bytes(templates[i])
                assert left[a] == row[int(r["left_start"]):int(r["left_start"]) + int(r["left_len"])]
                assert right[b] == row[int(r["right_start"]):int(r["right_start"]) + int(r["right_len"])]
    # the table is primer_pairs' where every region has one slot
    l1, r1, p1, regions = reports.primer_pairs(templates, shortlist[:, 0])
    l2, r2, p2, i2 = reports.shortlist_pairs(templates, shortlist[:, :1])
    assert (l1, r1, p1.tolist()) == (l2, r2, p2.tolist())
    assert [i2[i, 0] for i in (0, 1, 3)] == [next(p for p, rr in enumerate(regions) if k in rr) for k in range(3)]
    # nothing filled; a letter the table does not take
    e = reports.shortlist_pairs(templates, np.zeros((4, 2), dtype=DESIGN_RECORD))
    assert e[0] == [] and e[1] == [] and e[2].shape == (0, 2) and (e[3] == -1).all()
    bad = templates.copy()
    bad[0, 5] = ord("N")
    with pytest.raises(ValueError, match="other than A, C, G, T"):
        reports.shortlist_pairs(bad, shortlist)


def test_shortlist_pairs_has_no_loop_over_the_regions():
    """8 slots of 20 000 regions, nearly all of them distinct pairs: the table is right at that size and comes in a fraction
    of a second (0.3 s where this was written; the bound leaves a loaded machine room)"""
    import time
    rng = np.random.default_rng(3)
    n, W = 20000, 100
    templates = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, W))]
    shortlist = np.zeros((n, 8), dtype=DESIGN_RECORD)
    shortlist["found"] = 1
    shortlist["left_start"] = rng.integers(0, 6, size=(n, 8))
    shortlist["left_len"] = rng.integers(18, 25, size=(n, 8))
    shortlist["right_start"] = rng.integers(70, 76, size=(n, 8))
    shortlist["right_len"] = rng.integers(18, 25, size=(n, 8))
    t0 = time.perf_counter()
    left, right, pairs, index = reports.shortlist_pairs(templates, shortlist)
    dt = time.perf_counter() - t0
    print(f"{n} regions x 8: {len(left)} left, {len(right)} right, {len(pairs)} pairs in {dt:.3f} s")
    assert (index >= 0).all() and int(index.max()) == len(pairs) - 1 and dt < 5.0
    for i, j in ((0, 0), (n - 1, 7), (n // 2, 3)):
        r, (a, b) = shortlist[i, j], pairs[index[i, j]]
        assert left[a] == bytes(templates[i, int(r["left_start"]):int(r["left_start"]) + int(r["left_len"])])
        assert right[b] == bytes(templates[i, int(r["right_start"]):int(r["right_start"]) + int(r["right_len"])])
    assert left == sorted(set(left)) and right == sorted(set(right))


def test_the_writer(tmp_path):
    W = 40
    t0, t1, t2 = "ACGTTGCAAGGCTTAACCGGATATCGCGTTAAGGCCTTAA", "T" * W, "GGCATCGATTACGCATGCAAATTTCCCGGGATCGATCGTA"
    templates = np.frombuffer((t0 + t1 + t2).encode(), dtype=np.uint8).reshape(3, W)
    shortlist = np.zeros((3, 2), dtype=DESIGN_RECORD)
    _slot(shortlist[0, 0], 1, 10, 28, 11)
    _slot(shortlist[0, 1], 2, 10, 28, 11)
    _slot(shortlist[2, 0], 0, 12, 27, 10)
    shortlist["pair_penalty"] = [[500, 700], [0, 0], [40, 0]]
    index = np.array([[0, 1], [-1, -1], [2, -1]])
    tallies = np.array([[4, 2, 1, 9, 9, 9, 9, 3], [4, 0, 0, 9, 9, 9, 9, 1], [1 << 33, 0, 0, 0, 0, 0, 0, 5]], dtype=np.uint64)
    _, ranks, _ = reports.pick_pairs(shortlist, index, tallies, 1)
    path = tmp_path / "c.tsv"
    reports.write_primer_candidates(str(path), templates, shortlist, index, tallies, ranks, 1)
    lines = path.read_text().split("\n")
    assert lines[0] == reports.PRIMER_CANDIDATE_HEADER and lines[-1] == ""
    assert lines[0].split("\t") == ["region", "rank", "shortlisted", "pair_penalty", "product_size", "left_sequence", "right_sequence",
                                    "left_start", "left_length", "right_start", "right_length", "products", "picked"]
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))          # noqa: E731
    assert [ln.split("\t") for ln in lines[1:-1]] == [
        ["0", "1", "2", "500", "38", t0[1:11], rc(t0[28:39]), "1", "10", "28", "11", "3,4,2,1", "0"],
        ["0", "2", "2", "700", "37", t0[2:12], rc(t0[28:39]), "2", "10", "28", "11", "1,4,0,0", "1"],
        # (the region without a pair is not numbered: this is region 1, as --out_primer_products counts)
        ["1", "1", "1", "40", "37", t2[0:12], rc(t2[27:37]), "0", "12", "27", "10", f"5,{1 << 33},0,0", "1"],
    ]


# ----------------------------------------------------------------------------
# the cases' shape facts: design_cases.py as it stands holds the edges of the list (no pair, fewer than N, exactly N, more)
# ----------------------------------------------------------------------------
def _pair_counts(geo, **extra):
    ts = design_cases.templates(*geo, design_cases.GEOMETRIES[geo]["n_random"])
    passed = SR.passing_all(ts, *geo, **dict(design_cases.GEOMETRIES[geo]["base"], **extra))
    return len(ts), Counter(len(p[2]) for p in passed)


def test_the_cases_hold_the_edges_of_the_list():
    n, c = _pair_counts((12, 4, 12), gc=(45, 55))
    assert n == 52 and c[0] == 38
    assert {k: v for k, v in c.items() if 0 < k <= 8} == {1: 1, 2: 1, 4: 2, 5: 1, 8: 3}
    assert sum(v for k, v in c.items() if k > 8) == 6
    _, c = _pair_counts((12, 4, 12), gc_clamp=1)
    assert {1, 2, 3, 4, 5, 6, 8, 9} <= set(c)
    _, c = _pair_counts((40, 20, 25), max_sec_tm=-50)
    assert c[8] == 2
    _, c = _pair_counts((256, 60, 256))
    assert c[5] == 1


def test_the_reference_shortlist_starts_with_the_reference_pick():
    """slot 0 of the reference's shortlist is design_reference's / hairpin_reference's record, and the slots ascend"""
    import design_reference as DR
    import hairpin_reference as HR
    geo = (12, 4, 12)
    ts = design_cases.templates(*geo, 30)
    opts = design_cases.option_sets(geo)[3]
    for hairpins in (False, True):
        passed = SR.passing_all(ts, *geo, hairpins=hairpins, **opts)
        got = SR.shortlist(passed, 8, hairpins)
        want = HR.design(ts, *geo, **opts) if hairpins else DR.design(ts, *geo, **opts)
        assert got[:, 0].tobytes() == want.tobytes()
        for i, (_, _, rows) in enumerate(passed):
            keys = [tuple(int(got[i, j][k]) for k in ("pair_penalty", "left_start", "left_len", "right_start", "right_len"))
                    for j in range(min(len(rows), 8))]
            assert keys == sorted(set(keys)) and int((got[i]["found"] != 0).sum()) == len(keys)
