"""scan_reference.py -- the locate and the near-match scan as numpy definitions over every position of a text -- tied to
what is already pinned: ref_locate / ref_near equal the slow file-level definitions (py_locate, test_locate_host.py; py_near,
test_near_host.py) on the golden cases, positions mapped to (record_index, start) through ref_seps.  And the census of the
generator the GPU tests draw their random cases from (test_gpu_scan_properties.cases): with the reference alone it asserts
what the default seeds cover, so that an edit of the generator cannot hollow out the GPU comparison unnoticed."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

from krisp_amd import codec, fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_scan_properties as G                                                             # noqa: E402
from scan_reference import COMP, ref_locate, ref_near, ref_seps, ref_windows                     # noqa: E402
from test_locate_host import FC, _COMP, golden_groups, golden_paths, py_locate                   # noqa: E402
from test_near_host import case_amplicon, golden_targets, py_near                                # noqa: E402

GOLDEN_CASES = [c for c in FC if ("csv" in c or "filtered_canon" in c) and golden_groups(c) is not None]


def geometry(case):
    k = case_amplicon(case)
    return codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])


def uploaded(path):
    """the bytes a genome has on the device: its records joined by '\\n', U as T -> (text, RNA)"""
    recs = fasta.read_records(path)
    rna = bool(fasta.detect_rna(recs))
    if rna:
        recs = [r.replace(b"U", b"T").replace(b"u", b"t") for r in recs]
    return np.frombuffer(b"\n".join(recs), dtype=np.uint8), rna


def in_records(hits, text, k, rna):
    """-> (record_index, start, end, strand, sequence) of every hit"""
    seps = ref_seps(text).astype(np.int64)
    pos = hits["pos"]
    ri = np.searchsorted(seps, pos)
    start = pos - (np.where(ri > 0, seps[np.maximum(ri - 1, 0)] + 1, 0) if len(seps) else 0)
    seqs = [bytes(r).decode() for r in ref_windows(text, hits, k)]
    if rna:
        seqs = [s.replace("T", "U") for s in seqs]
    return ri.tolist(), start.tolist(), (start + k).tolist(), ["+-"[s] for s in hits["strand"]], seqs


def test_the_complement_map_is_the_one_of_the_slow_definitions():
    assert bytes(COMP.tolist()) == bytes(range(256)).translate(_COMP)
    assert np.array_equal(COMP[COMP], np.arange(256))


def test_hand_cases():
    #       0123456789
    text = b"ACGTTnACG\nCGTAA"
    hits = ref_locate(text, 2, 1, 1, False, np.frombuffer(b"ACT" b"CGA", dtype=np.uint8).reshape(2, 3))
    # ACGT at 0 is row 0 on '+' and (its own reverse complement) on '-'; CGTA at 10 is row 1 on '+'
    assert hits.tolist() == [(0, 0, 0), (0, 1, 0), (10, 0, 1)]
    assert ref_seps(text).tolist() == [9]
    near = ref_near(text, 2, 1, 1, False, np.frombuffer(b"ACGA", dtype=np.uint8).reshape(1, 4), 1)
    # ACGT (and its reverse complement): one mismatch, in the right flank; every other window differs in three columns or four
    assert near.tolist() == [(0, 0, 0, 1, 1), (0, 1, 0, 1, 1)]
    assert [bytes(r) for r in ref_windows(b"acgtN", np.array([(1, 1)], dtype=[("pos", "i8"), ("strand", "i8")]), 3)] == [b"ACG"]
    low = ref_locate(b"acgt", 2, 1, 1, True, np.frombuffer(b"ACT", dtype=np.uint8).reshape(1, 3))
    assert len(low) == 0 and len(ref_locate(b"acgt", 2, 1, 1, False, np.frombuffer(b"ACT", dtype=np.uint8).reshape(1, 3))) == 2


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=lambda c: c["name"])
def test_ref_locate_equals_py_locate_on_the_golden_cases(case, tmp_path):
    paths = golden_paths(case, tmp_path)
    files = [paths[f] for f in case["ingroup"] + case["outgroup"]]
    L, D, R = geometry(case)
    k = L + D + R
    pairs = [(lf.replace("U", "T"), rt.replace("U", "T")) for lf, rt in sorted(golden_groups(case))]
    flanks = np.frombuffer("".join(a + b for a, b in pairs).encode(), dtype=np.uint8).reshape(len(pairs), L + R)
    rows = []
    for fi, path in enumerate(files):
        text, rna = uploaded(path)
        hits = ref_locate(text, L, D, R, case["omit_soft"], flanks)
        for g, (ri, s, e, st, seq) in zip(hits["group"].tolist(), zip(*in_records(hits, text, k, rna))):
            rows.append((g, fi, ri, s, st == "-", (g, path, ri, s, e, st, seq)))
    rows.sort(key=lambda r: r[:5])
    want = [(g, path, ri, s, e, st, seq) for g, path, _rid, ri, s, e, st, seq in py_locate(files, pairs, L, D, R, case["omit_soft"])]
    assert [r[5] for r in rows] == want


PACKED = [c for c in GOLDEN_CASES if not KF._is_wide(*geometry(c))]


@pytest.mark.parametrize("case", PACKED, ids=lambda c: c["name"])
def test_ref_near_equals_py_near_on_the_golden_cases(case, tmp_path):
    """every distance M = 0 .. min(3, k - 1); py_near's rows within M are its rows within 3 that have <= M mismatches"""
    paths = golden_paths(case, tmp_path)
    files = [paths[f] for f in case["ingroup"] + case["outgroup"]]
    L, D, R = geometry(case)
    k = L + D + R
    targets = golden_targets(case, files, len(case["ingroup"]))
    if not targets:
        return
    T = np.frombuffer("".join(t for _, t in targets).encode(), dtype=np.uint8).reshape(len(targets), k)
    texts = [uploaded(p) for p in files]
    top = min(3, k - 1)
    slow = py_near(files, targets, L, D, R, top, case["omit_soft"])
    for M in range(top + 1):
        rows = []
        for fi, (path, (text, rna)) in enumerate(zip(files, texts)):
            hits = ref_near(text, L, D, R, case["omit_soft"], T, M)
            for ti, mm, fm, (ri, s, e, st, seq) in zip(hits["target"].tolist(), hits["mismatches"].tolist(),
                                                       hits["flank_mismatches"].tolist(), zip(*in_records(hits, text, k, rna))):
                rows.append((ti, fi, ri, s, st == "-", (targets[ti][0], targets[ti][1], path, ri, s, e, st, mm, fm, seq)))
        rows.sort(key=lambda r: r[:5])
        want = [(rg, t, path, ri, s, e, st, mm, fm, seq) for rg, t, path, _rid, ri, s, e, st, mm, fm, seq in slow if mm <= M]
        assert [r[5] for r in rows] == want, M


# ----------------------------------------------------------------------------
# the census of test_gpu_scan_properties.cases over its default seeds
# ----------------------------------------------------------------------------
IUPAC = set(b"RYKMSWBDHV")


def valid_window(c, p):
    w = c["text"][p:p + c["k"]]
    bad = (w == 10) | (w == ord("N")) | (w == ord("n"))
    return not (bad.any() or (c["omit"] and (w >= 97).any()))


def tally(c, hits, tag, count):
    """what one case's expected hits add to the census under `tag` ("locate" or the distance M)"""
    k, n = c["k"], len(c["text"])
    pos, strand = hits["pos"], hits["strand"]
    count[tag, "cases"] += 1
    count[tag, "cases with hits"] += len(hits) > 0
    count[tag, "hits"] += len(hits)
    count[tag, "across a tile edge"] += int(((pos // G.TILE + 1) * G.TILE <= pos + k - 1).sum())
    count[tag, "on a thread's last start"] += int((pos % G.THREAD == G.THREAD - 1).sum())
    count[tag, "on a thread's first start"] += int((pos % G.THREAD == 0).sum())
    count[tag, "on the last window"] += int((pos == n - k).sum())
    both = bool((strand == 0).any() and (strand == 1).any())
    count[tag, "cases with both strands"] += both
    count[tag, "cases with both strands and L != R"] += both and c["L"] != c["R"]
    for what, yes in (("L = 0", c["L"] == 0), ("R = 0", c["R"] == 0), ("D = 0", c["D"] == 0), ("k = 32", k == 32),
                      ("a flank > 64 and k > 256", max(c["L"], c["R"]) > 64 and k > 256), ("k = M + 1", k == c["M"] + 1)):
        count[tag, "cases with hits at " + what] += yes and len(hits) > 0
    rowof = "group" if tag == "locate" else "target"
    table = c["flanks"] if tag == "locate" else c["targets"]
    hit_rows = set(hits[rowof].tolist())
    in_text = set(np.unique(c["text"] & 0xDF).tolist()) & IUPAC
    count[tag, "cases with a hit of a row that holds IUPAC letters"] += any(set(table[r].tolist()) & in_text for r in hit_rows)
    if c["palindrome"] is not None:
        at = hits[pos == c["palindrome"]]
        count[tag, "cases with a palindromic row hit on both strands"] += any(
            ((at[rowof] == r) & (at["strand"] == 0)).any() and ((at[rowof] == r) & (at["strand"] == 1)).any() for r in set(at[rowof].tolist()))


def test_census_of_the_random_cases():
    count = Counter()
    for seed in range(G.SEEDS):
        c = G.cases(seed)
        L, D, R, k, M = c["L"], c["D"], c["R"], c["k"], c["M"]
        loc = ref_locate(c["text"], L, D, R, c["omit"], c["flanks"])
        near = ref_near(c["text"], L, D, R, c["omit"], c["targets"], M)
        tally(c, loc, "locate", count)
        tally(c, near, M, count)
        # several rows under one key: flank pairs with one left flank, targets with one piece
        lefts = Counter(bytes(f[:L]) for f in c["flanks"]) if L else Counter()
        shared = {bytes(f[:L]) for f in c["flanks"] if lefts[bytes(f[:L])] > 1}
        count["locate", "cases with a hit of a row that shares its left flank"] += any(
            bytes(c["flanks"][g][:L]) in shared for g in set(loc["group"].tolist()))
        # (an entry of the seed table is a target or its reverse complement: a palindromic target shares every piece with itself)
        off = G.pieces(k, M)
        entry = {(t, s): (G.rc(row) if s else row) for t, row in enumerate(c["targets"]) for s in (0, 1)}
        share = False
        for j in range(M + 1):
            seen = Counter(bytes(e[off[j]:off[j + 1]]) for e in entry.values())
            share |= any(seen[bytes(entry[ts][off[j]:off[j + 1]])] > 1 for ts in set(zip(near["target"].tolist(), near["strand"].tolist())))
        count[M, "cases with a hit of a target that shares a piece"] += share
        count[M, "hits with exactly M mismatches"] += int((near["mismatches"] == M).sum())
        count[M, "hits without a flank mismatch"] += int((near["flank_mismatches"] == 0).sum())
        count[M, "hits with a flank mismatch"] += int((near["flank_mismatches"] > 0).sum())
        count[M, "hits with a flank mismatch on '-' where L != R"] += int(
            ((near["flank_mismatches"] > 0) & (near["strand"] == 1)).sum()) if L != R else 0
        # the planted copies: reported with their distance up to M, not reported at M + 1
        rows = {(p, s, t): mm for p, s, t, mm in zip(near["pos"].tolist(), near["strand"].tolist(), near["target"].tolist(),
                                                     near["mismatches"].tolist())}
        for p, s, t, j in c["plants"]:
            if not valid_window(c, p):
                assert (p, s, t) not in rows
            elif j <= M:
                assert rows[p, s, t] == j
                count[M, "planted copies within M, reported"] += 1
            else:
                assert (p, s, t) not in rows
                count[M, "planted copies at M + 1, not reported"] += 1
    for key in sorted(count, key=str):
        print(key, count[key])
    # every case is compared on the GPU (test_random_cases_equal_the_definition has no skip and no assume): SEEDS of them
    assert G.SEEDS == 4 * len(G.GEOMETRIES) and count["locate", "cases"] == G.SEEDS
    assert count["locate", "cases with hits"] >= 0.9 * G.SEEDS
    assert sum(count[M, "cases with hits"] for M in range(4)) >= 0.9 * G.SEEDS
    for tag in ("locate", 0, 1, 2, 3):
        assert count[tag, "cases"] == (G.SEEDS if tag == "locate" else G.SEEDS // 4)
        assert count[tag, "across a tile edge"] >= 20, tag
        assert count[tag, "on a thread's last start"] >= 20, tag
        assert count[tag, "on a thread's first start"] >= 20, tag
        assert count[tag, "on the last window"] >= 1, tag
        assert count[tag, "cases with both strands and L != R"] >= 1, tag
        assert count[tag, "cases with a palindromic row hit on both strands"] >= 1, tag
    for what in ("L = 0", "R = 0", "D = 0", "k = 32"):
        assert count["locate", "cases with hits at " + what] >= 1, what
        assert sum(count[M, "cases with hits at " + what] for M in range(4)) >= 1, what
    assert count["locate", "cases with hits at a flank > 64 and k > 256"] >= 3
    assert count["locate", "cases with a hit of a row that shares its left flank"] >= 1
    assert count["locate", "cases with a hit of a row that holds IUPAC letters"] >= 1
    assert sum(count[M, "cases with a hit of a row that holds IUPAC letters"] for M in range(4)) >= 1
    for M in range(4):
        assert count[M, "cases with hits at k = M + 1"] >= 1, M
        assert count[M, "cases with a hit of a target that shares a piece"] >= 1, M
        assert count[M, "hits with exactly M mismatches"] >= 1, M
        assert count[M, "planted copies within M, reported"] >= 1 and count[M, "planted copies at M + 1, not reported"] >= 1, M
        assert count[M, "hits without a flank mismatch"] >= 1, M
        if M:           # (at M = 0 no column differs)
            assert count[M, "hits with a flank mismatch"] >= 1, M
            assert count[M, "hits with a flank mismatch on '-' where L != R"] >= 1, M
