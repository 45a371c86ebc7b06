"""--out_near on the host: py_near, the definition of the near-match table as a slow program (every record, every start,
both strands, a numpy compare against all targets) that the GPU tests (test_gpu_near.py) hold the device's rows to, pinned
here by hand-written cases; KF.near_targets on the three forms of groups and on the golden cases' recorded output; the
command line's surface and refusals."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import amplicon, codec, fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_locate_host import (FC, _COMP, codec_key, golden_groups, golden_paths, labels_of,       # noqa: E402
                              py_record_ids)


# ----------------------------------------------------------------------------
# the definition, slowly
# ----------------------------------------------------------------------------
def py_near(files, targets, L, D, R, M, omit_soft):
    """rows (region, target, file, record, record_index, start, end, strand, mismatches, flank_mismatches, sequence) in
    the TSV's order; targets = [(region, text in DNA letters)] ordered by (region, text)"""
    k = L + D + R
    if not targets:
        return []
    T = np.frombuffer("".join(t for _, t in targets).encode(), dtype=np.uint8).reshape(-1, k)
    flank = np.zeros(k, dtype=bool)
    flank[:L] = True
    flank[L + D:] = True
    rows = []
    for fi, path in enumerate(files):
        recs = fasta.read_records(path)
        rna = bool(fasta.detect_rna(recs))
        ids = py_record_ids(fasta._read_raw_lines(path))
        assert len(ids) == len(recs)
        for ri, rec in enumerate(recs):
            if rna:
                rec = rec.replace(b"U", b"T").replace(b"u", b"t")
            for s in range(len(rec) - k + 1):
                w = rec[s:s + k]
                if omit_soft:
                    if not w.isupper():
                        continue
                else:
                    w = w.upper()
                if b"N" in w:
                    continue
                for strand, x in (("+", w), ("-", w[::-1].translate(_COMP))):
                    ne = T != np.frombuffer(x, dtype=np.uint8)
                    d = ne.sum(axis=1)
                    for ti in np.flatnonzero(d <= M).tolist():
                        seq = x.decode()
                        rows.append((ti, fi, ri, s, strand == "-",
                                     (targets[ti][0], targets[ti][1], path, ids[ri], ri, s, s + k, strand, int(d[ti]),
                                      int(ne[ti][flank].sum()), seq.replace("T", "U") if rna else seq)))
    rows.sort(key=lambda r: r[:5])
    return [r[5] for r in rows]


def near_rows(arr):
    """a NEAR array as py_near's tuples"""
    return list(zip(arr["region"].tolist(), arr["target"], arr["file"], arr["record"], arr["record_index"].tolist(),
                    arr["start"].tolist(), arr["end"].tolist(), arr["strand"], arr["mismatches"].tolist(),
                    arr["flank_mismatches"].tolist(), arr["sequence"]))


def case_amplicon(case):
    a = case.get("main_args", [])
    if "--amplicon" in a:
        return int(a[a.index("--amplicon") + 1])
    return case["L"] + case["D"] + case["R"]


def golden_targets(case, files, n_ingroup):
    """the targets the recorded reference output promises: [(region, text)]"""
    gg = golden_groups(case)
    ingroup = set(labels_of(files)[:n_ingroup]) if len(files) > n_ingroup else None
    out = []
    for i, key in enumerate(sorted(gg)):
        texts = {seq.replace("U", "T") for seq, labs in gg[key] if ingroup is None or ingroup & set(labs)}
        out += [(i, t) for t in sorted(texts)]
    return out


def _fa(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text)
    return str(p)


#        LLLLLDRRRR   (5/1/4)
TGT = "ACGTTGCATC"
RC_TGT = TGT.encode()[::-1].translate(_COMP).decode()      # GATGCAACGT


def _sub(s, i, ch):
    assert s[i] != ch
    return s[:i] + ch + s[i + 1:]


def _one(tmp_path, seq, M=1, omit=False, targets=None, name="g.fa"):
    p = _fa(tmp_path, name, seq if isinstance(seq, bytes) else seq.encode())
    rows = py_near([p], targets or [(0, TGT)], 5, 1, 4, M, omit)
    return [r[3:] for r in rows]      # (record, record_index, start, end, strand, mismatches, flank_mismatches, sequence)


def test_py_near_one_substitution_in_each_part_and_on_the_reverse_strand(tmp_path):
    pad = "TTTTTTTTTTTT"
    for col, fm in ((1, 1), (8, 1), (5, 0)):
        ch = "A" if TGT[col] != "A" else "C"
        w = _sub(TGT, col, ch)
        got = _one(tmp_path, f">r\n{pad}{w}{pad}\n")
        assert got == [("r", 0, 12, 22, "+", 1, fm, w)]
        assert _one(tmp_path, f">r\n{pad}{w}{pad}\n", M=0) == []
        # the same window written on the other strand: the row gives the window as that strand reads it
        rc = w.encode()[::-1].translate(_COMP).decode()
        got = _one(tmp_path, f">r\n{pad}{rc}{pad}\n")
        assert got == [("r", 0, 12, 22, "-", 1, fm, w)]


def test_py_near_no_row_across_records_with_n_or_masked(tmp_path):
    w = _sub(TGT, 2, "C")
    assert _one(tmp_path, f">a\nTTTT{w[:6]}\n>b\n{w[6:]}TTTT\n") == []                     # straddles two records
    assert _one(tmp_path, f">a\nTTTT{w[:6]}\n{w[6:]}TTTT\n") == [("a", 0, 4, 14, "+", 1, 1, w)]  # (one record, two lines)
    assert _one(tmp_path, f">a\nTTTT{_sub(w, 7, 'N')}TTTT\n", M=3) == []                  # holds an N
    assert _one(tmp_path, f">a\nTTTT{_sub(w, 7, 'n')}TTTT\n", M=3) == []
    low = w[:3] + w[3:6].lower() + w[6:]
    assert _one(tmp_path, f">a\nTTTT{low}TTTT\n") == [("a", 0, 4, 14, "+", 1, 1, w)]      # lower case: upper-cased
    assert _one(tmp_path, f">a\nTTTT{low}TTTT\n", omit=True) == []                         # ... or omitted


def test_py_near_palindromes_distance_zero_and_two_targets(tmp_path):
    pal = "ACGTATACGT"
    assert pal.encode()[::-1].translate(_COMP).decode() == pal
    got = _one(tmp_path, f">r\nCCCC{pal}CCCC\n", M=0, targets=[(0, pal)])
    assert got == [("r", 0, 4, 14, "+", 0, 0, pal), ("r", 0, 4, 14, "-", 0, 0, pal)]      # both strands
    # a window at distance 0 with M = 2: one row (one per target, window and strand -- not one per seed)
    got = _one(tmp_path, f">r\nCCCCC{TGT}CCCCC\n", M=2)
    assert got == [("r", 0, 5, 15, "+", 0, 0, TGT)]
    # two targets of one region, both within M of one window: two rows, in target order
    t2 = _sub(TGT, 5, "A")
    p = _fa(tmp_path, "two.fa", f">r\nCCCCC{_sub(TGT, 5, 'T')}CCCCC\n".encode())
    rows = py_near([p], [(0, t2), (0, TGT)], 5, 1, 4, 1, False)
    assert [(r[0], r[1], r[5], r[7], r[8], r[9]) for r in rows] == [(0, t2, 5, "+", 1, 0), (0, TGT, 5, "+", 1, 0)]


def test_py_near_rna_genomes_and_iupac_letters(tmp_path):
    w = _sub(TGT, 1, "G")
    got = _one(tmp_path, f">r\nCCCC{w.replace('T', 'U')}CCCC\n")
    assert got == [("r", 0, 4, 14, "+", 1, 1, w.replace("T", "U"))]                        # sequence in U
    p = _fa(tmp_path, "rna.fa", f">r\nCCCC{w.replace('T', 'U')}CCCC\n".encode())
    assert py_near([p], [(0, TGT)], 5, 1, 4, 1, False)[0][1] == TGT                        # target in T
    # an IUPAC letter is a letter: R differs from A and from G
    assert _one(tmp_path, f">r\nCCCC{_sub(TGT, 0, 'R')}CCCC\n") == [("r", 0, 4, 14, "+", 1, 1, "R" + TGT[1:])]
    assert _one(tmp_path, f">r\nCCCC{_sub(_sub(TGT, 0, 'R'), 9, 'Y')}CCCC\n") == []
    # ... and the reverse strand complements it (R <-> Y)
    rc = ("R" + TGT[1:]).encode()[::-1].translate(_COMP).decode()
    assert "Y" in rc
    assert _one(tmp_path, f">r\nCCCC{rc}CCCC\n") == [("r", 0, 4, 14, "-", 1, 1, "R" + TGT[1:])]


def test_py_near_orders_rows_by_region_target_file_record_start_strand(tmp_path):
    a = _fa(tmp_path, "a.fa", f">x\nGG{TGT}GG\n>y\n{RC_TGT}\n".encode())
    b = _fa(tmp_path, "b.fa", f">z\n{_sub(TGT, 9, 'G')}\n".encode())
    other = "GGGGGAGGGG"
    rows = py_near([a, b], [(0, TGT), (1, other)], 5, 1, 4, 1, False)
    assert [(r[0], os.path.basename(r[2]), r[3], r[5], r[7], r[8]) for r in rows] == [
        (0, "a.fa", "x", 2, "+", 0), (0, "a.fa", "y", 0, "-", 0), (0, "b.fa", "z", 0, "+", 1)]


# ----------------------------------------------------------------------------
# the targets of each kind of group list
# ----------------------------------------------------------------------------
def test_near_targets_of_records_windows_and_lists_agree():
    L, D, R = 3, 1, 2
    seqs = ["AAAGCC", "AAATCC", "ACGTTT", "CCCAGG", "CCCCGG", "TTTAAA"]       # left|diag|right
    keys = np.array(sorted(codec_key(s, L, D, R) for s in seqs), dtype=np.uint64)
    # (two genomes: g0 carries every sequence, g1 only the first of each group)
    recs = np.zeros(len(keys) + 4, dtype=[("key", "<u8"), ("genome", "<u4"), ("count", "<u4")])
    firsts = [codec_key(s, L, D, R) for s in ("AAAGCC", "ACGTTT", "CCCAGG", "TTTAAA")]
    recs["key"] = np.concatenate([keys, np.array(firsts, dtype=np.uint64)])
    recs["genome"][len(keys):] = 1
    recs["count"] = 1
    recs = recs[np.lexsort((recs["genome"], recs["key"]))]
    labels = ["g0", "g1"]
    rg = amplicon.RecordGroups(recs, labels, L, D, R)
    lists = amplicon.groups_from_records(recs, labels, L, D, R)
    rows = np.frombuffer("".join(seqs[::-1] + ["AAAGCC", "ACGTTT", "CCCAGG", "TTTAAA"]).encode(), dtype=np.uint8).reshape(-1, 6)
    genome = np.array([0] * 6 + [1] * 4)
    wg = amplicon.WindowGroups(rows, np.arange(len(rows)), genome, labels, L, D, R)
    want_all = [(0, "AAAGCC"), (0, "AAATCC"), (1, "ACGTTT"), (2, "CCCAGG"), (2, "CCCCGG"), (3, "TTTAAA")]
    want_g1 = [(0, "AAAGCC"), (1, "ACGTTT"), (2, "CCCAGG"), (3, "TTTAAA")]
    for g in (rg, lists, wg):
        assert KF.near_targets(g, None) == want_all
        assert KF.near_targets(g, ["g0"]) == want_all
        assert KF.near_targets(g, ["g1"]) == want_g1
        assert KF.near_targets(g, ["elsewhere"]) == []
    # U is written as T, equal texts are one target, a region's targets go by their bytes
    rna = [[amplicon.Amplicon("AAU", "G", "CU", ["x"]), amplicon.Amplicon("AAT", "G", "CT", ["y"]),
            amplicon.Amplicon("AAU", "C", "CU", ["x"])]]
    assert KF.near_targets(rna, ["x", "y"]) == [(0, "AATCCT"), (0, "AATGCT")]


@pytest.mark.parametrize("case", [c for c in FC if ("csv" in c or "filtered_canon" in c) and golden_groups(c) is not None],
                         ids=lambda c: c["name"])
def test_near_targets_of_the_golden_cases_recorded_output(case, tmp_path):
    gg = golden_groups(case)
    paths = golden_paths(case, tmp_path)
    files = [paths[f] for f in case["ingroup"] + case["outgroup"]]
    labels = labels_of(files)
    ingroup = labels[:len(case["ingroup"])] if case["outgroup"] else None
    # the recorded lines as the list form of groups (regions by (left, right), sequences by diag)
    groups = []
    for key in sorted(gg):
        groups.append([amplicon.Amplicon(seq[:len(key[0])], seq[len(key[0]):len(seq) - len(key[1])],
                                         seq[len(seq) - len(key[1]):], labs) for seq, labs in gg[key]])
    assert KF.near_targets(groups, ingroup) == golden_targets(case, files, len(case["ingroup"]))


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_the_parser_takes_out_near_and_near_mismatches():
    args = KF.build_parser().parse_args(["a.fa", "-c", "5", "-d", "1", "--out_near", "near.tsv", "--near-mismatches", "2"])
    assert args.out_near == "near.tsv" and args.near_mismatches == 2
    args = KF.build_parser().parse_args(["a.fa", "-c", "5", "-d", "1"])
    assert args.out_near is None and args.near_mismatches is None


REFUSALS = [
    (["-c", "5", "-d", "1", "--out_near", "n.tsv", "--primer3"], "--out_near cannot be combined with --primer3"),
    (["-c", "5", "-d", "1", "--out_near", "n.tsv", "--near-mismatches", "-1"], "between 0 and 3"),
    (["-c", "5", "-d", "1", "--out_near", "n.tsv", "--near-mismatches", "4"], "between 0 and 3"),
    (["-c", "1", "-d", "1", "--out_near", "n.tsv", "--near-mismatches", "3"], "smaller than the amplicon length"),
    (["-c", "5", "-d", "1", "--near-mismatches", "1"], "--near-mismatches needs --out_near"),
    (["-c", "16", "-d", "1", "--out_near", "n.tsv"], "at most 32 bases"),
    (["-c", "5", "-d", "17", "--out_near", "n.tsv"], "at most 16 diagnostic bases"),
]


@pytest.mark.parametrize("argv,message", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_exit_2_before_any_genome_is_read(argv, message, capsys, monkeypatch):
    for name in ("find_regions", "find_regions_multi_device", "find_regions_distributed", "near_matches"):
        monkeypatch.setattr(KF, name, lambda *a, **k: pytest.fail("no run may start"))
    with pytest.raises(SystemExit) as e:
        KF.main(["no_such_file.fa"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and err.count("\n") == 1


def test_near_matches_refuses_what_the_command_line_refuses():
    for L, R, k, M in ((5, 5, 11, 4), (5, 5, 11, -1), (1, 1, 3, 3), (16, 16, 33, 1), (5, 5, 27, 1)):
        with pytest.raises(ValueError):
            KF.near_matches([], ["a.fa"], [], L, R, k, mismatches=M)
    assert KF.near_refusal(1, 1, 3, 2) is None and KF.near_refusal(1, 1, 4, 3) is None
    assert KF.near_refusal(15, 15, 32, 3) is None


GROUPS = [[amplicon.Amplicon("AAAAA", "C", "GGGGG", ["in0"]), amplicon.Amplicon("AAAAA", "T", "GGGGG", ["out0"])]]


def test_main_without_the_flag_calls_nothing_of_the_near_pass(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (GROUPS, {"kmers": 0, "device_s": 0.0}))
    for name in ("near_matches", "near_targets", "write_near", "near_refusal"):
        monkeypatch.setattr(KF, name, lambda *a, **k: pytest.fail("no near pass without --out_near"))
    aln = tmp_path / "a.txt"
    assert KF.main(["in0.fa", "--outgroup", "out0.fa", "-c", "5", "-d", "1", "-o", str(aln)]) == 0
    csv, align = amplicon.render(GROUPS, ["in0"])
    assert capsys.readouterr().out == csv
    assert aln.read_text() == align
    assert not list(tmp_path.glob("*.tsv"))


def test_main_writes_what_near_matches_returns(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (GROUPS, {"kmers": 0, "device_s": 0.0}))
    seen = {}

    def fake(g, ing, outg, L, R, k, mismatches=1, omit_soft=False, device=0):
        seen.update(groups=g, ing=ing, outg=outg, geo=(L, R, k), M=mismatches, omit=omit_soft, device=device)
        out = np.empty(2, dtype=KF.NEAR)
        out[0] = (0, "AAAAACGGGGG", "in0.fa", "chr1", 0, 5, 16, "+", 0, 0, "AAAAACGGGGG")
        out[1] = (0, "AAAAACGGGGG", "out0.fa", "chr2", 3, 7, 18, "-", 2, 1, "ATAAACGGGGC")
        return out
    monkeypatch.setattr(KF, "near_matches", fake)
    monkeypatch.setattr(KF, "locate_regions", lambda *a, **k: pytest.fail("no locate pass without --out_locations"))
    tsv = tmp_path / "near.tsv"
    assert KF.main(["in0.fa", "--outgroup", "out0.fa", "-c", "5", "-d", "1", "--out_near", str(tsv), "--near-mismatches", "2",
                    "--omit-soft"]) == 0
    assert seen["groups"] is GROUPS and seen["ing"] == ["in0.fa"] and seen["outg"] == ["out0.fa"]
    assert seen["geo"] == (5, 5, 11) and seen["M"] == 2 and seen["omit"] is True and seen["device"] == 0
    assert tsv.read_text() == (KF.NEAR_HEADER + "\n0\tAAAAACGGGGG\tin0.fa\tchr1\t0\t5\t16\t+\t0\t0\tAAAAACGGGGG\n"
                               "0\tAAAAACGGGGG\tout0.fa\tchr2\t3\t7\t18\t-\t2\t1\tATAAACGGGGC\n")
    assert capsys.readouterr().out == amplicon.render(GROUPS, ["in0"])[0]
    assert KF.NEAR_HEADER.split("\t") == list(KF.NEAR.names)
    # the default distance is 1
    assert KF.main(["in0.fa", "--outgroup", "out0.fa", "-c", "5", "-d", "1", "--out_near", str(tsv)]) == 0
    assert seen["M"] == 1
