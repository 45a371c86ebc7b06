"""--out_locations on the host: the record-ID helper (fasta.record_ids / record_ids_text) against the reader's rules, the
flank table of each kind of group list, the command line's surface -- and py_locate, a slow pure-Python locator that the
GPU tests (test_gpu_locate.py) hold the device's rows to.  py_locate is checked here against the golden cases' filtered
files: every (group, label, sequence) is found as often as the reference's merged file counts it."""
import bz2
import gzip
import json
import os
import sys
from collections import Counter

import numpy as np
import pytest

from krisp_amd import amplicon, codec, fasta
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_cases import FC as _FC0, FC6, canon_lines       # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FC = _FC0 + FC6
RC = json.load(open(os.path.join(GOLDEN, "reader_cases.json")))

_COMP = bytes.maketrans(b"ATGCRYMKSWBVDHN", b"TACGYRKMSWVBHDN")


# ----------------------------------------------------------------------------
# the slow locator (the reference's window rules, kstream.py:617-677, record by record)
# ----------------------------------------------------------------------------
def py_record_ids(lines, one_shot=True):
    """record IDs by read_records' loop, line by line"""
    fa = bool(lines) and b">" in lines[0]
    first = fasta.strip_line(lines[0]) if lines else b""
    if one_shot:
        lines = lines[1:]
    if not fa:
        return [""] * len(lines)
    last = KF_header(first) if first.startswith(b">") else ""
    ids, cur = [], False
    for ln in lines:
        ln = fasta.strip_line(ln)
        if ln.startswith(b">"):
            last, cur = KF_header(ln), False
        elif ln and not cur:
            ids.append(last)
            cur = True
    return ids


def KF_header(line):
    w = line[1:].decode("utf-8", "surrogateescape").split()
    return w[0] if w else ""


def py_locate(files, flank_pairs, L, D, R, omit_soft):
    """rows (region, file, record, record_index, start, end, strand, sequence) in the TSV's order; flank_pairs[i] = group
    i's (left, right) as str, U written as T"""
    k = L + D + R
    want = {(lf.encode(), rt.encode()): i for i, (lf, rt) in enumerate(flank_pairs)}
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
                    g = want.get((x[:L], x[L + D:]))
                    if g is not None:
                        seq = x.decode()
                        rows.append((g, fi, path, ids[ri], ri, s, s + k, strand, seq.replace("T", "U") if rna else seq))
    rows.sort(key=lambda r: (r[0], r[1], r[4], r[5], r[7] == "-"))
    return [(g, path, rid, ri, s, e, st, seq) for g, _fi, path, rid, ri, s, e, st, seq in rows]


def golden_paths(case, tmp_path):
    if case["name"].startswith("c1_"):
        return {fn: os.path.join(GOLDEN, "c1", fn) for fn in case["ingroup"] + case["outgroup"]}
    out = {}
    for fn, text in case["files"].items():
        p = tmp_path / fn
        p.write_text(text)
        out[fn] = str(p)
    return out


def parse_labels(text):
    out = []
    for part in text.split(";"):
        if part.endswith(")") and "(" in part:
            name, n = part[:-1].rsplit("(", 1)
            out += [name] * int(n)
        else:
            out.append(part)
    return out


def golden_groups(case):
    """the golden filtered file (the merged file where nothing is filtered) as {(left, right): [(sequence, [labels])]}, or
    None when only its hash was kept"""
    lines = canon_lines(case["filtered_canon"] if "filtered_canon" in case else case["merged_canon"])
    if lines is None:
        return None
    groups = {}
    for ln in lines:
        left, diag, right, labels = ln.split(",", 3)
        groups.setdefault((left, right), []).append((left + diag + right, parse_labels(labels)))
    return groups


def multiplicities(groups, order):
    """Counter of (region, label, sequence) the groups promise; order: (left, right) of region i"""
    c = Counter()
    for i, key in enumerate(order):
        for seq, labels in groups[key]:
            for lab in labels:
                c[(i, lab, seq)] += 1
    return c


def labels_of(files):
    return ["merged_file"] if len(files) == 1 else [KF.simplename(f) for f in files]


# ----------------------------------------------------------------------------
# record IDs
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in RC if c["source"] != "list"], ids=lambda c: c["name"])
def test_record_ids_follow_read_records_on_every_reader_case(case, tmp_path):
    src = str(tmp_path / case["source"])
    with (gzip.open if src.endswith(".gz") else open)(src, "wb") as f:
        f.write(case["text"].encode())
    ids = fasta.record_ids(src)
    assert len(ids) == len(fasta.read_records(src)) == len(case["records"])
    assert ids == py_record_ids(fasta._read_raw_lines(src))
    raw = open(src, "rb").read()
    if not src.endswith(".gz"):
        assert fasta.record_ids_text(np.frombuffer(raw, dtype=np.uint8), True) == ids


@pytest.mark.parametrize("case", [c for c in FC if "files" in c], ids=lambda c: c["name"])
def test_record_ids_follow_read_records_on_the_golden_genomes(case, tmp_path):
    for path in golden_paths(case, tmp_path).values():
        ids = fasta.record_ids(path)
        assert len(ids) == len(fasta.read_records(path))
        assert ids == py_record_ids(fasta._read_raw_lines(path))


HAND = [
    ("consecutive_headers", b">a\n>b x\nAC\nGT\n>c\nTT\n", ["b", "c"]),
    ("header_without_sequence", b">a\nAC\n>b\n>c\nGG\n>d\n", ["a", "c"]),
    ("first_line_gt_inside", b"AC>G\nTT\nAA\n>x\nGG\n", ["", "x"]),
    ("first_line_header_only", b">only\n", []),
    ("empty_records_dropped", b">a\n\n  \n>b\n\t\nA\n", ["b"]),
    ("line_mode", b"ACGT\nGT\n\nTT\n", ["", "", ""]),
    ("line_mode_no_final_newline", b"A\nC", [""]),
    ("crlf_and_strip", ">a desc\r\n ACGT \r\n\x1c>b x\r\n　GG \r\n>\r\nTT\r\n".encode(), ["a", "b", ""]),
    ("gt_inside_sequence_lines", b">r1\nAC>GT\n>r2 y\n>>z\nCC\n", ["r1", ">z"]),
    ("lone_cr", b">a\rAC\r>b\rGG", ["a", "b"]),
]


@pytest.mark.parametrize("name,text,want", HAND, ids=[h[0] for h in HAND])
@pytest.mark.parametrize("ext", [".fa", ".fa.gz", ".fa.bz2"])
def test_record_ids_hand_cases(name, text, want, ext, tmp_path):
    src = str(tmp_path / ("x" + ext))
    opener = {".fa": open, ".fa.gz": gzip.open, ".fa.bz2": bz2.open}[ext]
    with opener(src, "wb") as f:
        f.write(text)
    got = fasta.record_ids(src)
    assert len(got) == len(fasta.read_records(src))
    assert got == py_record_ids(fasta._read_raw_lines(src))
    if ext == ".fa" or b"\r" not in text:
        assert got == want
    else:
        # (a compressed file's lines break at '\n' only: a lone CR stays in its line)
        assert got == py_record_ids(fasta._read_raw_lines(src))


# ----------------------------------------------------------------------------
# the slow locator against the golden filtered files
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in FC if "csv" in c], ids=lambda c: c["name"])
def test_py_locate_meets_the_multiplicity_contract_on_the_golden_cases(case, tmp_path):
    groups = golden_groups(case)
    if groups is None:
        pytest.skip("this case keeps only a hash of its filtered file")
    paths = golden_paths(case, tmp_path)
    files = [paths[f] for f in case["ingroup"] + case["outgroup"]]
    labels = labels_of(files)
    L, D, R = codec.effective_geometry(case["L"], case["D"], case["R"])
    order = sorted(groups)
    rows = py_locate(files, [(lf.replace("U", "T"), rt.replace("U", "T")) for lf, rt in order], L, D, R, case["omit_soft"])
    got = Counter((g, labels[files.index(path)], seq) for g, path, _r, _ri, _s, _e, _st, seq in rows)
    assert got == multiplicities(groups, order)


# ----------------------------------------------------------------------------
# the flank table of each kind of group list
# ----------------------------------------------------------------------------
def test_group_flanks_of_records_windows_and_lists_agree():
    L, D, R = 3, 1, 2
    seqs = ["AAAGCC", "AAATCC", "ACGTTT", "CCCAGG", "CCCCGG", "TTTAAA"]       # left|diag|right
    keys = np.array(sorted(codec_key(s, L, D, R) for s in seqs), dtype=np.uint64)
    recs = np.zeros(len(keys), dtype=[("key", "<u8"), ("genome", "<u4"), ("count", "<u4")])
    recs["key"], recs["count"] = keys, 1
    rg = amplicon.RecordGroups(recs, ["g0"], L, D, R)
    lists = amplicon.groups_from_records(recs, ["g0"], L, D, R)
    rows = np.frombuffer("".join(seqs[::-1]).encode(), dtype=np.uint8).reshape(-1, L + D + R)
    wg = amplicon.WindowGroups(rows, np.arange(len(seqs)), np.zeros(len(seqs)), ["g0"], L, D, R)
    want = np.array([list((g[0].left + g[0].right).encode()) for g in lists], dtype=np.uint8)
    for g in (rg, lists, wg):
        assert np.array_equal(KF._group_flanks(g, L, R), want)
    rna = [[amplicon.Amplicon("AAU", "G", "CU", ["x"])]]
    assert KF._group_flanks(rna, 3, 2).tobytes() == b"AATCT"


def codec_key(s, L, D, R):
    t = s[:L] + s[L + D:] + s[L:L + D]
    key = 0
    for i, ch in enumerate(t):
        key |= "ACGT".index(ch) << (62 - 2 * i)
    return key


# ----------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------
def test_out_locations_with_primer3_exits_2(capsys, monkeypatch):
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: pytest.fail("no run may start"))
    with pytest.raises(SystemExit) as e:
        KF.main(["x.fa", "-c", "5", "-d", "1", "--out_locations", "loc.tsv", "--primer3"])
    assert e.value.code == 2
    assert "--out_locations cannot be combined with --primer3" in capsys.readouterr().err


def test_the_parser_takes_out_locations():
    args = KF.build_parser().parse_args(["a.fa", "-c", "5", "-d", "1", "--out_locations", "loc.tsv"])
    assert args.out_locations == "loc.tsv"
    assert KF.build_parser().parse_args(["a.fa", "-c", "5", "-d", "1"]).out_locations is None


def test_main_without_the_flag_writes_what_it_wrote_and_locates_nothing(tmp_path, monkeypatch, capsys):
    groups = [[amplicon.Amplicon("AAAAA", "C", "GGGGG", ["in0"]), amplicon.Amplicon("AAAAA", "T", "GGGGG", ["out0"])]]
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (groups, {"kmers": 0, "device_s": 0.0}))
    monkeypatch.setattr(KF, "locate_regions", lambda *a, **k: pytest.fail("no locate pass without --out_locations"))
    aln = tmp_path / "a.txt"
    assert KF.main(["in0.fa", "--outgroup", "out0.fa", "-c", "5", "-d", "1", "-o", str(aln)]) == 0
    csv, align = amplicon.render(groups, ["in0"])
    assert capsys.readouterr().out == csv
    assert aln.read_text() == align
    assert not list(tmp_path.glob("*.tsv"))


def test_main_writes_the_locations_of_what_locate_regions_returns(tmp_path, monkeypatch, capsys):
    groups = [[amplicon.Amplicon("AAAAA", "C", "GGGGG", ["in0"]), amplicon.Amplicon("AAAAA", "T", "GGGGG", ["out0"])]]
    monkeypatch.setattr(KF, "find_regions", lambda *a, **k: (groups, {"kmers": 0, "device_s": 0.0}))
    seen = {}

    def fake(g, ing, outg, L, R, k, omit_soft=False, device=0):
        seen.update(groups=g, ing=ing, outg=outg, geo=(L, R, k), omit=omit_soft, device=device)
        out = np.empty(1, dtype=KF.LOCATION)
        out[0] = (0, "in0.fa", "chr1", 0, 5, 16, "+", "AAAAACGGGGG")
        return out
    monkeypatch.setattr(KF, "locate_regions", fake)
    tsv = tmp_path / "loc.tsv"
    assert KF.main(["in0.fa", "--outgroup", "out0.fa", "-c", "5", "-d", "1", "--out_locations", str(tsv),
                    "--device", "0"]) == 0
    assert seen["groups"] is groups and seen["ing"] == ["in0.fa"] and seen["outg"] == ["out0.fa"]
    assert seen["geo"] == (5, 5, 11)
    assert tsv.read_text() == KF.LOCATION_HEADER + "\n0\tin0.fa\tchr1\t0\t5\t16\t+\tAAAAACGGGGG\n"
    assert capsys.readouterr().out == amplicon.render(groups, ["in0"])[0]
