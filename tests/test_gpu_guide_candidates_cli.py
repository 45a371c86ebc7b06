"""--guide-candidates end to end on the GPU, on the golden case of test_gpu_guides.py's command-line test, alone and with
--design-primers: N = 1 is today's pick; with N = 4 every picked row's tally is the count of its region's outgroup rows in
the --out_guide_hits file and the pick is the least (tally, rank) of the candidates file; an extra outgroup genome with a
decoy record that holds the rank-1 protospacers makes those regions pick another rank."""
import gzip
import io
import os
import random
import sys
from collections import Counter
from contextlib import redirect_stdout

import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_shortlist_reference as ref                                    # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _argv, _files                                  # noqa: E402
from test_gpu_primers import _design_options                               # noqa: E402

pytestmark = pytest.mark.gpu

COPIES = 5                          # of a protospacer in the decoy: more exact hits than three related genomes can hold of another


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _table(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


def _by_region(cands):
    out = {}
    for c in cands:
        out.setdefault(c[0], []).append(c)
    return out


def _check_candidates(cands, guides, M, N):
    """the candidates file against itself and the guides file: by region then rank, ranks 1 .. shortlisted <= N, one picked
    row a region, the least by (tally, rank), equal to the region's row of the guides file"""
    assert [(int(c[0]), int(c[11])) for c in cands] == sorted((int(c[0]), int(c[11])) for c in cands)
    picked = {}
    for region, rows in _by_region(cands).items():
        assert [int(c[11]) for c in rows] == list(range(1, len(rows) + 1)) and len(rows) <= N
        assert all(int(c[12]) == len(rows) and len(c[13].split(",")) == M + 1 and c[14] in "01" for c in rows)
        rank, _ = ref.pick([[int(x) for x in c[13].split(",")] for c in rows], M)
        assert [c[14] for c in rows] == ["1" if j == rank else "0" for j in range(len(rows))], (region, rows)
        picked[region] = rows[rank][:14]
    assert [g[0] for g in guides] == list(picked) and all(g == picked[g[0]] for g in guides)
    return picked


@pytest.mark.parametrize("design", [False, True], ids=["plain", "design_primers"])
def test_the_command_line_on_c1_30_40_30(design, tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    if design:
        g, pam5, pam3, gc, min_mm, M = 20, "TV", "", (20, 80), 0, 1
        for name, v in _design_options(case).items():
            argv += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
        argv += ["--design-primers"]
    else:
        g, pam5, pam3, gc, min_mm, M = 28, "", "H", (30, 70), 0, 2
    flags = ["--guide-size", str(g), "--guide-gc", str(gc[0]), str(gc[1]), "--guide-min-mismatches", str(min_mm)]
    flags += (["--pam5", pam5] if pam5 else []) + (["--pam3", pam3] if pam3 else [])
    f = {n: str(tmp_path / n) for n in ("a.align", "b.align", "c.align", "plain.tsv", "one.tsv", "four.tsv", "four_c.tsv", "hits.tsv",
                                        "plain_hits.tsv", "decoy.tsv", "decoy_c.tsv", "decoy.fasta", "neutral.tsv", "neutral_c.tsv",
                                        "neutral.fasta")}
    picked_header = KF.GUIDE_HEADER + "\trank\tshortlisted\toutgroup_hits"
    mm = ["--guide-hit-mismatches", str(M)]

    # ---- without the option, and N = 1
    csv_plain = _main(argv + flags + ["-o", f["a.align"], "--out_guides", f["plain.tsv"], "--out_guide_hits", f["plain_hits.tsv"]] + mm)
    csv_one = _main(argv + flags + ["-o", f["b.align"], "--out_guides", f["one.tsv"], "--guide-candidates", "1"] + mm)
    plain = _table(f["plain.tsv"], KF.GUIDE_HEADER)
    one = _table(f["one.tsv"], picked_header)
    assert len(plain) > 0 and [r[:11] for r in one] == plain
    assert all(r[11] == "1" and r[12] == "1" for r in one)
    assert csv_one == csv_plain and csv_plain.count("\n") > 1
    assert open(f["a.align"], "rb").read() == open(f["b.align"], "rb").read() and os.path.getsize(f["a.align"]) > 0

    # ---- N = 4 with the hits and the candidates
    csv_four = _main(argv + flags + ["-o", f["c.align"], "--out_guides", f["four.tsv"], "--guide-candidates", "4", "--out_guide_hits",
                                     f["hits.tsv"], "--out_guide_candidates", f["four_c.tsv"]] + mm)
    assert csv_four == csv_plain and open(f["a.align"], "rb").read() == open(f["c.align"], "rb").read()
    four = _table(f["four.tsv"], picked_header)
    cands = _table(f["four_c.tsv"], picked_header + "\tpicked")
    hits = _table(f["hits.tsv"], KF.GUIDE_HIT_HEADER)
    assert [r[0] for r in four] == [r[0] for r in plain]
    counted = Counter((h[0], int(h[7])) for h in hits if h[1] in out)
    for r in four:
        assert [int(x) for x in r[13].split(",")] == [counted[(r[0], m)] for m in range(M + 1)], r
    picked = _check_candidates(cands, four, M, 4)
    assert [c[:11] for c in cands if c[11] == "1"] == plain                  # (rank 1 is today's guide)
    assert any(len(rows) > 1 for rows in _by_region(cands).values())
    # the candidates' tallies without the pick: N = 1 searches rank 1 alone and counts the same
    assert [r[13] for r in one] == [c[13] for c in cands if c[11] == "1"]
    print("design", design, "regions", len(four), "candidates", len(cands), "ranks", [r[11] for r in four],
          "tallies", [r[13] for r in four])

    # ---- a decoy.  A region's flanks lie in every genome, so an outgroup genome of random letters alone leaves no region: the
    # extra genome is the last outgroup genome once more, and the decoy is that genome with one more record -- random
    # letters that hold the rank-1 protospacers of a few regions, their motifs beside them, and nothing else of a template.
    # Both runs find the same regions with the same shortlists; the record's hits are all that differs
    raw = (gzip.open(out[-1], "rb") if out[-1].endswith(".gz") else open(out[-1], "rb")).read()
    raw += b"" if raw.endswith(b"\n") else b"\n"
    at = argv.index("--outgroup") + 1 + len(out)
    run = {}
    some = None
    for name in ("neutral", "decoy"):
        record = b""
        if name == "decoy":
            rng = random.Random(5)
            some = [c for c in run["neutral"][1] if c[11] == "1" and int(c[12]) > 1][:3]
            assert some
            text = ["".join(rng.choices("ACGT", k=300)) + c[4] + c[6] + c[5] for c in some for _ in range(COPIES)]
            record = (">decoy\n" + "".join(text) + "".join(rng.choices("ACGT", k=300)) + "\n").encode("ascii")
        with open(f[name + ".fasta"], "wb") as fa:
            fa.write(raw + record)
        csv = _main(argv[:at] + [f[name + ".fasta"]] + argv[at:] + flags + ["--out_guides", f[name + ".tsv"], "--guide-candidates", "4",
                                                                          "--out_guide_candidates", f[name + "_c.tsv"]] + mm)
        guides = _table(f[name + ".tsv"], picked_header)
        cands_ = _table(f[name + "_c.tsv"], picked_header + "\tpicked")
        run[name] = (csv, cands_, _check_candidates(cands_, guides, M, 4))      # (the rank the reference pick computes)
    (csv_n, cands_n, picked_n), (csv_d, cands_d, picked_d) = run["neutral"], run["decoy"]
    assert csv_n == csv_d and csv_n.count("\n") > 1                          # (the same regions)
    assert [c[:13] for c in cands_d] == [c[:13] for c in cands_n]             # (the same shortlists)
    was = {c[0]: c for c in cands_n if c[11] == "1"}
    now = {c[0]: c for c in cands_d if c[11] == "1"}
    changed = 0
    for c in some:
        region = c[0]
        assert int(now[region][13].split(",")[0]) >= int(was[region][13].split(",")[0]) + COPIES
        assert int(picked_d[region][11]) > 1, (region, _by_region(cands_d)[region])
        changed += picked_d[region][11] != picked_n[region][11]
    # a region the record does not name keeps its tallies
    assert all(c == d for c, d in zip(cands_n, cands_d) if c[0] not in {x[0] for x in some})
    print("decoyed", [c[0] for c in some], "ranks", [picked_d[c[0]][11] for c in some], "before", [picked_n[c[0]][11] for c in some])
    assert changed >= 1
