"""--primer-candidates end to end on the GPU, on the golden case c1_30_40_30: N = 1 writes the bytes of the run without the
option; with N = 4 every picked pair's tally is the count of its region's rows in the --out_primer_products file of the same
run, the pick is the plain-loop pick of the candidates file's own tallies and rank 1 is the pair of the run without the
option; an extra outgroup genome with a decoy record that holds the rank-1 primers' sites makes a region pick another rank,
and the picked pair reaches the files downstream."""
import gzip
import io
import os
import random
import sys
from collections import Counter
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import design_shortlist_reference as SR                                    # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402
from test_gpu_primers import _design_options                               # noqa: E402

pytestmark = pytest.mark.gpu

COPIES = 3                          # of a pair's two sites in the decoy
M = 1                               # --primer-mismatches
G, PAM5, GC, MIN_MM = 20, "TV", (20, 80), 0      # the guide options of test_gpu_guide_candidates_cli.py's design run
_COMP = str.maketrans("ACGT", "TGCA")


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _table(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [ln.split("\t") for ln in lines[1:-1]]


def _by_region(rows):
    out = {}
    for r in rows:
        out.setdefault(r[0], []).append(r)
    return out


def _check_candidates(cands, N):
    """the candidates file against itself: by region then rank, ranks 1 .. shortlisted <= N, one picked row a region, the one
    the plain loops pick from the file's own tallies -> the picked row of every region"""
    assert [(int(c[0]), int(c[1])) for c in cands] == sorted((int(c[0]), int(c[1])) for c in cands)
    picked = {}
    by = _by_region(cands)
    assert [int(r) for r in by] == list(range(len(by)))             # (every region with a pair, numbered in order)
    for region, rows in by.items():
        assert [int(c[1]) for c in rows] == list(range(1, len(rows) + 1)) and len(rows) <= N
        assert all(int(c[2]) == len(rows) and len(c[11].split(",")) == 2 * M + 2 and c[12] in "01" for c in rows)
        rank = SR.pick([tuple(int(x) for x in c[11].split(",")) for c in rows])
        assert [c[12] for c in rows] == ["1" if j == rank else "0" for j in range(len(rows))], (region, rows)
        picked[region] = rows[rank]
    return picked


def _csv_pairs(csv):
    """the CSV's data rows -> (left_sequence, right_sequence, left_start, left_length, right_start, right_length) each"""
    lines = csv.split("\n")
    header = lines[0].split(",")
    at = [header.index(n) for n in ("left_sequence", "right_sequence", "left_start", "left_length", "right_start", "right_length")]
    return [[ln.split(",")[i] for i in at] for ln in lines[1:-1]]


def test_the_command_line_on_c1_30_40_30(tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out)
    for name, v in _design_options(case).items():
        argv += ["--" + name] + [str(x) for x in (v if isinstance(v, tuple) else (v,))]
    argv += ["--design-primers"]
    guide_flags = ["--guide-size", str(G), "--guide-gc", str(GC[0]), str(GC[1]), "--guide-min-mismatches", str(MIN_MM), "--pam5", PAM5]
    mm = ["--primer-mismatches", str(M)]

    def outputs(tag):
        f = {n: str(tmp_path / f"{tag}.{n}") for n in ("align", "products", "guides", "assay", "cands")}
        return f, ["-o", f["align"], "--out_primer_products", f["products"], "--out_guides", f["guides"], "--out_assay_hits",
                   f["assay"]] + guide_flags + mm

    # ---- without the option, and N = 1: every output's bytes
    fp, flags = outputs("plain")
    csv_plain = _main(argv + flags)
    f1, flags = outputs("one")
    csv_one = _main(argv + flags + ["--primer-candidates", "1", "--out_primer_candidates", f1["cands"]])
    assert csv_one == csv_plain and csv_plain.count("\n") > 1
    for n in ("align", "products", "guides", "assay"):
        assert open(f1[n], "rb").read() == open(fp[n], "rb").read() and os.path.getsize(fp[n]) > 0, n
    plain_pairs = _csv_pairs(csv_plain)
    one = _table(f1["cands"], KF.PRIMER_CANDIDATE_HEADER)
    assert [c[5:11] for c in one] == plain_pairs and all(c[1] == "1" and c[2] == "1" and c[12] == "1" for c in one)

    # ---- N = 4 with the products and the candidates
    f4, flags = outputs("four")
    csv_four = _main(argv + flags + ["--primer-candidates", "4", "--out_primer_candidates", f4["cands"]])
    cands = _table(f4["cands"], KF.PRIMER_CANDIDATE_HEADER)
    prods = _table(f4["products"], KF.PRODUCT_HEADER)
    picked = _check_candidates(cands, 4)
    assert [c[5:11] for c in cands if c[1] == "1"] == plain_pairs             # (rank 1 is the pair of the run without the option)
    assert [c[11] for c in cands if c[1] == "1"] == [c[11] for c in one]       # (N = 1 searches rank 1 alone and counts the same)
    assert any(len(rows) > 1 for rows in _by_region(cands).values())
    assert _csv_pairs(csv_four) == [picked[str(r)][5:11] for r in range(len(picked))]
    by_sum = Counter((p[0], int(p[8]) + int(p[9])) for p in prods)
    clean = Counter(p[0] for p in prods if p[10] == "0" and p[11] == "0")
    for region, c in picked.items():
        assert [int(x) for x in c[11].split(",")] == [clean[region]] + [by_sum[(region, m)] for m in range(2 * M + 1)], c
        assert clean[region] >= len(ing)                                      # (the designed locus in every ingroup genome)
    print("regions", len(picked), "candidates", len(cands), "ranks", [c[1] for c in picked.values()],
          "tallies", [c[11] for c in picked.values()])

    # ---- a decoy.  The extra genome is the last outgroup genome once more (an outgroup genome of random letters alone would
    # leave no region); the decoy is that genome with one more record: random letters that hold, for a few regions, the rank-1
    # left primer, a spacer and the rank-1 right primer's site.  Both runs find the same regions with the same shortlists
    raw = (gzip.open(out[-1], "rb") if out[-1].endswith(".gz") else open(out[-1], "rb")).read()
    raw += b"" if raw.endswith(b"\n") else b"\n"
    at = argv.index("--outgroup") + 1 + len(out)
    run, some = {}, None
    for name in ("neutral", "decoy"):
        record = b""
        if name == "decoy":
            rng = random.Random(5)
            some = [c for c in run["neutral"][1] if c[1] == "1" and int(c[2]) > 1][:4]
            assert some
            text = ["".join(rng.choices("ACGT", k=300)) + c[5] + "".join(rng.choices("ACGT", k=40)) + c[6][::-1].translate(_COMP)
                    for c in some for _ in range(COPIES)]
            record = (">decoy\n" + "".join(text) + "".join(rng.choices("ACGT", k=300)) + "\n").encode("ascii")
        fasta = str(tmp_path / (name + ".fasta"))
        with open(fasta, "wb") as fa:
            fa.write(raw + record)
        f, flags = outputs(name)
        csv = _main(argv[:at] + [fasta] + argv[at:] + flags + ["--primer-candidates", "4", "--out_primer_candidates", f["cands"]])
        cands_ = _table(f["cands"], KF.PRIMER_CANDIDATE_HEADER)
        run[name] = (csv, cands_, _check_candidates(cands_, 4), f)          # (every pick equals the plain-loop pick)
    (csv_n, cands_n, picked_n, _), (csv_d, cands_d, picked_d, fd) = run["neutral"], run["decoy"]
    assert [c[:11] for c in cands_d] == [c[:11] for c in cands_n] and csv_n.count("\n") == csv_d.count("\n") > 1
    was = {c[0]: c for c in cands_n if c[1] == "1"}
    now = {c[0]: c for c in cands_d if c[1] == "1"}
    named = {c[0] for c in some}
    for region in named:
        a, b = ([int(x) for x in t[region][11].split(",")] for t in (was, now))
        assert b[0] >= a[0] + COPIES and b[1] >= a[1] + COPIES               # (clean and exact products of the decoy)
    assert all(c == d for c, d in zip(cands_n, cands_d) if c[0] not in named)
    moved = [r for r in sorted(named, key=int) if int(picked_d[r][1]) > 1]
    print("decoyed", sorted(named, key=int), "ranks", [picked_d[r][1] for r in sorted(named, key=int)],
          "before", [picked_n[r][1] for r in sorted(named, key=int)])
    assert moved and any(picked_d[r][1] != picked_n[r][1] for r in moved)

    # ---- the picked pair reaches the files downstream: the CSV row, the products and the guide's bounds of a moved region
    csv_pairs = _csv_pairs(csv_d)
    prods_d = _by_region(_table(fd["products"], KF.PRODUCT_HEADER))
    for region in moved:
        c = picked_d[region]
        assert csv_pairs[int(region)] == c[5:11] != was[region][5:11]
        exact = [p for p in prods_d[region] if p[8:12] == ["0", "0", "0", "0"]]
        assert all(any(p[1] == f and p[7] == c[4] for p in exact) for f in ing)    # (the new pair's product in every ingroup genome)
        assert [int(x) for x in c[11].split(",")][0] == sum(1 for p in prods_d[region] if p[10] == "0" and p[11] == "0")
    # the guides file is what the guide pass gives between the picked pairs' primers
    k = _amplicon(case)
    groups, _ = KF.find_regions(ing, out + [str(tmp_path / "decoy.fasta")], case["L"], case["R"], k, omit_soft=case["omit_soft"])
    ingroup = [KF.simplename(f) for f in ing]
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **_design_options(case))
    found = records["found"] != 0
    assert int(found.sum()) == len(picked_d)
    bounds = np.zeros((len(records), 2), dtype=np.uint32)
    for region, c in picked_d.items():
        bounds[np.flatnonzero(found)[int(region)]] = (int(c[7]) + int(c[8]), int(c[9]))
    guides = KF.design_guides(groups, ingroup, G, PAM5, "", GC, MIN_MM, bounds=bounds, templates=templates)
    want = str(tmp_path / "want.guides")
    KF.write_guides(want, templates[0], guides, G, pam5_len=len(PAM5), pam3_len=0, regions=np.cumsum(found) - 1)
    assert open(want, "rb").read() == open(fd["guides"], "rb").read() and os.path.getsize(want) > len(KF.GUIDE_HEADER) + 1
