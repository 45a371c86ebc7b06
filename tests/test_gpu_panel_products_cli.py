"""--out_panel_products and --out_panel_summary end to end on the GPU, on the golden case c1_30_40_30 with --design-primers
--primer_size 18 24 --amp_size 70 100 --panel 8 and one more outgroup genome: the last one with a decoy record that holds
member 1's left primer facing itself, its two primers facing each other away from the locus, and a diverging pair.  The
file equals the reference's rows (multiplex_reference.py) on the inputs' text; every --out_primer_products row of a member's
region is a `pair` row and the converse; the single plant is a row, the diverging plant none; the summary is the rows
counted; every other output is byte-equal with and without the two options.  (The golden case gives one member: `cross`
is covered at KF.panel_products and below, in test_gpu_multiplex.py.)"""
import gzip
import io
import os
import random
import sys
from contextlib import redirect_stdout

import pytest

from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiplex_reference import rc                                         # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402
from test_gpu_multiplex import py_panel_rows                               # noqa: E402

pytestmark = pytest.mark.gpu

DESIGN = dict(primer_size=(18, 24), amp_size=(70, 100))
N = 8
APART = 1100                        # random letters between two plants: more than --max-product's default, no product spans two


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _table(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [tuple(ln.split("\t")) for ln in lines[1:-1]]


def test_the_command_line_on_c1_30_40_30_with_a_decoy(tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    k, omit = _amplicon(case), case["omit_soft"]
    # ---- the primers, from a first run of the stages
    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], k, omit_soft=omit)
    ingroup = [KF.simplename(p) for p in ing] if out else None
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **DESIGN)
    order = KF.panel_candidates(records)
    members, _ = KF.select_panel(templates[0], records, order, N, **DESIGN)
    oligos = KF.panel_oligos(templates[0], records, order, members)
    assert len(members) >= 1 and oligos[0][0] == "1L" and oligos[1][0] == "1R"
    L1, R1 = oligos[0][1], oligos[1][1]
    rcs = lambda t: rc(t.encode()).decode()                                                   # noqa: E731
    # ---- the decoy: the last outgroup genome once more, with one more record
    rng = random.Random(24)
    fill = lambda n: "".join(rng.choices("ACGT", k=n))                                        # noqa: E731
    plants = [L1 + fill(40) + rcs(L1), L1 + fill(55) + rcs(R1), rcs(R1) + fill(40) + L1]
    record, at = fill(APART), []
    for x in plants:
        at.append(len(record))
        record += x + fill(APART)
    raw = (gzip.open(out[-1], "rb") if out[-1].endswith(".gz") else open(out[-1], "rb")).read()
    raw += b"" if raw.endswith(b"\n") else b"\n"
    decoy = str(tmp_path / "decoy.fasta")
    with open(decoy, "wb") as fa:
        fa.write(raw + (">decoy\n" + record + "\n").encode("ascii"))
    out2 = out + [decoy]
    argv = _argv(case, tmp_path, ing, out2) + ["--design-primers", "--primer_size", "18", "24", "--amp_size", "70", "100"]
    f = {n: str(tmp_path / n) for n in ("a.align", "b.align", "a_prim", "b_prim", "a_panel", "b_panel", "rows", "summary", "summary_only")}
    common = lambda s: ["--out_primer_products", f[s + "_prim"], "--panel", str(N), "--out_panel", f[s + "_panel"]]   # noqa: E731
    csv_a = _main(argv + ["-o", f["a.align"]] + common("a"))
    csv_b = _main(argv + ["-o", f["b.align"]] + common("b") + ["--out_panel_products", f["rows"], "--out_panel_summary", f["summary"]])
    # ---- every other output is byte-equal
    assert csv_a == csv_b and csv_a.count("\n") > 1
    for x, y in (("a.align", "b.align"), ("a_prim", "b_prim"), ("a_panel", "b_panel")):
        assert open(f[x], "rb").read() == open(f[y], "rb").read() and os.path.getsize(f[x]) > 0, x
    # ... and the summary alone, for which no product comes to the host, has the same bytes
    _main(argv + common("b")[2:] + ["--out_panel_summary", f["summary_only"]])
    assert open(f["summary_only"], "rb").read() == open(f["summary"], "rb").read()
    panel = _table(f["b_panel"], KF.PANEL_HEADER)
    assert [(p[4], p[5]) for p in panel] == [(oligos[2 * j][1], oligos[2 * j + 1][1]) for j in range(len(members))]

    # ---- the file equals the reference's rows on the inputs' text
    got = _table(f["rows"], KF.PANEL_PRODUCT_HEADER)
    want = [tuple(str(v) for v in r) for r in py_panel_rows(ing + out2, oligos, 1, 1000, omit)]
    print("members", len(members), "rows", len(got), "kinds", sorted({r[8] for r in got}), "files", len({r[0] for r in got}))
    assert got == want and len(got) > 0

    # ---- every --out_primer_products row of a member's region is a pair row, column for column, and the converse
    prim = _table(f["b_prim"], KF.PRODUCT_HEADER)
    pair_rows = set()
    for j, p in enumerate(panel):
        lf, rt = f"{j + 1}L", f"{j + 1}R"
        for r in prim:
            if r[0] != p[1]:
                continue
            # (region, file, record, record_index, start, end, strand, length, left_mm, right_mm, left_end_mm, right_end_mm)
            where = r[1:6] + (r[7],)
            pair_rows.add(where + ((lf, rt, "pair", r[8], r[9], r[10], r[11]) if r[6] == "+" else (rt, lf, "pair", r[9], r[8], r[11], r[10])))
    assert pair_rows == {r for r in got if r[8] == "pair"} and len(pair_rows) >= len(ing)
    assert len(pair_rows) == sum(1 for r in got if r[8] == "pair")

    # ---- the plants: the single one is a row, the pair away from the locus too, the diverging one none
    in_decoy = [r for r in got if r[0] == decoy and r[1] == "decoy"]
    single = tuple(str(v) for v in (at[0], at[0] + len(plants[0]), len(plants[0]))) + ("1L", "1L", "single", "0", "0", "0", "0")
    assert any(r[3:] == single for r in in_decoy)
    assert any(r[3:9] == (str(at[1]), str(at[1] + len(plants[1])), str(len(plants[1])), "1L", "1R", "pair") for r in in_decoy)
    assert not any(int(r[4]) > at[2] for r in in_decoy)            # nothing ends inside or behind the diverging plant
    assert {r[8] for r in got} >= {"pair", "single"}

    # ---- the summary equals the rows counted
    names = [n for n, _ in oligos]
    files = ing + out2
    counted = {}
    for r in got:
        c = counted.setdefault((files.index(r[0]), names.index(r[6]), names.index(r[7])), [r, 0, 0])
        c[1] += 1
        c[2] += r[11] == "0" and r[12] == "0"
    want_sum = [(c[0][0], c[0][6], c[0][7], c[0][8], str(c[1]), str(c[2])) for _, c in sorted(counted.items())]
    assert _table(f["summary"], KF.PANEL_SUMMARY_HEADER) == want_sum and len(want_sum) >= 2
