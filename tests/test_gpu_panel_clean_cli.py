"""--panel-clean end to end on the GPU, on a small synthetic family (krisp_amd.synth, the recipe of tools/panel_profile.py:
2 ingroup and 2 outgroup genomes at 30/40/30, --design-primers --primer_size 18 24 --amp_size 70 100 --panel 8) and one more
outgroup genome: the last one with a decoy record that holds member 1's left primer facing member 2's right primer and
member 3's left primer facing itself, for the members of the run WITHOUT the option.  That run's --out_panel_products has a
cross and a single row; the --panel-clean run's has pair rows only, member 3 is gone and so is one of members 1 and 2;
every output not derived from the panel is byte-equal with and without the option.

Two lengths.  At 200 kbp the files and the rows are checked.  At 40 kbp --out_panel is also held to the reference's selection
(panel_clean_reference.py) on the stages' own templates and records: the reference compares every candidate's primers with
every position of every file in plain loops, which at 200 kbp (some 700 candidates) takes minutes."""
import io
import os
import random
import sys
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest

from krisp_amd import fasta, synth, thermo
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_clean_reference as ref                                        # noqa: E402
from multiplex_reference import rc                                         # noqa: E402
from panel_reference import primers                                        # noqa: E402

pytestmark = pytest.mark.gpu

DESIGN = dict(primer_size=(18, 24), amp_size=(70, 100))
FLAGS = ["--primer_size", "18", "24", "--amp_size", "70", "100"]
N = 8
APART = 1100                        # random letters between two plants: more than --max-product's default, no product spans two


def _main(argv):
    out, err = io.StringIO(), io.StringIO()
    with redirect_stdout(out), redirect_stderr(err):
        assert KF.main(argv) == 0
    return out.getvalue(), err.getvalue()


def _table(path, header):
    lines = open(path).read().split("\n")
    assert lines[0] == header and lines[-1] == ""
    return [tuple(ln.split("\t")) for ln in lines[1:-1]]


def _stages(ing, out):
    groups, _ = KF.find_regions(ing, out, 30, 30, 100)
    ingroup = [KF.simplename(p) for p in ing]
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **DESIGN)
    return templates, records, KF.panel_candidates(records)


def _want_panel(templates, records, order, files):
    """the file's text from the reference's selection on the files' records joined by '\\n', the rows formatted here"""
    text = [bytes(r).decode("ascii") for r in templates]
    cands = order.tolist()
    pairs = [tuple(int(records[i][f]) for f in ("left_start", "left_len", "right_start", "right_len")) for i in cands]
    uploads = [b"\n".join(fasta.read_records(p)) for p in files]
    members, fates, drops = ref.select([text[i] for i in cands], pairs, N, thermo.options(**DESIGN)["max_sec"], uploads, False, 1, 1000)
    rank = np.cumsum(records["found"] != 0) - 1
    lines = [KF.PANEL_HEADER + "\tdropped_cross"]
    for j, m in enumerate(members):
        i = cands[m["position"]]
        left, right = primers(text[i], pairs[m["position"]])
        lines.append("\t".join([str(j + 1), str(int(rank[i])), thermo.milli(int(records[i]["pair_penalty"])),
                                str(int(records[i]["product_size"])), left, right, thermo.celsius(m["cross_any"]),
                                thermo.celsius(m["cross_end"]), str(m["dropped"][0]), str(m["dropped"][1]), str(drops[1 + j])]))
    return "\n".join(lines) + "\n", fates, drops


@pytest.mark.parametrize("length,with_reference", [(200_000, False), (40_000, True)], ids=["200kbp", "40kbp_reference"])
def test_the_command_line_on_a_synthetic_family_with_a_decoy(length, with_reference, tmp_path):
    paths = []
    for name, _ing, text in synth.family(7, 2, 2, length, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01):
        paths.append(str(tmp_path / f"{name}.fasta"))
        synth.write_fasta(paths[-1], text)
    ing, out = paths[:2], paths[2:]
    # ---- the members of the run without the option, from a first run of the stages
    templates, records, order = _stages(ing, out)
    plain, _ = KF.select_panel(templates[0], records, order, N, **DESIGN)
    oligos = dict(KF.panel_oligos(templates[0], records, order, plain))
    assert len(plain) >= 3, len(plain)                                     # the precondition: the test cannot pass empty
    # ---- the decoy: the last outgroup genome once more, with one more record
    rng = random.Random(26)
    fill = lambda n: "".join(rng.choices("ACGT", k=n))                                        # noqa: E731
    rcs = lambda t: rc(t.encode()).decode()                                                   # noqa: E731
    record = fill(APART) + oligos["1L"] + fill(40) + rcs(oligos["2R"]) + fill(APART) + oligos["3L"] + fill(40) + rcs(oligos["3L"]) + fill(APART)
    decoy = str(tmp_path / "decoy.fasta")
    with open(decoy, "wb") as fa:
        fa.write(open(out[-1], "rb").read() + (">decoy\n" + record + "\n").encode("ascii"))
    out2 = out + [decoy]
    templates2, records2, order2 = _stages(ing, out2)
    assert templates2[0].tobytes() == templates[0].tobytes() and records2.tobytes() == records.tobytes()    # the decoy moves no region
    argv = ing + ["--outgroup"] + out2 + ["--conserved", "30", "--amplicon", "100", "--design-primers"] + FLAGS
    f = {n: str(tmp_path / n) for n in ("a.align", "b.align", "a_prim", "b_prim", "a_panel", "b_panel", "a_rows", "b_rows", "a_sum", "b_sum")}
    common = lambda s: ["-o", f[s + ".align"], "--out_primer_products", f[s + "_prim"], "--panel", str(N), "--out_panel", f[s + "_panel"],   # noqa: E731
                        "--out_panel_products", f[s + "_rows"], "--out_panel_summary", f[s + "_sum"]]
    csv_a, err_a = _main(argv + common("a"))
    csv_b, err_b = _main(argv + common("b") + ["--panel-clean"])
    # ---- every output not derived from the panel is byte-equal
    assert csv_a == csv_b and csv_a.count("\n") > 1
    for x, y in (("a.align", "b.align"), ("a_prim", "b_prim")):
        assert open(f[x], "rb").read() == open(f[y], "rb").read() and os.path.getsize(f[x]) > 0, x
    assert "--panel-clean" not in err_a and "candidates prime with themselves" in err_b

    # ---- the plain run: its panel is the stages', its products hold the planted cross and single rows
    a_panel = _table(f["a_panel"], KF.PANEL_HEADER)
    assert [(p[4], p[5]) for p in a_panel] == [(oligos[f"{j + 1}L"], oligos[f"{j + 1}R"]) for j in range(len(plain))]
    a_rows = _table(f["a_rows"], KF.PANEL_PRODUCT_HEADER)
    assert any(r[0] == decoy and r[1] == "decoy" and r[6:9] == ("1L", "2R", "cross") for r in a_rows)
    assert any(r[0] == decoy and r[1] == "decoy" and r[6:9] == ("3L", "3L", "single") for r in a_rows)

    # ---- the clean run: pair rows only, plain member 3 gone, one of plain members 1 and 2 gone
    b_panel = _table(f["b_panel"], KF.PANEL_HEADER + "\tdropped_cross")
    b_rows = _table(f["b_rows"], KF.PANEL_PRODUCT_HEADER)
    kinds = {r[8] for r in b_rows}
    print("length", length, "candidates", len(order), "plain members", len(plain), "clean members", len(b_panel), "plain kinds",
          sorted({r[8] for r in a_rows}), "clean kinds", sorted(kinds), "rows", len(a_rows), len(b_rows), err_b.strip().split("\n")[-1])
    assert kinds == {"pair"} and len(b_rows) >= len(b_panel) * len(ing) > 0
    assert {r[3] for r in _table(f["b_sum"], KF.PANEL_SUMMARY_HEADER)} == {"pair"}
    kept = {(p[4], p[5]) for p in b_panel}
    assert (oligos["3L"], oligos["3R"]) not in kept
    assert (oligos["1L"], oligos["1R"]) not in kept or (oligos["2L"], oligos["2R"]) not in kept
    assert sum(int(p[10]) for p in b_panel) >= 1                            # a member says it dropped a candidate as cross

    # ---- the file equals the reference's selection on the stages' own templates and records
    if with_reference:
        want, fates, drops = _want_panel(templates[0], records, order, ing + out2)
        print("reference fates", np.bincount([x[0] for x in fates], minlength=6).tolist(), "drops", drops)
        assert open(f["b_panel"]).read() == want
        assert f"{drops[0]} of {len(order)} candidates" in err_b
