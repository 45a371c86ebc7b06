"""--panel end to end on the GPU, on the golden case c1_30_40_30 with --design-primers --primer_size 18 24 --amp_size 70 100
--panel 8: the file equals the reference's selection (panel_reference.py) computed from the same templates and records, alone
and with --out_guides (then no member is without a guide and the order follows min_mismatches); with and without the option
the CSV, the alignments and every other --out_* file are byte-equal."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import thermo
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_reference as ref                                               # noqa: E402
from test_locate_host import FC                                            # noqa: E402
from test_gpu_locate import _amplicon, _argv, _files                       # noqa: E402

pytestmark = pytest.mark.gpu

DESIGN = dict(primer_size=(18, 24), amp_size=(70, 100))
GUIDES = dict(guide_size=20, pam5="TV", pam3="", gc=(20, 80), min_mismatches=0)
N = 8


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _want(templates, records, guides):
    """the file's text from the reference's selection: the order by a plain sort, the rows formatted here"""
    text = [bytes(r).decode("ascii") for r in templates]
    cands = [i for i in range(len(records)) if int(records[i]["found"]) and (guides is None or int(guides[i]["found"]))]
    if guides is None:
        cands.sort(key=lambda i: (int(records[i]["pair_penalty"]), i))
    else:
        cands.sort(key=lambda i: (-int(guides[i]["min_mismatches"]), int(records[i]["pair_penalty"]), i))
    pairs = [tuple(int(records[i][f]) for f in ("left_start", "left_len", "right_start", "right_len")) for i in cands]
    members, fates = ref.select([text[i] for i in cands], pairs, N, thermo.options(**DESIGN)["max_sec"])
    rank = np.cumsum(records["found"] != 0) - 1
    lines = [KF.PANEL_HEADER]
    for j, m in enumerate(members):
        i = cands[m["position"]]
        left, right = ref.primers(text[i], pairs[m["position"]])
        lines.append("\t".join([str(j + 1), str(int(rank[i])), thermo.milli(int(records[i]["pair_penalty"])),
                                str(int(records[i]["product_size"])), left, right, thermo.celsius(m["cross_any"]),
                                thermo.celsius(m["cross_end"]), str(m["dropped"][0]), str(m["dropped"][1])]))
    return "\n".join(lines) + "\n", cands, members, fates


@pytest.mark.parametrize("with_guides", [False, True], ids=["pairs", "pairs_and_guides"])
def test_the_command_line_on_c1_30_40_30(with_guides, tmp_path):
    case = next(c for c in FC if c["name"] == "c1_30_40_30")
    ing, out = _files(case, tmp_path)
    argv = _argv(case, tmp_path, ing, out) + ["--design-primers", "--primer_size", "18", "24", "--amp_size", "70", "100"]
    others = ["products", "guides", "hits", "assay"] if with_guides else ["products"]
    f = {n: str(tmp_path / n) for n in ["a.align", "b.align", "panel.tsv", "again.tsv"] + [s + x for s in ("a_", "b_") for x in others]}

    def outputs(side):
        o = ["--out_primer_products", f[side + "products"]]
        if with_guides:
            g = GUIDES
            o += ["--out_guides", f[side + "guides"], "--guide-size", str(g["guide_size"]), "--pam5", g["pam5"], "--guide-gc",
                  str(g["gc"][0]), str(g["gc"][1]), "--guide-min-mismatches", str(g["min_mismatches"]), "--out_guide_hits",
                  f[side + "hits"], "--guide-hit-mismatches", "1", "--out_assay_hits", f[side + "assay"]]
        return o

    csv_a = _main(argv + ["-o", f["a.align"]] + outputs("a_"))
    csv_b = _main(argv + ["-o", f["b.align"]] + outputs("b_") + ["--panel", str(N), "--out_panel", f["panel.tsv"]])
    _main(argv + outputs("b_") + ["--panel", str(N), "--out_panel", f["again.tsv"]])
    assert csv_a == csv_b and csv_a.count("\n") > 1
    assert open(f["a.align"], "rb").read() == open(f["b.align"], "rb").read() and os.path.getsize(f["a.align"]) > 0
    for x in others:
        assert open(f["a_" + x], "rb").read() == open(f["b_" + x], "rb").read() and os.path.getsize(f["a_" + x]) > 0, x
    got = open(f["panel.tsv"]).read()
    assert got == open(f["again.tsv"]).read()

    # ---- the stages again, and the reference's selection on what they give
    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], _amplicon(case), omit_soft=case["omit_soft"])
    ingroup = [KF.simplename(p) for p in ing] if out else None
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **DESIGN)
    found = records["found"] != 0
    guides = None
    if with_guides:
        lo = records["left_start"].astype(np.int64) + records["left_len"]
        bounds = np.where(found[:, None], np.stack([lo, records["right_start"].astype(np.int64)], axis=1), 0).astype(np.uint32)
        g = GUIDES
        guides = KF.design_guides(groups, ingroup, g["guide_size"], g["pam5"], g["pam3"], g["gc"], g["min_mismatches"], bounds=bounds,
                                  templates=templates)
    want, cands, members, fates = _want(templates[0], records, guides)
    print("guides", with_guides, "regions", len(groups), "with a pair", int(found.sum()), "candidates", len(cands), "members", len(members),
          "fates", fates)
    assert got == want
    assert KF.panel_candidates(records, guides).tolist() == cands
    lines = got.split("\n")
    assert lines[0] == KF.PANEL_HEADER and lines[-1] == "" and len(lines) - 2 == len(members)
    assert 1 <= len(members) <= N
    # a member's region is a data row of the CSV, and its primers are that row's
    header = csv_b.split("\n")[0].split(",")
    data = [ln.split(",") for ln in csv_b.split("\n")[1:-1]]
    for ln in lines[1:-1]:
        c = ln.split("\t")
        row = dict(zip(header, data[int(c[1])]))
        assert (row["left_sequence"], row["right_sequence"], row["pair_penalty"], row["product_size"]) == (c[4], c[5], c[2], c[3])
    if with_guides:
        with_guide = {ln.split("\t")[0] for ln in open(f["b_guides"]).read().split("\n")[1:-1]}
        assert all(ln.split("\t")[1] in with_guide for ln in lines[1:-1])
        mm = [int(guides[i]["min_mismatches"]) for i in cands]
        assert mm == sorted(mm, reverse=True)
