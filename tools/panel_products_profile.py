"""Time the multiplex pass (krisp_fasta --out_panel_products / --out_panel_summary: KF.panel_products, kr_multiplex_*).

  python tools/panel_products_profile.py [--length 50000000] [--kernel] [--files] [--out FILE.json]

The four synthetic genomes of tools/panel_profile.py (2 ingroup / 2 outgroup) at 30/40/30 with the command line's default
primer options except --primer_size 18 24 and --amp_size 70 100; M = 1, max_product = 1000.
--kernel: the regions, their pairs and the panel at N = 8 and N = 64; then, per genome resident on the device,
kr_multiplex_scan over the panel's oligos beside kr_primers_scan over the same members' pairs (a warm-up and three timed
calls each, the least; the host clock around a call that ends in a synchronise), kr_multiplex_tally, and the numbers of
sites and products beside the times.  The site scan is k_prim_scan over the same number of entries in both passes: a
multiplex time far above the primer pass's points at the join or at dense output, and the counts say which.
--files: the command line end to end with --design-primers --panel 8, without and with the two options, each in five fresh
processes (a process per run, each under its own time limit; a failing run ends the tool): medians.
Progress goes to stderr; prints one JSON object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from krisp_amd import codec  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from design_profile import FLAGS, OPTS, _timed, write_genomes  # noqa: E402

M, MAX_PRODUCT = 1, 1000
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def say(text):
    print(f"[panel_products_profile] {text}", file=sys.stderr, flush=True)


def kernel_part(paths):
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    say(f"{len(groups)} regions")
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **OPTS)
    order = KF.panel_candidates(records)
    res = {"regions": len(groups), "candidates": len(order), "mismatches": M, "max_product": MAX_PRODUCT}
    if len(order) == 0:
        return res
    Le, De, Re = codec.effective_geometry(30, 40, 30)
    for n in (8, 64):
        members, _ = KF.select_panel(templates[0], records, order, n, **OPTS)
        oligos = KF.panel_oligos(templates[0], records, order, members)
        texts, _owners = KF.panel_texts(oligos)
        # the same members' pairs for the primer pass: a right text is the template's text under the right primer
        left = [t.encode() for _, t in oligos[0::2]]
        right = [t.encode()[::-1].translate(_COMP) for _, t in oligos[1::2]]
        pairs = [(m, m) for m in range(len(left))]

        def tables(eng):
            eng.multiplex_table(texts, M, MAX_PRODUCT)
            eng.primers_table(left + right, len(left), pairs, M, MAX_PRODUCT)

        per = []
        for eng, fi, path, _rna, _names in KF._scan_genomes(paths, Le, De, Re, 100, False, 0, tables):
            mux_s, products = _timed(lambda: eng.multiplex_scan(0))
            tally_s, tally = _timed(eng.multiplex_tally)
            prim_s, pair_products = _timed(lambda: eng.primers_scan(0))
            per.append({"file": os.path.basename(path), "multiplex_scan_s": mux_s, "primers_scan_s": prim_s, "tally_s": tally_s,
                        "sites": len(eng.multiplex_sites()), "primer_sites": len(eng.primer_sites()), "products": int(products),
                        "pair_products": int(pair_products), "tally_cells": int((tally.sum(axis=2) != 0).sum()),
                        "clean_end_products": int(tally[:, :, 1].sum())})
            say(f"N = {n} {per[-1]}")
        res[f"panel_{n}"] = {"members": len(members), "oligo_texts": len(texts), "genomes": per}
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv"), "--design-primers"] + FLAGS + \
        ["--panel", "8", "--out_panel", os.path.join(td, "panel.tsv")]
    both = ["--out_panel_products", os.path.join(td, "pp.tsv"), "--out_panel_summary", os.path.join(td, "ps.tsv")]
    res = {}
    for tag, extra in (("cli_without_s", []), ("cli_with_s", both)):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
            say(f"{tag}: {times[-1]:.2f} s")
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    for name in ("pp.tsv", "ps.tsv"):
        with open(os.path.join(td, name)) as f:
            res[name + "_rows"] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="kr_multiplex_scan and kr_multiplex_tally beside kr_primers_scan, per genome")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_panel_products_") as td:
        say("writing the genomes")
        paths = write_genomes(args.length, td)
        say("genomes written")
        if args.kernel:
            res.update(kernel_part(paths))
        if args.files:
            res.update(files_part(paths, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
