"""Time the clean panel selection (krisp_fasta --panel-clean: KF.select_panel_clean, kr_panel_sites_*, kr_panel_run_clean,
DESIGN §26).

  python tools/panel_clean_profile.py [--length 50000000] [--kernel] [--files] [--out FILE.json]

The four synthetic genomes of tools/design_profile.py (2 ingroup / 2 outgroup) at 30/40/30 with the command line's default
primer options except --primer_size 18 24 and --amp_size 70 100; M = 1, --max-product 1000.
--kernel: the regions, their templates and pairs, the candidates in the panel's order and their distinct primer texts.  One
pass over the files with two tables in one engine: per file kr_primers_scan over the same candidates' pairs and
kr_panel_sites_scan (a warm-up and three timed calls each, the least; the host clock around a call that ends in a
synchronise), and the file's site count.  A second pass builds the store once more -- every file scanned once -- and times
kr_panel_run and kr_panel_run_clean over all candidates at N = 8 and N = 64 the same way, with the fates by cause.
--files: the command line end to end with --design-primers --panel 8, without --panel-clean and with it, each in five fresh
processes (a process per run, each under its own time limit; a failing run ends the tool): medians.
Progress goes to stderr (the kernel part's figures as soon as they stand); prints one JSON object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from krisp_amd import codec, reports, thermo  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from design_profile import FLAGS, OPTS, _timed, write_genomes  # noqa: E402

MISMATCHES, MAX_PRODUCT = 1, 1000


def say(text):
    print(f"[panel_clean_profile] {text}", file=sys.stderr, flush=True)


def kernel_part(paths):
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **OPTS)
    order = KF.panel_candidates(records)
    res = {"regions": len(records), "candidates": len(order)}
    say(f"{len(records)} regions, {len(order)} candidates")
    if len(order) == 0:
        return res
    t0 = time.time()
    texts, rows = KF.panel_candidate_texts(templates[0], records, order)
    res["texts_s"] = time.time() - t0
    res["texts"] = len(texts)
    t = np.ascontiguousarray(templates[0][order])
    pairs = np.stack([records[f][order] for f in ("left_start", "left_len", "right_start", "right_len")], axis=1).astype(np.uint16)
    # the primer pass over the same candidates: --out_primer_products' own table of the records (distinct texts and pairs)
    left, right, ppairs, _ = reports.primer_pairs(templates[0], records)
    res["primer_pass_texts"], res["primer_pass_pairs"] = len(left) + len(right), len(ppairs)
    Le, De, Re = codec.effective_geometry(30, 40, 30)

    def both_tables(eng):
        eng.primers_table(left + right, len(left), ppairs, MISMATCHES, MAX_PRODUCT)
        t1 = time.time()
        eng.panel_sites_table(texts, MISMATCHES, MAX_PRODUCT)
        res["panel_sites_table_s"] = time.time() - t1

    for eng, fi, _path, _rna, _recs in reports._scan_genomes(paths, Le, De, Re, 100, False, 0, both_tables):
        res[f"primers_scan_file{fi}_s"], products = _timed(lambda: eng.primers_scan(0))
        res[f"primers_products_file{fi}"] = products
        res[f"panel_sites_scan_file{fi}_s"], sites = _timed(lambda: eng.panel_sites_scan(0))
        res[f"sites_file{fi}"] = sites
        say(f"file {fi}: kr_primers_scan {res[f'primers_scan_file{fi}_s']:.4f} s ({products} products), kr_panel_sites_scan "
            f"{res[f'panel_sites_scan_file{fi}_s']:.4f} s ({sites} sites)")

    def selections(eng):
        res["stored_sites"] = len(eng.panel_sites()[1])
        eng.design_table(thermo.params(**OPTS))
        for n in (8, 64):
            res[f"panel_{n}_s"], (members, fates) = _timed(lambda: eng.panel(t, pairs, n))
            res[f"panel_{n}_fates"] = np.bincount(fates["fate"], minlength=6).tolist()
            res[f"panel_clean_{n}_s"], (cmembers, cfates, drops) = _timed(lambda: eng.panel_clean(t, pairs, rows, n))
            # alive, members, same locus, clash, cross, self-priming
            res[f"panel_clean_{n}_fates"] = np.bincount(cfates["fate"], minlength=6).tolist()
            res[f"panel_clean_{n}_members"] = len(cmembers)
            res[f"panel_clean_{n}_same_bytes_as_panel"] = int(cmembers.tobytes() == members.tobytes() and cfates.tobytes() == fates.tobytes())
            say(f"N = {n}: kr_panel_run {res[f'panel_{n}_s']:.4f} s, kr_panel_run_clean {res[f'panel_clean_{n}_s']:.4f} s, drops {drops.tolist()[:4]}")

    for eng, _fi, _path, _rna, _recs in reports._scan_genomes(paths, Le, De, Re, 100, False, 0,
                                                              lambda eng: eng.panel_sites_table(texts, MISMATCHES, MAX_PRODUCT),
                                                              last=selections):
        eng.panel_sites_scan(0)
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv"), "--design-primers"] + FLAGS + \
        ["--panel", "8", "--out_panel", os.path.join(td, "panel.tsv")]
    res = {}
    for tag, extra in (("cli_panel_s", []), ("cli_panel_clean_s", ["--panel-clean"])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
            say(f"{tag}: {times[-1]:.2f} s")
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(os.path.join(td, "panel.tsv")) as f:
        res["panel_rows"] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="the scans and the selections, call by call")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length, "mismatches": MISMATCHES, "max_product": MAX_PRODUCT}
    with tempfile.TemporaryDirectory(prefix="krisp_panel_clean_") as td:
        say("writing the genomes")
        paths = write_genomes(args.length, td)
        say("genomes written")
        if args.kernel:
            res.update(kernel_part(paths))
            say(json.dumps(res))
        if args.files:
            res.update(files_part(paths, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
