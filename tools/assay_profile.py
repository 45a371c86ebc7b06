"""Time the assay join (krisp_fasta --out_assay_hits: kr_assay_join) beside the two scans it follows, and the command line
with the option against the two files a user had to join before.

  python tools/assay_profile.py [--length 50000000] [--kernel] [--files] [--runs 5] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup, the files of tools/design_profile.py)
at 30/40/30, designed with --primer_size 18 24 --amp_size 70 100, guides of --guide-size 20 --pam5 TTTV
--guide-min-mismatches 0 between the primers, --primer-mismatches 1, --guide-hit-mismatches 2.
--kernel: the regions, their primer pairs, their guides and the links; then every genome is uploaded alone in one locate
context that holds the three tables, and kr_primers_scan, kr_guide_hits_scan and kr_assay_join are each called once to warm
up and three times under the host clock (a call ends in a synchronise; no fetch is timed): the least time per genome, and
the products, hits and assay hits of each.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/assay_profile.py
--kernel` (no counters in the same run) for the kernels' own times: k_assay_join<false / true> beside k_prim_scan,
k_prim_join, k_near_scan and k_ghit_finish.
--files: the command line end to end with --design-primers --out_guides, once with --out_primer_products --out_guide_hits
(the two files) and once with --out_assay_hits alone, each in `--runs` fresh processes (a process per run, each under its
own time limit; a failing run ends the tool): medians, and the rows of each file.
Prints one JSON object."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from krisp_amd import krisp_fasta as KF  # noqa: E402
from krisp_amd.reports import _scan_genomes  # noqa: E402
from design_profile import write_genomes  # noqa: E402

G, MP, MG, MAX_PRODUCT = 20, 1, 2, 1000
DESIGN = dict(primer_size=(18, 24), amp_size=(70, 100))
GUIDE = dict(guide_size=G, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=0)
FLAGS = ["--design-primers", "--primer_size", "18", "24", "--amp_size", "70", "100", "--guide-size", str(G), "--pam5", "TTTV",
         "--guide-min-mismatches", "0", "--primer-mismatches", str(MP), "--guide-hit-mismatches", str(MG)]


def _least(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def kernel_part(paths):
    import numpy as np
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    templates = KF.design_templates(groups, ingroup)
    records = KF.design_primers(groups, ingroup, templates=templates, **DESIGN)
    found = records["found"] != 0
    lo = records["left_start"].astype(np.int64) + records["left_len"]
    bounds = np.where(found[:, None], np.stack([lo, records["right_start"].astype(np.int64)], axis=1), 0).astype(np.uint32)
    regions = np.cumsum(found) - 1
    guides = KF.design_guides(groups, ingroup, bounds=bounds, templates=templates, **GUIDE)
    left, right, pairs, pairs_regions = KF.primer_pairs(templates[0], records)
    texts, text_regions = KF.guide_texts(templates[0], guides, G, regions=regions)
    links, _ = KF.assay_links(pairs_regions, text_regions)
    res = {"regions": len(groups), "regions_with_a_pair": int(found.sum()), "primer_pairs": len(pairs), "guide_texts": len(texts),
           "links": len(links), "guide_size": G, "primer_mismatches": MP, "guide_hit_mismatches": MG, "per_genome": []}
    if not len(links):
        return res
    t = np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(-1, G)

    def tables(eng):
        eng.primers_table(left + right, len(left), pairs, MP, MAX_PRODUCT)
        eng.guide_hits_table(t, MG, GUIDE["pam5"], GUIDE["pam3"], False)
        eng.assay_table(links)

    for eng, fi, path, _rna, _names in _scan_genomes(paths, 0, G, 0, G, False, 0, tables):
        tp, n_products = _least(lambda: eng.primers_scan(0))
        th, n_hits = _least(lambda: eng.guide_hits_scan(0))
        tj, n_assay = _least(lambda: eng.assay_join(0))
        res["per_genome"].append({"file": os.path.basename(path), "primers_scan_s": round(tp, 5), "guide_hits_scan_s": round(th, 5),
                                  "assay_join_s": round(tj, 5), "products": int(n_products), "hits": int(n_hits),
                                  "assay_hits": int(n_assay)})
        print(f"genome {fi}: {res['per_genome'][-1]}", file=sys.stderr, flush=True)
    for key in ("primers_scan_s", "guide_hits_scan_s", "assay_join_s"):
        res[key + "_sum"] = round(sum(g[key] for g in res["per_genome"]), 5)
    return res


def _rows(path):
    with open(path) as f:
        return sum(1 for _ in f) - 1


def files_part(paths, td, runs, limit=600):
    f = {n: os.path.join(td, n + ".tsv") for n in ("guides", "primer_products", "guide_hits", "assay_hits")}
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv")] + FLAGS + ["--out_guides", f["guides"]]
    res = {}
    for tag, extra in (("cli_two_files_s", ["--out_primer_products", f["primer_products"], "--out_guide_hits", f["guide_hits"]]),
                       ("cli_assay_hits_s", ["--out_assay_hits", f["assay_hits"]])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
            print(f"{tag}: {times[-1]:.3f}", file=sys.stderr, flush=True)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(x, 3) for x in times]
    res["primer_product_rows"] = _rows(f["primer_products"])
    res["guide_hit_rows"] = _rows(f["guide_hits"])
    res["assay_hit_rows"] = _rows(f["assay_hits"])
    res["guide_rows"] = _rows(f["guides"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="the two scans and the join over every genome")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_assay_") as td:
        paths = write_genomes(args.length, td)
        if args.kernel:
            res.update(kernel_part(paths))
            if args.out:                                   # (the scans' figures are kept if a command-line run fails)
                with open(args.out, "w") as f:
                    f.write(json.dumps(res) + "\n")
        if args.files:
            res.update(files_part(paths, td, args.runs))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
