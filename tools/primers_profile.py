"""Time the primer-product pass (krisp_fasta --design-primers --out_primer_products: KF.primer_products, kr_primers_*) beside
the flank pass (kr_products_*) on the same genomes.

  python tools/primers_profile.py [--length 50000000] [--runs 5] [--no-cli] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup) as .fasta.gz, 30/40/30, designed with
--primer_size 18 24 --amp_size 70 100.  The command line end to end with --design-primers, without and with
--out_primer_products at M = 1, each in `--runs` fresh processes (a process per run, each under its own time limit; a
failing run ends the tool): medians.  Then, in this process, every genome uploaded alone and scanned by kr_primers_scan
against the designed pairs and by kr_products_scan against the regions' flanks, M = 1, max_product 1000 (a warm-up and
three timed calls each: the host clock around calls that end in a synchronise; the least of the three).
Prints one JSON object."""
import argparse
import gzip
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

from krisp_amd import codec, synth  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from krisp_amd.reports import _group_flanks, _scan_genomes  # noqa: E402

DESIGN = ["--primer_size", "18", "24", "--amp_size", "70", "100"]


def _timed(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.time()
        out = call()
        times.append(time.time() - t0)
    return min(times), out


def write_family(length, td):
    fam = synth.family(7, 2, 2, length, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01)
    paths = []
    for name, _ing, text in fam:
        plain = os.path.join(td, f"{name}.fasta")
        synth.write_fasta(plain, text)
        p = plain + ".gz"
        with open(plain, "rb") as src, gzip.open(p, "wb", compresslevel=1) as dst:
            while True:
                block = src.read(1 << 24)
                if not block:
                    break
                dst.write(block)
        os.remove(plain)
        paths.append(p)
    return paths


def cli_part(paths, td, runs, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv"), "--design-primers"] + DESIGN
    res = {}
    prod = os.path.join(td, "primer_products.tsv")
    for tag, extra in (("cli_design_s", []), ("cli_design_with_primer_products_M1_s", ["--out_primer_products", prod])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(prod) as f:
        res["primer_product_rows"] = sum(1 for _ in f) - 1
    with open(os.path.join(td, "out.csv")) as f:
        res["csv_rows"] = sum(1 for _ in f) - 1
    return res


def scan_part(paths):
    L, R, k, M, mp = 30, 30, 100, 1, 1000
    ing, out = paths[:2], paths[2:]
    groups, _ = KF.find_regions(ing, out, L, R, k)
    ingroup = [KF.simplename(f) for f in ing]
    records = KF.design_primers(groups, ingroup, primer_size=(18, 24), amp_size=(70, 100))
    rows, _, _, _ = KF.design_templates(groups, ingroup)
    left, right, pairs, regions = KF.primer_pairs(rows, records)
    Le, De, Re = codec.effective_geometry(L, k - L - R, R)
    flanks = _group_flanks(groups, Le, Re)
    fl, li = np.unique(flanks[:, :Le], axis=0, return_inverse=True)
    fr, ri = np.unique(flanks[:, Le:], axis=0, return_inverse=True)
    fpairs = np.stack([li.ravel(), ri.ravel()], axis=1).astype(np.uint32)
    res = {"regions": len(groups), "regions_with_a_pair": int((records["found"] != 0).sum()), "primer_texts": len(left) + len(right),
           "primer_pairs": len(pairs), "primer_lengths": sorted({len(t) for t in left + right}), "flank_texts": len(fl) + len(fr),
           "per_genome": []}

    def tables(eng):
        eng.primers_table(left + right, len(left), pairs, M, mp)
        eng.products_table(fl, fr, fpairs, M, mp)

    for eng, fi, path, _rna, _names in _scan_genomes(paths, Le, De, Re, k, False, 0, tables):
        tp, hp = _timed(lambda: eng.primer_products(0))
        nsp = len(eng.primer_sites())
        tf, hf = _timed(lambda: eng.products(0))
        res["per_genome"].append({"file": os.path.basename(path), "primers_scan_s": round(tp, 4), "primer_sites": nsp,
                                  "primer_products": len(hp), "products_scan_s": round(tf, 4), "flank_sites": len(eng.product_sites()),
                                  "flank_products": len(hf)})
    res["primers_scan_s_median"] = statistics.median(g["primers_scan_s"] for g in res["per_genome"])
    res["products_scan_s_median"] = statistics.median(g["products_scan_s"] for g in res["per_genome"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true", help="the scans alone")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_primers_") as td:
        paths = write_family(args.length, td)
        res.update(scan_part(paths))
        if args.out:                                       # (the scans' figures are kept if a command-line run fails)
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        if not args.no_cli:
            res.update(cli_part(paths, td, args.runs))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
