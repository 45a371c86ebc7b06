"""Time the product pass (krisp_fasta --out_products: KF.predict_products, kr_products_*) and, beside it in the same run,
the locate pass's scan and the near-match scan.

  python tools/products_profile.py [--scan-bases 3000000000] [--groups 64] [--files] [--length 50000000] [--out FILE.json]

--scan-bases N: one genome of N random bases (no file: uploaded from memory, tools/near_profile.py's genome: the same seed)
with `--groups` windows of 100 bases cut from it as regions at 30/40/30, a third of them copied elsewhere with an insertion
and a substitution in a flank; kr_locate_scan against their flanks, then for M = 1 and M = 3 kr_near_scan against the
windows (the library takes any geometry; the command line's --out_near does not offer this one) and kr_products_scan
against the flanks (a warm-up and three timed calls each: the host clock around calls that end in a synchronise).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/products_profile.py ...` for the kernels' own times
(k_prod_scan<M + 1, 1, false> = the counting pass, <M + 1, 1, true> = the emitting pass over the tiles with sites,
k_prod_rec, k_prod_join; k_near_scan; k_loc_scan).
--files: four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup) as .fasta.gz, 30/40/30: the
command line end to end without --out_products and with it at M = 1, each in five fresh processes (a process per run,
each under its own time limit; a failing run ends the tool): medians.
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

from krisp_amd import _native, synth  # noqa: E402


def _timed(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.time()
        out = call()
        times.append(time.time() - t0)
    return min(times), out


def scan_part(n, groups):
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    bases[rng.integers(0, n, n // 10_000_000 + 1)] = ord("\n")
    L, D, R, k = 30, 40, 30, 100
    starts = rng.integers(0, n - k, groups)
    targets = np.unique(bases[starts[:, None] + np.arange(k)], axis=0)
    targets = targets[~(targets == ord("\n")).any(axis=1)]
    # a third of the regions once more elsewhere: five bases more in the diagnostic stretch, a substitution in the left flank
    for i, t in enumerate(targets[::3]):
        p = int(rng.integers(0, n - 2 * k))
        copy = np.concatenate([t[:L + 20], t[L + 5:L + 10], t[L + 20:]])
        copy[7] = ord("A") if copy[7] != ord("A") else ord("C")
        bases[p:p + len(copy)] = copy
    flanks = np.unique(np.concatenate([targets[:, :L], targets[:, L + D:]], axis=1), axis=0)
    left, li = np.unique(flanks[:, :L], axis=0, return_inverse=True)
    right, ri = np.unique(flanks[:, L:], axis=0, return_inverse=True)
    pairs = np.stack([li.ravel(), ri.ravel()], axis=1)
    res = {"scan_bases": n, "scan_targets": len(targets), "scan_regions": len(flanks), "geometry": [L, D, R]}
    with _native.Engine() as eng:
        eng.set_params_locate(L, D, R, False, max_bases=n)
        eng.upload(0, bases)
        eng.locate_table(flanks)
        res["locate_scan_s"], hits = _timed(lambda: eng.locate(0))
        res["locate_hits"] = len(hits)
        for M in (1, 3):
            eng.near_table(targets, M)
            res[f"near_scan_s_M{M}"], hits = _timed(lambda: eng.near(0))
            res[f"near_hits_M{M}"] = len(hits)
            eng.products_table(left, right, pairs, M, 1000)
            res[f"products_scan_s_M{M}"], hits = _timed(lambda: eng.products(0))
            res[f"products_M{M}"] = len(hits)
            res[f"products_inexact_M{M}"] = int(np.count_nonzero((hits["length"] != k) | (hits["left_mm"] > 0) | (hits["right_mm"] > 0)))
            res[f"product_sites_M{M}"] = len(eng.product_sites())
    return res


def files_part(length, td, runs=5, limit=600):
    fam = synth.family(7, 2, 2, length, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01)
    paths = []
    for name, _ing, text in fam:
        plain = os.path.join(td, f"{name}.fasta")
        synth.write_fasta(plain, text)
        p = plain + ".gz"
        with open(plain, "rb") as src, gzip.open(p, "wb", compresslevel=6) as dst:
            while True:
                block = src.read(1 << 24)
                if not block:
                    break
                dst.write(block)
        os.remove(plain)
        paths.append(p)
    del fam
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv")]
    res = {"genomes": len(paths), "bases_per_genome": length}
    prod = os.path.join(td, "products.tsv")
    for tag, extra in (("cli_without_products_s", []),
                       ("cli_with_products_M1_s", ["--out_products", prod, "--primer-mismatches", "1"])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(prod) as f:
        res["product_rows"] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scan-bases", type=int, default=0)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {}
    if args.scan_bases:
        res.update(scan_part(args.scan_bases, args.groups))
    if args.files:
        with tempfile.TemporaryDirectory(prefix="krisp_products_") as td:
            res.update(files_part(args.length, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
