"""Time the locate pass (krisp_fasta --out_locations: KF.locate_regions, kr_locate_*) alone and inside the command line.

  python tools/locate_profile.py [--length 50000000] [--scan-bases 3000000000] [--no-files] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup) are written as FASTA files; then,
from those files, at 25/1/2:
  * find_regions alone and locate_regions alone;
  * the command line end to end without --out_locations and with it (in this Python process: the library is loaded
    once for both; the better of two runs each).
--scan-bases N: one genome of N random bases (no file: uploaded from memory) with a few regions planted, the scan alone
(kr_locate_scan), at the scale of a human genome.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/locate_profile.py ...` for the kernels' own times (k_loc_scan,
k_loc_sep, k_loc_cut); the bytes per base of the scan = its reads (the bases once, plus k - 1 of overlap per 16 K starts)
over the bases.  Prints one JSON object."""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from krisp_amd import _native, synth  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402


def files_part(args, td):
    fam = synth.family(7, 2, 2, args.length, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01)
    paths = []
    for name, _ing, text in fam:
        p = os.path.join(td, f"{name}.fa")
        synth.write_fasta(p, text)
        paths.append(p)
    del fam
    ing, out = paths[:2], paths[2:]
    res = {"genomes": len(paths), "bases_per_genome": args.length}
    KF.find_regions(ing, out, 25, 2, 28)                     # warm-up: code objects, host threads
    t0 = time.time()
    groups, _ = KF.find_regions(ing, out, 25, 2, 28)
    res["find_regions_s"] = time.time() - t0
    res["regions"] = len(groups)
    KF.locate_regions(groups, ing, out, 25, 2, 28)
    t0 = time.time()
    locs = KF.locate_regions(groups, ing, out, 25, 2, 28)
    res["locate_regions_s"] = time.time() - t0
    res["rows"] = len(locs)
    argv = ing + ["--outgroup"] + out + ["--conserved-left", "25", "--conserved-right", "2", "--diagnostic", "1"]
    for tag, extra in (("cli_without_flag_s", []), ("cli_with_flag_s", ["--out_locations", os.path.join(td, "loc.tsv")])):
        best = None
        for _ in range(2):
            t0 = time.time()
            with redirect_stdout(io.StringIO()):
                KF.main(argv + extra)
            dt = time.time() - t0
            best = dt if best is None else min(best, dt)
        res[tag] = best
    res["locate_share_of_cli"] = (res["cli_with_flag_s"] - res["cli_without_flag_s"]) / res["cli_with_flag_s"]
    return res


def scan_part(n):
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    bases[rng.integers(0, n, n // 10_000_000 + 1)] = ord("\n")
    k = 28
    starts = rng.integers(0, n - k, 64)
    flanks = np.unique(np.concatenate([bases[starts[:, None] + np.arange(25)], bases[starts[:, None] + 26 + np.arange(2)]],
                                      axis=1), axis=0)
    flanks = flanks[~(flanks == ord("\n")).any(axis=1)]
    res = {"scan_bases": n, "scan_groups": len(flanks)}
    with _native.Engine() as eng:
        eng.set_params_locate(25, 1, 2, False, max_bases=n)
        eng.upload(0, bases)
        eng.locate_table(flanks)
        eng.locate(0)                                      # warm-up
        times = []
        for _ in range(3):
            t0 = time.time()
            hits = eng.locate(0)
            times.append(time.time() - t0)
        res["scan_s"] = min(times)
        res["scan_hits"] = len(hits)
        res["scan_bytes_per_base"] = (n + (n // (256 * 64) + 1) * (k - 1)) / n
        res["scan_fraction_of_8TBps"] = n * res["scan_bytes_per_base"] / res["scan_s"] / 8e12
        t0 = time.time()
        seps = eng.locate_seps(0)
        res["seps_s"] = time.time() - t0
        res["seps"] = len(seps)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--scan-bases", type=int, default=0)
    ap.add_argument("--no-files", action="store_true", help="skip the part from files")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {}
    if not args.no_files:
        with tempfile.TemporaryDirectory(prefix="krisp_locate_") as td:
            res.update(files_part(args, td))
    if args.scan_bases:
        res.update(scan_part(args.scan_bases))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
