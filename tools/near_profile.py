"""Time the near-match pass (krisp_fasta --out_near: KF.near_matches, kr_near_*) and, beside it, the locate pass's scan.

  python tools/near_profile.py [--scan-bases 3000000000] [--groups 64] [--files] [--length 50000000] [--out FILE.json]

--scan-bases N: one genome of N random bases (no file: uploaded from memory, tools/locate_profile.py's genome: the same seed)
with `--groups` windows cut from it as targets at 25/1/2; kr_locate_scan against their flanks, then kr_near_scan for
M = 0, 1, 2, 3 (a warm-up and three timed calls each: the host clock around calls that end in a synchronise).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/near_profile.py ...` for the kernels' own times
(k_near_scan<M + 1, false> = the counting pass, <M + 1, true> = the emitting pass over the tiles with hits; k_loc_scan).
--files: four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup) as .fasta.gz, 25/1/2: the
command line end to end without --out_near and with it at M = 1, each in five fresh processes (a process per run, each
under its own time limit; a failing run ends the tool): medians.
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


def scan_part(n, groups):
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    bases[rng.integers(0, n, n // 10_000_000 + 1)] = ord("\n")
    k = 28
    starts = rng.integers(0, n - k, groups)
    targets = np.unique(bases[starts[:, None] + np.arange(k)], axis=0)
    targets = targets[~(targets == ord("\n")).any(axis=1)]
    flanks = np.unique(np.concatenate([targets[:, :25], targets[:, 26:]], axis=1), axis=0)
    res = {"scan_bases": n, "scan_targets": len(targets), "scan_groups": len(flanks)}
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
        res["locate_scan_s"] = min(times)
        res["locate_hits"] = len(hits)
        for M in range(4):
            eng.near_table(targets, M)
            eng.near(0)                                    # warm-up
            times = []
            for _ in range(3):
                t0 = time.time()
                hits = eng.near(0)
                times.append(time.time() - t0)
            res[f"near_scan_s_M{M}"] = min(times)
            res[f"near_hits_M{M}"] = len(hits)
            res[f"near_hits_flank_M{M}"] = int(np.count_nonzero(hits["flank_mismatches"]))
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
        ["--conserved-left", "25", "--conserved-right", "2", "--diagnostic", "1", "--out_csv", os.path.join(td, "out.csv")]
    res = {"genomes": len(paths), "bases_per_genome": length}
    near = os.path.join(td, "near.tsv")
    for tag, extra in (("cli_without_near_s", []), ("cli_with_near_M1_s", ["--out_near", near, "--near-mismatches", "1"])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(near) as f:
        res["near_rows"] = sum(1 for _ in f) - 1
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
        with tempfile.TemporaryDirectory(prefix="krisp_near_") as td:
            res.update(files_part(args.length, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
