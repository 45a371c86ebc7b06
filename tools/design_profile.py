"""Time the primer design pass (krisp_fasta --design-primers: KF.design_primers, kr_design_*).

  python tools/design_profile.py [--length 50000000] [--kernel] [--hairpins] [--files] [--reference 40] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup, the files of tools/products_profile.py)
at 30/40/30 with the command line's default primer options except --primer_size 18 24 and --amp_size 70 100 (the defaults,
25 .. 35 in flanks of 30 and products of 70 .. 150, leave a handful of candidates a region).
--kernel: the regions of the genomes (KF.find_regions), then kr_design_run over their templates: a warm-up and three timed
calls, the host clock around a call that ends in a synchronise, and the same over the templates repeated to a million
regions.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/design_profile.py --kernel` for k_design's own
time.
--hairpins: with --kernel, the same calls again with the hairpin check on (kr_design_hairpins: k_design<true>), after the
plain ones, so that a kernel trace holds k_design<false> and k_design<true> beside each other.
--files: the command line end to end without --design-primers and with it, each in five fresh processes (a process per
run, each under its own time limit; a failing run ends the tool): medians.
--reference N: the brute-force reference of the tests (tests/design_reference.py) over the first N regions on the CPU:
regions per second, the comparison.
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

from krisp_amd import _native, synth, thermo  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402

OPTS = dict(tm=(53, 68), gc=(40, 70), amp_size=(70, 100), primer_size=(18, 24), max_sec_tm=40, gc_clamp=1, max_end_gc=4)
FLAGS = ["--primer_size", "18", "24", "--amp_size", "70", "100"]


def write_genomes(length, td):
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
    return paths


def _timed(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.time()
        out = call()
        times.append(time.time() - t0)
    return min(times), out


def kernel_part(paths, nref, hairpins=False):
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    t0 = time.time()
    rows, L, D, R = KF.design_templates(groups, ingroup)
    res = {"regions": len(rows), "geometry": [L, D, R], "options": {k: list(v) if isinstance(v, tuple) else v for k, v in OPTS.items()},
           "templates_s": time.time() - t0}
    if len(rows) == 0:
        return res
    many = np.tile(rows, ((1_000_000 + len(rows) - 1) // len(rows), 1))[:1_000_000]
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**OPTS))
        res["design_s"], recs = _timed(lambda: eng.design(rows, L, D, R))
        res["with_a_pair"] = int(recs["found"].sum())
        res["design_million_s"], recs_m = _timed(lambda: eng.design(many, L, D, R))
        res["million_regions_per_s"] = len(many) / res["design_million_s"]
        assert recs_m[:len(rows)].tobytes() == recs.tobytes()
        if hairpins:
            eng.design_hairpins(thermo.hairpin_params())
            res["design_hairpins_s"], recs_h = _timed(lambda: eng.design(rows, L, D, R))
            res["with_a_pair_hairpins"] = int(recs_h["found"].sum())
            res["winners_changed_by_hairpins"] = int(np.any([recs_h[n] != recs[n] for n in recs.dtype.names], axis=0).sum())
            res["design_hairpins_million_s"], _ = _timed(lambda: eng.design(many, L, D, R))
            eng.design_hairpins(None)
    if nref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from design_reference import design as ref_design
        n = min(nref, len(rows))
        t0 = time.time()
        want = ref_design([bytes(r) for r in rows[:n]], L, D, R, **OPTS)
        res["reference_regions"] = n
        res["reference_regions_per_s"] = n / (time.time() - t0)
        res["reference_agrees"] = bool(want.tobytes() == recs[:n].tobytes())
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv")] + FLAGS
    res = {}
    for tag, extra in (("cli_without_design_s", []), ("cli_with_design_s", ["--design-primers"])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(os.path.join(td, "out.csv")) as f:
        res["design_csv_rows"] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="kr_design_run over the regions' templates")
    ap.add_argument("--hairpins", action="store_true", help="with --kernel: the timed calls again with the hairpin check on")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--reference", type=int, default=0, metavar="N", help="with --kernel: the CPU reference over N regions")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_design_") as td:
        paths = write_genomes(args.length, td)
        if args.kernel:
            res.update(kernel_part(paths, args.reference, args.hairpins))
        if args.files:
            res.update(files_part(paths, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
