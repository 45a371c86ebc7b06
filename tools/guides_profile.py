"""Time the guide pass (krisp_fasta --out_guides: KF.design_guides, kr_guides_*).

  python tools/guides_profile.py [--length 50000000] [--kernel] [--files] [--reference 200] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup, the files of tools/design_profile.py)
at 30/40/30 with --guide-size 28 --pam5 TTTV --guide-min-mismatches 0 (the synthetic ingroups differ from each other in
their diagnostic column, so with the default of 1 mismatch most regions have no candidate to weigh).
--kernel: the regions of the genomes (KF.find_regions), the host's rows (KF.guide_rows, timed), then kr_guides_run over
them: a warm-up and three timed calls, the host clock around a call that ends in a synchronise.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/guides_profile.py --kernel` for k_guides' own time.
--files: the command line end to end without --out_guides and with it, each in five fresh processes (a process per run,
each under its own time limit; a failing run ends the tool): medians.
--reference N: the reference of the tests (tests/guides_reference.py) over the first N regions on the CPU: regions per
second, the comparison.
Prints one JSON object."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from krisp_amd import _native  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from design_profile import write_genomes  # noqa: E402

OPTS = dict(guide_size=28, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=0)
FLAGS = ["--guide-size", "28", "--pam5", "TTTV", "--guide-min-mismatches", "0"]


def _timed(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.time()
        out = call()
        times.append(time.time() - t0)
    return min(times), out


def kernel_part(paths, nref):
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    t0 = time.time()
    templates = KF.design_templates(groups, ingroup)
    t1 = time.time()
    rows, off, L, D, R = KF.guide_rows(groups, ingroup, templates)
    res = {"regions": len(off) - 1, "rows": len(rows), "geometry": [L, D, R],
           "options": {k: list(v) if isinstance(v, tuple) else v for k, v in OPTS.items()}, "templates_s": t1 - t0,
           "guide_rows_s": time.time() - t1}
    n = len(off) - 1
    if n == 0:
        return res
    bounds = np.tile(np.array([0, L + D + R], dtype=np.uint32), (n, 1))
    with _native.Engine() as eng:
        eng.guides_table(OPTS["guide_size"], KF.motif_masks(OPTS["pam5"]), KF.motif_masks(OPTS["pam3"]), OPTS["gc"],
                         OPTS["min_mismatches"])
        res["guides_s"], recs = _timed(lambda: eng.guides(rows, off, bounds, L, D))
    res["with_a_guide"] = int(recs["found"].sum())
    res["regions_per_s"] = n / res["guides_s"]
    if nref:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from guides_reference import FIELDS, guides
        m = min(nref, n)
        text = [bytes(r).decode("ascii") for r in rows[:int(off[m])]]
        regs = [(text[int(off[i]):int(off[i + 1])], 0, L + D + R) for i in range(m)]
        t0 = time.time()
        want = guides(regs, L, D, OPTS["guide_size"], OPTS["pam5"], OPTS["pam3"], OPTS["gc"], OPTS["min_mismatches"])
        res["reference_regions"] = m
        res["reference_regions_per_s"] = m / (time.time() - t0)
        res["reference_agrees"] = all(int(recs[f][i]) == want[i][f] for i in range(m) for f in FIELDS)
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv")]
    res = {}
    for tag, extra in (("cli_without_guides_s", []), ("cli_with_guides_s", FLAGS + ["--out_guides", os.path.join(td, "guides.tsv")])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    with open(os.path.join(td, "guides.tsv")) as f:
        res["guide_rows_written"] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="kr_guides_run over the regions' rows")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--reference", type=int, default=0, metavar="N", help="with --kernel: the CPU reference over N regions")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_guides_") as td:
        paths = write_genomes(args.length, td)
        if args.kernel:
            res.update(kernel_part(paths, args.reference))
        if args.files:
            res.update(files_part(paths, td))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
