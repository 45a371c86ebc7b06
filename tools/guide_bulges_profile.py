"""Time the bulged guide-hit scan (krisp_fasta --guide-hit-bulges: kr_guide_bulges_scan) beside the scan it extends.

  python tools/guide_bulges_profile.py [--length 50000000] [--kernel] [--files] [--bulges 2] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup, the files of tools/design_profile.py)
at 30/40/30 with --guide-size 28 --pam5 TTTV --guide-min-mismatches 0 --guide-hit-mismatches 2, as tools/guides_profile.py.
--kernel: the regions of the genomes, their guides (KF.design_guides) and the guides' distinct texts; then every genome is
uploaded alone in one locate context that holds both tables, and kr_guide_hits_scan and kr_guide_bulges_scan are each
called once to warm up and three times under the host clock (a call ends in a synchronise; the fetch is not timed): the
least time per genome, summed over the four, and the rows of either.  Run it under `rocprofv3 --kernel-trace --stats --
python tools/guide_bulges_profile.py --kernel` for the kernels' own times (k_near_scan in both, k_ghit_finish,
k_gbulge_extend).
--files: the command line end to end with --out_guides --out_guide_hits, without --guide-hit-bulges and with it, each in
five fresh processes (a process per run, each under its own time limit; a failing run ends the tool): medians.
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

OPTS = dict(guide_size=28, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=0)
FLAGS = ["--guide-size", "28", "--pam5", "TTTV", "--guide-min-mismatches", "0", "--guide-hit-mismatches", "2"]
M = 2


def _least(call):
    call()                                                 # warm-up
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def kernel_part(paths, bulges):
    import numpy as np
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    templates = KF.design_templates(groups, ingroup)
    guides = KF.design_guides(groups, ingroup, templates=templates, **OPTS)
    texts, _ = KF.guide_texts(templates[0], guides, OPTS["guide_size"])
    G = OPTS["guide_size"]
    res = {"regions": len(groups), "texts": len(texts), "size": G, "mismatches": M, "bulges": bulges, "half": (G - bulges) // 2,
           "guide_hits_scan_s": 0.0, "guide_bulges_scan_s": 0.0, "guide_hits": 0, "guide_bulge_hits": 0}
    if not texts:
        return res
    t = np.frombuffer(b"".join(texts), dtype=np.uint8).reshape(-1, G)

    def tables(eng):
        eng.guide_hits_table(t, M, OPTS["pam5"], OPTS["pam3"], False)
        eng.guide_bulges_table(t, M, bulges, OPTS["pam5"], OPTS["pam3"], False)

    for eng, fi, path, rna, names in _scan_genomes(paths, 0, G, 0, G, False, 0, tables):
        s, n = _least(lambda: eng._check(eng.lib.kr_guide_hits_scan(eng.ctx, 0), "kr_guide_hits_scan"))
        res["guide_hits_scan_s"] += s
        res["guide_hits"] += int(n)
        s, n = _least(lambda: eng._check(eng.lib.kr_guide_bulges_scan(eng.ctx, 0), "kr_guide_bulges_scan"))
        res["guide_bulges_scan_s"] += s
        res["guide_bulge_hits"] += int(n)
        print(f"genome {fi}: {res['guide_hits_scan_s']:.4f} s / {res['guide_bulges_scan_s']:.4f} s so far", file=sys.stderr, flush=True)
    return res


def files_part(paths, td, bulges, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv")] + FLAGS + \
        ["--out_guides", os.path.join(td, "guides.tsv"), "--out_guide_hits", os.path.join(td, "hits.tsv")]
    res = {}
    for tag, extra in (("cli_without_bulges_s", []), ("cli_with_bulges_s", ["--guide-hit-bulges", str(bulges)])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
            print(f"{tag}: {times[-1]:.3f}", file=sys.stderr, flush=True)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(x, 3) for x in times]
        with open(os.path.join(td, "hits.tsv")) as f:
            res[tag.replace("_s", "_rows")] = sum(1 for _ in f) - 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="the two scans over every genome")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--bulges", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_guide_bulges_") as td:
        paths = write_genomes(args.length, td)
        if args.kernel:
            res.update(kernel_part(paths, args.bulges))
        if args.files:
            res.update(files_part(paths, td, args.bulges))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
