"""Time the pieces of --primer-candidates: kr_design_run_top, kr_primers_tally, the search per file.

  python tools/primer_shortlist_profile.py [--length 50000000] [--kernel] [--files] [--out FILE.json]

Four synthetic genomes (krisp_amd/synth.py, 8 records each, 2 ingroup / 2 outgroup, the files of tools/design_profile.py) at
30/40/30 with --primer_size 18 24 --amp_size 70 100.
--kernel: in each of five fresh processes -- the regions of the genomes (KF.find_regions) and their templates, then
  kr_design_run (k_design, the kernel of --design-primers without the option) and kr_design_run_top at N = 1, 4, 8 over the
  same templates, a warm-up and three timed calls each, the host clock around a call that ends in a synchronise, the least of
  the three; per N shortlist_pairs and its distinct pairs, and per file kr_primers_scan over those pairs and the
  kr_primers_tally that follows it, timed the same way, then pick_pairs; whether rank 1 of every N is kr_design_run's record.
  The medians of the five processes are printed.
--files: the command line end to end with --design-primers alone and with --primer-candidates 4 and 8, each in five fresh
  processes (a process per run, each under its own time limit; a failing run ends the tool): medians.
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

from krisp_amd import _native, codec, reports, thermo  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from design_profile import _timed, write_genomes  # noqa: E402

TOPS = (1, 4, 8)
MISMATCHES, MAX_PRODUCT = 1, 1000
OPTS = dict(primer_size=(18, 24), amp_size=(70, 100))
FLAGS = ["--primer_size", "18", "24", "--amp_size", "70", "100"]


def kernel_once(paths):
    """one process's figures, as a dict of numbers"""
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    rows, L, D, R = templates = KF.design_templates(groups, ingroup)
    n = len(rows)
    res = {"regions": n}
    if n == 0:
        return res
    shortlists = {}
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**OPTS))
        res["design_run_s"], one = _timed(lambda: eng.design(rows, L, D, R))
        res["with_a_pair"] = int(one["found"].sum())
        same = True
        for top in TOPS:
            res[f"design_run_top{top}_s"], shortlists[top] = _timed(lambda: eng.design_top(rows, L, D, R, top))
            same = same and np.ascontiguousarray(shortlists[top][:, 0]).tobytes() == one.tobytes()
            res[f"filled_slots_top{top}"] = int(shortlists[top]["found"].sum())
        res["rank_1_is_design_run"] = int(same)
    Le, De, Re = codec.effective_geometry(30, 40, 30)
    for top in TOPS:
        t0 = time.time()
        left, right, pairs, index = reports.shortlist_pairs(templates[0], shortlists[top])
        res[f"shortlist_pairs_top{top}_s"] = time.time() - t0
        res[f"pairs_top{top}"], res[f"texts_top{top}"] = len(pairs), len(left) + len(right)
        total = np.zeros((len(pairs), 8), dtype=np.uint64)
        products = 0
        for eng, fi, _, _, _ in reports._scan_genomes(paths, Le, De, Re, 100, False, 0,
                                                      lambda eng: eng.primers_table(left + right, len(left), pairs, MISMATCHES,
                                                                                    MAX_PRODUCT)):
            res[f"scan_top{top}_file{fi}_s"], nh = _timed(lambda: eng.primers_scan(0))
            res[f"tally_top{top}_file{fi}_s"], tally = _timed(eng.primers_tally)
            products += nh
            total += tally
        res[f"products_top{top}"] = products
        assert int(total[:, :7].sum()) == products
        t0 = time.time()
        _, ranks, _ = reports.pick_pairs(shortlists[top], index, total, MISMATCHES)
        res[f"pick_top{top}_s"] = time.time() - t0
        res[f"picked_above_rank_1_top{top}"] = int((ranks > 0).sum())
    return res


def kernel_part(paths, runs=5, limit=900):
    """kernel_once in `runs` fresh processes: the median of every figure, and all values of the timed ones"""
    all_runs = []
    for i in range(runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--once"] + paths, cwd=ROOT, check=True, timeout=limit,
                           stdout=subprocess.PIPE)
        all_runs.append(json.loads(p.stdout.decode().strip().split("\n")[-1]))
        print(f"kernel process {i + 1} of {runs} done", file=sys.stderr, flush=True)
    res = {}
    for k in all_runs[0]:
        vals = [r[k] for r in all_runs]
        res[k] = statistics.median(vals)
        if k.endswith("_s"):
            res[k + "_all"] = [round(v, 6) for v in vals]
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv"), "--design-primers"] + FLAGS
    res = {}
    for tag, extra in (("cli_design_primers_s", []), ("cli_primer_candidates_4_s", ["--primer-candidates", "4"]),
                       ("cli_primer_candidates_8_s", ["--primer-candidates", "8"])):
        times = []
        for _ in range(runs):
            t0 = time.time()
            subprocess.run(argv + extra, cwd=ROOT, check=True, timeout=limit)      # (a failure or a time limit ends the tool)
            times.append(time.time() - t0)
        print(tag, "done", file=sys.stderr, flush=True)
        res[tag] = statistics.median(times)
        res[tag + "_all"] = [round(t, 3) for t in times]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--length", type=int, default=50_000_000)
    ap.add_argument("--kernel", action="store_true", help="the library's entry points over the regions' templates and the files")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--once", nargs=4, metavar="FASTA", help="one process of --kernel over these files, 2 ingroup then 2 outgroup")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.once:
        print(json.dumps(kernel_once(args.once)))
        return
    res = {"genomes": 4, "bases_per_genome": args.length, "mismatches": MISMATCHES, "max_product": MAX_PRODUCT,
           "options": {k: list(v) for k, v in OPTS.items()}}
    with tempfile.TemporaryDirectory(prefix="krisp_shortlist_") as td:
        paths = write_genomes(args.length, td)
        print("genomes written", file=sys.stderr, flush=True)
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
