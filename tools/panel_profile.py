"""Time the panel pass (krisp_fasta --panel: KF.select_panel, kr_panel_*).

  python tools/panel_profile.py [--length 50000000] [--kernel] [--files] [--out FILE.json]

The four synthetic genomes of tools/design_profile.py (2 ingroup / 2 outgroup) at 30/40/30 with the command line's default
primer options except --primer_size 18 24 and --amp_size 70 100.
--kernel: the regions (KF.find_regions), their templates and pairs (kr_design_run: a warm-up and three timed calls, the
least), the candidates in the panel's order, then kr_panel_run at N = 8 and N = 64 (the same: a warm-up, the least of three
calls, the host clock around a call that ends in a synchronise and the copies back), and how many candidates each cause
dropped.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/panel_profile.py --kernel` for k_panel_round's own
time.
--files: the command line end to end with --design-primers, without --panel and with --panel 8, each in five fresh
processes (a process per run, each under its own time limit; a failing run ends the tool): medians.
Progress goes to stderr; prints one JSON object."""
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

from krisp_amd import _native, thermo  # noqa: E402
from krisp_amd import krisp_fasta as KF  # noqa: E402
from design_profile import FLAGS, OPTS, _timed, write_genomes  # noqa: E402


def say(text):
    print(f"[panel_profile] {text}", file=sys.stderr, flush=True)


def kernel_part(paths):
    groups, _ = KF.find_regions(paths[:2], paths[2:], 30, 30, 100)
    ingroup = [KF.simplename(f) for f in paths[:2]]
    say(f"{len(groups)} regions")
    rows, L, D, R = KF.design_templates(groups, ingroup)
    res = {"regions": len(rows), "geometry": [L, D, R], "options": {k: list(v) if isinstance(v, tuple) else v for k, v in OPTS.items()}}
    if len(rows) == 0:
        return res
    with _native.Engine() as eng:
        eng.design_table(thermo.params(**OPTS))
        res["design_s"], recs = _timed(lambda: eng.design(rows, L, D, R))
        t0 = time.time()
        order = KF.panel_candidates(recs)
        res["order_s"] = time.time() - t0
        res["candidates"] = len(order)
        say(f"{len(order)} candidates")
        if len(order) == 0:
            return res
        t = np.ascontiguousarray(rows[order])
        pairs = np.stack([recs[f][order] for f in ("left_start", "left_len", "right_start", "right_len")], axis=1).astype(np.uint16)
        for n in (8, 64):
            res[f"panel_{n}_s"], (members, fates) = _timed(lambda: eng.panel(t, pairs, n))
            res[f"panel_{n}_members"] = len(members)
            res[f"panel_{n}_fates"] = np.bincount(fates["fate"], minlength=4).tolist()     # alive, members, same locus, clash
            res[f"panel_{n}_dropped_by_member"] = members["dropped"].tolist()
            say(f"N = {n}: {res[f'panel_{n}_s']:.4f} s, {len(members)} members")
    return res


def files_part(paths, td, runs=5, limit=600):
    argv = [sys.executable, "-m", "krisp_amd.krisp_fasta"] + paths[:2] + ["--outgroup"] + paths[2:] + \
        ["--conserved", "30", "--amplicon", "100", "--out_csv", os.path.join(td, "out.csv"), "--design-primers"] + FLAGS
    res = {}
    for tag, extra in (("cli_without_panel_s", []), ("cli_with_panel_s", ["--panel", "8", "--out_panel", os.path.join(td, "panel.tsv")])):
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
    ap.add_argument("--kernel", action="store_true", help="kr_panel_run over the designed pairs, beside kr_design_run")
    ap.add_argument("--files", action="store_true", help="the end-to-end part from .fasta.gz files")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    res = {"genomes": 4, "bases_per_genome": args.length}
    with tempfile.TemporaryDirectory(prefix="krisp_panel_") as td:
        say("writing the genomes")
        paths = write_genomes(args.length, td)
        say("genomes written")
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
