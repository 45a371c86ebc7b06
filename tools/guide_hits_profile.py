"""Time the guide-hit scan (krisp_fasta --out_guide_hits: kr_guide_hits_scan) against the near-match scan it is built on.

  python tools/guide_hits_profile.py [--bases 50000000] [--guides 64] [--size 28] [--pam5 TTTV] [--pam3 ""] [--repeats 5]
                                     [--out FILE.json]

One genome of `--bases` random bases (uploaded from memory, a separator every 10 Mbp or so) and `--guides` windows of
`--size` bases cut from it: the same bytes are the guides of kr_guide_hits_table and the targets of kr_near_table in ONE
locate context (0 / size / 0), so both calls run the same scan kernels (k_near_scan) over tables of the same entries;
what the guide-hit call adds is the per-hit kernel (k_ghit_finish, csrc/ghit_step.inc) over the true hits.  For
M = 0 .. 3: a warm-up of each scan, then `--repeats` timed calls of each, alternating (the host clock around a call that ends in a synchronise; the fetch is
not timed).  The yardstick is the near scan: its own spread between repeated calls (max - min) stands beside the
difference of the two.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/guide_hits_profile.py ...` for the
kernels' own times (k_near_scan<M + 1, false / true> in both calls, k_ghit_finish).
Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from krisp_amd import _native  # noqa: E402


def profile(n, nguides, G, pam5, pam3, repeats):
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    bases[rng.integers(0, n, n // 10_000_000 + 1)] = ord("\n")
    starts = rng.integers(0, n - G, nguides)
    texts = np.unique(bases[starts[:, None] + np.arange(G)], axis=0)
    texts = np.ascontiguousarray(texts[~(texts == ord("\n")).any(axis=1)])
    res = {"bases": n, "guides": len(texts), "size": G, "pam5": pam5, "pam3": pam3, "repeats": repeats}
    with _native.Engine() as eng:
        eng.set_params_locate(0, G, 0, False, max_bases=n)
        eng.upload(0, bases)
        scans = {"near": lambda: eng._check(eng.lib.kr_near_scan(eng.ctx, 0), "kr_near_scan"),
                 "guide_hits": lambda: eng._check(eng.lib.kr_guide_hits_scan(eng.ctx, 0), "kr_guide_hits_scan")}
        for M in range(4):
            eng.near_table(texts, M)
            eng.guide_hits_table(texts, M, pam5, pam3, False)
            times = {name: [] for name in scans}
            hits = {}
            for name, scan in scans.items():
                scan()                                     # warm-up
            for _ in range(repeats):
                for name, scan in scans.items():
                    t0 = time.perf_counter()
                    hits[name] = scan()
                    times[name].append(time.perf_counter() - t0)
            for name in scans:
                res[f"{name}_scan_s_M{M}"] = statistics.median(times[name])
                res[f"{name}_scan_s_M{M}_all"] = [round(t, 5) for t in times[name]]
                res[f"{name}_hits_M{M}"] = int(hits[name])
            res[f"near_spread_s_M{M}"] = max(times["near"]) - min(times["near"])
            res[f"ratio_M{M}"] = res[f"guide_hits_scan_s_M{M}"] / res[f"near_scan_s_M{M}"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--guides", type=int, default=64)
    ap.add_argument("--size", type=int, default=28)
    ap.add_argument("--pam5", type=str, default="TTTV")
    ap.add_argument("--pam3", type=str, default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    line = json.dumps(profile(args.bases, args.guides, args.size, args.pam5, args.pam3, args.repeats))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
