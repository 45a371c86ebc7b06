"""The option sets and regions of test_gpu_guide_shortlist.py: the sets of guide_cases.py and one more, LANES, planted so that
a region's best candidates share a lane of k_guides_top (PYTHONPATH=. python tests/guide_shortlist_cases.py prints, per set,
the regions with more than 8 candidates and those whose first 8 put two into one lane; test_guide_shortlist_host.py asserts
the plants' counts).

The kernel's lane of the candidate (window start p, strand) of a region with the bounds [lo, hi) is (2 (p - lo) + strand) mod
64: in the random sets two of a region's first 8 seldom meet in one.  LANES: K = 300 (130 / 40 / 130), g = 20, pam5 = TTTV,
GC 0 .. 100, at least 1 mismatch.  A template's background holds no T and no run above two letters -- no TTT, no AAA: no
candidate on either strand -- and TTTC in front of a window makes it a '+' candidate, the only kind there is.  Plants 32
columns apart share their lane."""
import random

import guide_cases

LANES = "lanes_300_g20_tttv"
SETS = dict(guide_cases.SETS)
SETS[LANES] = dict(geo=(130, 40, 130), g=20, pam5="TTTV", pam3="", gc=(0, 100), min_mismatches=1, n=0)
TOPS = (1, 2, 8)
K, G = 300, 20


def options(name):
    s = SETS[name]
    return dict(g=s["g"], pam5=s["pam5"], pam3=s["pam3"], gc=s["gc"], min_mismatches=s["min_mismatches"])


def _background(rng, n=K):
    t = ""
    while len(t) < n:
        ch = rng.choice("ACG")
        if t[-2:] != ch * 2:
            t += ch
    return t


def _template(rng, starts):
    t = _background(rng)
    for p in starts:
        t = guide_cases._put(t, p - 4, "TTTC")
    return t


def _outgroup(rng, T, starts, counts):
    """a row that differs from T in counts[i] columns of the window at starts[i] (windows 32 apart do not overlap)"""
    cols = [c for p, n in zip(starts, counts) for c in rng.sample(range(p, p + G), n)]
    return guide_cases._mutate(rng, T, cols)


def lane_regions(seed=11):
    """-> [(label, (rows, lo, hi), the region's number of candidates)]"""
    rng = random.Random(seed)
    out = []

    def add(label, starts, counts=(), lo=0, hi=K, n=None):
        T = _template(rng, starts)
        rows = [T] + [_outgroup(rng, T, starts, c) for c in counts]
        out.append((label, (rows, lo, hi), len(starts) if n is None else n))

    nine = [4 + 32 * i for i in range(9)]
    # ranks 1 to 3 are the windows 2, 5 and 7: d = 6; d = 4, s = 9; d = 4, s = 8.  The others: d = 1, s = 2 or 3, then the centre
    add("nine in one lane", nine, [[1, 1, 6, 1, 1, 5, 1, 4, 1], [1, 2, 6, 1, 1, 4, 2, 4, 1]])
    add("nine in one lane, no outgroup row", nine)
    add("nine in one lane, all equal but p and the centre", nine, [[2] * 9, [3] * 9])
    for n in (8, 7, 2, 1, 0):
        add(f"exactly {n}", nine[:n], [[2 + (i * 5) % 3 for i in range(n)]])
    # bounds that cut the first plant's PAM (lo = 1: the motif begins at column 0) and the last one's window (hi = 279: it ends
    # at 280); lo counts in the lane, which stays one for all
    add("bounds cut the footprint", nine, [[1, 3, 1, 2, 1, 3, 1, 2, 1]], lo=1, hi=279, n=7)
    add("bounds that keep all nine", nine, [[1, 3, 1, 2, 1, 3, 1, 2, 1]], lo=0, hi=280)
    # 17 plants 16 columns apart: two lanes, eight or nine candidates each (a window may hold the next plant's T: GC is free)
    sixteen = [4 + 16 * i for i in range(17)]
    T = _template(rng, sixteen)
    rows = [T] + [guide_cases._mutate(rng, T, rng.sample(range(K), 60)) for _ in range(3)]
    out.append(("seventeen in two lanes", (rows, 0, K), 17))
    return out


def regions(name):
    return [r for _, r, _ in lane_regions()] if name == LANES else guide_cases.regions(name)


if __name__ == "__main__":
    import guide_shortlist_reference as ref
    for name, s in SETS.items():
        o = options(name)
        many = shared = 0
        regs = regions(name)
        for rows, lo, hi in regs:
            n, ln = ref.lanes(rows, lo, hi, s["geo"][0], s["geo"][1], o["g"], 8, o["pam5"], o["pam3"], o["gc"][0], o["gc"][1],
                              o["min_mismatches"])
            many += n > 8
            shared += len(set(ln)) < len(ln)
        print(name, "regions", len(regs), "with more than 8 candidates", many, "with two of the first 8 in one lane", shared, flush=True)
