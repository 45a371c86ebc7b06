"""The option sets and regions of test_gpu_guides.py, in a module of their own so that the reference can be run and timed
over exactly them without a GPU (PYTHONPATH=. python tests/guide_cases.py prints the counts and the seconds).

A region is (rows, lo, hi): texts of K letters, the template first.  Every set has seeded random regions; the set PLANTED
(30/40/30, g = 28, TTTV, at least 2 mismatches) also has the planted regions, each with the record the plant is meant to
produce (`expect`: the fields named there must equal the reference's -- test_guides_host.py checks that)."""
import random

from guides_reference import rc

# name -> geometry, guide size, motifs, GC, min mismatches, random regions
SETS = {
    "12_4_12_g12": dict(geo=(12, 4, 12), g=12, pam5="TTV", pam3="", gc=(25, 75), min_mismatches=1, n=300),
    "12_4_12_g28": dict(geo=(12, 4, 12), g=28, pam5="", pam3="", gc=(30, 70), min_mismatches=1, n=65),
    "30_40_30_g28_tttv": dict(geo=(30, 40, 30), g=28, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=2, n=200),
    "30_40_30_g28_h": dict(geo=(30, 40, 30), g=28, pam5="", pam3="H", gc=(40, 60), min_mismatches=1, n=65),
    "30_40_30_g20_tttv": dict(geo=(30, 40, 30), g=20, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=0, n=65),
    "30_40_30_g20_h": dict(geo=(30, 40, 30), g=20, pam5="", pam3="H", gc=(30, 70), min_mismatches=3, n=65),
    "30_40_30_g20_both": dict(geo=(30, 40, 30), g=20, pam5="TTTV", pam3="H", gc=(30, 70), min_mismatches=1, n=65),
    "256_60_256_g40": dict(geo=(256, 60, 256), g=40, pam5="NNNNTTTV", pam3="HNNNNNNN", gc=(30, 70), min_mismatches=1, n=65),
    "k2047": dict(geo=(1000, 47, 1000), g=28, pam5="TTTV", pam3="", gc=(30, 70), min_mismatches=1, n=1),
}
PLANTED = "30_40_30_g28_tttv"
ROW_COUNTS = (1, 3, 64, 65, 130)


def options(name):
    s = SETS[name]
    return dict(g=s["g"], pam5=s["pam5"], pam3=s["pam3"], gc=s["gc"], min_mismatches=s["min_mismatches"])


def _rand(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def _other(rng, ch):
    return rng.choice([x for x in "ACGT" if x != ch])


def _mutate(rng, row, cols):
    t = list(row)
    for c in cols:
        t[c] = _other(rng, t[c]) if t[c] in "ACGT" else "A"
    return "".join(t)


def random_regions(name, seed=7):
    """random templates (some with an IUPAC letter), 0 .. 5 outgroup rows -- and one region each with 64, 65 and 130 --
    that are the template with a few substitutions and now and then an N, bounds that are the whole template, a random
    stretch or empty"""
    s = SETS[name]
    L, D, R = s["geo"]
    K, g = L + D + R, s["g"]
    rng = random.Random(f"{name}/{seed}")
    out = []
    for i in range(s["n"]):
        T = _rand(rng, K)
        if rng.random() < 0.15:
            c = rng.randrange(K)
            T = T[:c] + rng.choice("RYNKMSWBDHV") + T[c + 1:]
        nout = rng.choice((0, 1, 1, 2, 3, 5))
        if s["n"] >= 65 and i in (10, 20, 30):
            nout = (64, 65, 130)[i // 10 - 1]
        whole = s["n"] == 1                  # (a set of one region: the whole template against three rows far from it)
        if whole:
            nout = 3
        rows = [T]
        for _ in range(nout):
            cols = [rng.randrange(K) for _ in range(K // 4 if whole else rng.choice((0, 1, 2, 4, 8, K // 4)))]
            o = _mutate(rng, T, cols)
            if rng.random() < 0.2:
                c = rng.randrange(K)
                o = o[:c] + rng.choice("NRY") + o[c + 1:]
            rows.append(o)
        u = rng.random()
        if u < 0.6 or whole:
            lo, hi = 0, K
        elif u < 0.9:
            lo = rng.randrange(0, K)
            hi = rng.randrange(lo, K + 1)
            if hi - lo < g and rng.random() < 0.7:
                lo = rng.randrange(0, K - g + 1)
                hi = rng.randrange(lo + g, K + 1)
        else:
            lo = hi = rng.randrange(0, K + 1)
        out.append((rows, lo, hi))
    return out


# ----------------------------------------------------------------------------
# the plants of PLANTED: K = 100, L = 30, D = 40 (the centre is 2 L + D = 100: a window at p = 36 is centred), g = 28,
# pam5 = TTTV (on '-' the template holds BAAA behind the window), no pam3, GC 30 .. 70, at least 2 mismatches
# ----------------------------------------------------------------------------
def _quiet(rng, K=100):
    """a template without a candidate: random orders of ACGT one after the other -- no run longer than 2, so no TTT and
    no AAA, and every window of 28 has 12 .. 16 G or C"""
    t = ""
    while len(t) < K:
        t += "".join(rng.sample("ACGT", 4))
    return t[:K]


def _put(t, at, text):
    assert 0 <= at and at + len(text) <= len(t)
    return t[:at] + text + t[at + len(text):]


def _plus(t, p):
    """a '+' candidate at p: GTTTC in front of the window (the G keeps the T from joining a run)"""
    return _put(t, p - 5, "GTTTC") if p >= 5 else _put(t, p - 4, "TTTC")


def _minus(t, p, g=28):
    """a '-' candidate at p: GAAAC behind the window (read on '-': TTTC in front of it)"""
    return _put(t, p + g, "GAAAC") if p + g + 5 <= len(t) else _put(t, p + g, "GAAA")


def planted_regions(seed=3):
    """-> [(label, (rows, lo, hi), expect)]"""
    rng = random.Random(seed)
    g, K = 28, 100
    out = []

    def add(label, rows, lo=0, hi=K, **expect):
        out.append((label, (rows, lo, hi), expect))

    none = dict(found=0, candidates=0)
    # a region without outgroup rows: d = g, s = 0
    T = _plus(_quiet(rng), 40)
    add("no outgroup rows", [T], found=1, strand=0, start=40, min_mismatches=g, sum_mismatches=0, candidates=1)
    # 1, 3, 64, 65, 130 outgroup rows with 2 .. 5 substitutions each inside the window
    for n in ROW_COUNTS:
        T = _plus(_quiet(rng), 40)
        counts = [rng.randrange(2, 6) for _ in range(n)]
        rows = [T] + [_mutate(rng, T, rng.sample(range(40, 68), m)) for m in counts]
        add(f"{n} outgroup rows", rows, found=1, strand=0, start=40, min_mismatches=min(counts), sum_mismatches=sum(counts),
            candidates=1)
    # an outgroup row with N / an IUPAC letter on a column that would otherwise discriminate: 3 differences, one unreadable
    for letter in "NR":
        T = _plus(_quiet(rng), 40)
        o = _mutate(rng, T, (45, 50, 55))
        add(f"outgroup {letter}", [T, _put(o, 50, letter)], found=1, start=40, min_mismatches=2, sum_mismatches=2, candidates=1)
        add(f"outgroup {letter}: the twin with a base", [T, o], found=1, start=40, min_mismatches=3, sum_mismatches=3, candidates=1)
    # the template has an IUPAC letter inside the protospacer; only inside the PAM stretch (V is in TTTV's last set as a
    # letter of the motif, not as a letter of the template)
    T = _plus(_quiet(rng), 40)
    add("template IUPAC in the protospacer", [_put(T, 55, "R")], **none)
    add("template IUPAC in the PAM only", [_put(T, 39, "V")], **none)
    add("template IUPAC beside the footprint", [_put(T, 35, "R")], found=1, start=40, candidates=1)
    # a PAM that would need column -1 (p = 3 on '+') or column K (p + g = K - 3 on '-'); and their neighbours that fit
    add("PAM at column -1", [_put(_quiet(rng), 0, "TTC")], **none)
    add("PAM at column K", [_put(_quiet(rng), K - 3, "GAA")], **none)
    add("PAM at column 0", [_put(_quiet(rng), 0, "TTTC")], found=1, strand=0, start=4, candidates=1)
    add("PAM at column K - 1", [_put(_quiet(rng), K - 4, "GAAA")], found=1, strand=1, start=K - 4 - g, candidates=1)
    # bounds that leave exactly one window (hi - lo = g + a + b = 32) and one less, on either side; lo = hi
    T = _plus(_quiet(rng), 40)
    add("bounds of one window", [T], 36, 68, found=1, strand=0, start=40, candidates=1)
    add("bounds one short on the right", [T], 36, 67, **none)
    add("bounds one short on the left", [T], 37, 68, **none)
    add("lo = hi", [T], 50, 50, **none)
    add("lo = hi = 0", [T], 0, 0, **none)
    add("lo = hi = K", [T], K, K, **none)
    # a guide only the '-' strand offers
    T = _minus(_quiet(rng), 40)
    add("minus strand only", [T], found=1, strand=1, start=40, min_mismatches=g, candidates=1)
    # ties, level by level.  Two windows A = [32, 60) and B = [40, 68), both 8 off the centre: columns 32 .. 39 are A's
    # alone, 60 .. 67 B's alone (B's PAM lies in 36 .. 39: the template's, the outgroup rows differ wherever they like)
    T = _plus(_plus(_quiet(rng), 32), 40)
    rows = [T, _mutate(rng, T, (33, 34, 35, 61, 62)), _mutate(rng, T, (33, 34, 35, 61, 62, 63, 64, 65, 66))]
    add("d decides", rows, found=1, start=32, min_mismatches=3, sum_mismatches=6, candidates=2)      # B: d = 2, s = 8
    rows = [T, _mutate(rng, T, (33, 34, 61, 62)), _mutate(rng, T, (33, 34, 61, 62, 63))]
    add("d ties, s decides", rows, found=1, start=40, min_mismatches=2, sum_mismatches=5, candidates=2)   # A: d = 2, s = 4
    # A = [30, 58) is 12 off the centre, B = [36, 64) is centred; the differences lie in both
    T = _plus(_plus(_quiet(rng), 30), 36)
    add("d and s tie, the centre decides", [T, _mutate(rng, T, (44, 45))], found=1, start=36, min_mismatches=2, sum_mismatches=2,
        candidates=2)
    # '-' at 32 and '+' at 40, both 8 off the centre
    T = _plus(_minus(_quiet(rng), 32), 40)
    add("d, s and the centre tie, the strand decides", [T, _mutate(rng, T, (44, 45))], found=1, strand=0, start=40, min_mismatches=2,
        sum_mismatches=2, candidates=2)
    T = _plus(_plus(_quiet(rng), 32), 40)
    add("all but p tie", [T, _mutate(rng, T, (44, 45))], found=1, strand=0, start=32, min_mismatches=2, sum_mismatches=2, candidates=2)
    # a window failing only GC (8 of 28 G or C: 28.6 percent; 9 pass), only the run of five (four pass); d one below
    # --guide-min-mismatches.  (What is put into the window begins and ends so that no TTT or AAA arises beside it.)
    T = _plus(_quiet(rng), 40)
    add("GC alone fails", [_put(T, 40, "ATCATGTA" + "ATCATGAT" + "ACATTGAT" + "TACG")], **none)
    add("GC just passes", [_put(T, 40, "ATCATGTA" + "ATCACGAT" + "ACATTGAT" + "TACG")], found=1, start=40, gc=9, candidates=1)
    add("a run of five alone fails", [_put(T, 50, "CATGGGGGTAC")], **none)
    add("a run of four passes", [_put(T, 50, "CATGGGGATAC")], found=1, start=40, candidates=1)
    add("d one below the least", [T, _mutate(rng, T, (44, 45)), _mutate(rng, T, (50,))], **none)
    add("d at the least", [T, _mutate(rng, T, (44, 45)), _mutate(rng, T, (50, 51))], found=1, start=40, min_mismatches=2,
        sum_mismatches=4, candidates=1)
    return out


def regions(name):
    """the regions of a set: the plants first where it has them"""
    return ([r for _, r, _ in planted_regions()] if name == PLANTED else []) + random_regions(name)


def pack(regs):
    """regions -> (rows text list, row offsets, bounds): what the library takes, as plain lists"""
    rows, off, bounds = [], [0], []
    for r, lo, hi in regs:
        rows += r
        off.append(len(rows))
        bounds.append((lo, hi))
    return rows, off, bounds


if __name__ == "__main__":
    import time
    from guides_reference import guides
    assert rc("TTTC") == "GAAA"
    t00 = time.time()
    for name, s in SETS.items():
        t0 = time.time()
        regs = regions(name)
        recs = guides(regs, s["geo"][0], s["geo"][1], **options(name))
        print(name, "regions", len(regs), "rows", sum(len(r[0]) for r in regs), "with a guide", sum(r["found"] for r in recs),
              "on '-'", sum(r["strand"] for r in recs), "candidates", sum(r["candidates"] for r in recs), f"{time.time() - t0:.1f} s",
              flush=True)
    print(f"total {time.time() - t00:.1f} s")
