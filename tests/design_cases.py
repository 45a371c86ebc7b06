"""The templates and option sets of test_gpu_design.py, in a module of their own so that the brute-force reference can be
run and timed over exactly them without a GPU (PYTHONPATH=. python tests/design_cases.py prints the counts and the seconds)."""
import random

from design_reference import rc

# per geometry: the base option set, then one set per filter that moves ONE figure of the base so that the filter binds
GEOMETRIES = {
    (30, 40, 30): dict(n_random=12, base=dict(primer_size=(18, 24), tm=(48, 66), gc=(30, 70), amp_size=(80, 100), max_sec_tm=25,
                                              gc_clamp=0, max_end_gc=5),
                       sets=[dict(tm=(56, 60)), dict(gc=(50, 56)), dict(gc_clamp=2), dict(max_end_gc=1), dict(max_sec_tm=-60),
                             dict(amp_size=(96, 100))]),
    (12, 4, 12): dict(n_random=30, base=dict(primer_size=(10, 12), tm=(15, 50), gc=(20, 80), amp_size=(24, 28), max_sec_tm=10,
                                             gc_clamp=0, max_end_gc=5),
                      sets=[dict(tm=(30, 36)), dict(gc=(45, 55)), dict(gc_clamp=1), dict(max_end_gc=2), dict(max_sec_tm=-90)]),
    (40, 20, 25): dict(n_random=16, base=dict(primer_size=(16, 22), tm=(45, 64), gc=(30, 70), amp_size=(60, 85), max_sec_tm=20,
                                              gc_clamp=1, max_end_gc=4),
                       sets=[dict(gc_clamp=3), dict(max_sec_tm=-50)]),
    (256, 60, 256): dict(n_random=2, base=dict(primer_size=(30, 31), tm=(60, 76), gc=(35, 65), amp_size=(300, 304), max_sec_tm=30,
                                               gc_clamp=1, max_end_gc=3),
                         sets=[]),
}


def _rand(rng, n, weights=(1, 1, 1, 1)):
    return "".join(rng.choices("ACGT", weights=weights, k=n))


def templates(L, D, R, n_random, seed=1):
    """random templates, then templates with planted structure: a self-complementary 3' end, left and right primers
    complementary to each other, poly-X runs, GC-rich and AT-rich flanks, an IUPAC letter, nothing but A"""
    rng = random.Random(1000 * L + R + seed)
    W = L + D + R
    out = [_rand(rng, W) for _ in range(n_random)]
    for _ in range(3):
        # the left flank ends in a palindrome: every left primer that ends there folds onto itself at its 3' end
        pal = _rand(rng, 4)
        t = list(_rand(rng, W))
        t[L - 8:L] = pal + rc(pal)
        out.append("".join(t))
        # the right flank is the left flank again: the right primer is the reverse complement of the left one
        t = _rand(rng, L + D)
        m = min(L, R)
        out.append(t + t[L - m:L] + _rand(rng, R - m))
        # the 3' ends of a left and a right primer pair with each other: a copy of the left flank's end, reversed and
        # complemented by the right primer's own reverse complement, sits at the start of the right flank
        t = _rand(rng, W)
        out.append(t[:L + D] + t[L - 8:L] + t[L + D + 8:])
        # poly-X runs in both flanks
        t = list(_rand(rng, W))
        p = rng.randrange(0, L - 6)
        t[p:p + 6] = rng.choice("ACGT") * 6
        p = rng.randrange(L + D, W - 6)
        t[p:p + 5] = rng.choice("ACGT") * 5
        out.append("".join(t))
        out.append(_rand(rng, L, (1, 4, 4, 1)) + _rand(rng, D) + _rand(rng, R, (1, 3, 3, 1)))      # GC-rich
        out.append(_rand(rng, L, (4, 1, 1, 4)) + _rand(rng, D) + _rand(rng, R, (3, 1, 1, 3)))      # AT-rich
        t = list(_rand(rng, W))
        t[rng.randrange(0, L)] = rng.choice("RYNKM")
        t[rng.randrange(L + D, W)] = "N"
        out.append("".join(t))
    out.append("A" * W)
    return out


def option_sets(geo):
    g = GEOMETRIES[geo]
    return [dict(g["base"])] + [dict(g["base"], **s) for s in g["sets"]]


if __name__ == "__main__":
    import time
    from design_reference import design
    t00 = time.time()
    for geo, g in GEOMETRIES.items():
        ts = templates(*geo, g["n_random"])
        base = None
        for opts in option_sets(geo):
            t0 = time.time()
            recs = design(ts, *geo, **opts)
            base = recs if base is None else base
            print(geo, opts, "found", int(recs["found"].sum()), "of", len(ts), "differ from base", int((recs != base).sum()),
                  f"{time.time() - t0:.1f} s", flush=True)
    print(f"total {time.time() - t00:.1f} s")
