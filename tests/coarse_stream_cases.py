"""Seeded genomes for the coarse route's ONE launch over all coarse genomes of a call and its pipelined key loop (DESIGN
§10b): the builders of tests/coarse_cases.py, put together so that several genomes share a table, buckets sit at the edges
of the loop's iteration, a unit's hits sit at the edges of the queue, and different coarse genomes of one call show
different outcomes for one candidate.  tests/test_coarse_stream_cases.py counts the shapes with the oracle alone,
tests/test_gpu_coarse_stream.py runs them on the device.

Exact bucket sizes come from records of ONE window: a record of 28 bases whose last base is G gives one key whose top byte is
the window's first four bases and, from the other strand, one key whose top byte begins with C.  A genome made of such
records only ("mini genome") has keys in the top bytes it names and in 0x40 .. 0x7F, and nowhere else."""
import functools
import zlib

import numpy as np

import coarse_cases as CC

ITER = 8192                 # keys of one iteration of the probe's key loop (2 CO_T CO_UNROLL: one register set)
QCAP = 2048                 # queued keys of one UNIT; a unit with more is read again and looked up in place
A, C, G, T = 0, 1, 2, 3
_ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rng(name):
    return np.random.default_rng(zlib.crc32(("coarse stream " + name).encode()))


def _text(records):
    """records (code arrays) -> ASCII text, '\\n' between them"""
    out = np.full(sum(len(r) for r in records) + len(records) - 1, 10, dtype=np.uint8)
    p = 0
    for r in records:
        out[p:p + len(r)] = _ASCII[r]
        p += len(r) + 1
    return out


def head_byte(head):
    return int(sum(CC._BASES.index(c) << (6 - 2 * i) for i, c in enumerate(head)))


def mini_prefix(rng, head):
    """a random 54-bit prefix whose first four bases are `head` and whose last base (the window's last) is G"""
    codes = rng.integers(0, 4, size=CC.L + CC.R, dtype=np.uint8)
    codes[:4] = CC._codes(head)
    codes[-1] = G
    p = 0
    for j, c in enumerate(codes):
        p |= int(c) << (62 - 2 * j)
    return p


def _mini(prefix, base):
    """the record of one window"""
    return CC.window(prefix | (base << CC.DIAG_SHIFT))


def _family(rng, n, length, flags, every, mu=0.001, skewed=False):
    """codes of n genomes over one ancestor, an ingroup / outgroup site every `every` bases"""
    anc = (rng.choice(4, size=length, p=[0.7, 0.1, 0.1, 0.1]) if skewed else rng.integers(0, 4, size=length)).astype(np.uint8)
    sites = np.arange(every // 2, length, every)
    b1 = rng.integers(0, 4, size=len(sites), dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=len(sites), dtype=np.uint8)) & 3
    codes = []
    for g in range(n):
        c = anc.copy()
        CC._mutate(rng, c, mu)
        c[sites] = b1 if flags[g] else b2
        codes.append(c)
    return codes


def _records(codes, records=CC.RECORDS):
    rl = (len(codes) + records - 1) // records
    return [codes[i:i + rl] for i in range(0, len(codes), rl)]


def _plants(rng, heads_counts):
    """-> [(prefix, b_in, b_out)]: windows every genome of a case holds, the ingroup with b_in, the outgroup with b_out"""
    out = []
    for head, n in heads_counts:
        for _ in range(n):
            b1 = int(rng.integers(0, 4))
            out.append((mini_prefix(rng, head), b1, CC._other(rng, b1)))
    return out


# ----------------------------------------------------------------------------
# a. several genomes per table
# ----------------------------------------------------------------------------
MULTI = (3, 5)
MULTI_PLANTS = 48
_MULTI_FLAGS = {3: [True, True, False, False, True], 5: [True, True, False, False, True, False, True]}
_MULTI_LEN = [450_000, 250_000, 600_000, 350_000]        # the family's coarse genomes, in the order of their ids


@functools.lru_cache(maxsize=None)
def multi(ncoarse):
    """-> texts, flags, plants.  Pillars of 600 kbp over a 70 % A ancestor (top bytes 0 and 255 hold several chunks); ncoarse - 1
    coarse genomes cut to different lengths -- different chunk counts per genome in one top byte --; the last coarse genome is
    a mini genome of the plants alone: shorter than one iteration, and without a key in nearly every top byte that has
    candidates.  The plants are held by every genome, so the final list is not empty."""
    flags = _MULTI_FLAGS[ncoarse]
    n = len(flags)
    rng = _rng(f"multi {ncoarse}")
    codes = _family(rng, n - 1, 600_000, flags, 1500, mu=0.002, skewed=True)
    plants = _plants(rng, [(h, MULTI_PLANTS // 4) for h in ("AAAA", "AGTA", "GGAT", "TTTT")])
    texts, k = [], 0
    for g in range(n):
        mine = [_mini(p, b1 if flags[g] else b2) for p, b1, b2 in plants]
        if g == n - 1:
            texts.append(_text(mine))
            continue
        c = codes[g]
        if g not in CC.pillars(flags):
            c = c[:_MULTI_LEN[k]]
            k += 1
        texts.append(_text(_records(c) + mine))
    return texts, flags, plants


# ----------------------------------------------------------------------------
# b. prefetch edges: one mini genome with exact buckets
# ----------------------------------------------------------------------------
EDGES = [("AAAC", 1), ("AAGA", ITER - 1), ("GAAA", ITER + 1), ("GTAA", 2 * ITER + 1), ("TTTT", ITER)]
EDGES_PLANTS = 1            # candidates per named top byte (a top byte without candidates has no unit)


@functools.lru_cache(maxsize=None)
def edges():
    """-> texts, flags, plants.  2 in / 2 out; genome 1 (ingroup, coarse) is a mini genome whose named top bytes hold exactly
    1, ITER - 1, ITER + 1, 2 ITER + 1 and -- in top byte 255, the LAST bucket of its key array -- ITER keys; its other keys
    (the other strand's) lie in 0x40 .. 0x7F.  The pillars and genome 3 (outgroup, coarse) are a family of 120 kbp that holds
    the plants too: in every named top byte genome 1's unit is followed by a unit of genome 3.  The text of genome 1 has
    one record per key (1.2 MB): nothing shorter gives exact bucket sizes."""
    flags = [True, True, False, False]
    rng = _rng("edges")
    codes = _family(rng, 4, 120_000, flags, 2000)
    plants = _plants(rng, [(h, EDGES_PLANTS) for h, _ in EDGES])
    texts = []
    for g in range(4):
        mine = [_mini(p, b1 if flags[g] else b2) for p, b1, b2 in plants]
        if g != 1:
            texts.append(_text(_records(codes[g]) + mine))
            continue
        fill = [_mini(mini_prefix(rng, h), int(rng.integers(0, 4))) for h, n in EDGES for _ in range(n - EDGES_PLANTS)]
        texts.append(_text(mine + fill))
    return texts, flags, plants


# ----------------------------------------------------------------------------
# c. the queue
# ----------------------------------------------------------------------------
QUEUE = (QCAP - 1, QCAP, QCAP + 1)
QUEUE_HEAD = "GATA"


@functools.lru_cache(maxsize=None)
def queue(hits):
    """-> texts, flags, plants.  2 in / 2 out of 300 kbp; `hits` plants in ONE top byte, held by every genome; genome 1 (coarse)
    is a mini genome of the plants alone: its unit of that top byte holds `hits` keys, every one a true hit, and nothing
    else passes the prefilter there"""
    flags = [True, True, False, False]
    rng = _rng(f"queue {hits}")
    codes = _family(rng, 4, 300_000, flags, 2000)
    plants = _plants(rng, [(QUEUE_HEAD, hits)])
    texts = []
    for g in range(4):
        mine = [_mini(p, b1 if flags[g] else b2) for p, b1, b2 in plants]
        texts.append(_text(mine if g == 1 else _records(codes[g]) + mine))
    return texts, flags, plants


# ----------------------------------------------------------------------------
# d. sides across genomes
# ----------------------------------------------------------------------------
SPREAD_FLAGS = [True, True, True, False, False, False]


@functools.lru_cache(maxsize=None)
def spread():
    """-> texts, flags, plants: the kinds of coarse_cases.sides() over two ingroup and two outgroup coarse genomes.  Every
    pillar holds the planted window, the ingroup pillar with b1 and the outgroup pillar with b2; the coarse genomes hold it
    with their side's base, but for ONE of them -- plant i deviates in coarse genome (i & 1) of the side the kind names:
    "in_shows_out" b2, "in_shows_third" a third base, "out_shows_in" b1, "twice" the window a second time with a third base
    (odd plants) or b2 (even plants), "lacks" a substitution inside the left flank.  The same candidate so meets different
    outcomes in the coarse genomes of one call; plants[kind] = [(prefix, deviating genome)]"""
    rng = _rng("spread")
    flags = SPREAD_FLAGS
    codes, _ = CC._family_codes(57, 3, 3, 300_000, 0.001)
    pin, pout = CC.pillars(flags)
    cin = [g for g in CC.coarse(flags) if flags[g]]
    cout = [g for g in CC.coarse(flags) if not flags[g]]
    assert len(cin) == 2 and len(cout) == 2
    slot = CC._slots()
    plants = {k: [] for k in CC.SIDES_KINDS}
    for kind in CC.SIDES_KINDS:
        for i in range(CC.SIDES_EACH):
            p = int(rng.integers(0, 1 << 54, dtype=np.uint64)) << 10
            b1 = int(rng.integers(0, 4))
            b2 = CC._other(rng, b1)
            b3 = CC._other(rng, b1, b2)
            at, at2 = next(slot), next(slot)
            dev = (cout if kind == "out_shows_in" else cin)[i & 1]
            plants[kind].append((p, dev))
            show = {g: (b1 if flags[g] else b2) for g in range(len(flags))}
            if kind == "in_shows_out":
                show[dev] = b2
            elif kind == "in_shows_third":
                show[dev] = b3
            elif kind == "out_shows_in":
                show[dev] = b1
            for g, b in show.items():
                CC._put(codes[g], at, CC.window(p | b << CC.DIAG_SHIFT))
            if kind == "twice":
                CC._put(codes[dev], at2, CC.window(p | (b3 if i & 1 else b2) << CC.DIAG_SHIFT))
            elif kind == "lacks":
                codes[dev][at + 11] = (codes[dev][at + 11] + 1) & 3
    return CC._texts(codes), flags, plants


def spread_kept(K):
    """per kind, per plant of spread(): does the oracle's final list keep the planted prefix?  Recorded, not prescribed"""
    texts, flags, plants = spread()
    c = CC.census(K, "spread", texts, flags)
    return {kind: [bool(x) for x in CC.held(c["cands"]["prefix"], [p for p, _ in ps])] for kind, ps in plants.items()}


def prefixes(plants):
    return np.array([p for p, _, _ in plants], dtype=np.uint64)
