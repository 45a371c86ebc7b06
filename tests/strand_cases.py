"""Seeded genomes for the one-strand form of the coarse route (a coarse genome's pass 1 writes the forward record
of every window, k_coarse_probe asks each key both ways -- krisp_amd/csrc/co_strand.inc): no code of krisp_amd/ but synth.
Every case returns (texts, flags) or (texts, flags, plants); the genomes are [ingroup pillar, coarse ingroup, outgroup pillar,
coarse outgroup] (coarse_cases.pillars / coarse).

tests/test_strand_cases.py shows, with oracle/kmer_oracle alone, that each case forces the branch it is named for;
tests/test_gpu_coarse_strand.py runs them on the device.  The readings, digits and classes are restated here base by base."""
import functools

import numpy as np

import coarse_cases as CC

A, C, G, T = 0, 1, 2, 3


# ----------------------------------------------------------------------------
# windows, keys, digits -- base by base, for any (L, 1, R)
# ----------------------------------------------------------------------------
def rc(win):
    return (3 - np.asarray(win, dtype=np.uint8))[::-1].copy()


def key_of(win, L, R):
    """the key of a window in text order: left, right, then the diagnostic base"""
    b = list(win[:L]) + list(win[L + 1:]) + [win[L]]
    k = 0
    for j, c in enumerate(b):
        k |= int(c) << (62 - 2 * j)
    return k


def pmask(L, R):
    return ((1 << (2 * (L + R))) - 1) << (64 - 2 * (L + R))


def prefix_of(win, L, R):
    return key_of(win, L, R) & pmask(L, R)


def digit_positions(R):
    return [i for i in range(5) if i != R][:4]


def digit_of(win, R):
    """the bucket of a window's forward key: its bases at the first four positions other than R"""
    d = 0
    for i in digit_positions(R):
        d = (d << 2) | int(win[i])
    return d


def prefix_window(prefix, L, R):
    """a prefix (key & pmask) -> the L + R bases of its sequence, in text order (the diagnostic column left out)"""
    return np.array([(int(prefix) >> (62 - 2 * j)) & 3 for j in range(L + R)], dtype=np.uint8)


def class_fwd(prefix, L, R):
    """the digit of the windows that meet `prefix` with their forward record"""
    p = prefix_window(prefix, L, R)
    w = np.concatenate([p[:L], [0], p[L:]])              # (position L is not a digit position: any base)
    return digit_of(w, R)


def class_rev(prefix, L, R):
    """the digit of the windows that meet `prefix` with their REVERSE record: such a window w has rc(w) = left, x, right, so
    w = rc(right), comp(x), rc(left) -- its first four positions other than R are the first four bases of rc(prefix)"""
    s = rc(prefix_window(prefix, L, R))
    d = 0
    for c in s[:4]:
        d = (d << 2) | int(c)
    return d


def forward_keys(text, L, R):
    """-> (keys, digits) of the FORWARD record of every valid window of a text (uint8 ASCII, '\\n' between records)"""
    k = L + 1 + R
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
        code[ch | 0x20] = i
    c = code[np.asarray(text, dtype=np.uint8)]
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    ok = np.flatnonzero(bad[k:] - bad[:-k] == 0)
    c = c.astype(np.uint64) & np.uint64(3)
    keys = np.zeros(len(ok), dtype=np.uint64)
    order = list(range(L)) + list(range(L + 1, k)) + [L]
    for j, i in enumerate(order):
        keys |= c[ok + i] << np.uint64(62 - 2 * j)
    dig = np.zeros(len(ok), dtype=np.int64)
    for i in digit_positions(R):
        dig = (dig << 2) | c[ok + i].astype(np.int64)
    return keys, dig


def text_pos(at, n, records=CC.RECORDS):
    """position `at` of the codes -> its position in the text (one separator behind every record)"""
    rl = (n + records - 1) // records
    return at + at // rl


# ----------------------------------------------------------------------------
# a. uniform families
# ----------------------------------------------------------------------------
UNIFORM_LDR = (20, 1, 6)
OTHER_R = (0, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def uniform(config=71, n_in=2, n_out=2, length=300_000):
    from krisp_amd import synth
    fam = synth.family(config, n_in, n_out, length, records=CC.RECORDS, snp_every=2000)
    texts, flags = [t for _, _, t in fam], [f for _, f, _ in fam]
    # (pillars first on each side, as everywhere: in, in, out, out)
    return texts, flags


# ----------------------------------------------------------------------------
# b. planted windows at (25, 1, 2), 800 kbp
# ----------------------------------------------------------------------------
PLANT_LDR = (25, 1, 2)
PLANT_LEN = 800_000
PIN, CIN, POUT, COUT = 0, 1, 2, 3
KINDS = ("fwd", "rev", "both", "base0", "base1", "base2", "base3", "palin", "nrun", "recend_a", "recend_b")


@functools.lru_cache(maxsize=None)
def planted():
    """-> texts, flags, plants.  plants[kind] = (W_in, W_out): the window every ingroup / outgroup genome holds under the kind's
    candidate (they differ at position L only); plants["two"] = (V, U): see below.  What the COARSE genomes' texts hold:
      fwd       the window itself: only its forward record lies under the candidate
      rev       its reverse complement: only the REVERSE record of that text's window does
      both      both texts, at two places: the key twice, once of each reading
      base0..3  its reverse complement, the ingroup's diagnostic base being A, C, G, T: the base the reverse record shows
      palin     a window that is its own reverse complement in the ingroup genomes (k is even): two equal records of one window
      nrun      the window between two N (written into the texts): the windows next to it hold a bad base
      recend_a / recend_b   the window as the last / the first k bases of a record
      two       ONE window V in the coarse ingroup genome whose forward record lies under candidate P1 = prefix(V) and whose
                reverse record lies under candidate P2 = prefix(U), U = rc(V): the pillars hold V with position L varied (P1's
                site) and, elsewhere, U with ITS position L varied (P2's site)"""
    L, _, R = PLANT_LDR
    k = L + 1 + R
    rng = CC._rng("strand planted")
    codes, flags = CC._family_codes(61, 2, 2, PLANT_LEN, 0.001)
    assert flags == [True, True, False, False]
    codes = [codes[0], codes[1], codes[2], codes[3]]
    slot = CC._slots()
    plants = {}
    nmark = []
    rl = (PLANT_LEN + CC.RECORDS - 1) // CC.RECORDS

    def site(b1=None):
        w = rng.integers(0, 4, size=k, dtype=np.uint8)
        b1 = int(rng.integers(0, 4)) if b1 is None else b1
        b2 = CC._other(rng, b1)
        wi, wo = w.copy(), w.copy()
        wi[L], wo[L] = b1, b2
        return wi, wo

    for kind in KINDS:
        wi, wo = site(b1={"base0": A, "base1": C, "base2": G, "base3": T}.get(kind))
        if kind == "palin":
            half = rng.integers(0, 4, size=k // 2, dtype=np.uint8)
            wi = np.concatenate([half, rc(half)])
            assert np.array_equal(wi, rc(wi))
            wo = wi.copy()
            wo[L] = CC._other(rng, int(wi[L]))
        plants[kind] = (wi, wo)
        at, at2 = next(slot), next(slot)
        if kind == "recend_a":
            at = rl - k
        elif kind == "recend_b":
            at = rl
        for g in range(4):
            w = wi if flags[g] else wo
            coarse = g in (CIN, COUT)
            if coarse and (kind == "rev" or kind.startswith("base")):
                CC._put(codes[g], at, rc(w))
            else:
                CC._put(codes[g], at, w)
            if coarse and kind == "both":
                CC._put(codes[g], at2, rc(w))
        if kind == "nrun":
            nmark.append(at)
    # "two"
    V = rng.integers(0, 4, size=k, dtype=np.uint8)
    a, c = int(V[L]), int(V[R])
    a2, c2 = CC._other(rng, a), CC._other(rng, c)
    Va2, Vc2 = V.copy(), V.copy()
    Va2[L] = a2
    Vc2[R] = c2
    at_a, at_b = next(slot), next(slot)
    CC._put(codes[PIN], at_a, V)
    CC._put(codes[PIN], at_b, rc(V))
    CC._put(codes[POUT], at_a, Va2)
    CC._put(codes[POUT], at_b, rc(Vc2))
    CC._put(codes[CIN], at_a, V)                         # the one window
    CC._put(codes[COUT], at_a, Va2)
    CC._put(codes[COUT], at_b, rc(Vc2))
    plants["two"] = (V, rc(V))
    texts = CC._texts(codes)
    for at in nmark:
        for g in (CIN, COUT):
            p = text_pos(at, PLANT_LEN)
            assert texts[g][p - 1] != 10 and texts[g][p + k] != 10
            texts[g][p - 1] = ord("N")
            texts[g][p + k] = ord("N")
    return texts, flags, plants


# ----------------------------------------------------------------------------
# c. a digit without keys: genomes without G
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gfree():
    """800 kbp over A, C, T.  A coarse genome's forward keys hold no G: the digits with a G are buckets without keys.  The
    pillars' reverse records do hold G, and the candidates among them (a planted site at position R of a window) are in
    forward classes of such digits -- the coarse genomes hold them through reverse records, found in a digit that has keys"""
    n, mu, every = PLANT_LEN, 0.001, 2000
    rng = CC._rng("strand gfree")
    alpha = np.array([A, C, T], dtype=np.uint8)
    anc = alpha[rng.integers(0, 3, size=n)]
    sites = np.arange(every // 2, n, every)
    i1 = rng.integers(0, 3, size=len(sites))
    i2 = (i1 + rng.integers(1, 3, size=len(sites))) % 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        m = rng.binomial(n, mu)
        c[rng.integers(0, n, size=m)] = alpha[rng.integers(0, 3, size=m)]
        c[sites] = alpha[i1 if f else i2]
        codes.append(c)
    return CC._texts(codes), flags


# ----------------------------------------------------------------------------
# d. digits with candidates of one reading only: a short list
# ----------------------------------------------------------------------------
SPARSE_SITES = 12


@functools.lru_cache(maxsize=None)
def sparse():
    """four equal genomes of 800 kbp but for SPARSE_SITES single bases that differ between the sides: two candidates per site
    (the window with the site at position L, and the reverse record of the window with the site at position R) -- far fewer
    candidates than classes, so nearly every digit that has candidates has them in one reading only"""
    rng = CC._rng("strand sparse")
    anc = rng.integers(0, 4, size=PLANT_LEN, dtype=np.uint8)
    sites = 5000 + 60_000 * np.arange(SPARSE_SITES)
    b1 = rng.integers(0, 4, size=SPARSE_SITES, dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=SPARSE_SITES, dtype=np.uint8)) & 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        c[sites] = b1 if f else b2
        codes.append(c)
    return CC._texts(codes), flags


# ----------------------------------------------------------------------------
# the oracle's view of a case, once per case
# ----------------------------------------------------------------------------
_CENSUS = {}


def census(K, name, texts, flags, ldr):
    """-> dict: keys (sorted, per genome), C (the pillars' filtered list), cands / recs (the final list and its records, sorted by
    key and genome), hits[g] (the records of coarse genome g under a prefix of C, sorted)"""
    if name not in _CENSUS:
        L, D, R = ldr
        keys = [K.sorted_keys(t.tobytes(), L, D, R) for t in texts]
        pin, pout = CC.pillars(flags)
        Cl = K.intersect([keys[pin], keys[pout]], [True, False], L, D, R, apply_filter=True)
        cands = K.intersect(keys, flags, L, D, R, apply_filter=True)
        recs = np.sort(K.collect(keys, cands, L, D, R), order=["key", "genome"])
        pm = np.uint64(pmask(L, R))
        hits = {g: keys[g][np.isin(keys[g] & pm, Cl["prefix"])] for g in CC.coarse(flags)}
        out = dict(keys=keys, C=Cl, cands=cands, recs=recs, hits=hits)
        for arr in keys + [Cl, cands, recs] + list(hits.values()):
            arr.setflags(write=False)
        _CENSUS[name] = out
    return _CENSUS[name]


def classes(Cl, ldr):
    """-> (forward, reverse): candidates of C per digit and reading"""
    L, _, R = ldr
    f = np.bincount([class_fwd(p, L, R) for p in Cl["prefix"]], minlength=256)
    r = np.bincount([class_rev(p, L, R) for p in Cl["prefix"]], minlength=256)
    return f, r
