"""Seeded genomes for "one test, one pass" of the coarse probe (krisp_amd/csrc/co_pass.inc): a key of a one-strand
genome is tested once, under M = the key's bits without window positions L and R, and a pass of a digit holds a forward and a
reverse round of its candidates in one table.  No code of krisp_amd/ but synth.  All cases are at (25, 1, 2); the genomes are
[ingroup pillar, coarse ingroup, outgroup pillar, coarse outgroup] as in strand_cases.py, whose windows, keys, digits and
classes are used here.

tests/test_onepass_cases.py shows, with oracle/kmer_oracle alone, that each case forces the branch it is named for;
tests/test_gpu_coarse_onepass.py runs them on the device."""
import functools

import numpy as np

import coarse_cases as CC
import coarse_stream_cases as SC
import strand_cases as S

LDR = S.PLANT_LDR
L, _, R = LDR
KW = L + 1 + R
LEN = S.PLANT_LEN
PIN, CIN, POUT, COUT = S.PIN, S.CIN, S.POUT, S.COUT
QCAP = 2048                 # k_coarse.inc CO_QCAP: queued keys of one unit
TCAP = CC.CO_TCAP
DIGIT_POS = S.digit_positions(R)            # window positions 0, 1, 3, 4


def _with_digits(rng, fwd, rev):
    """a random window whose forward digit is `fwd` and whose reverse complement's digit is `rev`"""
    w = rng.integers(0, 4, size=KW, dtype=np.uint8)
    for j, i in enumerate(DIGIT_POS):
        w[i] = (fwd >> (6 - 2 * j)) & 3
        w[KW - 1 - i] = 3 - ((rev >> (6 - 2 * j)) & 3)
    assert S.digit_of(w, R) == fwd and S.digit_of(S.rc(w), R) == rev
    return w


def window_of(key):
    """a key -> the codes of its window in text order (strand_cases.key_of backwards)"""
    b = [(int(key) >> (62 - 2 * j)) & 3 for j in range(KW)]
    return np.array(b[:L] + [b[L + R]] + b[L:L + R], dtype=np.uint8)


def _site(rng, w):
    """-> (ingroup window, outgroup window): w with two different bases at position L"""
    b1 = int(rng.integers(0, 4))
    wi, wo = w.copy(), w.copy()
    wi[L], wo[L] = b1, CC._other(rng, b1)
    return wi, wo


def _equal_genomes(rng):
    anc = rng.integers(0, 4, size=LEN, dtype=np.uint8)
    return [anc.copy() for _ in range(4)], [True, True, False, False]


# ----------------------------------------------------------------------------
# a. entries with equal pattern & M
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def siblings():
    """-> texts, flags, plants over the family of strand_cases.planted.  plants:
      "fwd4"  four candidates whose prefixes differ at window position R only: equal P & M.  The coarse genomes hold each
              window itself: every one of those keys lies under exactly one of the four forward entries
      "rev3"  three candidates u_c (u with base c at position R) which the coarse genomes hold as rc(u_c): forward windows
              that differ at THEIR position L only, found through reverse entries whose Q differ at position L only
      "lone"  rc(u_3), in the coarse ingroup genome alone: it shares key & M with the windows of "rev3" and lies under no entry
      "fwd3" / "lone_f"  the same with three forward siblings and the window of the fourth base at position R"""
    rng = CC._rng("onepass siblings")
    codes, flags = CC._family_codes(62, 2, 2, LEN, 0.001)
    slot = CC._slots()
    plants = {"fwd4": [], "rev3": [], "fwd3": []}

    def group(kind, n, as_rc):
        w = rng.integers(0, 4, size=KW, dtype=np.uint8)
        wi, wo = _site(rng, w)
        for c in range(4):
            xi, xo = wi.copy(), wo.copy()
            xi[R], xo[R] = c, c
            at = next(slot)
            if c < n:
                plants[kind].append((xi, xo))
                for g in range(4):
                    x = xi if flags[g] else xo
                    CC._put(codes[g], at, S.rc(x) if as_rc and g in (CIN, COUT) else x)
            else:
                plants["lone" if as_rc else "lone_f"] = xi
                CC._put(codes[CIN], at, S.rc(xi) if as_rc else xi)

    group("fwd4", 4, False)
    group("rev3", 3, True)
    group("fwd3", 3, False)
    return CC._texts(codes), flags, plants


# ----------------------------------------------------------------------------
# b. digits whose readings take different numbers of rounds
# ----------------------------------------------------------------------------
# (a digit with reverse plants is not the reverse complement of a named digit: the other strand's candidate of such a plant has
# the digit's reverse complement for its reverse class)
UNEVEN_F, UNEVEN_R = 0x1B, 0x05             # a digit with forward candidates only, one with reverse candidates only
UNEVEN_X = {1: (0x2D, 3, 1), 10: (0x71, 25, 5), 50: (0x93, 120, 20)}       # KR_COARSE_TCAP -> (digit, forward, reverse): rf = 3, rr = 1
UNEVEN_ONE = 5


STRETCH = L + KW - R        # bases around a site that reach one of its two candidates: the window with the site at position L, and
                            # the window of the other strand with the site at position L, which starts R bases in front of the site


def stretch_classes(p):
    """the four classes of the two candidates of the site at position L of a stretch: (forward, reverse) of the window that
    starts the stretch, (forward, reverse) of the other strand's"""
    w, x = p[:KW], p[L - R:]
    return S.digit_of(w, R), S.digit_of(S.rc(w), R), S.digit_of(S.rc(x), R), S.digit_of(x, R)


def _stretch(rng, d, forward, avoid):
    """a random stretch whose first window has the forward (or the reverse) class d; its three other classes avoid `avoid`"""
    for _ in range(10_000):
        p = rng.integers(0, 4, size=STRETCH, dtype=np.uint8)
        for j, i in enumerate(DIGIT_POS):
            if forward:
                p[i] = (d >> (6 - 2 * j)) & 3
            else:
                p[KW - 1 - i] = 3 - ((d >> (6 - 2 * j)) & 3)
        cl = stretch_classes(p)
        mine = 0 if forward else 1
        if cl[mine] == d and not any(c in avoid for j, c in enumerate(cl) if j != mine):
            return p
    raise AssertionError(f"no stretch for digit {d:#x}")


@functools.lru_cache(maxsize=None)
def uneven():
    """-> texts, flags, plan.  Four equal genomes of 800 kbp but for the planted sites (strand_cases.sparse): the candidates are
    the plants alone.  plan[digit] = (forward, reverse) candidates of the digit; every other class of a planted candidate lies
    in a digit that is not named here.  Odd plants stand as their reverse complement in the coarse genomes: both readings hit"""
    rng = CC._rng("onepass uneven")
    codes, flags = _equal_genomes(rng)
    slot = CC._slots()
    plan = {UNEVEN_F: (UNEVEN_ONE, 0), UNEVEN_R: (0, UNEVEN_ONE)}
    plan.update({d: (nf, nr) for d, nf, nr in UNEVEN_X.values()})
    named = tuple(plan)
    i = 0
    for d, (nf, nr) in plan.items():
        for q in range(nf + nr):
            p = _stretch(rng, d, q < nf, named)
            b1 = int(rng.integers(0, 4))
            pi, po = p.copy(), p.copy()
            pi[L], po[L] = b1, CC._other(rng, b1)
            at = next(slot)
            for g in range(4):
                x = pi if flags[g] else po
                CC._put(codes[g], at, S.rc(x) if (i & 1) and g in (CIN, COUT) else x)
            i += 1
    return CC._texts(codes), flags, plan


# ----------------------------------------------------------------------------
# c. a full table and a second pass
# ----------------------------------------------------------------------------
FULL_BLOCKS = 6600
FULL_DIGIT = 0


@functools.lru_cache(maxsize=None)
def full():
    """coarse_cases.dense at 800 kbp with blocks A A x A A ... T T s T T (s = the site at position L): every block-aligned
    window's forward class AND reverse class is digit 0, so the first pass of digit 0 holds 6144 + 6144 entries -- 12 288 of
    the table's 16 384 slots -- and a second pass holds the rest"""
    n, mu, at = LEN, 0.001, 20_000
    rng = CC._rng("onepass full")
    anc = rng.integers(0, 4, size=n, dtype=np.uint8)
    body = rng.integers(0, 4, size=(FULL_BLOCKS, KW), dtype=np.uint8)
    for i in DIGIT_POS:
        body[:, i] = 0
        body[:, KW - 1 - i] = 3
    anc[at:at + KW * FULL_BLOCKS] = body.reshape(-1)
    sites = at + KW * np.arange(FULL_BLOCKS) + L
    b1 = rng.integers(0, 4, size=FULL_BLOCKS, dtype=np.uint8)
    b2 = (b1 + rng.integers(1, 4, size=FULL_BLOCKS, dtype=np.uint8)) & 3
    codes, flags = [], [True, True, False, False]
    for f in flags:
        c = anc.copy()
        CC._mutate(rng, c, mu)
        c[sites] = b1 if f else b2
        codes.append(c)
    return CC._texts(codes), flags


# ----------------------------------------------------------------------------
# d. the queue, with hits of both readings
# ----------------------------------------------------------------------------
QUEUE = (QCAP - 1, QCAP, QCAP + 1)
QUEUE_DIGIT = 0x8C          # G A (x) T A


@functools.lru_cache(maxsize=None)
def queue(hits):
    """-> texts, flags, plants.  coarse_stream_cases.queue for the one-strand form: `hits` plants whose forward AND reverse
    class is QUEUE_DIGIT, held by every genome; genome 1 (coarse) is a mini genome of the plants alone, one record per window,
    the odd ones as their reverse complement: its bucket of that digit is one unit of `hits` keys, every one a true hit -- the
    even ones of the forward reading, the odd ones of the reverse reading --, and nothing else passes the prefilter there"""
    flags = [True, True, False, False]
    rng = SC._rng(f"onepass queue {hits}")
    codes = SC._family(rng, 4, LEN, flags, 2000)
    plants = [_site(rng, _with_digits(rng, fwd=QUEUE_DIGIT, rev=QUEUE_DIGIT)) for _ in range(hits)]
    texts = []
    for g in range(4):
        mine = [wi if flags[g] else wo for wi, wo in plants]
        if g == CIN:
            texts.append(SC._text([S.rc(w) if i & 1 else w for i, w in enumerate(mine)]))
        else:
            texts.append(SC._text(SC._records(codes[g]) + mine))
    return texts, flags, plants


# ----------------------------------------------------------------------------
# the passes of a call, from the census
# ----------------------------------------------------------------------------
def passes(c, texts, flags, tcap=TCAP, one_pass=1):
    """-> (forward rounds, reverse rounds, passes) of one call: per digit in which a coarse genome has a key, the tables its
    candidates of each reading take, and the passes they share (one_pass) or take one after the other"""
    f, r = S.classes(c["C"], LDR)
    have = np.zeros(256, dtype=bool)
    for g in CC.coarse(flags):
        have |= np.bincount(S.forward_keys(texts[g], L, R)[1], minlength=256) > 0
    rf, rr = -(-f[have] // tcap), -(-r[have] // tcap)
    return int(rf.sum()), int(rr.sum()), int(np.maximum(rf, rr).sum() if one_pass else (rf + rr).sum())
