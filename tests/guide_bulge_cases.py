"""Seeded texts for the bulged guide-hit search with what each of them must produce: no code of krisp_amd/.

A case is a protospacer length G, a distance M, a largest bulge B and a motif pair: every (G, M, B) of GS x MS x BS, its
motifs by rotation, so that every motif pair meets every G, every M and every B (24 cases; the motifs do not change which
cut is taken, only the pam field and need_pam's selection, so their full product with the cuts would test nothing more).
case(name) is a text of three tiles of 16 384 window starts and a begun fourth, as guide_hit_cases.N_TEXT, its guides and
its PLANTS: windows written into the random text, each with the row it pins.  short_texts(name) are texts shorter than
G - B, of exactly G - b and of exactly G + b bytes; dense(...) is a period-G repeat of a guide whose seed pairs own more
rows than there are pairs.  reference() is guide_bulges_reference.ref_bulge_hits on a case, computed once and shared.

A plant writes entry text T (the guide, or its reverse complement for strand 1) as T[:q] + b random bases + T[q:] (DNA) or
T[:q] + T[q + b:] (RNA), with `subs` aligned columns substituted.  Repeats can move the canonical cut and lower the
distance, so the row a plant pins is the definition's, said once more in plain Python over the FINISHED text
(guide_bulges_reference.window_row: no numpy, no tables): the plant fixes the key (pos, strand, guide, bulge), that the row
exists (or does not) and that its distance is at most `subs`; window_row fills in the rest.  The guide sets differ by G
because a reference call is held to MAX_COMPARISONS byte comparisons."""
import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_bulges_reference as ref                                        # noqa: E402
from guide_hit_cases import INSTANCE, NON_INSTANCE, N_TEXT, THREAD, TILE, MAX_COMPARISONS, _Text, _other, _rand   # noqa: E402,F401

GS = (20, 21, 28, 40)
MS = (0, 1, 2)
BS = (1, 2)
MOTIF_NAMES = ("none", "tttv", "long")
MOTIFS = {"none": ("", ""), "tttv": ("TTTV", ""), "long": ("NNNNTTTV", "HNNNNNNN")}
CASES = {f"g{G}_m{M}_b{B}_{MOTIF_NAMES[(gi + M + B) % 3]}": dict(G=G, M=M, B=B, motifs=MOTIF_NAMES[(gi + M + B) % 3])
         for gi, G in enumerate(GS) for M in MS for B in BS}
PAD = 9                             # bytes beside a planted window that belong to the plant (a motif has 8 at most)


def half(G, B):
    """the seeds' length: every cut leaves one half whole"""
    return (G - B) // 2


@functools.lru_cache(maxsize=None)
def guides(G):
    """-> (texts, roles): roles name the index of 'random', 'homopolymer', 'dinucleotide', 'palindrome' (even G), 'equal'
    (the first of two equal texts) where the set has one"""
    rng = np.random.default_rng(zlib.crc32(f"bulge guides {G}".encode()))
    out, roles = [], {}

    def add(role, t):
        roles[role] = len(out)
        out.append(t)

    def fresh():
        while True:
            t = _rand(rng, G)
            if t not in out and t != ref.rc(t):
                return t

    add("random", fresh())
    add("homopolymer", "A" * G)
    if G != 40:
        add("dinucleotide", ("AC" * G)[:G])
    if G % 2 == 0:
        h = _rand(rng, G // 2)
        add("palindrome", h + ref.rc(h))
    if G in (20, 21):
        add("equal", fresh())
        out.append(out[-1])
    return out, roles


def _window(T, bulge, q, insert):
    b = abs(bulge)
    return T[:q] + insert + T[q:] if bulge > 0 else T[:q] + T[q + b:]


def plant(T, rng, kind, gs, gi, pos, strand, bulge, q, pam5, pam3, subs=0, motifs=("hit", "hit"), damage=None, lower=False,
          present=True, also=()):
    """writes the bulged window of guide gi at pos (see the module's text).  q: the cut in the ENTRY's orientation.  damage:
    (window index, byte) written over the finished window ("lower": that letter in lower case).  -> the plant"""
    g = gs[gi]
    G, a = len(g), len(pam5)
    b = abs(bulge)
    Lw = G + bulge
    n = len(T.t)
    T.own(pos - PAD, pos + Lw + PAD)
    E = g if strand == 0 else ref.rc(g)
    aligned = [c for c in range(G) if bulge > 0 or not q <= c < q + b]
    cols = sorted(rng.choice(aligned, size=subs, replace=False).tolist()) if subs else []
    E2 = list(E)
    for c in cols:
        E2[c] = _other(E2[c])
    insert = "".join(_other(E[q]) for _ in range(b)) if bulge > 0 else ""
    w = _window("".join(E2), bulge, q, insert)
    assert len(w) == Lw
    T.put(pos, w.lower() if lower else w)
    bits = [1, 1]
    for side, (motif, how) in enumerate(zip((pam5, pam3), motifs)):
        if not motif:
            continue
        m = INSTANCE[motif] if how == "hit" else NON_INSTANCE[motif]
        for j, ch in enumerate(m):
            if side == 0:
                i = pos + Lw + a - 1 - j if strand else pos - a + j
            else:
                i = pos - 1 - j if strand else pos + Lw + j
            if not 0 <= i < n:
                bits[side] = 0
            T.put(i, ref.rc(ch) if strand else ch)
        if how != "hit":
            bits[side] = 0
    omit_present = present and not lower
    if damage is not None:
        i, byte = damage
        if byte == "lower":
            T.put(pos + i, chr(T.t[pos + i]).lower())
            omit_present = False
        else:
            T.put(pos + i, byte)
            present = omit_present = False
    return dict(kind=kind, keys=[(pos, strand, x, bulge) for x in (gi,) + tuple(also)], subs=subs, pam=bits[0] | (bits[1] << 1),
                present=(present, omit_present), q=q)


def pin(plants, text, gs, M):
    """fills in every plant's rows over the finished text: rows[omit] = {key: (mismatches, columns, bulge_column)} by the
    definition in plain Python; a plant that must be present is, within its substitutions"""
    for omit in (0, 1):
        S, bad = ref.plain.stage(text, omit)
        S, bad = S.tolist(), bad.tolist()
        for p in plants:
            rows = {}
            for pos, strand, gi, bulge in p["keys"]:
                E = gs[gi] if strand == 0 else ref.rc(gs[gi])
                r = ref.window_row(S, bad, pos, E, strand == 1, bulge, M)
                if p["present"][omit]:
                    assert r is not None and r[0] <= p["subs"], (p["kind"], pos, strand, gi, bulge, r)
                    rows[(pos, strand, gi, bulge)] = r
                elif p["kind"].startswith("absent"):
                    assert r is None, (p["kind"], pos, strand, gi, bulge, r)
            p.setdefault("rows", {})[omit] = rows
    return plants


def _bulges(B):
    return [s * b for b in range(1, B + 1) for s in (1, -1)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(text, guides, roles, G, M, B, pam5, pam3, plants)"""
    c = CASES[name]
    G, M, B = c["G"], c["M"], c["B"]
    gs, roles = guides(G)
    pam5, pam3 = MOTIFS[c["motifs"]]
    h = half(G, B)
    rng = np.random.default_rng(zlib.crc32(f"bulge case {name}".encode()))
    T = _Text(rng, N_TEXT)
    plants = []
    R = roles["random"]

    def P(kind, pos, strand, bulge, q, gi=R, **kw):
        plants.append(plant(T, rng, kind, gs, gi, pos, strand, bulge, q, pam5, pam3, **kw))
        return plants[-1]

    def cuts(bulge):
        return range(1, G if bulge > 0 else G + bulge)

    # ---- seams.  The scan's windows are the halves' (h letters): tile t's first window is t * TILE.  A right half (entry
    # orientation) that is the first window of a tile belongs to a row whose window starts in the tile before (its cut lies
    # left of the half: q = 2, so the right half owns the row); a left half that is the last window of a tile owns the row
    # whose cut lies right of it (q = G - 3).  The same at thread edges; either strand over the tiles
    rot = list(CASES).index(name)
    bl = _bulges(B)
    seams = [("right", TILE, rot % 2), ("left", 2 * TILE, rot % 2), ("right" if rot % 4 < 2 else "left", 3 * TILE, 1 - rot % 2),
             ("left", TILE + THREAD * 40, 1 - rot % 2), ("right", TILE + THREAD * 80, 1 - rot % 2),
             ("left", 2 * TILE + THREAD * 40, rot % 2), ("right", 2 * TILE + THREAD * 80, rot % 2)]
    for i, (side, edge, strand) in enumerate(seams):
        bulge = bl[(rot + i) % len(bl)]
        Lw = G + bulge
        if side == "right":
            P(f"seam_right_half_{edge}", edge + h - Lw, strand, bulge, 2, subs=M if i % 2 else 0)
        else:
            P(f"seam_left_half_{edge}", edge - 1, strand, bulge, Lw - 3 - max(bulge, 0), subs=0 if i % 2 else M)
    # ---- the text's ends: position 0 and the last window (short_texts has a right half whose window would start before the text)
    P("first", 0, 0, 1, G // 2)
    P("last", N_TEXT - (G + B), 1, B, G // 2)
    P("last_rna", N_TEXT - 200 - (G - B), 0, -B, G // 2)
    # ---- the background: two separators, a run of N, a stretch of lower case
    for at, s_ in ((9001, "\n"), (33333, "\n"), (21000, "N" * 11)):
        T.own(at, at + len(s_))
        T.put(at, s_)
    T.own(40000, 40400)
    T.put(40000, bytes(T.t[40000:40400]).decode("ascii").lower())
    slots = iter(range(300, N_TEXT - 300, 8))

    def slot(width):
        while True:
            p = next(slots)
            if T.free(p - PAD, p + width + PAD):
                return p

    # ---- one byte short: the window runs into a record's end, or starts on one; N, a separator and lower case in the
    # aligned part and in the unpartnered bases
    for strand in (0, 1):
        for bulge in _bulges(B):
            Lw = G + bulge
            q = G // 2
            P("absent_record_end", slot(Lw), strand, bulge, q, damage=(Lw - 1, "\n"))
            P("absent_record_start", slot(Lw), strand, bulge, q, damage=(0, "\n"))
            P("absent_N_aligned", slot(Lw), strand, bulge, q, damage=(q // 2, "N"))
            P("lower_aligned", slot(Lw), strand, bulge, q, damage=(Lw - 2, "lower"))
            if bulge > 0:
                P("absent_N_unpartnered", slot(Lw), strand, bulge, q, damage=(q + bulge - 1, "N"))
                P("absent_separator_unpartnered", slot(Lw), strand, bulge, q, damage=(q, "\n"))
                P("lower_unpartnered", slot(Lw), strand, bulge, q, damage=(q, "lower"))
    # ---- every cut of every bulge on both strands, with 0 and with M substitutions in turn, the motifs beside two of three
    i = 0
    for strand in (0, 1):
        for bulge in _bulges(B):
            for q in cuts(bulge):
                i += 1
                P("cut", slot(G + bulge), strand, bulge, q, subs=M if i % 2 else 0,
                  motifs=("hit", "hit") if i % 3 else (("miss", "hit") if i % 2 else ("hit", "miss")))
    # ---- the straddling cut: an RNA bulge of 2 at q = G / 2 - 1 lies in both halves of G / 2 letters; h = (G - B) / 2 keeps
    # one of them clear of it
    if B == 2:
        for strand in (0, 1):
            P("straddle", slot(G - 2), strand, -2, G // 2 - 1, subs=M)
    # ---- the table: ties (a homopolymer, a dinucleotide repeat: one pair owns up to 2 B rows), a palindrome, equal texts
    for role in ("homopolymer", "dinucleotide", "palindrome"):
        if role in roles:
            for strand in (0, 1):
                for bulge in _bulges(B):
                    P(role, slot(G + bulge), strand, bulge, G // 3, gi=roles[role])
    if "equal" in roles:
        e = roles["equal"]
        for bulge in _bulges(B):
            P("equal_texts", slot(G + bulge), bulge > 0, bulge, G - 2 if bulge > 0 else G + bulge - 2, gi=e, also=(e + 1,), subs=M)
    text = bytes(T.t)
    pin(plants, text, gs, M)
    return dict(text=text, guides=gs, roles=roles, G=G, M=M, B=B, pam5=pam5, pam3=pam3, plants=plants)


@functools.lru_cache(maxsize=None)
def short_texts(name):
    """-> list of (text, plants): the empty text, one byte, G - B - 1 bytes, the guide's last G - 1 letters (a right half
    whose window would start before the text), and for every bulge and strand the window alone (exactly G + b or G - b
    bytes: position 0 is the last window), the window one byte short at either end, and the window inside 2 * 20 more bytes"""
    c = CASES[name]
    G, M, B = c["G"], c["M"], c["B"]
    gs, roles = guides(G)
    pam5, pam3 = MOTIFS[c["motifs"]]
    rng = np.random.default_rng(zlib.crc32(f"bulge short {name}".encode()))
    g = gs[roles["random"]]
    out = [(b"", []), (b"A", []), (g[:G - B - 1].encode("ascii"), []), (g[1:].encode("ascii"), []), (ref.rc(g)[:G - 1].encode("ascii"), [])]
    for strand in (0, 1):
        for bulge in _bulges(B):
            Lw = G + bulge
            q = (G // 2 + bulge) if strand else G // 2 - 1
            T = _Text(rng, Lw)
            out.append((T, [plant(T, rng, "alone", gs, roles["random"], 0, strand, bulge, q, pam5, pam3)]))
            for cutoff in (slice(1, None), slice(None, -1)):                # one byte short at the start, at the end
                T2 = _Text(rng, Lw)
                plant(T2, rng, "short", gs, roles["random"], 0, strand, bulge, q, pam5, pam3)
                out.append((bytes(T2.t)[cutoff], []))
            T = _Text(rng, Lw + 40)
            out.append((T, [plant(T, rng, "inside", gs, roles["random"], 20, strand, bulge, q, pam5, pam3, subs=M)]))
    done = []
    for t, pl in out:
        text = bytes(t.t) if isinstance(t, _Text) else t
        done.append((text, pin(pl, text, gs, M)))
    return done


def seed_pairs(text, omit, gs, M, B):
    """how many seed pairs the near scan finds: positions x entries x halves whose h staged bytes hold no bad byte and
    differ from the half in at most M columns (brute force)"""
    from numpy.lib.stride_tricks import sliding_window_view
    G = len(gs[0])
    h = half(G, B)
    up, bad = ref.plain.stage(text, omit)
    if len(up) < h:
        return 0
    valid = ~sliding_window_view(bad, h).any(axis=1)
    windows = sliding_window_view(up, h)
    total = 0
    for g in gs:
        for E in (g, ref.rc(g)):
            for t in (E[:h], E[G - h:]):
                d = np.count_nonzero(windows != np.frombuffer(t.encode("ascii"), dtype=np.uint8), axis=1)
                total += int(np.count_nonzero(valid & (d <= M)))
    return total


@functools.lru_cache(maxsize=None)
def dense(G=20, repeats=400):
    """a period-G repeat of one random guide, some 800 seed pairs: with M = 2 and B = 2 every exact site is
    shadowed by bulged rows next to its ends, so a block of pairs owns more rows than it has pairs.
    -> (text, [guide], M, B)"""
    rng = np.random.default_rng(zlib.crc32(f"bulge dense {G}".encode()))
    while True:
        g = _rand(rng, G)
        if g != ref.rc(g) and len(set(g)) == 4:
            break
    return (g * repeats).encode("ascii"), [g], 2, 2


@functools.lru_cache(maxsize=None)
def reference(name, omit, need_pam=False):
    """the reference's hits of case(name): computed once, shared, never written to.  need_pam: the rows with pam = 3 of the
    list without it, which is all the definition's need_pam does (the step's CPU test asks the definition itself)"""
    if need_pam:
        hits = reference(name, omit)
        hits = hits[hits["pam"] == 3]
        hits.setflags(write=False)
        return hits
    c = case(name)
    assert ref.comparisons(len(c["text"]), c["guides"], c["B"]) < MAX_COMPARISONS
    hits = ref.ref_bulge_hits(c["text"], omit, c["guides"], c["M"], c["B"], c["pam5"], c["pam3"], need_pam)
    hits.setflags(write=False)
    return hits


def rows_of(hits):
    """(pos, strand, guide, bulge) -> (mismatches, columns, bulge_column, pam)"""
    return {(int(x["pos"]), int(x["strand"]), int(x["guide"]), int(x["bulge"])):
            (int(x["mismatches"]), int(x["columns"]), int(x["bulge_column"]), int(x["pam"])) for x in hits}


def check_plants(plants, hits, omit, shift=0, pam=True):
    """every plant's rows are in the list (or are not) with the distance, the mask and the bulge column that the plain-Python
    definition gives and -- for a plant whose motifs lie in the text -- the motif bits.  shift: the hits' positions are
    those of a slice that starts at `shift`"""
    got = rows_of(hits)
    for p in plants:
        for key in p["keys"]:
            row = got.get((key[0] - shift,) + key[1:])
            want = p["rows"][omit].get(key)
            if want is None:
                if not p["present"][omit] and p["kind"].startswith("absent"):
                    assert row is None, (p["kind"], key, row)
                continue
            assert row is not None, (p["kind"], key)
            assert row[:3] == want, (p["kind"], key, row, want)
            if pam and p["kind"] == "cut":
                assert row[3] == p["pam"], (p["kind"], key, row, p["pam"])
