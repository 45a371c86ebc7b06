"""Long texts for the scans whose expected lists are exact and cheap: no code of krisp_amd/.

For a case text T of the existing generators, U = T + b"\\n" and the long text is U repeated R times.  No window and no motif
crosses a separator, and a motif position on a bad byte reads as one outside the text does (no match), so every list of the
long text is the list of T, repeated with the positions shifted by i * len(U) -- test_scan_repeat_cases.py asserts that with
the brute-force references themselves at R = 3.  len(U) is no multiple of the tile, so the copies meet the tile and thread
seams at every phase.  count() is the least R that gives 1100 tiles: beyond 1024 tiles every thread of k_loc_offsets owns
more than one count, and a list of more than 262 144 sites or seed pairs gives the joins and the extend step as many blocks."""
import numpy as np

TILE = 16384                        # LOC_T * LOC_S window starts
MIN_TILES = 1100
OFFSET_THREADS = 1024               # k_loc_offsets: one workgroup
BLOCK = 256                         # sites of a join's block, seed pairs of the extend step's

# the cases of the long runs (test_scan_repeat_cases.py asserts what they were chosen for)
LOCATE_SEED = 45                    # test_gpu_scan_properties.cases: four tiles, k = 261, some 50 hits of either pass
PRODUCT_SEED = 2                    # product_scan_cases.cases: M = 2, 30 texts a side, more than 500 sites in either pass
BULGE_CASE = "g20_m2_b2_tttv"       # guide_bulge_cases.CASES: B = 2, M = 2, more than 2000 seed pairs


def unit(text):
    """U: the text and a separator"""
    t = text.tobytes() if isinstance(text, np.ndarray) else bytes(text)
    return t + b"\n"


def count(text, tiles=MIN_TILES):
    """the least R whose text has `tiles` tiles of bytes"""
    return -(-tiles * TILE // len(unit(text)))


def long_text(text, R):
    return np.frombuffer(unit(text) * R, dtype=np.uint8)


def repeated(rows, R, period, field="pos"):
    """a structured list of one copy -> the list of R copies `period` bytes apart (tiled and shifted once)"""
    out = np.tile(rows, R)
    if len(rows):
        out[field] += np.repeat(np.arange(R, dtype=np.int64) * period, len(rows)).astype(out[field].dtype)
    return out


def repeated_positions(pos, R, period):
    """ascending positions of one copy -> those of R copies"""
    pos = np.asarray(pos, dtype=np.int64)
    return (np.tile(pos, R) + np.repeat(np.arange(R, dtype=np.int64) * period, len(pos))).astype(np.uint64)


# ----------------------------------------------------------------------------
# the definition's lists of a text, per long case: name -> a structured array with a pos field (the separators: uint64)
# ----------------------------------------------------------------------------
def locate_case():
    from test_gpu_scan_properties import cases
    return cases(LOCATE_SEED)


def locate_lists(text):
    from scan_reference import ref_locate, ref_near, ref_seps
    c = locate_case()
    return dict(locate=ref_locate(text, c["L"], c["D"], c["R"], c["omit"], c["flanks"]),
                near=ref_near(text, c["L"], c["D"], c["R"], c["omit"], c["targets"], c["M"]), seps=ref_seps(text))


def product_case(kind):
    import product_scan_cases as PS
    return PS.cases(PRODUCT_SEED)[kind]


def product_lists(kind, text):
    """kind: "flank" or "primer" (product_scan_cases) -> sites, products, seps"""
    import primers_reference as PR
    import product_scan_cases as PS
    import products_reference as FR
    from scan_reference import ref_seps
    c = product_case(kind)
    if kind == "flank":
        lf, rt = PS.u8(c["left"], c["Le"]), PS.u8(c["right"], c["Re"])
        sites = FR.ref_sites(text, c["omit"], lf, rt, c["Le"], c["Re"], c["M"])
        prods = FR.ref_products(text, c["omit"], lf, rt, c["Le"], c["Re"], c["pairs"], c["M"], c["max_product"])
    else:
        texts = c["left"] + c["right"]
        sites = PR.ref_sites(text, c["omit"], texts, len(c["left"]), c["M"])
        prods = PR.ref_products(text, c["omit"], texts, len(c["left"]), c["pairs"], c["M"], c["max_product"], sites=sites)
    return dict(sites=sites, products=prods, seps=ref_seps(text))


GUIDE_HIT_M = 3                     # the unbulged pass over the bulged case's upload
NEAR_TARGETS = 3                    # ... and the near pass with the first guides as its table, at the case's M


def bulge_case():
    import guide_bulge_cases as BC
    return BC.case(BULGE_CASE)


def bulge_lists(text, guides=None, bulges=True):
    """-> bulges (guides: a part of the case's guides -- the reference's time; bulges=False: not these), guide_hits, near"""
    import guide_bulges_reference as bref
    import guide_hits_reference as href
    from scan_reference import ref_near
    c = bulge_case()
    gs = c["guides"] if guides is None else guides
    G = c["G"]
    out = {}
    if bulges:
        out["bulges"] = bref.ref_bulge_hits(text, False, gs, c["M"], c["B"], c["pam5"], c["pam3"])
    out["guide_hits"] = href.ref_hits(text, False, gs, GUIDE_HIT_M, c["pam5"], c["pam3"])
    targets = np.frombuffer("".join(gs[:NEAR_TARGETS]).encode("ascii"), dtype=np.uint8).reshape(-1, G)
    out["near"] = ref_near(text, 0, G, 0, False, targets, c["M"])
    return out
