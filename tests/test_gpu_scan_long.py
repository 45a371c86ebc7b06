"""The scans over texts of more than 1024 tiles, with lists of more than 1024 blocks' worth of sites and seed pairs: the
regime of a production genome.  k_loc_offsets gives each of its 1024 threads ceil(n / 1024) counts -- one in every other test
--; a workgroup of a scan takes several tiles without any cap (the device holds fewer workgroups than the text has tiles);
the windows' text passes the million bytes up to which an element-stride launch has a thread per byte.

The texts are scan_repeat_cases.py's: a case text and a separator, repeated.  Every expected list is the case text's own,
tiled and shifted once with numpy (test_scan_repeat_cases.py asserts that identity with the references themselves), and is
compared whole.  No variable is set: these are the launches of a production run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_bulge_cases as BC                                             # noqa: E402
import guide_bulges_reference as bref                                      # noqa: E402
import guide_hits_reference as href                                        # noqa: E402
import product_scan_cases as PS                                            # noqa: E402
import scan_repeat_cases as RC                                             # noqa: E402
import test_gpu_guide_bulges as GB                                         # noqa: E402
import test_gpu_guide_hits as GH                                           # noqa: E402
import test_gpu_product_scan_properties as PP                              # noqa: E402
import test_gpu_scan_properties as SP                                      # noqa: E402
from scan_reference import ref_windows                                     # noqa: E402

pytestmark = pytest.mark.gpu


def long_geometry(eng, what, blocks=False):
    """debug_scan() after a scan of a long text: more tiles (and, of a join or the extend step, blocks) than k_loc_offsets
    has threads; no cap; prints the natural grid"""
    d = eng.debug_scan()
    print(what, "tiles", d["tiles"], "natural grid", d["grid"], "blocks of the latest two-pass list", d["blocks"])
    assert d["cap"] == 0 and d["tiles"] >= RC.OFFSET_THREADS + 1 and 1 <= d["grid"] <= d["tiles"], d
    if blocks:
        assert d["blocks"] >= RC.OFFSET_THREADS + 1, d
    return d


def equal_fields(got, want, fields, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in fields:
        assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), (what, f)


def text_rows(windows, width):
    """a list of str -> uint8 [n, width], padded with zero bytes"""
    return np.frombuffer(b"".join(w.encode("ascii").ljust(width, b"\0") for w in windows), dtype=np.uint8).reshape(-1, width)


def test_locate_and_near_beyond_1024_tiles():
    c = RC.locate_case()
    T, k = c["text"], c["k"]
    R, period = RC.count(T), len(RC.unit(T))
    text = RC.long_text(T, R)
    one = RC.locate_lists(T)
    with SP.engine(c["L"], c["D"], c["R"], c["omit"], len(text)) as eng:
        eng.upload(0, text)
        eng.locate_table(c["flanks"])
        eng.near_table(c["targets"], c["M"])
        got = eng.locate(0)
        long_geometry(eng, "locate")
        equal_fields(got, RC.repeated(one["locate"], R, period), ("pos", "strand", "group"), "locate")
        rows = eng.locate_windows(k)
        assert rows.nbytes > 4 << 20 and np.array_equal(rows, np.tile(ref_windows(T, one["locate"], k), (R, 1)))
        near = eng.near(0)
        long_geometry(eng, "near")
        assert not near["pad"].any() and (np.diff(near["pos"].astype(np.int64)) >= 0).all()
        order = np.lexsort((near["target"], near["strand"], near["pos"]))
        equal_fields(near[order], RC.repeated(one["near"], R, period), ("pos", "strand", "target", "mismatches", "flank_mismatches"),
                     "near")
        rows = eng.near_windows(k)
        assert rows.nbytes > 4 << 20 and np.array_equal(rows[order], np.tile(ref_windows(T, one["near"], k), (R, 1)))
        assert np.array_equal(eng.locate_seps(0), np.flatnonzero(text == 10))


@pytest.mark.parametrize("kind", ["flank", "primer"])
def test_products_beyond_1024_tiles_and_1024_join_blocks(kind):
    c = RC.product_case(kind)
    f = RC.product_case("flank")
    T = c["text"]
    R, period = RC.count(T), len(RC.unit(T))
    text = RC.long_text(T, R)
    one = RC.product_lists(kind, T)
    with PP.engine(f["Le"], f["Re"], c["omit"], len(text)) as eng:
        eng.upload(0, text)
        if kind == "flank":
            eng.products_table(PS.u8(c["left"], c["Le"]), PS.u8(c["right"], c["Re"]), c["pairs"], c["M"], c["max_product"])
            hits, sites = eng.products(0), eng.product_sites()
        else:
            eng.primers_table(c["left"] + c["right"], len(c["left"]), c["pairs"], c["M"], c["max_product"])
            hits, sites = eng.primer_products(0), eng.primer_sites()
        d = long_geometry(eng, kind, blocks=True)
        assert d["blocks"] == (len(sites) + RC.BLOCK - 1) // RC.BLOCK
        assert not sites["pad"].any() and not hits["pad"].any()
        assert (np.diff(sites["pos"].astype(np.int64)) >= 0).all()
        order = np.lexsort((sites["entry"], sites["pos"]))
        equal_fields(sites[order], RC.repeated(one["sites"], R, period), one["sites"].dtype.names, "sites")
        equal_fields(hits, RC.repeated(one["products"], R, period), one["products"].dtype.names, "products")
        assert np.array_equal(eng.locate_seps(0), np.flatnonzero(text == 10))


def test_bulged_guide_hits_beyond_1024_tiles_and_1024_extend_blocks():
    """... and, on the same upload, the unbulged pass and the near pass with a small table"""
    from krisp_amd import _native
    c = RC.bulge_case()
    T, G, M, B = c["text"], c["G"], c["M"], c["B"]
    R, period = RC.count(T), len(RC.unit(T))
    text = RC.long_text(T, R)
    t_bytes = GB._texts(c["guides"])
    one = RC.bulge_lists(T, bulges=False)
    one["bulges"] = BC.reference(RC.BULGE_CASE, 0)
    with _native.Engine() as eng:
        GB._locate(eng, G, False, len(text), False)
        eng.upload(0, text)
        eng.guide_bulges_table(t_bytes, M, B, c["pam5"], c["pam3"])
        got = eng.guide_bulges(0)
        long_geometry(eng, "bulged guide hits", blocks=True)
        mine, order = GB._as_hits(got)
        equal_fields(mine, RC.repeated(one["bulges"], R, period), bref.FIELDS, "bulges")
        rows = eng.guide_bulge_windows(G + B)
        assert rows.nbytes > 4 << 20
        assert np.array_equal(rows[order], np.tile(text_rows(bref.ref_windows(T, one["bulges"]), G + B), (R, 1)))

        eng.guide_hits_table(t_bytes, RC.GUIDE_HIT_M, c["pam5"], c["pam3"])
        got = eng.guide_hits(0)
        long_geometry(eng, "guide hits")
        mine, order = GH._as_hits(got)
        equal_fields(mine, RC.repeated(one["guide_hits"], R, period), href.FIELDS, "guide hits")
        rows = eng.guide_hit_windows(G)
        assert np.array_equal(rows[order], np.tile(text_rows(href.ref_windows(T, one["guide_hits"], G), G), (R, 1)))

        eng.near_table(t_bytes[:RC.NEAR_TARGETS], M)
        near = eng.near(0)
        long_geometry(eng, "near")
        assert (np.diff(near["pos"].astype(np.int64)) >= 0).all()
        order = np.lexsort((near["target"], near["strand"], near["pos"]))
        equal_fields(near[order], RC.repeated(one["near"], R, period), ("pos", "strand", "target", "mismatches", "flank_mismatches"),
                     "near")
        assert np.array_equal(eng.near_windows(G)[order], np.tile(ref_windows(T, one["near"], G), (R, 1)))
