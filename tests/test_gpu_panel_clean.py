"""--panel-clean on the GPU (kr_panel_sites_*, kr_panel_run_clean, csrc/k_panel_clean.inc): over every set of
panel_clean_cases.py the device's members, running figures, drop counts, fates and drops equal the reference's
(panel_clean_reference.py) field for field, on two runs; the store equals the reference's sites per file, with the record
numbers; an empty store gives kr_panel_run's bytes; kr_panel_run and the multiplex pass keep their bytes beside it; the
library's refusals and states."""
import os
import sys

import numpy as np
import pytest

from krisp_amd import thermo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panel_clean_cases as CC                                             # noqa: E402
import panel_clean_reference as ref                                        # noqa: E402

pytestmark = pytest.mark.gpu

KR_ERR_PARAM, KR_ERR_CAPACITY, KR_ERR_STATE = -2, -3, -4                   # include/krisp_hip.h


def _rows(templates):
    return np.frombuffer("".join(templates).encode("ascii"), dtype=np.uint8).reshape(len(templates), -1)


def _params(max_sec):
    p = thermo.params()
    p.max_sec = max_sec
    return p


def _engine(omit, max_bases):
    from krisp_amd import _native
    eng = _native.Engine()
    eng.set_params_locate(7, 6, 7, omit, max_bases=max(int(max_bases), 1))
    return eng


def _scan_all(eng, c, texts):
    """the table and every file of the set -> the sites per file"""
    eng.panel_sites_table(texts, c["M"], c["max_product"])
    return [(eng.upload(0, np.frombuffer(f, dtype=np.uint8)), eng.panel_sites_scan(0))[1] for f in c["files"]]


def _compare(got, want, what):
    members, fates, drops = got
    wm, wf, wd = want
    assert fates.tolist() == [tuple(f) for f in wf], (what, [(i, a, b) for i, (a, b) in enumerate(zip(fates.tolist(), wf)) if tuple(a) != tuple(b)][:5])
    for field in ("position", "cross_any", "cross_end", "dropped"):
        assert members[field].tolist() == [m[field] for m in wm], (what, field)
    assert drops.tolist() == wd, what


@pytest.mark.parametrize("name", list(CC.SETS))
def test_every_set_equals_the_reference_and_the_store_the_reference_sites(name):
    c = CC.case(name)
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
    texts, trows = ref.table(c["templates"], c["pairs"])
    with _engine(c["omit"], max(len(f) for f in c["files"])) as eng:
        counts = _scan_all(eng, c, texts)
        sites, unit = eng.panel_sites()
        eng.design_table(_params(c["max_sec"]))
        got = eng.panel_clean(rows, pairs, trows, c["size"])
        again = eng.panel_clean(rows, pairs, trows, c["size"])
        sites2, unit2 = eng.panel_sites()
    want_store = ref.store(c["files"], c["omit"], texts, c["M"])
    print(name, "candidates", len(rows), "texts", len(texts), "sites", counts, "members", len(got[0]), "of", c["size"], "fates",
          np.bincount(got[1]["fate"], minlength=6).tolist(), "drops", got[2].tolist())
    # the store: a file's sites in position order, the files in scan order, the units the reference's
    assert counts == [sum(1 for s in want_store if s[0] == fi) for fi in range(len(c["files"]))]
    assert not sites["pad"].any() and sites.tobytes() == sites2.tobytes() and unit.tobytes() == unit2.tobytes()
    at, got_store = 0, []
    for fi, n in enumerate(counts):
        part, u = sites[at:at + n], unit[at:at + n]
        assert (np.diff(part["pos"].astype(np.int64)) >= 0).all()
        got_store += sorted(zip([fi] * n, part["pos"].tolist(), part["entry"].tolist(), part["mismatches"].tolist(),
                                part["end_mismatches"].tolist(), u.tolist()))
        at += n
    assert at == len(sites) and got_store == want_store
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    _compare(got, CC.expected(name), name)


def test_an_empty_store_gives_kr_panel_run_s_bytes_and_kr_panel_run_keeps_its_own():
    """one engine: kr_panel_run; a table without a scan and a clean run; a scan of a file without a site and a clean run;
    the real scans and a clean run; kr_panel_run again"""
    for name in ("random_300", "clash_and_cross", "locus_and_cross"):
        c = CC.case(name)
        rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
        texts, trows = ref.table(c["templates"], c["pairs"])
        with _engine(c["omit"], max(len(f) for f in c["files"])) as eng:
            eng.design_table(_params(c["max_sec"]))
            plain = eng.panel(rows, pairs, c["size"])
            eng.panel_sites_table(texts, c["M"], c["max_product"])
            no_scan = eng.panel_clean(rows, pairs, trows, c["size"])
            eng.upload(0, np.frombuffer(b"N" * 500 + b"\n" + b"N" * 500, dtype=np.uint8))
            assert eng.panel_sites_scan(0) == 0 and len(eng.panel_sites()[0]) == 0
            empty = eng.panel_clean(rows, pairs, trows, c["size"])
            for got in (no_scan, empty):
                assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
                assert got[2].tolist() == [0] * (1 + len(plain[0]))
            _scan_all(eng, c, texts)
            clean = eng.panel_clean(rows, pairs, trows, c["size"])
            _compare(clean, CC.expected(name), name)
            after = eng.panel(rows, pairs, c["size"])
            assert after[0].tobytes() == plain[0].tobytes() and after[1].tobytes() == plain[1].tobytes()
            # (the empty scan's records count: the units of the later scans lie behind them, the verdicts are the same)
            if name == "random_300":
                assert clean[1].tobytes() != plain[1].tobytes()


def test_a_new_table_empties_the_store_and_the_store_survives_growth():
    c = CC.case("next_block")
    texts, _ = ref.table(c["templates"], c["pairs"])
    data = np.frombuffer(c["files"][0], dtype=np.uint8)
    nrec = c["files"][0].count(b"\n") + 1
    with _engine(False, len(data)) as eng:
        eng.panel_sites_table(texts, 0, c["max_product"])
        eng.upload(0, data)
        n = eng.panel_sites_scan(0)
        assert n > 500
        first = eng.panel_sites()
        for _ in range(4):                                                  # the same genome again: the buffers grow twice
            assert eng.panel_sites_scan(0) == n
        sites, unit = eng.panel_sites()
        assert len(sites) == 5 * n
        assert sites[:n].tobytes() == first[0].tobytes() and unit[:n].tobytes() == first[1].tobytes()
        for k in range(1, 5):                                               # the same sites, the units of later records
            again = slice(k * n, (k + 1) * n)
            assert sites[again].tobytes() == first[0].tobytes()
            assert (unit[again].astype(np.int64) - first[1].astype(np.int64) == k * nrec).all()
        eng.panel_sites_table(texts, 0, c["max_product"])
        assert len(eng.panel_sites()[0]) == 0
        assert eng.panel_sites_scan(0) == n and eng.panel_sites()[1].tobytes() == first[1].tobytes()


def test_a_multiplex_table_and_scan_in_the_same_engine_are_untouched():
    c = CC.case("random_65")
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
    texts, trows = ref.table(c["templates"], c["pairs"])
    data = np.frombuffer(c["files"][0], dtype=np.uint8)
    P = ref.product_pairs(c["files"][:1], False, texts, 1, 80)
    some = sorted({texts[x] for ab in P for x in ab})[:128]                 # the texts with a product in the first file
    with _engine(False, 6000) as alone:
        alone.upload(0, data)
        alone.multiplex_table(some, 1, 80)
        want = (alone.multiplex_products(0).tobytes(), alone.multiplex_sites().tobytes(), alone.multiplex_tally().tobytes())
    assert len(want[0]) > 0
    with _engine(False, 6000) as eng:
        eng.upload(0, data)
        eng.multiplex_table(some, 1, 80)
        got = (eng.multiplex_products(0).tobytes(), eng.multiplex_sites().tobytes(), eng.multiplex_tally().tobytes())
        assert got == want
        _scan_all(eng, c, texts)
        eng.design_table(_params(c["max_sec"]))
        _compare(eng.panel_clean(rows, pairs, trows, c["size"]), CC.expected("random_65"), "beside a multiplex table")
        # fetched WITHOUT a new scan: nothing of the multiplex pass was written
        from krisp_amd._native import MULTIPLEX_HIT, _ptr
        n = len(want[0]) // MULTIPLEX_HIT.itemsize
        hits = np.empty(n, dtype=MULTIPLEX_HIT)
        assert eng.lib.kr_multiplex_fetch(eng.ctx, _ptr(hits), n) == n and hits.tobytes() == want[0]
        assert eng.multiplex_sites().tobytes() == want[1] and eng.multiplex_tally().tobytes() == want[2]
        eng.upload(0, data)
        assert (eng.multiplex_products(0).tobytes(), eng.multiplex_sites().tobytes(), eng.multiplex_tally().tobytes()) == want
        assert len(eng.panel_sites()[0]) > 0


def test_the_library_says_what_it_does_not_take():
    from krisp_amd import _native
    from krisp_amd._native import _ptr
    c = CC.case("cross_forward")
    rows, pairs = _rows(c["templates"]), np.array(c["pairs"], dtype=np.uint16)
    texts, trows = ref.table(c["templates"], c["pairs"])
    a, b = b"ACGTACGTAC", b"GGATCCATTGCA"

    def code(call, *args, match):
        with pytest.raises(_native.KrispHipError, match=match) as e:
            call(*args)
        return e.value.code

    with _native.Engine() as eng:                                            # no locate context
        assert code(eng.panel_sites_table, [a], 0, 100, match="kr_set_params_locate first") == KR_ERR_STATE
        eng.design_table(_params(c["max_sec"]))
        assert code(eng.panel_clean, rows, pairs, trows, 3, match="kr_panel_sites_table first") == KR_ERR_STATE
    with _engine(False, len(c["files"][0])) as eng:
        eng.upload(0, np.frombuffer(c["files"][0], dtype=np.uint8))
        assert code(eng.panel_sites_scan, 0, match="kr_panel_sites_table first") == KR_ERR_STATE
        assert code(eng.panel_sites, match="kr_panel_sites_table first") == KR_ERR_STATE
        for bad in (a[:9], a * 6 + b"A"):
            assert code(eng.panel_sites_table, [a, bad], 1, 200, match="10 .. 60 are taken") == KR_ERR_PARAM
        for M in (-1, 4):
            assert code(eng.panel_sites_table, [a, b], M, 200, match="mismatches <= 3") == KR_ERR_PARAM
        assert code(eng.panel_sites_table, [], 1, 200, match="1 .. 16777215 texts") == KR_ERR_PARAM
        assert code(eng.panel_sites_table, [a, b], 1, 23, match="twice the longest text") == KR_ERR_PARAM
        assert code(eng.panel_sites_scan, 0, match="kr_panel_sites_table first") == KR_ERR_STATE      # a refused table is no table
        many = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(i).integers(0, 4, size=12)]) for i in range(200)]
        assert eng.panel_sites_table(many, 1, 200) > 0                          # more than the multiplex pass's 128 texts
        assert eng.panel_sites_table(texts, 0, 24) > 0                          # max_product = twice the longest
        assert code(eng.panel_sites_scan, 5, match="genome 5 not uploaded") == KR_ERR_STATE
        assert code(eng.panel_clean, rows, pairs, trows, 3, match="kr_design_table first") == KR_ERR_STATE
        eng.design_table(_params(c["max_sec"]))
        out = np.zeros(4, dtype=np.uint32)
        assert eng.lib.kr_panel_clean_drops(eng.ctx, _ptr(out), 4) == KR_ERR_STATE                    # no run yet
        # kr_panel_run's checks, under the new name
        assert code(eng.panel_clean, rows, pairs, trows, 0, match="kr_panel_run_clean: a panel of 1 .. 64") == KR_ERR_PARAM
        assert code(eng.panel_clean, rows, pairs, trows, 65, match="a panel of 1 .. 64") == KR_ERR_PARAM
        wide = np.zeros((3, 2048), dtype=np.uint8)
        assert code(eng.panel_clean, wide, pairs, trows, 3, match="a template of 1 .. 2047") == KR_ERR_PARAM
        short = pairs.copy()
        short[1, 1] = 9
        assert code(eng.panel_clean, rows, short, trows, 3, match="candidate 1: a primer of 10 .. 60") == KR_ERR_PARAM
        beyond = np.array(trows, dtype=np.uint32)
        beyond[2, 1] = len(texts)
        assert code(eng.panel_clean, rows, pairs, beyond, 3, match=f"candidate 2 names text {len(texts)}") == KR_ERR_PARAM
        assert eng.lib.kr_panel_fetch(eng.ctx, _ptr(out), 4) == KR_ERR_STATE                            # a refused run is no run
        members, fates, drops = eng.panel_clean(rows, pairs, trows, 3)
        assert len(members) == 3 and drops.tolist() == [0, 0, 0, 0]              # (no scan since the table: an empty store)
        assert eng.lib.kr_panel_clean_drops(eng.ctx, _ptr(out), 3) == KR_ERR_CAPACITY
        members, fates, drops = eng.panel_clean(rows[:0], pairs[:0], np.empty((0, 2), dtype=np.uint32), 3)
        assert len(members) == 0 and len(fates) == 0 and drops.tolist() == [0]
        # the store against the context's budget: the count is named, the earlier content stands
        d = CC.case("next_block")
        dtexts, _ = ref.table(d["templates"], d["pairs"])
        eng.panel_sites_table(dtexts, 0, d["max_product"])
        eng.upload(0, np.frombuffer(d["files"][0], dtype=np.uint8))
        n = eng.panel_sites_scan(0)
        before = eng.panel_sites()
        assert eng.lib.kr_debug_budget_set(eng.ctx, 4096) == 0
        assert code(eng.panel_sites_scan, 0, match=f"a store of {2 * n} primer sites does not fit") == KR_ERR_CAPACITY
        assert eng.lib.kr_debug_budget_set(eng.ctx, 1 << 30) == 0
        sites, unit = eng.panel_sites()
        assert sites.tobytes() == before[0].tobytes() and unit.tobytes() == before[1].tobytes()
    # another soft-mask mode is another context: the table and the store are dropped
    with _engine(False, 1000) as eng:
        eng.panel_sites_table(texts, 0, c["max_product"])
        assert len(eng.panel_sites()[0]) == 0
        eng.set_params_locate(7, 6, 7, True, max_bases=1000)
        assert code(eng.panel_sites, match="kr_panel_sites_table first") == KR_ERR_STATE
