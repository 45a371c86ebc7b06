"""The two-genome join (k_join2.inc): one ingroup and one outgroup genome, one diagnostic column, filter on.

The rule of every test: candidates (prefix, in_mask, out_mask) in order and the records of kr_collect are BIT-IDENTICAL between
KR_JOIN2 = 1 and = 0 and equal to oracle/kmer_oracle.c; debug_isect() says whether the route was taken.  The cases are
tests/join2_cases.py's (tests/test_join2_cases.py holds each to the branch it is named for, without a GPU).  A few seconds
per test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join2_cases as J                                                    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


@pytest.fixture(scope="module")
def D():
    from krisp_amd import distributed
    return distributed


@pytest.fixture(autouse=True)
def _one_sort_unit(monkeypatch):
    """the route's geometry is that of ONE sort unit; the switches of the route are each test's own"""
    for v in ("KR_SLICE_BASES", "KR_JOIN2", "KR_JOIN2_GRID", "KR_ISECT_FMT", "KR_ISECT_KERNEL", "KR_FUSE_ANCHOR"):
        monkeypatch.delenv(v, raising=False)


def _run(N, monkeypatch, texts, flags, ldr, join2, grid=None, lanes=None, apply_filter=True, calls=1, mixed=False, step=None):
    """one engine made under KR_JOIN2 = join2 (and KR_JOIN2_GRID) -> dict(cands, recs, isect)"""
    monkeypatch.setenv("KR_JOIN2", str(join2))
    if grid is None:
        monkeypatch.delenv("KR_JOIN2_GRID", raising=False)
    else:
        monkeypatch.setenv("KR_JOIN2_GRID", str(grid))
    ids = list(range(len(texts)))
    out = dict(cands=[], recs=[])
    with N.Engine() as e:
        if lanes is not None:
            e.set_option(N.OPT_LANES, lanes)
        e.set_params(*ldr, max_bases=max(len(t) for t in texts))
        if mixed:
            e.set_mixed_alphabets(True)
        for g, t in zip(ids, texts):
            e.upload(g, t)
        for _ in range(calls):
            if step is not None:
                n, nrec = step(e, ids, flags, 1, apply_filter=apply_filter)
                recs = e.fetch_records(nrec)
            else:
                for g in ids:
                    e.sort(g)
                n = e.intersect(ids, flags, apply_filter=apply_filter)
                recs = e.collect(ids)
            out["cands"].append(e.cands().copy())
            out["recs"].append(np.sort(recs, order=["key", "genome"]))
            assert n == len(out["cands"][-1])
        out["isect"] = e.debug_isect()
        out["info"] = e.debug_info()
    return out


def _ab(N, K, monkeypatch, name, texts, flags, ldr=J.LDR, taken=True, handed_on=None, **kw):
    """KR_JOIN2 = 1 against = 0 and against the oracle -> the run with the route on"""
    calls = kw.get("calls", 1)
    on = _run(N, monkeypatch, texts, flags, ldr, 1, **kw)
    off = _run(N, monkeypatch, texts, flags, ldr, 0, **{k: v for k, v in kw.items() if k != "grid"})
    assert off["isect"]["join2_launches"] == 0 and off["isect"]["join2_handed_on"] == 0
    if kw.get("apply_filter", True) and not kw.get("mixed", False):
        ref = J.census(K, name, texts, flags, ldr)
    else:
        ref = None
    for x, y in zip(on["cands"], off["cands"]):
        assert np.array_equal(x, y), "candidates differ between KR_JOIN2 = 1 and 0"
        if ref is not None:
            assert len(x) == len(ref["cands"])
            for f in ("prefix", "in_mask", "out_mask"):
                assert np.array_equal(x[f], ref["cands"][f]), f
    for x, y in zip(on["recs"], off["recs"]):
        assert np.array_equal(x, y), "records differ between KR_JOIN2 = 1 and 0"
        if ref is not None:
            assert np.array_equal(x, ref["recs"])
    if taken:
        assert on["isect"]["join2_launches"] >= calls and on["isect"]["heads32"] == 1, on["isect"]
    else:
        assert on["isect"]["join2_launches"] == 0, on["isect"]
    if handed_on is not None:
        assert (on["isect"]["join2_handed_on"] > 0) == handed_on, on["isect"]
    return on


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("anchor", [0, 1])
def test_uniform_family(N, K, monkeypatch, masked, anchor):
    """the general path, the anchor the ingroup genome and the outgroup genome, with N runs and soft-masked stretches"""
    texts, flags, _ = J.uniform(71, masked, anchor)
    on = _ab(N, K, monkeypatch, f"uniform {masked} {anchor}", texts, flags, J.UNIFORM_LDR, handed_on=False)
    assert len(on["cands"][0]) > 50


@pytest.mark.parametrize("anchor", [0, 1])
def test_overlap_trap(N, K, monkeypatch, anchor):
    texts, flags, plants = J.trap(anchor)
    on = _ab(N, K, monkeypatch, f"trap {anchor}", texts, flags, handed_on=False)
    c = on["cands"][0]
    for kind, keep in (("overlap", False), ("two_out", True), ("dup", True), ("shared", False)):
        assert all(bool(np.isin(np.uint64(p), c["prefix"])) == keep for p in plants[kind]), kind
    two = c[np.isin(c["prefix"], np.array(plants["two_out"], dtype=np.uint64))]
    assert np.all(two["in_mask"] == 1) and np.all(two["out_mask"] == 0b0110)


def test_screen_collisions(N, K, monkeypatch):
    texts, flags, plants = J.screen_collide()
    on = _ab(N, K, monkeypatch, "screen collide", texts, flags, handed_on=False)
    c = on["cands"][0]["prefix"]
    for kind in J.SCREEN_KINDS:
        for p, q in plants[kind]:
            assert not np.isin(np.uint64(p), c)
            assert bool(np.isin(np.uint64(q), c)) == (kind == "cand_and_shared"), kind


def test_exact_table_collisions(N, K, monkeypatch):
    texts, flags, plants = J.table_collide()
    on = _ab(N, K, monkeypatch, "table collide", texts, flags, handed_on=False)
    c = on["cands"][0]
    for kind in J.TABLE_KINDS:
        for p, q in plants[kind]:
            for x, (im, om) in ((p, (1, 2)), (q, (4, 8))):
                row = c[c["prefix"] == np.uint64(x)]
                assert len(row) == 1 and (int(row["in_mask"][0]), int(row["out_mask"][0])) == (im, om), kind


def test_range_edges_and_more_than_one_batch(N, K, monkeypatch):
    """an item the anchor lacks, one the other genome lacks, one anchor key, the last bucket, and an item where the other genome's
    run takes more than one batch beside three anchor keys"""
    texts, flags, plants = J.edges()
    on = _ab(N, K, monkeypatch, "edges", texts, flags, handed_on=False)
    assert on["isect"]["threads"] == J.PLANT_GEO["T"] and on["isect"]["buckets_per_item_log2"] == J.PLANT_GEO["mlog"]
    assert on["info"]["b"] == J.PLANT_GEO["b"]
    c = on["cands"][0]["prefix"]
    for p in plants["multi"][:J.MULTI_A] + plants["single"] + plants["last"]:
        assert np.isin(np.uint64(p), c)


def test_dense_item_goes_through_the_redo(N, K, monkeypatch):
    texts, flags, plants = J.dense()
    on = _ab(N, K, monkeypatch, "dense", texts, flags, handed_on=False)
    assert on["isect"]["chunk_kernel_items"] >= 1
    assert np.isin(np.array(plants["dense"], dtype=np.uint64), on["cands"][0]["prefix"]).sum() > J.DENSE_BLOCKS * 0.9


@pytest.mark.parametrize("count", [J.ALL_CAND, J.FULL])
def test_every_prefix_of_an_item_survives(N, K, monkeypatch, count):
    """several hundred survivors of one item in order; with more live keys than the exact table holds the item is handed on"""
    texts, flags, plants = J.many_survivors(count)
    on = _ab(N, K, monkeypatch, f"survivors {count}", texts, flags, handed_on=count == J.FULL)
    assert np.isin(np.array(plants["all"], dtype=np.uint64), on["cands"][0]["prefix"]).sum() > count * 0.9


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("case", ["uniform", "screen", "edges"])
def test_few_workgroups_walk_many_items(N, K, monkeypatch, grid, case):
    if case == "uniform":
        texts, flags, _ = J.uniform(71, False, 0)
        _ab(N, K, monkeypatch, "uniform False 0", texts, flags, J.UNIFORM_LDR, grid=grid, handed_on=False)
    elif case == "screen":
        texts, flags, _ = J.screen_collide()
        _ab(N, K, monkeypatch, "screen collide", texts, flags, grid=grid, handed_on=False)
    else:
        texts, flags, _ = J.edges()
        _ab(N, K, monkeypatch, "edges", texts, flags, grid=grid, handed_on=False)


def _family(config, n_in, n_out, length=J.UNIFORM_LEN):
    from krisp_amd import synth
    fam = synth.family(config, n_in, n_out, length, records=J.RECORDS, mu=0.01, snp_every=2000)
    return [t for _, _, t in fam], [f for _, f, _ in fam]


@pytest.mark.parametrize("what", ["three_genomes", "no_filter", "two_columns", "filter_mode_2", "one_side"])
def test_route_not_taken(N, K, monkeypatch, what):
    ldr, kw = J.UNIFORM_LDR, {}
    if what == "three_genomes":
        texts, flags = _family(72, 2, 1)
    elif what == "one_side":
        texts, _ = _family(72, 2, 0)
        flags = [True, True]
    else:
        texts, flags = _family(72, 1, 1)
        if what == "no_filter":
            kw["apply_filter"] = False
        elif what == "two_columns":
            ldr = (20, 2, 5)
        else:
            kw["mixed"] = True
    on = _ab(N, K, monkeypatch, f"not taken {what}", texts, flags, ldr, taken=False, **kw)
    assert on["isect"]["heads32"] == 1           # (the n-way kernel with 32-bit heads took the call: the geometry was the route's)
    if what in ("no_filter", "filter_mode_2"):
        ref = K.intersect([K.sorted_keys(t.tobytes(), *ldr) for t in texts], flags, *ldr,
                          apply_filter=False) if what == "no_filter" else None
        if ref is not None:
            for f in ("prefix", "in_mask", "out_mask"):
                assert np.array_equal(on["cands"][0][f], ref[f])


def test_three_calls_on_one_engine(N, K, monkeypatch):
    texts, flags, _ = J.uniform(71, False, 0)
    on = _ab(N, K, monkeypatch, "uniform False 0", texts, flags, J.UNIFORM_LDR, calls=3, handed_on=False)
    assert np.array_equal(on["cands"][0], on["cands"][2]) and np.array_equal(on["recs"][0], on["recs"][2])


@pytest.mark.parametrize("lanes", [1, 3])
def test_lanes_with_the_sorts_in_flight(N, K, monkeypatch, lanes):
    texts, flags, _ = J.uniform(71, True, 1)
    _ab(N, K, monkeypatch, "uniform True 1", texts, flags, J.UNIFORM_LDR, lanes=lanes, calls=2, handed_on=False)


def test_sharded_step_with_four_genomes(N, K, D, monkeypatch):
    """the coarse route behind the new list: the pillars take k_join2, the other two genomes are probed against its list"""
    texts, flags = _family(73, 2, 2)
    on = _ab(N, K, monkeypatch, "step 2 2", texts, flags, J.UNIFORM_LDR, step=D.sharded_step, calls=2, handed_on=False)
    assert len(on["cands"][0]) > 20
