"""Coarse genomes (kr_genome_partition): with the diagnostic filter on, the genomes beside one sorted ingroup
and one sorted outgroup genome stop behind pass 1 and answer the sorted pair's short candidate list (k_coarse_probe).

The rule of every test: candidates (prefix, in_mask, out_mask) in order, records in the order kr_fetch returns them,
count(g) and -- where asked -- keys(g) of a coarse genome (which sorts it fine after all) are BIT-IDENTICAL between
KR_OPT_COARSE_REST = 1 and = 0, and equal to oracle/kmer_oracle.c (coarse_run.py, shared with test_gpu_coarse_shapes.py).
Uniform genomes of 300 kbp: more than 256 fine buckets (b >= 9), about 2 300 keys per top byte -- ONE work unit and one
iteration of the probe's key loop per top byte, fewer units than workgroups, about 1 % of the keys hit.  This file is about
which calls take the route and which promote; the probe's chunks, rounds, seams and overflow branches are
test_gpu_coarse_shapes.py's.  A few seconds per test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coarse_run import _ab, _reference                                      # noqa: E402

pytestmark = pytest.mark.gpu

LEN = 300_000


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


def _family(config, n_in, n_out, length=LEN, **kw):
    from krisp_amd import synth
    kw.setdefault("records", 4)
    kw.setdefault("snp_every", 2000)
    fam = synth.family(config, n_in, n_out, length, **kw)
    return [t for _, _, t in fam], [f for _, f, _ in fam]


@pytest.mark.parametrize("n_in,n_out", [(2, 2), (1, 2), (2, 1), (3, 3)])
def test_sharded_step_with_coarse_rest(N, K, D, n_in, n_out):
    texts, flags = _family(31, n_in, n_out)
    rest = [g for g in range(len(texts)) if g not in (flags.index(True), flags.index(False))]       # (the genomes the step partitions)
    on = _ab(N, K, f"fam31_{n_in}_{n_out}", texts, flags, step=D.sharded_step, coarse_expected=n_in + n_out - 2,
             promoted_expected=0, keys_of=(rest[-1],))
    assert len(on["cands"][0]) > 20                      # (planted sites survive: the comparison is not of empty lists)
    # fetching the keys of a partitioned genome sorted it fine
    assert on["lazy_after_keys"]["coarse_promoted"] == 1


def test_two_genomes_nothing_coarse(N, K, D):
    texts, flags = _family(32, 1, 1)
    _ab(N, K, "fam32_1_1", texts, flags, step=D.sharded_step, coarse_expected=0, promoted_expected=0)


def test_all_ingroup_promotes(N, K):
    texts, _ = _family(33, 3, 0)
    # (no filter can prune one side only: without it the list is every shared prefix -- the usual path's to make)
    on = _ab(N, K, "fam33_all_in", texts, [True] * 3, coarse_ids={2}, coarse_expected=0, promoted_expected=1)
    assert len(on["cands"][0]) > 1000


def test_without_filter_promotes(N, K):
    texts, flags = _family(34, 2, 1)
    _ab(N, K, "fam34_nofilter", texts, flags, coarse_ids={1}, apply_filter=False, coarse_expected=0, promoted_expected=1)


def test_two_diagnostic_columns_promote(N, K):
    texts, flags = _family(35, 2, 2)
    _ab(N, K, "fam35_25_2_2", texts, flags, ldr=(25, 2, 2), coarse_ids={1, 3}, coarse_expected=0, promoted_expected=2)


def test_pillars_of_one_side_promote(N, K):
    """the sorted genomes are both ingroup: their list is not pruned, the coarse outgroup genomes are sorted fine"""
    texts, flags = _family(36, 2, 2)
    _ab(N, K, "fam36_one_sided", texts, flags, coarse_ids={2, 3}, coarse_expected=0, promoted_expected=2)


@pytest.mark.parametrize("omit", [False, True])
def test_masked_input(N, K, D, omit):
    texts, flags = _family(37, 2, 2, n_frac=0.02, lower_frac=0.1)
    _ab(N, K, f"fam37_masked_{omit}", texts, flags, step=D.sharded_step, omit=omit, coarse_expected=2, promoted_expected=0,
        keys_of=(1,))


def _plant(texts, flags, at, unit_in, unit_out, copies, gap):
    out = []
    for t, f in zip(texts, flags):
        t = t.copy()
        u = np.frombuffer(unit_in if f else unit_out, dtype=np.uint8)
        for i in range(copies):
            p = at + i * gap
            t[p:p + len(u)] = u
        out.append(t)
    return out


def test_satellite_overflows_an_arena_row_and_poly_a_crowds_a_bucket(N, K, D):
    """a 28-mer that differs in its diagnostic base between the sides, 20 copies per genome: its candidate survives and a coarse
    genome holds 20 keys under it -- more than an arena row (8): kr_collect sorts the genomes whole.  A poly-A block fills
    top byte 0 with equal keys (no candidate: both sides hold them)."""
    texts, flags = _family(38, 2, 2)
    left, right = b"ACGTTGCAAGCTTAGGCATCGATCA", b"GT"
    texts = _plant(texts, flags, 10_000, left + b"A" + right + b"CCTGACTG", left + b"C" + right + b"CCTGACTG", 20, 36)
    for t in texts:
        t[40_000:46_000] = ord("A")
    on = _ab(N, K, "fam38_satellite", texts, flags, step=D.sharded_step, coarse_expected=2)
    assert on["lazy"]["coarse_promoted"] == 2            # (the collect's overflow route)
    assert max(on["recs"][0]["count"]) >= 20


def test_identical_genomes_leave_no_candidate(N, K, D):
    texts, _ = _family(39, 1, 0)
    texts, flags = [texts[0]] * 4, [True, True, False, False]
    on = _ab(N, K, "fam39_identical", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)
    assert len(on["cands"][0]) == 0 and len(on["recs"][0]) == 0


def test_small_mu_nearly_every_prefix_shared(N, K, D):
    texts, flags = _family(40, 2, 2, mu=0.0002)
    _ab(N, K, "fam40_small_mu", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)


def test_tiny_table_takes_rounds(N, K, D, monkeypatch):
    """KR_COARSE_TCAP (test knob): 5 candidates per table, so a top byte's candidates take several rounds over its keys"""
    monkeypatch.setenv("KR_COARSE_TCAP", "5")
    texts, flags = _family(31, 2, 2)
    _ab(N, K, "fam31_2_2", texts, flags, step=D.sharded_step, coarse_expected=2, promoted_expected=0)


def test_tiny_hit_list_overflows_into_promotion(N, K, D, monkeypatch):
    """KR_COARSE_HITCAP (test knob): a hit list of 16 keys overflows; nothing is truncated -- the genomes are sorted fine and the
    call runs over all of them"""
    monkeypatch.setenv("KR_COARSE_HITCAP", "16")
    texts, flags = _family(31, 2, 2)
    _ab(N, K, "fam31_2_2", texts, flags, step=D.sharded_step, coarse_expected=0, promoted_expected=2)


@pytest.mark.parametrize("lanes", [1, 3])
def test_lanes(N, K, D, lanes):
    texts, flags = _family(31, 2, 2)
    _ab(N, K, "fam31_2_2", texts, flags, step=D.sharded_step, lanes=lanes, coarse_expected=2, promoted_expected=0)


def test_two_steps_on_one_engine(N, K, D):
    texts, flags = _family(31, 3, 3)
    on = _ab(N, K, "fam31_3_3", texts, flags, step=D.sharded_step, steps=2, coarse_expected=8, promoted_expected=0)
    assert np.array_equal(on["cands"][0], on["cands"][1]) and np.array_equal(on["recs"][0], on["recs"][1])


def test_a_coarse_genome_uploaded_again_and_sorted(N, K):
    texts, flags = _family(31, 2, 2)
    other, _ = _family(41, 2, 2)
    keys, cands, recs = _reference(K, "fam31_with_41", texts[:3] + [other[3]], flags, (25, 1, 2))
    for rest in (1, 0):
        with N.Engine() as e:
            e.set_option(N.OPT_COARSE_REST, rest)
            e.set_params(25, 1, 2, max_bases=LEN + 16)
            for g, t in enumerate(texts):
                e.upload(g, t)
            e.sort(0)
            e.partition(1)
            e.sort(2)
            e.partition(3)
            e.upload(3, other[3])
            e.sort(3)
            assert e.intersect([0, 1, 2, 3], flags) == len(cands)
            got = e.cands()
            for f in ("prefix", "in_mask", "out_mask"):
                assert np.array_equal(got[f], cands[f])
            assert np.array_equal(np.sort(e.collect([0, 1, 2, 3]), order=["key", "genome"]), recs)
            assert [e.count(g) for g in range(4)] == [len(k) for k in keys]
            lazy = e.debug_lazy()
            assert (lazy["coarse"], lazy["coarse_promoted"]) == ((1, 0) if rest else (0, 0))


def test_collect_of_a_loaded_list_sorts_the_coarse_genomes(N, K):
    """a candidate list from outside (kr_cands_load) is not the one the hit lists were made for"""
    texts, flags = _family(31, 2, 2)
    keys, cands, recs = _reference(K, "fam31_2_2", texts, flags, (25, 1, 2))
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=LEN + 16)
        for g, t in enumerate(texts):
            e.upload(g, t)
            (e.partition if g in (1, 3) else e.sort)(g)
        assert e.intersect([0, 1, 2, 3], flags) == len(cands)
        e.load_cands(e.cands())
        assert np.array_equal(np.sort(e.collect([0, 1, 2, 3]), order=["key", "genome"]), recs)
        assert e.debug_lazy()["coarse_promoted"] == 2
