"""Every route of the genome sort (csrc/h_core.inc: genome_sort, order_genome, finalize) at the smallest shape that reaches
it: the fetched keys equal oracle/kmer_oracle.c's, and the sort's LAUNCH PLAN -- kr_stage_launches of every stage -- equals
PLAN below.

PLAN was recorded once, with these shapes, on the commit BEFORE the sort's host path was cut into named passes, and is
kept as literals: it is that commit's plan, not something the code under test computes.  A route that loses or gains a
launch, or moves one to another stage, fails here by name.  Per case the counts are read twice: behind the sort(s) --
genome_sort's own launches -- and behind the fetch, whose difference is what order_genome and finalize added (under
KR_OPT_LAZY_ORDER, the default, the LDS sort shows up only there).  Stages that did not run are left out of a row: a
row is compared against the non-zero counts of ALL stages.

The premises of a route (the fan-out above 2^8, the slice count, an oversized bucket, what the coarse pool did) are
asserted too, so that a changed constant shows up as a failed premise and not as a wrong table.  The wide path's
genome_sort(..., reuse_count = true) runs under every kr_wide_run -- tests/test_gpu_kernels.py's
test_wide_composite_keys_as_lists_change_nothing among others -- and is not repeated here; the retreat to one lane needs
an allocation failure and is not run.  A case takes a second or two."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coarse_run import _oracle, _reference                                 # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABET = b"ACGT" * 12 + b"acgtN"          # N runs and soft-masked bases, as test_gpu_kernels' random genomes
N_BASES = 300_000                           # 2 n / 256 > BUCKET_AVG: the fan-out is above 2^8


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(scope="module")
def K():
    from oracle import kmer_oracle
    kmer_oracle.build()
    return kmer_oracle


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("KR_SLICE_ROUTE", "KR_LANES", "KR_LAZY_ORDER", "KR_SLICE_BASES", "KR_COARSE_POOL", "KR_COARSE_REST",
                 "KR_PLACE_TRIES", "KR_PLACE_MIN_BYTES", "KR_P1_FAST", "KR_LAZY_WIDE"):
        monkeypatch.delenv(name, raising=False)


def _rand_text(seed, n, alphabet=ALPHABET, records=5):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    t = a[rng.integers(0, len(a), size=n)]
    for p in rng.integers(0, n, size=records - 1):
        t[p] = 10
    return t


def _satellite_text():
    """test_gpu_kernels' oversized-bucket genome, shorter: a run of one base and a short tandem repeat"""
    return np.concatenate([_rand_text(9, 200_000, b"ACGT", records=4), np.frombuffer(b"A" * 60_000, dtype=np.uint8),
                           _rand_text(11, 50_000, b"ACGT", records=1), np.frombuffer(b"ACACACACAC" * 3000, dtype=np.uint8)])


def forward_keys(text, k):
    """the forward strand's keys of windows of k bases with L = k, D = R = 0 (2 bits a base from the top of the word,
    A C G T = 0 1 2 3, lower case as upper), and their reverse complements' -- sorted; together they are the oracle's"""
    code = np.full(256, 4, dtype=np.uint64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = i
    c = code[text]
    ok = np.convolve((c < 4).astype(np.int64), np.ones(k, dtype=np.int64), "valid") == k
    fwd = np.zeros(len(c) - k + 1, dtype=np.uint64)
    rc = np.zeros(len(c) - k + 1, dtype=np.uint64)
    for j in range(k):
        cj = c[j:len(c) - k + 1 + j] & np.uint64(3)
        fwd |= cj << np.uint64(62 - 2 * j)
        rc |= (np.uint64(3) - cj) << np.uint64(62 - 2 * (k - 1 - j))
    return np.sort(fwd[ok]), np.sort(rc[ok])


def _launches(e, since=None):
    """the non-zero launch counts of all stages (less those of `since`)"""
    now = {name: n for name, (_, n) in e.stage_times().items()}
    if since is not None:
        now = {name: n - since.get(name, 0) for name, n in now.items()}
    assert all(n >= 0 for n in now.values())
    return {name: n for name, n in now.items() if n}


def _sort_case(N, texts, want, ldr, options=(), strands=None, sorts=None):
    """one engine: options, upload, stage_reset, the sorts -> counts; the keys of every genome against `want` -> counts"""
    with N.Engine() as e:
        for opt, value in options:
            e.set_option(opt, value)
        e.set_params(*ldr, max_bases=max(len(t) for t in texts))
        if strands is not None:
            e.set_strands(strands)
        for g, t in enumerate(texts):
            e.upload(g, t)
        e.stage_reset()
        for g in (range(len(texts)) if sorts is None else sorts):
            e.sort(g)
        behind_sort = _launches(e)
        full = {name: n for name, (_, n) in e.stage_times().items()}
        for g in range(len(texts)):
            assert np.array_equal(e.keys(g), want[g]), f"sorted keys of genome {g}"
        return dict(sort=behind_sort, fetch=_launches(e, since=full)), e.debug_info()


# ---- the parent commit's launch plan (see the module's docstring)
PLAN = {
    "b8": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "chunks": 1},
        "fetch": {"localsort": 1},
    },
    "fine16": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1},
        "fetch": {"localsort": 1},
    },
    "hist2": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1},
        "fetch": {"localsort": 1},
    },
    "forward": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1, "localsort": 1},
        "fetch": {},
    },
    "eager": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1, "localsort": 1},
        "fetch": {},
    },
    "sliced2_route1": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 17, "scatter1": 17, "hist2": 1, "scan2": 1, "chunks": 16},
        "fetch": {"localsort": 16},
    },
    "sliced2_route0": {
        "sort": {"pack": 1, "hist8": 17, "reduce8": 17, "scatter1": 17, "chunks": 16},
        "fetch": {"localsort": 16},
    },
    "sliced3_lanes4": {
        "sort": {"pack": 3, "hist8": 3, "reduce8": 195, "scatter1": 195, "hist2": 3, "scan2": 3, "chunks": 192},
        "fetch": {"localsort": 128},
    },
    "sliced3_lanes1": {
        "sort": {"pack": 3, "hist8": 3, "reduce8": 195, "scatter1": 195, "hist2": 3, "scan2": 3, "chunks": 192},
        "fetch": {"localsort": 128},
    },
    "sliced3_short_left": {
        "sort": {"pack": 1, "hist8": 65, "reduce8": 65, "scatter1": 65, "chunks": 64},
        "fetch": {"localsort": 64},
    },
    "fallback": {
        "sort": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1},
        "fetch": {"localsort": 1, "fallback": 1},
    },
    "coarse_pool1": {
        "partitions": [
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
        ],
        "count": {},
        "keys": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1, "localsort": 1},
    },
    "coarse_pool0": {
        "partitions": [
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
            {"pack": 2, "hist8": 2, "reduce8": 4, "scatter1": 2},
        ],
        "count": {},
        "keys": {"pack": 1, "hist8": 1, "reduce8": 1, "scatter1": 1, "hist2": 1, "scan2": 1, "scatter2": 1, "chunks": 1, "localsort": 1},
    },
}


def _expect(name, got):
    assert got == PLAN[name], (name, got)


def test_one_unit_fanout_256_pass_2_is_the_copy(N, K):
    text = _rand_text(21, 40_000)
    got, info = _sort_case(N, [text], [K.sorted_keys(text.tobytes(), 25, 1, 2)], (25, 1, 2))
    assert info["b"] == 8 and info["nslices"] == 1
    _expect("b8", got)


_FINE = {}


def _fine_text(K):
    if not _FINE:
        text = _rand_text(22, N_BASES)
        _FINE["text"] = text
        for ldr in ((25, 1, 2), (3, 1, 2), (5, 1, 2)):
            _FINE[ldr] = K.sorted_keys(text.tobytes(), *ldr)
            _FINE[ldr].setflags(write=False)
        text.setflags(write=False)
    return _FINE


def test_one_unit_fine_offsets_from_the_codes(N, K):
    ref = _fine_text(K)
    got, info = _sort_case(N, [ref["text"]], [ref[(25, 1, 2)]], (25, 1, 2))
    assert info["b"] > 8 and info["nslices"] == 1 and info["overflow_segments"] == 0
    _expect("fine16", got)


def test_one_unit_fine_offsets_from_the_keys(N, K):
    """2 L < b: k_hist2 / k_scan2 on the pass-1 output"""
    ref = _fine_text(K)
    got, info = _sort_case(N, [ref["text"]], [ref[(3, 1, 2)]], (3, 1, 2))
    assert info["b"] > 8 and 2 * 3 < info["b"] and info["nslices"] == 1
    _expect("hist2", got)


def test_one_unit_single_strand(N, K):
    """forward keys only: no k_hist16, and the sort ends with the LDS sort whatever KR_OPT_LAZY_ORDER says"""
    ref = _fine_text(K)
    fwd, rc = forward_keys(ref["text"], 20)
    assert np.array_equal(np.sort(np.concatenate([fwd, rc])), K.sorted_keys(ref["text"].tobytes(), 20, 0, 0))
    got, info = _sort_case(N, [ref["text"]], [fwd], (20, 0, 0), strands=N.STRANDS_FORWARD)
    assert info["b"] > 8 and info["nslices"] == 1
    _expect("forward", got)


def test_eager_order(N, K):
    """KR_OPT_LAZY_ORDER = 0: the LDS sort is among the sort's own launches"""
    ref = _fine_text(K)
    got, info = _sort_case(N, [ref["text"]], [ref[(25, 1, 2)]], (25, 1, 2), options=[(N.OPT_LAZY_ORDER, 0)])
    assert info["b"] > 8
    assert got["sort"].get("localsort") == 1 and "localsort" not in got["fetch"]
    _expect("eager", got)


@pytest.mark.parametrize("route", [1, 0])
def test_sliced_16_slices(N, K, route, monkeypatch):
    """route 1: every slice's pass 1 is a k_scatter2 over its pass-0 buckets; KR_SLICE_ROUTE=0: the slices count again"""
    monkeypatch.setenv("KR_SLICE_ROUTE", str(route))
    ref = _fine_text(K)
    got, info = _sort_case(N, [ref["text"]], [ref[(25, 1, 2)]], (25, 1, 2), options=[(N.OPT_SLICE_BASES, 2)])
    assert info["nslices"] == 16
    _expect(f"sliced2_route{route}", got)


@pytest.mark.parametrize("lanes", [4, 1])
def test_sliced_64_slices_on_helper_lanes_or_one_lane(N, K, lanes):
    """two genomes and the first one again: with lanes the second genome lane makes its own pass-0 array, the slices take
    turns on the helper lanes, and the third sort waits for the helpers of the first"""
    ref = _fine_text(K)
    other = _rand_text(23, N_BASES - 12_345)
    want = [ref[(25, 1, 2)], K.sorted_keys(other.tobytes(), 25, 1, 2)]
    got, info = _sort_case(N, [ref["text"], other], want, (25, 1, 2),
                           options=[(N.OPT_SLICE_BASES, 3), (N.OPT_LANES, lanes)], sorts=[0, 1, 0])
    assert info["nslices"] == 64
    _expect(f"sliced3_lanes{lanes}", got)


def test_sliced_top_bits_beyond_left_count_again(N, K):
    """L = 5 at 3 slice bases: 8 + 6 top bits do not fit 2 L, the counted route without the switch"""
    ref = _fine_text(K)
    got, info = _sort_case(N, [ref["text"]], [ref[(5, 1, 2)]], (5, 1, 2), options=[(N.OPT_SLICE_BASES, 3)])
    assert info["nslices"] == 64
    _expect("sliced3_short_left", got)


def test_merge_fallback(N, K):
    text = _satellite_text()
    got, info = _sort_case(N, [text], [K.sorted_keys(text.tobytes(), 25, 1, 2)], (25, 1, 2))
    assert info["overflow_segments"] >= 1 and info["fallback_launches"] > 0
    _expect("fallback", got)


@pytest.mark.parametrize("pool", [1, 0])
def test_coarse_partitions_with_and_without_the_pool(N, K, pool, monkeypatch):
    """two sorted genomes, two partitioned ones, three steps (the pool grows behind the second step's intersection, the
    third step's partitions take its buffers), then a coarse genome's count, and its fine sort, which returns the buffer"""
    monkeypatch.setenv("KR_PLACE_MIN_BYTES", "0")
    monkeypatch.setenv("KR_PLACE_TRIES", "2")
    from krisp_amd import synth
    fam = synth.family(31, 2, 2, N_BASES, records=4, snp_every=2000)
    texts, flags = [t for _, _, t in fam], [f for _, f, _ in fam]
    ldr = (25, 1, 2)
    ref = _reference(K, "routes_fam31_2_2", texts, flags, ldr)
    ids = list(range(4))
    pillars = {flags.index(True), flags.index(False)}
    coarse = [g for g in ids if g not in pillars]
    got = {"partitions": [], "cands": [], "recs": []}
    with N.Engine() as e:
        e.set_option(N.OPT_COARSE_POOL, pool)
        e.set_params(*ldr, max_bases=max(len(t) for t in texts))
        for g in ids:
            e.upload(g, texts[g])
        assert e.debug_info()["b"] > 8
        for g in pillars:
            e.sort(g)
        for _ in range(3):
            e.stage_reset()
            for g in coarse:
                e.partition(g)
            got["partitions"].append(_launches(e))
            n = e.intersect(ids, flags, apply_filter=True)
            got["cands"].append(e.cands().copy())
            got["recs"].append(e.collect(ids).copy())
            assert n == len(got["cands"][-1])
        lazy = e.debug_lazy()
        assert lazy["coarse"] == 3 * len(coarse) and lazy["coarse_promoted"] == 0, lazy
        p = e.debug_coarse_pool()
        assert (p["total"], p["held"], p["partitions"]) == ((2, 2, 2) if pool else (0, 0, 0)), p
        e.stage_reset()
        got["counts"] = [e.count(g) for g in ids]
        behind_count = _launches(e)
        assert e.debug_lazy()["coarse_promoted"] == 0
        got["keys"] = {coarse[0]: e.keys(coarse[0])}
        behind_keys = _launches(e, since=behind_count)
        assert e.debug_lazy()["coarse_promoted"] == 1
        p = e.debug_coarse_pool()
        assert (p["total"], p["free"], p["held"]) == ((2, 1, 1) if pool else (0, 0, 0)), p
    _oracle(got, ref)
    assert len(got["cands"][0]) > 20
    _expect(f"coarse_pool{pool}", dict(partitions=got["partitions"], count=behind_count, keys=behind_keys))
