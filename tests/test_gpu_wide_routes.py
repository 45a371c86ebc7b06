"""Every route of kr_wide_run (csrc/h_wide.inc) at the smallest shape that reaches it: the run's FINGERPRINT equals FP
below.

FP was recorded once, with these shapes, on the commit BEFORE the wide host path was cut into named passes, and is kept
as literals: it is that commit's behaviour, not something the code under test computes.  A fingerprint is the return
value of wide_run, WIDE_NGROUPS, WIDE_COUNTS, the seven WIDE_SLOT_BITS, WIDE_BATCH_USED, WIDE_KEYS_LISTED, WIDE_LOCATED,
the sizes of WIDE_DICT_LEFT / WIDE_DICT_RIGHT / WIDE_GROUPS, the non-zero kr_stage_launches of ALL stages for the run
(they count the sorts, the intersections and the locate launches of a route) and a SHA-256 of the hits sorted by
(cand, genome, pos, strand).  A route that loses or gains a launch, takes another dictionary form or another memory
decision fails here by name.

The premises of a route (a key list was kept, the dense form ran, the run went in batches ...) are asserted too, so that a
changed constant shows up as a failed premise and not as a wrong table.  The `slots` and `genome_cache` decisions read
the device's free memory; at these sizes the margin is about a thousandfold.

Not reached at these sizes, and reviewed by reading instead: wide_make_room and the three-step give-back in front of the
locate pass (both need a nearly full device); the exchange of masks and the gather of hits over ranks run in
tests/test_gpu_cli.py's multi-rank tests.  Nor is count_slices' KR_RETRY_DENSE: KR_WIDE_KEYFRAC=0.0000001 leaves every
segment of a key list its floor of 256 entries, and a workgroup of k_hist8w (one of 2048) sees 96 window starts of
these genomes, 160 of the longer family's -- the lists hold, as the recorded WIDE_KEYS_LISTED says; a segment too short
needs genomes of more than half a million bases that are nearly alike.

BUDGET is the smallest of the budgets 2^30, 2^29 ... bytes under which that commit still completed the capacity-retry
case, and it did so in batches (64 MiB: all at once; 16 MiB: KR_ERR_CAPACITY).  The same run again in one context has,
on that commit too, one compaction less and one LDS sort more than a first run (AGAIN_LAUNCHES); everything else is
equal.  A case takes a second or two."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ENVS = ("KR_WIDE_SHARE", "KR_WIDE_SPECTRUM", "KR_WIDE_ORDERED", "KR_WIDE_SLOTS", "KR_WIDE_CANON", "KR_WIDE_KEYFRAC",
        "KR_WIDE_KEYLIST", "KR_WIDE_CACHE", "KR_WIDE_LOCLIST", "KR_WIDE_LOCCAP", "KR_WIDE_BATCH", "KR_SLICE_BASES", "KR_LANES")

BUDGET = 32 << 20       # (see the docstring; the next halving fails on the recording commit)

# name -> family, (L, D, R), environment, options (by name, of krisp_amd._native), apply_filter, hbm_budget
CASES = {
    "shared_minimizer":  dict(fam="A", geo=(32, 20, 32)),
    "short_index_slots": dict(fam="A", geo=(12, 30, 12)),
    "two_spectra":       dict(fam="A", geo=(20, 17, 9)),
    "two_pieces":        dict(fam="A", geo=(40, 12, 36)),
    "ordered":           dict(fam="A", geo=(32, 20, 32), options=[("OPT_WIDE_ORDERED", 1)]),
    "no_slots":          dict(fam="A", geo=(32, 20, 32), options=[("OPT_WIDE_SLOTS", 0)]),
    "no_share":          dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_SHARE": "0"}),
    "window_spectrum":   dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_SPECTRUM": "0"}),
    "key_lists":         dict(fam="B", geo=(32, 20, 32), env={"KR_WIDE_KEYFRAC": "0.12"}),
    "key_lists_short":   dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_KEYFRAC": "0.0000001"}),
    "members_dense":     dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_LOCLIST": "0"}),
    "members_overflow":  dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_LOCCAP": "7"}),
    "one_cache":         dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_CACHE": "0"}),
    "one_cache_dense":   dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_CACHE": "0", "KR_WIDE_LOCLIST": "0"}),
    "batch_1":           dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_BATCH": "1"}),
    "batch_2":           dict(fam="A", geo=(32, 20, 32), env={"KR_WIDE_BATCH": "2"}),
    "capacity_retry":    dict(fam="A", geo=(32, 20, 32), budget=BUDGET),
    "unfiltered":        dict(fam="A", geo=(32, 20, 32), filt=False),
    "empty":             dict(fam="U", geo=(32, 20, 32)),
}

_FAM = {}


def family(which):
    """A: test_gpu_kernels' _family(94, 4, 150_000) with its planted repeat and N runs; B: its sparse family (95) with its
    repeat; U: two unrelated random genomes.  Made once, read-only."""
    if which not in _FAM:
        from krisp_amd import synth
        if which == "A":
            fam = synth.family(94, 2, 2, 150_000, records=4, mu=0.01, snp_every=2000)
            rng = np.random.default_rng(11)
            texts = []
            for _, _, t in fam:
                t = t.copy()
                t[60_000:60_400] = t[20_000:20_400]
                for p in rng.integers(0, len(t) - 50, size=10):
                    t[p:p + int(rng.integers(1, 20))] = ord("N")
                texts.append(t)
            flags = [f for _, f, _ in fam]
        elif which == "B":
            fam = synth.family(95, 2, 2, 300_000, records=4, mu=0.03, snp_every=150)
            texts = []
            for _, _, t in fam:
                t = t.copy()
                t[70_000:70_300] = t[30_000:30_300]
                texts.append(t)
            flags = [f for _, f, _ in fam]
        else:
            acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
            texts = [acgt[np.random.default_rng(s).integers(0, 4, size=150_000)] for s in (96, 97)]
            flags = [True, False]
        for t in texts:
            t.setflags(write=False)
        _FAM[which] = (texts, flags)
    return _FAM[which]


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)


def _launches(e):
    """the non-zero launch counts of all stages"""
    return {name: n for name, (_, n) in e.stage_times().items() if n}


def fingerprint(N, e, ids, flags, filt):
    e.stage_reset()
    n = e.wide_run(ids, flags, apply_filter=filt)
    launches = _launches(e)
    hits = e.wide_fetch(N.WIDE_HITS)
    hits = hits[np.lexsort((hits["strand"], hits["pos"], hits["genome"], hits["cand"]))]
    one = lambda what: int(e.wide_fetch(what)[0])                       # noqa: E731
    return dict(n=int(n), ngroups=one(N.WIDE_NGROUPS), counts=[int(x) for x in e.wide_fetch(N.WIDE_COUNTS)],
                slot_bits=[int(x) for x in e.wide_fetch(N.WIDE_SLOT_BITS)], batch_used=one(N.WIDE_BATCH_USED),
                keys_listed=one(N.WIDE_KEYS_LISTED), located=one(N.WIDE_LOCATED), left=int(e.wide_count(N.WIDE_DICT_LEFT)),
                right=int(e.wide_count(N.WIDE_DICT_RIGHT)), groups=int(e.wide_count(N.WIDE_GROUPS)), launches=launches,
                hits=hashlib.sha256(np.ascontiguousarray(hits).tobytes()).hexdigest())


def load(N, e, name):
    """the case's options and geometry, its genomes up: -> ids, flags, apply_filter"""
    case = CASES[name]
    texts, flags = family(case["fam"])
    for opt, value in case.get("options", ()):
        e.set_option(getattr(N, opt), value)
    e.set_params_wide(*case["geo"], max_bases=max(len(t) for t in texts))
    for g, t in enumerate(texts):
        e.upload(g, t)
    return list(range(len(texts))), flags, case.get("filt", True)


def run_case(N, name, setenv, runs=1):
    """a fresh context under the case's environment: the fingerprints of `runs` runs"""
    case = CASES[name]
    for k, v in case.get("env", {}).items():
        setenv(k, v)
    with N.Engine(hbm_budget=case.get("budget", 0)) as e:
        ids, flags, filt = load(N, e, name)
        return [fingerprint(N, e, ids, flags, filt) for _ in range(runs)]


# ---- the recording commit's fingerprints (see the module's docstring)
FP = {
    "shared_minimizer": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "short_index_slots": dict(
        n=9296, ngroups=111090, counts=[298280, 298276, 298250, 298322], slot_bits=[16, 0, 0, 254, 254, 254, 16],
        batch_used=0, keys_listed=0, located=222852, left=182384, right=182384, groups=55545,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="f770ba55778b90d5d7208f1b3b37344780789c4f15e20d51a400256827f5b70d"),
    "two_spectra": dict(
        n=4340, ngroups=90698, counts=[298504, 298500, 298474, 298546], slot_bits=[255, 0, 0, 17, 0, 0, 16],
        batch_used=0, keys_listed=0, located=364171, left=131852, right=149878, groups=90698,
        launches={"hist8": 12, "reduce8": 12, "scatter1": 12, "chunks": 12, "localsort": 5, "intersect": 4, "compact": 7,
                  "locate": 4},
        hits="77bfcd4a2e3aedc2964cc261173c19c55860f9e4167c75afeb204bd1c8250bbe"),
    "two_pieces": dict(
        n=328, ngroups=12741, counts=[297328, 297324, 297298, 297370], slot_bits=[255, 255, 16, 17, 17, 16, 14],
        batch_used=0, keys_listed=0, located=51650, left=56748, right=66967, groups=12741,
        launches={"hist8": 28, "reduce8": 28, "scatter1": 28, "chunks": 28, "localsort": 10, "intersect": 9, "compact": 12,
                  "locate": 4},
        hits="3139caa02db1029ad9be266f1d57177e1a977d9c6fbbbd96f42f5ab2d82b58a7"),
    "ordered": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[0, 0, 0, 0, 0, 0, 14],
        batch_used=0, keys_listed=0, located=84566, left=80040, right=80040, groups=20962,
        launches={"hist8": 12, "reduce8": 12, "scatter1": 12, "chunks": 12, "localsort": 6, "intersect": 4, "compact": 6,
                  "locate": 4},
        hits="3b2582dc78a626e239187b66e3e39ee5fcfbb05ef4d152f23497ba1745bb4d1d"),
    "no_slots": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 0],
        batch_used=0, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "no_share": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 255, 0, 0, 14],
        batch_used=0, keys_listed=0, located=84566, left=80040, right=80040, groups=20962,
        launches={"hist8": 12, "reduce8": 12, "scatter1": 12, "chunks": 12, "localsort": 6, "intersect": 4, "compact": 6,
                  "locate": 4},
        hits="b3cd3089134de76ddf9cdcd430f87af1110eeea20cefceca98c96e8a8146b77b"),
    "window_spectrum": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=42283, left=78996, right=78996, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="62b087d88c75e3de2a870951b010af9f6981cec5e0212dcdd255c8bc63b16887"),
    "key_lists": dict(
        n=208, ngroups=180, counts=[599336, 599336, 599336, 599336], slot_bits=[255, 0, 0, 254, 254, 254, 6],
        batch_used=0, keys_listed=360, located=360, left=10382, right=10382, groups=90,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "hist2": 8, "scan2": 8, "scatter2": 8, "chunks": 8,
                  "localsort": 2, "intersect": 2, "compact": 3, "locate": 4},
        hits="22310a0e8d75334ff2f20fbe2fe3d9c8a11af72d2066c5966cce64da7fbeaeed"),
    "key_lists_short": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=42364, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "members_dense": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=0, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "members_overflow": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=0, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 8},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "one_cache": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "one_cache_dense": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=0, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "batch_1": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=1, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 8, "intersect": 2, "compact": 4,
                  "merge": 6, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "batch_2": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=2, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 7, "intersect": 3, "compact": 5,
                  "merge": 2, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "capacity_retry": dict(
        n=1152, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=2, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 16, "reduce8": 16, "scatter1": 16, "chunks": 16, "localsort": 12, "intersect": 6, "compact": 10,
                  "merge": 2, "locate": 4},
        hits="5205de469d5947aa5ddab34dae29a2576ebf93b93ef675795f9713b914f49c76"),
    "unfiltered": dict(
        n=84566, ngroups=20962, counts=[297440, 297436, 297410, 297482], slot_bits=[255, 0, 0, 254, 254, 254, 13],
        batch_used=0, keys_listed=0, located=42283, left=80040, right=80040, groups=10481,
        launches={"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 5, "intersect": 3, "compact": 5, "locate": 4},
        hits="2f140611d0a35e5279d0530a169e72dbc7fb74a7e055d9ca105e25cc3960c494"),
    "empty": dict(
        n=0, ngroups=0, counts=[299834, 299834], slot_bits=[0, 0, 0, 254, 254, 254, 0],
        batch_used=0, keys_listed=0, located=0, left=0, right=0, groups=0,
        launches={"hist8": 2, "reduce8": 2, "scatter1": 2, "chunks": 2, "localsort": 1, "intersect": 1, "compact": 1},
        hits="e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"),
}


# WIDE_SLOT_BITS: the dictionary took the minimizer form; it was never built (it mirrors the left one)
MINIMIZER, SHARED = 255, 254


def _premises(name, fp):
    bits = fp["slot_bits"]
    if name != "empty":
        assert fp["n"] > 0 and fp["groups"] > 0 and fp["left"] > 0 and fp["right"] > 0
    if name in ("shared_minimizer", "unfiltered"):
        assert bits[0] == MINIMIZER and bits[3] == SHARED and bits[6] > 0
        assert fp["located"] > 0 and fp["keys_listed"] == 0 and fp["batch_used"] == 0
        assert fp["ngroups"] > fp["groups"]                  # (one group of every mirror pair is listed)
    if name == "short_index_slots":
        assert bits[0] not in (0, MINIMIZER) and bits[3] == SHARED
    if name == "two_spectra":
        assert SHARED not in bits and bits[3] != MINIMIZER and fp["ngroups"] == fp["groups"]
    if name == "two_pieces":             # (a piece's own dictionary and the combinations, for both flanks)
        assert bits[3] != SHARED and 0 not in bits[:6]
    if name == "ordered":
        assert MINIMIZER not in bits and SHARED not in bits
    if name == "no_slots":
        assert bits[6] == 0 and bits[0] == MINIMIZER
    if name == "no_share":
        assert bits[3] == MINIMIZER
    if name == "key_lists":
        assert fp["keys_listed"] > 0
    if name == "key_lists_short":        # (segments of the floor of 256 entries: see the docstring)
        assert fp["keys_listed"] > 0
    if name in ("members_dense", "members_overflow", "one_cache_dense"):
        assert fp["located"] == 0
    if name == "one_cache":
        assert fp["located"] > 0
    if name == "members_overflow":
        assert fp["launches"]["locate"] == 2 * FP["shared_minimizer"]["launches"]["locate"]
    if name in ("batch_1", "batch_2"):
        assert fp["batch_used"] == int(name[-1])
    if name == "capacity_retry":
        assert fp["batch_used"] > 0
    if name == "empty":
        assert fp["n"] == 0 and fp["left"] == fp["right"] == fp["groups"] == 0 and "locate" not in fp["launches"]


@pytest.mark.parametrize("name", list(CASES))
def test_route(N, name, monkeypatch):
    fp, = run_case(N, name, monkeypatch.setenv)
    print(name, fp)
    _premises(name, fp)
    assert fp == FP[name], (name, fp)
    if name in ("no_slots", "key_lists_short", "members_dense", "members_overflow", "one_cache", "one_cache_dense", "batch_1",
                "batch_2", "capacity_retry"):
        for f in ("n", "ngroups", "counts", "groups", "hits"):        # switches that leave the groups' numbers as they are
            assert fp[f] == FP["shared_minimizer"][f], (name, f)


# the launches of a second run in the same context, recorded on that commit too: one compaction less and one LDS sort more
# than a first run's -- every other field of the fingerprint is the first run's
AGAIN_LAUNCHES = {"hist8": 8, "reduce8": 8, "scatter1": 8, "chunks": 8, "localsort": 6, "intersect": 3, "compact": 4, "locate": 4}


def test_the_same_run_twice_in_one_context(N, monkeypatch):
    """the second run finds every buffer of the first"""
    a, b = run_case(N, "shared_minimizer", monkeypatch.setenv, runs=2)
    print(a, b)
    assert a == FP["shared_minimizer"]
    assert b == dict(FP["shared_minimizer"], launches=AGAIN_LAUNCHES)


def test_two_geometries_one_after_the_other_in_one_context(N):
    """12/30/12 then 40/12/36: the second run finds the first's buffers, sized for another geometry; both as in fresh contexts"""
    with N.Engine() as e:
        for name in ("short_index_slots", "two_pieces"):
            ids, flags, filt = load(N, e, name)
            fp = fingerprint(N, e, ids, flags, filt)
            print(name, fp)
            assert fp == FP[name], (name, fp)
            for g in ids:
                e.free(g)
