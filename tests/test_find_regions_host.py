"""CPU tests of find_regions' one-GPU host flows (krisp_fasta: the in-core packed flow, the streaming flow, the wide flow)
over an engine that only records: every call the flows make, with its plain arguments, in order.

The traces in tests/golden/find_regions_host_traces.json were recorded with this very module from the commit BEFORE the
flows became drivers over named phases (`python tests/test_find_regions_host.py FILE` writes them; it was run with that
commit's krisp_fasta.py in the tree): the refactored flows must make the same device calls with the same arguments in the
same order, print the same lines, read the files as often and return stats with the same keys.  A trace that differs
says the flow changed what the device sees -- the fixture is not what gets adjusted.  No GPU."""
import contextlib
import gc
import io
import json
import os
import sys
import threading
import weakref

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from krisp_amd import _native
from krisp_amd import krisp_fasta as KF

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "find_regions_host_traces.json")
L, D, R = 4, 1, 2
K = L + D + R
SWITCHES = ("KRISP_RESERVE", "KRISP_RESERVE_MIN", "KRISP_STREAM_MIN", "KRISP_STREAM_BATCH")


def _plain(x):
    """an argument as the trace holds it: numbers, strings, lists; candidate lists by their prefixes, bytes by length"""
    if isinstance(x, np.ndarray):
        if x.dtype == _native.CAND:
            return {"cands": [int(p) for p in x["prefix"]]}
        if x.dtype == np.uint8:
            return {"bytes": int(x.size)}
        return x.tolist()
    if isinstance(x, (bytes, bytearray, memoryview)):
        return {"bytes": len(x)}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return x.item()
    return x


def _capacity(what):
    e = _native.KrispHipError(f"{what}: out of device memory")
    e.code = _native.ERR_CAPACITY
    return e


class FakeEngine:
    """records (name, arguments) of every call and answers from the scenario's script:
      counts       {genome: k-mers}                         (default 100 + genome)
      cands        [(left, right), ...]   the candidate list, ascending; intersect / probe_cands number i leaves the
      running      [n0, n1, ...]          first running[i] of them (default: all)
      avail        mem_info()["avail"]
      fail         {(name, i): what}      the i-th call of `name` raises KrispHipError, code ERR_CAPACITY
      outgroup     genomes whose records carry diag C (the others A)
      wide         [{"hits": [(cand, genome, pos, strand)], "ngroups": n}, ...]   one per wide_run
    One object serves every context a scenario opens ("open" / "close" in the trace)."""

    def __init__(self, script):
        self.script = script
        self.trace = []
        self.seen = {}
        self.bases = {}
        self.on_call = None
        pre = sorted(KF._prefix_key(l, r) for l, r in script.get("cands", []))
        self.all_cands = np.zeros(len(pre), dtype=_native.CAND)
        self.all_cands["prefix"] = np.array(pre, dtype=np.uint64)
        self.cur = self.all_cands[:0]
        self.steps = 0
        self.wide_runs = -1

    def __enter__(self):
        self.trace.append(["open"])
        return self

    def __exit__(self, *exc):
        self.trace.append(["close"])

    def log(self, name, *args, **kw):
        self.trace.append([name] + [_plain(a) for a in args] + ([{k: _plain(v) for k, v in sorted(kw.items())}] if kw else []))
        if self.on_call is not None:
            self.on_call(name)
        i = self.seen.get(name, 0)
        self.seen[name] = i + 1
        if (name, i) in self.script.get("fail", {}):
            raise _capacity(name)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **kw: self.log(name, *a, **kw)      # (set_params, reserve, free, sort, upload ...: no answer)

    def upload(self, gid, bases):
        self.log("upload", gid, bases)
        self.bases[gid] = np.array(bases, dtype=np.uint8)

    def fetch_bases(self, gid, n):
        self.log("fetch_bases", gid, n)
        return self.bases[gid][:n]

    def mem_info(self):
        self.log("mem_info")
        return {"avail": self.script.get("avail", 1 << 40)}

    def count(self, gid):
        self.log("count", gid)
        return self.script.get("counts", {}).get(gid, 100 + gid)

    def _step(self):
        running = self.script.get("running")
        n = running[self.steps] if running is not None else len(self.all_cands)
        self.steps += 1
        self.cur = self.all_cands[:n]
        return n

    def intersect(self, ids, flags, apply_filter=True):
        self.log("intersect", ids, flags, apply_filter=apply_filter)
        return self._step()

    def probe_cands(self, ids, flags, apply_filter=True):
        self.log("probe_cands", ids, flags, apply_filter=apply_filter)
        return self._step()

    def cands(self):
        self.log("cands")
        return self.cur.copy()

    def load_cands(self, cands):
        self.log("load_cands", cands)
        self.cur = np.array(cands, dtype=_native.CAND)

    def collect(self, ids, fetch=True):
        self.log("collect", ids)
        out = self.script.get("outgroup", ())
        rows = [(int(p) | ((1 if g in out else 0) << (62 - 2 * (L + R))), g, 1) for p in self.cur["prefix"] for g in ids]
        recs = np.array(rows, dtype=_native.RECORD) if rows else np.empty(0, dtype=_native.RECORD)
        return recs[np.argsort(recs["key"], kind="stable")]       # (kr_collect: by key, then position in the call)

    def wide_run(self, ids, flags, apply_filter=True):
        self.log("wide_run", ids, flags, apply_filter=apply_filter)
        self.wide_runs += 1
        return len(self._wide()["hits"])

    def _wide(self):
        w = self.script.get("wide", [])
        return w[self.wide_runs] if self.wide_runs < len(w) else {"hits": [], "ngroups": 0}

    def wide_fetch(self, what):
        self.log("wide_fetch", what)
        if what == _native.WIDE_HITS:
            return np.array([tuple(h) for h in self._wide()["hits"]], dtype=_native.WIDE_HIT)
        if what == _native.WIDE_NGROUPS:
            return np.array([self._wide()["ngroups"]], dtype=np.uint32)
        if what == _native.WIDE_COUNTS:
            return np.array([self.script.get("counts", {}).get(g, 100 + g) for g in range(self.script["n"])], dtype=np.uint64)
        return np.array([0], dtype=np.uint32)

    def wide_windows(self, k):
        self.log("wide_windows", k)
        rows = []
        for _c, g, pos, _s in self._wide()["hits"]:
            rows.append(self.bases[g][pos:pos + k])
        return np.array(rows, dtype=np.uint8).reshape(len(rows), k)


# ----------------------------------------------------------------------------
# scenarios: 3 to 6 tiny genomes each
# ----------------------------------------------------------------------------
def _seq(n, seed):
    return "".join("ACGT"[(i * 7 + seed * 3 + i // 5) % 4] for i in range(n))


INS = ["in0.fa", "in1.fa", "in2.fa"]
OUTS = ["out0.fa", "out1.fa"]
CANDS = [("AACC", "GG"), ("ACGA", "CA"), ("CCGA", "AG")]
BOTH = dict(ins=INS[:2], outs=OUTS, outgroup=(2, 3), cands=CANDS)
FIVE = dict(ins=INS, outs=OUTS, outgroup=(3, 4), cands=CANDS)
SCENARIOS = {
    "plan taken": dict(BOTH, patch={"RESERVE_MIN": 0}, iupac={"out0.fa": ["ACGTRGG"]}),
    "no plan": dict(BOTH, iupac={"in1.fa": ["AANCGGG", "ACGANCA"]}),
    "later file longer than the plan": dict(BOTH, patch={"RESERVE_MIN": 0}, est={f: 60 for f in INS + OUTS},
                                            lens={"out0.fa": 90}),
    "reserve refused": dict(BOTH, patch={"RESERVE_MIN": 0}, fail={("reserve", 0): 1}),
    "capacity error in a sort, again in batches": dict(FIVE, fail={("sort", 3): 1}, running=[3, 2, 2]),
    "forced batch of 2": dict(FIVE, env={"KRISP_STREAM_BATCH": "2"}, running=[3, 3, 2]),
    # (the plan: four genomes of 100 bases beside the scratch, of five)
    "a batch that does not fit once": dict(FIVE, est={f: 100 for f in INS + OUTS},
                                           avail=(2 << 30) + 51 * 100 + 100 + int(17.4 * 100 * 4) + 10,
                                           fail={("sort", 2): 1}, running=[3, 2, 2, 2]),
    "first batch of first_min does not fit": dict(FIVE, env={"KRISP_STREAM_BATCH": "2"}, fail={("sort", 1): 1}),
    "second pass": dict(FIVE, env={"KRISP_STREAM_BATCH": "2"}, patch={"STREAM_EAGER_MAX": 0}, running=[3, 2, 2],
                        iupac={"in1.fa": ["ACGTRGG"], "out1.fa": ["AANCGGG"]}),
    "DNA and RNA in core": dict(BOTH, rna={"in1.fa", "out1.fa"}, cands=CANDS + [("ATCA", "GG")]),
    "DNA and RNA in batches": dict(FIVE, env={"KRISP_STREAM_BATCH": "2"}, rna={"in0.fa", "out1.fa"},
                                   cands=CANDS + [("ATCA", "GG")]),
    "no filter, one side": dict(ins=INS, outs=[], outgroup=(), cands=CANDS, k=L + R, env={"KRISP_STREAM_BATCH": "1"}),
    "wide: device parse": dict(BOTH, wide=True, bare=True,
                               wide_runs=[{"hits": [(0, 0, 3, 0), (0, 1, 5, 0), (0, 2, 2, 0), (0, 3, 9, 0)], "ngroups": 1}]),
    "wide: touched pairs": dict(BOTH, wide=True, bare=True, lens={f: 120 for f in INS + OUTS}, iupac={"in0.fa": ["ACGTRGG"]},
                                wide_runs=[{"hits": [(0, 0, 3, 0), (0, 1, 5, 0), (0, 2, 2, 0), (0, 3, 9, 0)], "ngroups": 1},
                                           {"hits": [(0, 0, 0, 0), (0, 1, 11, 0)], "ngroups": 1}]),
    "wide: probe text longer than the genomes": dict(
        BOTH, wide=True, bare=True, iupac={"in0.fa": [a + b + "ACRG" + a for a in "ACGT" for b in "ACGT"]},        # (16 plain pairs: 127 bytes of probe text)
        wide_runs=[{"hits": [(0, 0, 3, 0), (0, 1, 5, 0), (0, 2, 2, 0), (0, 3, 9, 0)], "ngroups": 1}]),
    "wide: DNA and RNA": dict(BOTH, wide=True, bare=True, rna={"in1.fa"},
                              wide_runs=[{"hits": [(0, 0, 3, 0), (0, 1, 5, 0), (0, 2, 2, 0), (0, 3, 9, 0)], "ngroups": 1}]),
    "wide: every group fails the filter": dict(BOTH, wide=True, bare=True, r=0),
}


class Scenario:
    """one scenario's files in memory, the patches that serve them, its fake engine"""

    def __init__(self, name, monkeypatch):
        self.sc = sc = SCENARIOS[name]
        self.files = sc["ins"] + sc["outs"]
        lens = sc.get("lens", {})
        self.texts = {}
        for i, f in enumerate(self.files):
            body = _seq(lens.get(f, 40 + 3 * i), i)
            self.texts[f] = (body if sc.get("bare") else f">{f}\n{body}\n").encode()
        self.eng = FakeEngine({"n": len(self.files), "counts": {1: 7}, "cands": sc["cands"], "running": sc.get("running"),
                               "avail": sc.get("avail", 1 << 40), "fail": sc.get("fail", {}), "outgroup": sc["outgroup"],
                               "wide": sc.get("wide_runs", [])})
        self.reads = {}
        self.refs = {}
        self.lock = threading.Lock()
        for name_ in SWITCHES:
            monkeypatch.delenv(name_, raising=False)
        for k, v in sc.get("env", {}).items():
            monkeypatch.setenv(k, v)
        for k, v in sc.get("patch", {}).items():
            monkeypatch.setattr(KF, k, v)
        monkeypatch.setattr(KF, "_engine", lambda device: self.eng)
        monkeypatch.setattr(KF.fasta, "read_text", self.read_text)
        monkeypatch.setattr(KF.fasta, "estimate_text_bytes", lambda f: sc.get("est", {}).get(f, len(self.texts[f])))
        monkeypatch.setattr(KF.fasta, "sniff_rna", lambda f: f in sc.get("rna", ()))
        monkeypatch.setattr(KF.fasta, "ingest_on_device", self.ingest_on_device)
        monkeypatch.setattr(KF.fasta, "ingest", self.ingest)

    def read_text(self, f):
        text = np.frombuffer(self.texts[f], dtype=np.uint8).copy()
        with self.lock:
            self.reads[f] = self.reads.get(f, 0) + 1
            self.refs.setdefault(f, []).append(weakref.ref(text))
        return text, True

    def ingest_on_device(self, eng, gid, text, universal, k, omit_soft):
        f = self.files[gid]
        eng.log("ingest", gid, len(text), universal, k, omit_soft)
        if self.sc.get("wide"):
            eng.bases[gid] = np.array(text, dtype=np.uint8)       # (a wide run fetches them back: a copy, not the text)
        return len(text), f in self.sc.get("rna", ()), list(self.sc.get("iupac", {}).get(f, []))

    def ingest(self, f, k, omit_soft):
        with self.lock:
            self.reads[f] = self.reads.get(f, 0) + 1
        return (np.frombuffer(self.texts[f], dtype=np.uint8).copy(), f in self.sc.get("rna", ()),
                list(self.sc.get("iupac", {}).get(f, [])))

    def run(self):
        """find_regions over the scenario -> what the fixture holds of it"""
        sc = self.sc
        err = io.StringIO()
        out = {}
        with contextlib.redirect_stderr(err):
            try:
                groups, stats = KF.find_regions(sc["ins"], sc["outs"], L, sc.get("r", R), sc.get("k", K), verbose=True,
                                                wide=sc.get("wide"))
                out["groups"] = [type(groups).__name__,
                                 [[[a.left, a.diag, a.right, list(a.labels)] for a in g] for g in groups]]
                out["stats_keys"] = sorted(stats)
                out["stage_keys"] = sorted(stats.get("stage_s", {}))
                out["stats"] = {k: stats[k] for k in ("kmers", "candidates", "streamed", "batch", "passes", "batches",
                                                      "mixed_rna", "wide_batch") if k in stats}
            except _native.KrispHipError as e:
                out["error"] = [type(e).__name__, str(e), e.code]
        out["trace"] = self.eng.trace
        out["reads"] = dict(sorted(self.reads.items()))
        out["stderr"] = err.getvalue().splitlines()
        return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_scenario(recorded):
    assert sorted(recorded) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_flow_makes_the_recorded_device_calls(name, recorded, monkeypatch):
    got, want = Scenario(name, monkeypatch).run(), recorded[name]
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"call {i}: {g} where the parent commit made {w}"
    assert len(got["trace"]) == len(want["trace"])
    assert got == want


def _names(trace):
    return [c[0] for c in trace]


def test_the_scenarios_take_the_routes_they_are_named_for(recorded):
    """(the fixture itself: each recorded trace shows the route its scenario is about)"""
    t = {k: v["trace"] for k, v in recorded.items()}
    assert _names(t["plan taken"])[:4] == ["open", "mem_info", "set_params", "reserve"] and "free" not in _names(t["plan taken"])
    assert "reserve" not in _names(t["no plan"])
    later = _names(t["later file longer than the plan"])
    assert later.count("ingest") == 2 + 4 and later.count("free") == 4 and later.count("set_params") == 2
    assert recorded["later file longer than the plan"]["reads"] == {"in0.fa": 2, "in1.fa": 2, "out0.fa": 1, "out1.fa": 1}
    refused = _names(t["reserve refused"])
    assert refused[refused.index("reserve") + 1:][:5] == ["free"] * 4 + ["set_params"]
    again = recorded["capacity error in a sort, again in batches"]
    assert _names(again["trace"]).count("open") == 2 and again["stats"]["batch"] == 3
    forced = t["forced batch of 2"]
    assert [c[1] for c in forced if c[0] in ("intersect", "probe_cands")] == [[0, 3], [1, 4], [2]]     # (interleaved)
    assert [c[0] for c in forced if c[0] in ("intersect", "probe_cands")] == ["intersect", "probe_cands", "probe_cands"]
    assert [c[1] for c in forced if c[0] == "collect"] == [[0, 3], [1, 4], [2]]
    once = recorded["a batch that does not fit once"]
    assert once["stats"]["batch"] == 2 and max(once["reads"].values()) == 2
    assert "one ingroup and one outgroup genome" in recorded["first batch of first_min does not fit"]["error"][1]
    assert recorded["first batch of first_min does not fit"]["error"][2] == _native.ERR_CAPACITY
    assert recorded["second pass"]["stats"]["passes"] == 2
    for name in ("DNA and RNA in core", "DNA and RNA in batches"):
        assert _names(t[name]).index("set_mixed_alphabets") < _names(t[name]).index("intersect")
    wide = _names(t["wide: probe text longer than the genomes"])
    assert wide.count("open") == 2 and wide.count("ingest") == 4 and wide.count("set_params_wide") == 2
    assert t["wide: every group fails the filter"] == []


def test_texts_handed_over_under_a_standing_plan_are_let_go(monkeypatch):
    """When the memory plan stands, a genome's text goes to the device as it arrives and nothing on the host needs it
    again: by the time the flow intersects, every text array is dead.  Before the flow consumed its futures this test
    FAILED -- the list of futures lived until the flow returned, a concurrent.futures.Future keeps its result, and so
    every file's text stayed in host memory through the sorts, the intersection and the collect."""
    s = Scenario("plan taken", monkeypatch)
    alive = {}

    def at(name):
        if name == "intersect":
            gc.collect()
            alive.update({f: [r() is not None for r in refs] for f, refs in s.refs.items()})
    s.eng.on_call = at
    s.run()
    assert sorted(alive) == sorted(s.files)
    assert alive == {f: [False] for f in s.files}


# ----------------------------------------------------------------------------
# the pieces that need no engine
# ----------------------------------------------------------------------------
def _run_of(files, ins):
    return KF._describe_run([KF.simplename(f) for f in files], ins, L, R, K, False, 0, False)


@pytest.mark.parametrize("gz", [False, True], ids=["plain files", "a .gz among them"])
def test_ingest_plan_under_each_switch(gz, monkeypatch):
    files = ["a.fa", "b.fa.gz" if gz else "b.fa", "c.fa"]
    run = _run_of(files, files[:1])
    sizes = {files[0]: 1000, files[1]: 5000, files[2]: 3000}
    monkeypatch.setattr(KF.fasta, "estimate_text_bytes", lambda f: sizes[f])
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert KF._ingest_plan(files, run) == (5000, False, run.workers)             # (below RESERVE_MIN: no plan)
    monkeypatch.setenv("KRISP_RESERVE_MIN", "5000")
    assert KF._ingest_plan(files, run) == (5000, True, run.workers)              # (below STREAM_MIN: readers side by side)
    monkeypatch.setenv("KRISP_RESERVE_MIN", "5001")
    assert KF._ingest_plan(files, run) == (5000, False, run.workers)
    monkeypatch.setenv("KRISP_RESERVE_MIN", "0")
    monkeypatch.setenv("KRISP_RESERVE", "0")
    assert KF._ingest_plan(files, run) == (5000, False, run.workers)
    monkeypatch.setenv("KRISP_STREAM_MIN", "0")
    assert KF._ingest_plan(files, run) == (5000, False, run.workers)             # (one file per thread set only with a plan)
    monkeypatch.setenv("KRISP_RESERVE", "1")
    assert KF._ingest_plan(files, run) == (5000, True, 1 if gz else run.workers)
    monkeypatch.setenv("KRISP_STREAM_MIN", "5001")
    assert KF._ingest_plan(files, run) == (5000, True, run.workers)
    monkeypatch.delenv("KRISP_RESERVE_MIN")
    monkeypatch.delenv("KRISP_STREAM_MIN")
    monkeypatch.setattr(KF, "RESERVE_MIN", 4000)
    monkeypatch.setattr(KF, "STREAM_MIN", 4500)
    assert KF._ingest_plan(files, run) == (5000, True, 1 if gz else run.workers)
    sizes[files[2]] = (1 << 32) - 128                                            # (kr_reserve plans 32-bit texts only)
    assert KF._ingest_plan(files, run) == ((1 << 32) - 128, False, run.workers)
    sizes[files[2]] = (1 << 32) - 129
    assert KF._ingest_plan(files, run) == ((1 << 32) - 129, True, 1 if gz else run.workers)

    def gone(f):
        raise OSError(f)
    monkeypatch.setattr(KF.fasta, "estimate_text_bytes", gone)
    monkeypatch.setenv("KRISP_RESERVE_MIN", "0")
    assert KF._ingest_plan(files, run) == (0, True, run.workers)


@pytest.mark.parametrize("first", [True, False], ids=["first batch of the first pass", "any later batch"])
@pytest.mark.parametrize("first_min", [1, 2])
@pytest.mark.parametrize("n", range(1, 7))
def test_halving_a_batch_that_does_not_fit(n, first_min, first):
    batch = list(range(10, 10 + n))
    e = _capacity("kr_genome_sort")
    if n == 1:
        with pytest.raises(_native.KrispHipError) as got:
            KF._halve_batch(batch, first_min, first, e)
        assert got.value is e
    elif first and n <= first_min:
        with pytest.raises(_native.KrispHipError) as got:
            KF._halve_batch(batch, first_min, first, e)
        assert "one ingroup and one outgroup genome" in str(got.value) and str(e) in str(got.value)
        assert got.value.code == _native.ERR_CAPACITY and got.value.__cause__ is e
    else:
        a, b = KF._halve_batch(batch, first_min, first, e)
        assert a + b == batch and a and b
        assert len(a) == max((n + 1) // 2, first_min if first else 1)


def test_mixed_flags():
    assert KF._mixed([True, False]) and KF._mixed([False, True, True])
    assert not KF._mixed([True, True]) and not KF._mixed([False, False]) and not KF._mixed([])


if __name__ == "__main__":          # record the fixture (from the commit whose calls are the reference)
    traces = {}
    for name_ in SCENARIOS:
        mp = pytest.MonkeyPatch()
        try:
            traces[name_] = Scenario(name_, mp).run()
        finally:
            mp.undo()
    with open(sys.argv[1], "w") as fh:
        json.dump(traces, fh, indent=0, sort_keys=True)
        fh.write("\n")
