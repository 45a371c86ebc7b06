"""--out_near on the GPU (kr_near_*, csrc/k_near.inc): every packed golden case's table, for every distance, against the
slow definition (py_near, test_near_host.py) and against the locate pass; near matches planted into synthetic genomes at
scale; the flows (in core / batches / two ranks / BGZF inflated on the device) giving the same file; 10^5 targets that
share their seed pieces; positions beyond 2^32; two runs, the same bytes."""
import io
import os
import random
import sys
from collections import Counter
from contextlib import redirect_stdout

import numpy as np
import pytest

from krisp_amd import codec, fasta, synth
from krisp_amd import krisp_fasta as KF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_locate_host import FC, _COMP, golden_groups, golden_paths                          # noqa: E402
from test_near_host import case_amplicon, near_rows, py_near                                  # noqa: E402
from test_gpu_locate import _argv, _bgzf_file, _files, _write_family                          # noqa: E402

pytestmark = pytest.mark.gpu


def _packed(case):
    k = case_amplicon(case)
    L, D, R = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    return not KF._is_wide(L, D, R)


PACKED = [c for c in FC if ("csv" in c or "filtered_canon" in c) and _packed(c) and golden_groups(c) is not None]


def _golden_case(case, tmp_path):
    """one case, every distance: -> whether any distance had rows"""
    ing, out = _files(case, tmp_path)
    files = ing + out
    k = case_amplicon(case)
    omit = case["omit_soft"]
    name = case["name"]
    L, D, R = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    groups, _ = KF.find_regions(ing, out, case["L"], case["R"], k, omit_soft=omit)
    targets = KF.near_targets(groups, [KF.simplename(f) for f in ing] if out else None)
    locs = KF.locate_regions(groups, ing, out, case["L"], case["R"], k, omit_soft=omit)
    by_region = {}
    for i, t in targets:
        by_region.setdefault(i, []).append(t)
    any_rows = False
    for M in range(0, min(3, k - 1) + 1):
        got = near_rows(KF.near_matches(groups, ing, out, case["L"], case["R"], k, mismatches=M, omit_soft=omit))
        want = py_near(files, targets, L, D, R, M, omit)
        print(name, "M", M, "rows", len(got), "want", len(want), "flank>0", sum(1 for r in want if r[9] > 0))
        assert got == want, (name, M)
        any_rows |= bool(got)
        if not targets:
            assert got == [], (name, M)
        # the rows without a flank mismatch are the locate pass's rows whose diagnostic columns lie within M of a target
        # of that region, once per such target
        proj = Counter((r[0], r[2], r[4], r[5], r[7], r[10]) for r in got if r[9] == 0)
        expect = Counter()
        for r in locs:
            seq = r["sequence"].replace("U", "T")
            for t in by_region.get(int(r["region"]), []):
                if sum(a != b for a, b in zip(seq[L:L + D], t[L:L + D])) <= M:
                    expect[(int(r["region"]), r["file"], int(r["record_index"]), int(r["start"]), r["strand"], r["sequence"])] += 1
        assert proj == expect, (name, M)
        if M == 0:
            tset = set(targets)
            assert sorted((r[0], r[2], r[3], r[4], r[5], r[6], r[7], r[10]) for r in got) == \
                sorted(tuple(r) for r in locs.tolist() if (int(r[0]), r[7].replace("U", "T")) in tset), name
    return any_rows


def test_golden_cases_equal_py_near_and_agree_with_the_locate_pass(tmp_path):
    """every packed golden case with recorded lines, M = 0 .. min(3, k - 1): the table equals py_near's row for row, its
    rows without a flank mismatch are the locate pass's; at least 25 cases compared, at least 20 of them with rows"""
    with_rows = 0
    for n, case in enumerate(PACKED):
        d = tmp_path / str(n)
        d.mkdir()
        with_rows += _golden_case(case, d)
    assert len(PACKED) >= 25 and with_rows >= 20, (len(PACKED), with_rows)


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


@pytest.mark.parametrize("name", ["c1_25_1_2", "rand0_6_1_2", "mixed_in_dna_out_rna_6_1_3"])
def test_the_flows_write_the_same_file_twice(name, tmp_path, monkeypatch):
    case = [c for c in FC if c["name"] == name][0]
    argv = _argv(case, tmp_path)
    tsv = {}
    flows = ("in_core", "again", "batches", "with_locations") + (("devices",) if name.startswith("c1_") else ())
    for flow in flows:
        p = str(tmp_path / f"{flow}.tsv")
        extra = ["--devices", "0,0"] if flow == "devices" else []
        if flow == "with_locations":
            extra = ["--out_locations", str(tmp_path / "loc_both.tsv")]
        if flow == "batches":
            monkeypatch.setenv("KRISP_STREAM_BATCH", "1")
        else:
            monkeypatch.delenv("KRISP_STREAM_BATCH", raising=False)
        csv = _main(argv + extra + ["--out_near", p, "--near-mismatches", "2"])
        if "csv" in case:
            assert csv == case["csv"]
        tsv[flow] = open(p, "rb").read()
    assert tsv["in_core"].startswith((KF.NEAR_HEADER + "\n").encode()) and tsv["in_core"].count(b"\n") > 1
    for flow in tsv:
        assert tsv[flow] == tsv["in_core"], flow
    # --out_locations beside --out_near writes the file it writes alone
    _main(argv + ["--out_locations", str(tmp_path / "loc_alone.tsv")])
    assert open(tmp_path / "loc_both.tsv", "rb").read() == open(tmp_path / "loc_alone.tsv", "rb").read()


def test_bgzf_inflated_on_the_device_gives_the_rows_of_the_host_read(tmp_path, monkeypatch):
    import gzip
    case = [c for c in FC if c["name"] == "c1_25_1_2"][0]
    ing, out = _files(case, tmp_path)
    bg = []
    for p in ing + out:
        with gzip.open(p, "rb") as f:
            data = f.read()
        data = data.replace(b">", b">id_", 1)
        q = str(tmp_path / (os.path.basename(p).split(".")[0] + ".fa.gz"))
        _bgzf_file(q, data)
        bg.append(q)
    monkeypatch.setenv("KRISP_DEVICE_INFLATE_MIN", "0")
    rows = {}
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        groups, _ = KF.find_regions(bg[:2], bg[2:], 25, 2, 28)
        fasta.LAST_TIMINGS.clear()
        near = KF.near_matches(groups, bg[:2], bg[2:], 25, 2, 28, mismatches=2)
        assert all(bool(fasta.LAST_TIMINGS[q].get("device_inflate")) == (dev == "1") for q in bg)
        rows[dev] = near_rows(near)
    assert rows["1"] == rows["0"] and len(rows["1"]) >= 20
    assert all(r[3].startswith("id_") or r[4] > 0 for r in rows["1"])


# ----------------------------------------------------------------------------
# planted near matches at scale
# ----------------------------------------------------------------------------
def _rc(b):
    return b[::-1].translate(_COMP)


def test_planted_near_matches_in_four_genomes_of_50_mbp(tmp_path):
    """4 x 50 Mbp at 28/1/2: copies of targets with 0..3 substitutions written into the genomes at known places (both
    strands; across a record boundary; holding or next to an N; in lower case); M = 2, with and without --omit-soft"""
    L, D, R, k, M = 28, 1, 2, 31, 2
    fam = synth.family(7, 2, 2, 50_000_000, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01)
    paths = _write_family(tmp_path, fam)
    groups, _ = KF.find_regions(paths[:2], paths[2:], L, R, k)
    assert len(groups) > 0
    targets = KF.near_targets(groups, [KF.simplename(p) for p in paths[:2]])
    assert len(targets) >= len(groups)
    texts = [t.copy() for _, _, t in fam]
    del fam
    seps = [np.flatnonzero(t == 10) for t in texts]
    rng = random.Random(5)
    plants = []
    kinds = ["plain"] * 6 + ["boundary", "holds_n", "next_to_n", "lower"]
    for i in range(400):
        g = i % 4
        ti = rng.randrange(len(targets))
        nsub = rng.randrange(4)
        cols = sorted(rng.sample(range(k), nsub))
        tgt = targets[ti][1]
        mut = list(tgt)
        for c in cols:
            mut[c] = rng.choice([b for b in "ACGT" if b != tgt[c]])
        mut = "".join(mut).encode()
        strand = rng.choice("+-")
        kind = kinds[i % len(kinds)]
        text = texts[g]
        if kind == "boundary":
            p = int(seps[g][i % len(seps[g])]) - rng.randrange(1, k - 1)
        else:
            # (a slot of its own inside a record, clear of the separators)
            while True:
                p = 1000 + (i // 4) * 400_000 + rng.randrange(1000)
                j = int(np.searchsorted(seps[g], p))
                if not (j < len(seps[g]) and seps[g][j] < p + k + 2):
                    break
        written = np.frombuffer(mut if strand == "+" else _rc(mut), dtype=np.uint8).copy()
        if kind == "lower":
            written |= 0x20
        text[p:p + k] = written
        text[p - 1] = text[p + k] = ord("A")
        if kind == "boundary":
            text[seps[g]] = 10
        elif kind == "holds_n":
            text[p + rng.randrange(k)] = ord("N")
        elif kind == "next_to_n":
            text[p - 1] = text[p + k] = ord("N")
        fm = sum(1 for c in cols if c < L or c >= L + D)
        plants.append((g, ti, p, strand, nsub, fm, kind, mut.decode()))
    planted = []
    (tmp_path / "planted").mkdir()
    for g, text in enumerate(texts):
        q = str(tmp_path / "planted" / os.path.basename(paths[g]))      # (the genome keeps its label: the file's name)
        synth.write_fasta(q, text)
        planted.append(q)
    tindex = {t: i for i, t in enumerate(targets)}
    for omit in (False, True):
        near = KF.near_matches(groups, planted[:2], planted[2:], L, R, k, mismatches=M, omit_soft=omit)
        rows = near_rows(near)
        assert len({(r[0], r[1], r[2], r[4], r[5], r[7]) for r in rows}) == len(rows)
        table = {(tindex[(r[0], r[1])], planted.index(r[2]), r[4], r[5], r[7]): r for r in rows}
        found = 0
        for g, ti, p, strand, nsub, fm, kind, mut in plants:
            ri = int(np.searchsorted(seps[g], p))
            start = p - (int(seps[g][ri - 1]) + 1 if ri else 0)
            row = table.get((ti, g, ri, start, strand))
            expected = nsub <= M and kind not in ("boundary", "holds_n") and not (kind == "lower" and omit)
            if kind == "boundary":
                # (the planted bytes minus the separator: no window of the record holds the copy whole)
                assert row is None
                continue
            assert (row is not None) == expected, (g, ti, p, strand, nsub, kind, omit, row)
            if expected:
                found += 1
                assert (row[8], row[9], row[10], row[6] - row[5]) == (nsub, fm, mut, k)
        assert found >= 150
        # a sample of rows re-derived from the genomes' text
        recstart = [np.concatenate([[0], s + 1]) for s in seps]
        for i in random.Random(6).sample(range(len(rows)), min(4000, len(rows))):
            region, tgt, f, _rec, ri, start, end, strand, mm, fmm, seq = rows[i]
            g = planted.index(f)
            p = int(recstart[g][ri]) + start
            w = texts[g][p:p + k].tobytes()
            assert end - start == k and b"\n" not in w and b"N" not in w and b"n" not in w
            if omit:
                assert w.isupper()
            w = w.upper()
            if strand == "-":
                w = _rc(w)
            assert w.decode() == seq
            diff = [c for c in range(k) if seq[c] != tgt[c]]
            assert len(diff) == mm <= M and sum(1 for c in diff if c < L or c >= L + D) == fmm
            assert (region, tgt) in tindex


# ----------------------------------------------------------------------------
# many targets on one piece; the bitmap nearly full
# ----------------------------------------------------------------------------
def test_10_5_targets_that_share_their_pieces():
    """3000 flank pairs cut from the genome x 40 diagnostic fillings = 120 000 targets at 10/4/10 (every flank piece is
    shared by 40 targets and their reverse complements), M = 2 and M = 0, one genome of 3 Mbp with separators and N"""
    from krisp_amd import _native
    L, D, R, k = 10, 4, 10, 24
    rng = np.random.Generator(np.random.PCG64(11))
    n = 3_000_000
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    bases[np.arange(500_000, n, 500_000)] = 10
    for s in rng.integers(0, n - 50, size=300):
        bases[s:s + 3] = ord("N")
    fill = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows = []
    starts = rng.choice(n - k, size=3000, replace=False)
    for s in starts:
        w = bases[s:s + k]
        if (w == 10).any() or (w == ord("N")).any():
            w = np.frombuffer(b"ACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
        rows.append(w.copy())           # (the window itself: the genome holds every family at distance 0)
        for code in rng.choice(256, size=40, replace=False):
            t = w.copy()
            t[L:L + D] = fill[[(code >> 6) & 3, (code >> 4) & 3, (code >> 2) & 3, code & 3]]
            rows.append(t)
    T = np.unique(np.array(rows, dtype=np.uint8), axis=0)
    assert len(T) >= 100_000
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ATGC", b"TACG"):
        comp[a] = b
    with _native.Engine() as eng:
        eng.set_params_locate(L, D, R, False, max_bases=n)
        eng.upload(0, bases)
        eng.near_table(T, 0)
        h0 = eng.near(0)
        eng.near_table(T, 2)
        h2 = eng.near(0)
        w2 = eng.near_windows(k)
    win = np.lib.stride_tricks.sliding_window_view(bases, k)
    valid = ~((win == 10) | (win == ord("N"))).any(axis=1)
    # M = 0 by sorting: the windows (and their reverse complements) that are targets
    tv = np.ascontiguousarray(T).view(f"S{k}").ravel()
    want0 = []
    for strand, w in ((0, np.ascontiguousarray(win)), (1, np.ascontiguousarray(comp[win][:, ::-1]))):
        wv = w.view(f"S{k}").ravel()
        idx = np.searchsorted(tv, wv)
        idx[idx == len(tv)] = 0
        hit = np.flatnonzero((tv[idx] == wv) & valid)
        want0 += [(int(p), strand, int(idx[p])) for p in hit]
    got0 = sorted(zip(h0["pos"].tolist(), h0["strand"].tolist(), h0["target"].tolist()))
    assert got0 == sorted(want0) and len(got0) >= 2500
    assert not h0["mismatches"].any() and not h0["flank_mismatches"].any()
    # M = 2 at a sample of positions (the targets' own loci, their neighbours, random ones), by brute force
    assert h2["pos"].tolist() == sorted(h2["pos"].tolist())
    sample = set(int(s) for s in starts[:150]) | set(int(s) + 1 for s in starts[:50]) | \
        set(int(p) for p in rng.integers(0, n - k, size=100))
    flank = np.ones(k, dtype=bool)
    flank[L:L + D] = False
    got2 = {}
    for h, w in zip(h2.tolist(), w2):
        if h[5] in sample:
            got2.setdefault(h[5], []).append((h[1], h[0], h[2], h[3], bytes(w)))
    nrows = 0
    for p in sorted(sample):
        want = []
        if valid[p]:
            for strand, x in ((0, win[p]), (1, comp[win[p]][::-1])):
                ne = T != x
                d = ne.sum(axis=1)
                want += [(strand, int(ti), int(d[ti]), int(ne[ti][flank].sum()), x.tobytes()) for ti in np.flatnonzero(d <= 2)]
        assert sorted(got2.get(p, [])) == sorted(want), p
        nrows += len(want)
    assert nrows >= 1000


def test_positions_beyond_2_32():
    """one record of 2^32 + 2^20 bases (all A) with a target planted on both sides of 2^32, one substitution in the second"""
    from krisp_amd import _native
    n = (1 << 32) + (1 << 20)
    bases = np.full(n, ord("A"), dtype=np.uint8)
    win = b"CGTACGTTGACCAGTGCATGCAGTCAGG"
    w = np.frombuffer(win, dtype=np.uint8)
    lo, hi = (1 << 32) - 10, n - 500
    bases[lo:lo + 28] = w
    bases[hi:hi + 28] = w
    bases[hi + 3] = ord("T")        # (A in the target: a mismatch in the left flank)
    rc = np.frombuffer(_rc(win), dtype=np.uint8)
    bases[hi + 100:hi + 128] = rc
    bases[n - 100] = ord("\n")
    with _native.Engine() as eng:
        eng.set_params_locate(25, 1, 2, False, max_bases=n)
        eng.upload(0, bases)
        eng.near_table(w.reshape(1, 28), 1)
        hits = eng.near(0)
        assert hits["pos"].tolist() == [lo, hi, hi + 100] and hits["strand"].tolist() == [0, 0, 1]
        assert hits["mismatches"].tolist() == [0, 1, 0] and hits["flank_mismatches"].tolist() == [0, 1, 0]
        assert [bytes(r) for r in eng.near_windows(28)] == [win, win[:3] + b"T" + win[4:], win]
        assert eng.locate_seps(0).tolist() == [n - 100]
