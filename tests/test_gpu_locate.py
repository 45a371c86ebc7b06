"""--out_locations on the GPU (kr_locate_*, csrc/k_locate.inc): every golden case's rows against the multiplicity contract
(a group's label occurs in an Amplicon's labels as often as there are rows of that genome, group and sequence), every
row's window re-derived from the genome's text, the rows equal to the slow Python locator (test_locate_host.py), the flows
(in core / batches / two ranks / BGZF inflated on the device) giving the same file, synthetic genomes at scale, and
positions beyond 2^32."""
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
from test_locate_host import FC, golden_paths, labels_of, py_locate       # noqa: E402

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ATGCRYMKSWBVDHN", b"TACGYRKMSWVBHDN")


def _amplicon(case):
    a = case.get("main_args", [])
    if "--amplicon" in a:
        return int(a[a.index("--amplicon") + 1])
    return case["L"] + case["D"] + case["R"]


def _files(case, tmp_path):
    paths = golden_paths(case, tmp_path)
    return [paths[f] for f in case["ingroup"]], [paths[f] for f in case["outgroup"]]


def contract(groups, locs, files):
    """the multiplicity contract: Counter of (region, label, sequence) from the rows == from the groups"""
    labels = dict(zip(files, labels_of(files)))
    want = Counter()
    for i, g in enumerate(groups):
        for a in g:
            for lab in a.labels:
                want[(i, lab, a.sequence)] += 1
    got = Counter(zip(locs["region"].tolist(), [labels[f] for f in locs["file"]], locs["sequence"].tolist()))
    assert got == want


def rederive(groups, locs, k, omit_soft, sample=None):
    """every row's window cut again from the genome's records: the reference keeps it, its flanks are the group's"""
    recs, rnas = {}, {}
    idx = range(len(locs)) if sample is None else sample
    for i in idx:
        r = locs[i]
        if r["file"] not in recs:
            recs[r["file"]] = fasta.read_records(r["file"])
            rnas[r["file"]] = bool(fasta.detect_rna(recs[r["file"]]))
        rec = recs[r["file"]][r["record_index"]]
        assert r["end"] - r["start"] == k and r["end"] <= len(rec)
        w = rec[r["start"]:r["end"]]
        if rnas[r["file"]]:
            w = w.replace(b"U", b"T").replace(b"u", b"t")
        if omit_soft:
            assert w.isupper()
        w = w.upper()
        assert b"N" not in w and b"\n" not in w
        if r["strand"] == "-":
            w = w[::-1].translate(_COMP)
        seq = w.decode()
        if rnas[r["file"]]:
            seq = seq.replace("T", "U")
        assert seq == r["sequence"]
        g = groups[r["region"]][0]
        assert seq.startswith(g.left) and seq.endswith(g.right)


def _run(ing, out, L, R, k, omit):
    groups, _ = KF.find_regions(ing, out, L, R, k, omit_soft=omit)
    return groups, KF.locate_regions(groups, ing, out, L, R, k, omit_soft=omit)


GOLDEN_CASES = [c for c in FC if "csv" in c or "filtered_canon" in c]


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=lambda c: c["name"])
def test_golden_cases_keep_the_multiplicity_contract(case, tmp_path):
    ing, out = _files(case, tmp_path)
    k = _amplicon(case)
    groups, locs = _run(ing, out, case["L"], case["R"], k, case["omit_soft"])
    files = ing + out
    contract(groups, locs, files)
    rederive(groups, locs, k, case["omit_soft"])
    # the same rows as the slow locator (packed and wide geometries alike)
    L, D, R = codec.effective_geometry(case["L"], k - case["L"] - case["R"], case["R"])
    pairs = [(g[0].left.replace("U", "T"), g[0].right.replace("U", "T")) for g in groups]
    want = py_locate(files, pairs, L, D, R, case["omit_soft"])
    got = list(zip(locs["region"].tolist(), locs["file"], locs["record"], locs["record_index"].tolist(),
                   locs["start"].tolist(), locs["end"].tolist(), locs["strand"], locs["sequence"]))
    assert got == want
    if case["name"] == "rand8_3_1_0":
        assert len(groups) == 0 and len(locs) == 0


def _main(argv):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert KF.main(argv) == 0
    return buf.getvalue()


def _argv(case, tmp_path, ing=None, out=None):
    if ing is None:
        ing, out = _files(case, tmp_path)
    a = list(ing) + (["--outgroup"] + list(out) if out else []) + case["main_args"]
    return a + (["--omit-soft"] if case["omit_soft"] else [])


@pytest.mark.parametrize("name", ["c1_25_1_2", "c1_30_40_30", "long_70_10_70"])
def test_streaming_in_core_and_two_ranks_write_the_same_locations(name, tmp_path, monkeypatch):
    case = [c for c in FC if c["name"] == name][0]
    argv = _argv(case, tmp_path)
    tsv = {}
    flows = ("in_core", "batches", "devices") if name.startswith("c1_") else ("in_core", "batches")
    for flow in flows:
        p = str(tmp_path / f"{flow}.tsv")
        extra = ["--devices", "0,0"] if flow == "devices" else []
        if flow == "batches":
            monkeypatch.setenv("KRISP_STREAM_BATCH", "1")
        else:
            monkeypatch.delenv("KRISP_STREAM_BATCH", raising=False)
        csv = _main(argv + extra + ["--out_locations", p])
        if "csv" in case:
            assert csv == case["csv"]
        tsv[flow] = open(p).read()
    assert tsv["in_core"].startswith(KF.LOCATION_HEADER + "\n") and tsv["in_core"].count("\n") > 1
    assert tsv["batches"] == tsv["in_core"]
    assert tsv.get("devices", tsv["in_core"]) == tsv["in_core"]


def _bgzf_file(path, data, block=20000):
    import struct
    import zlib
    with open(path, "wb") as f:
        for i in list(range(0, len(data), block)) + [None]:
            ch = b"" if i is None else data[i:i + block]
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            cd = co.compress(ch) + co.flush()
            f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cd) + 25) + cd
                    + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch)))


def test_bgzf_inflated_on_the_device_gives_the_rows_of_the_host_read(tmp_path, monkeypatch):
    import gzip
    case = [c for c in FC if c["name"] == "c1_25_1_2"][0]
    ing, out = _files(case, tmp_path)
    bg = []
    for p in ing + out:
        with gzip.open(p, "rb") as f:
            data = f.read()
        # (headers with descriptions: the IDs come from the file read again)
        data = data.replace(b">", b">id_", 1)
        q = str(tmp_path / (os.path.basename(p).split(".")[0] + ".fa.gz"))
        _bgzf_file(q, data)
        bg.append(q)
    monkeypatch.setenv("KRISP_DEVICE_INFLATE_MIN", "0")
    rows = {}
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        fasta.LAST_TIMINGS.clear()
        groups, locs = _run(bg[:2], bg[2:], 25, 2, 28, False)
        assert all(bool(fasta.LAST_TIMINGS[q].get("device_inflate")) == (dev == "1") for q in bg)
        rows[dev] = [tuple(r) for r in locs.tolist()]
        contract(groups, locs, bg)
    assert rows["1"] == rows["0"] and rows["1"]


def _write_family(tmp_path, fam):
    paths = []
    for name, _ing, text in fam:
        p = str(tmp_path / f"{name}.fa")
        synth.write_fasta(p, text)
        paths.append(p)
    return paths


def test_four_genomes_of_50_mbp(tmp_path):
    """4 x 50 Mbp, 8 records each, at 28/1/2: the contract in full, 10^4 random rows re-derived from the text"""
    fam = synth.family(7, 2, 2, 50_000_000, records=8, mu=0.01, snp_every=2000, n_frac=0.001, lower_frac=0.01)
    paths = _write_family(tmp_path, fam)
    del fam
    groups, locs = _run(paths[:2], paths[2:], 28, 2, 31, False)
    assert len(groups) > 0
    contract(list(groups), locs, paths)
    rng = random.Random(1)
    rederive(list(groups), locs, 31, False, sample=rng.sample(range(len(locs)), min(10_000, len(locs))))


def test_a_million_regions_saturate_the_bitmap(tmp_path):
    """conserved regions without a diagnostic column (no filter): > 10^6 groups, every slot of the LDS bitmap set, every
    probe goes to the global table"""
    fam = synth.family(3, 4, 0, 700_000, records=4, mu=0.0005, snp_every=100000)
    paths = _write_family(tmp_path, fam)
    groups, locs = _run(paths, [], 12, 12, 24, False)
    assert len(groups) >= 1_000_000
    glist = list(groups)
    contract(glist, locs, paths)
    rng = random.Random(2)
    rederive(glist, locs, 24, False, sample=rng.sample(range(len(locs)), 10_000))


def test_positions_beyond_2_32():
    """one record of 2^32 + 2^20 bases (all A) with a region planted on both sides of 2^32 and a separator beyond it: the
    scan's positions and the separator list are 64-bit"""
    from krisp_amd import _native
    n = (1 << 32) + (1 << 20)
    bases = np.full(n, ord("A"), dtype=np.uint8)
    win = b"CGTACGTTGACCAGTGCATGCAGTCAGGT"      # (the region at 25/1/2: its first 28 bases)
    w = np.frombuffer(win[:28], dtype=np.uint8)
    lo, hi = (1 << 32) - 10, n - 500
    bases[lo:lo + 28] = w
    bases[hi:hi + 28] = w
    bases[n - 100] = ord("\n")
    with _native.Engine() as eng:
        eng.set_params_locate(25, 1, 2, False, max_bases=n)
        eng.upload(0, bases)
        eng.locate_table(np.frombuffer(win[:25] + win[26:28], dtype=np.uint8).reshape(1, 27))
        hits = eng.locate(0)
        assert hits["pos"].tolist() == [lo, hi] and hits["strand"].tolist() == [0, 0] and hits["group"].tolist() == [0, 0]
        assert [bytes(r) for r in eng.locate_windows(28)] == [win[:28]] * 2
        assert eng.locate_seps(0).tolist() == [n - 100]
