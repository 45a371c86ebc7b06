"""One plain gzip member inflated on the device (kr_genome_upload_gzip, csrc/k_gunzip.inc) against the host path: the
bases, records, special characters and alphabet of the text Python's gzip gives, parsed by kr_genome_upload_text.  Chunks
forced small so that many of them, false block starts and runs of windows occur."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden_cases import FC as _FC0, FC6, canon_equal       # noqa: E402
from test_gpu_cli import _paths, _run_main, _amplicon      # noqa: E402

FC = _FC0 + FC6


@pytest.fixture(scope="module")
def N():
    from krisp_amd import _native
    return _native


def _fasta(seed, n, alphabet=b"ACGT", width=60, nrec=3, lower=False, nrun=0):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    recs = []
    for r in range(nrec):
        s = a[rng.integers(0, len(a), size=n // nrec)].copy()
        if lower:
            for _ in range(20):
                p = int(rng.integers(0, max(1, len(s) - 3000)))
                s[p:p + int(rng.integers(10, 3000))] |= 0x20
        if nrun and r == 1:
            p = len(s) // 3
            s = np.concatenate([s[:p], np.full(nrun, ord("N"), dtype=np.uint8), s[p:]])
        body = b"\n".join(bytes(s[i:i + width]) for i in range(0, len(s), width))
        recs.append(b">rec%d some words\n" % r + body + b"\n")
    return b"".join(recs)


def _gzip(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush=zlib.Z_SYNC_FLUSH, flags=0, extra=b"",
          name=b"", comment=b"", pad=0):
    """one gzip member as gzip / zlib write it, header fields as asked, optional flush points, zero padding"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_every:
        parts = []
        for i in range(0, len(text), flush_every):
            parts.append(co.compress(text[i:i + flush_every]) + co.flush(flush))
        body = b"".join(parts) + co.flush()
    else:
        body = co.compress(text) + co.flush()
    flg = flags | (4 if extra else 0) | (8 if name else 0) | (16 if comment else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\x03"
    if extra:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\x00"
    if comment:
        head += comment + b"\x00"
    if flg & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF) + b"\x00" * pad


def _check(e, raw, text, chunk):
    got = e.upload_gzip(0, np.frombuffer(raw, dtype=np.uint8), chunk=chunk)
    assert got is not None, e.last_gzip
    want = e.upload_text(1, np.frombuffer(text, dtype=np.uint8), False)
    assert got[:5] == want
    assert np.array_equal(e.fetch_bases(0, got[0]), e.fetch_bases(1, want[0]))
    return got


CASES = {
    "l1": dict(level=1), "l6": dict(level=6), "l9": dict(level=9),
    "filtered": dict(strategy=zlib.Z_FILTERED), "rle": dict(strategy=zlib.Z_RLE),
    "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY), "fixed": dict(strategy=zlib.Z_FIXED),
    "stored": dict(level=0), "sync_flush": dict(flush_every=70_000), "full_flush": dict(flush_every=90_000, flush=zlib.Z_FULL_FLUSH),
}


@pytest.mark.parametrize("chunk", [16384, 65536])
@pytest.mark.parametrize("what", sorted(CASES))
def test_gzip_member_inflated_on_the_device_equals_the_host_path(N, what, chunk):
    """levels 1 / 6 / 9, zlib's strategies, stored blocks, flush points mid-stream: the same bases as the host path; where
    dynamic blocks carry the stream, chunks are joined (their found starts were real)"""
    text = _fasta(7, 1_500_000, width=80 if what == "l9" else 60)
    raw = _gzip(text, **CASES[what])
    assert gzip.decompress(raw) == text
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=len(text))
        got = _check(e, raw, text, chunk)
        if what not in ("stored", "fixed", "huffman_only"):
            assert got[7] >= 2, got


@pytest.mark.parametrize("what", ["soft", "rna", "iupac", "nrun", "random_bytes", "lines80", "empty", "one_byte"])
def test_gzip_data_kinds_on_the_device(N, what):
    """soft-masked text, RNA, IUPAC letters, a 20 MB run of Ns (inflates 1000:1: no fall-back), bytes of every value,
    80-column lines, an empty text, one byte"""
    if what == "soft":
        text = _fasta(1, 1_200_000, lower=True)
    elif what == "rna":
        text = _fasta(2, 1_200_000).replace(b"T", b"U")
    elif what == "iupac":
        text = _fasta(3, 1_200_000, alphabet=b"ACGTACGTACGTRYKMSWBDHVN")
    elif what == "nrun":
        text = _fasta(4, 1_500_000, nrun=20_000_000)
    elif what == "random_bytes":
        text = b">r\n" + bytes(np.random.default_rng(5).integers(0, 256, size=1_000_000, dtype=np.uint8))
    elif what == "lines80":
        text = _fasta(6, 1_200_000, width=80, nrec=7)
    elif what == "empty":
        text = b""
    else:
        text = b"A"
    raw = _gzip(text, level=6)
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=max(len(text), 64))
        got = _check(e, raw, text, 16384)
        if what in ("soft", "rna", "iupac", "lines80", "nrun"):
            assert got[7] >= 2, got


def test_window_runs_and_header_variants(N):
    """small chunks of a DNA stream: a chunk's last 32 KB still hold markers, so windows are resolved one after the other
    (a run >= 2); FNAME / FEXTRA / FCOMMENT / FHCRC and zero padding behind the trailer are parsed"""
    text = _fasta(8, 2_000_000)
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=len(text))
        got = _check(e, _gzip(text, level=6), text, 4096)
        assert got[8] >= 2, got
        for kw in (dict(name=b"genome.fa"), dict(extra=b"AB\x02\x00xy", name=b"x", comment=b"a comment"), dict(flags=2, name=b"g"),
                   dict(pad=100), dict(extra=b"", flags=2 | 16, comment=b"c", pad=3)):
            raw = _gzip(text, **kw)
            assert gzip.decompress(raw) == text
            _check(e, raw, text, 30000)


def test_damaged_or_foreign_files_upload_nothing(N):
    """a flipped bit mid-stream, truncation, a wrong CRC, a wrong ISIZE, garbage after the trailer, a second member, BGZF:
    None, and the genome is not uploaded"""
    text = _fasta(9, 1_000_000)
    raw = _gzip(text, level=6)
    bgzf = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
    bad = {
        "flip": raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 0x10]) + raw[len(raw) // 2 + 1:],
        "truncated": raw[:len(raw) - 5000],
        "crc": raw[:-8] + bytes([raw[-8] ^ 1]) + raw[-7:],
        "isize": raw[:-4] + struct.pack("<I", len(text) + 1),
        "garbage": raw + b"garbage",
        "second_member": raw + _gzip(b">s\nACGT\n"),
        "bgzf": bgzf + raw[10:],
    }
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=len(text) + 100)
        for what, b in bad.items():
            assert e.upload_gzip(0, np.frombuffer(b, dtype=np.uint8), chunk=16384) is None, what
            with pytest.raises(N.KrispHipError):
                e.fetch_bases(0, 10)
        assert e.upload_gzip(0, np.frombuffer(raw, dtype=np.uint8), chunk=16384) is not None


def _gz_copies(case, tmp_path, **kw):
    paths = _paths(case, tmp_path)
    out = {}
    for fn, p in paths.items():
        opener = gzip.open if p.endswith(".gz") else open
        with opener(p, "rb") as f:
            data = f.read()
        if p.endswith(".gz"):
            out[fn] = p                 # (the golden files themselves: written by gzip)
        else:
            q = str(tmp_path / (fn.split(".")[0] + ".fa.gz"))
            open(q, "wb").write(_gzip(data, **kw))
            out[fn] = q
    return out


@pytest.mark.parametrize("name,flow", [("c1_25_1_2", "in_core"), ("c1_25_1_2", "batches"), ("c1_30_40_30", "in_core"),
                                       ("c1_32_60_32", "in_core")])
def test_plain_gzip_genomes_through_the_cli_on_the_device(name, flow, tmp_path, monkeypatch):
    """the golden genomes (plain gzip files) with the device inflate: the in-core, streaming and long-amplicon flows give
    the golden output byte for byte, the files' timings say device_inflate; with KRISP_DEVICE_INFLATE=0 the same"""
    from krisp_amd import fasta
    case = [c for c in FC if c["name"] == name][0]
    files = _gz_copies(case, tmp_path)
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_CHUNK", "4096")
    if flow == "batches":
        monkeypatch.setenv("KRISP_STREAM_BATCH", "2")
    aln = str(tmp_path / "a.txt")
    argv = [files[f] for f in case["ingroup"]] + (["--outgroup"] + [files[f] for f in case["outgroup"]] if case["outgroup"] else []) \
        + case.get("main_args", []) + ["--out_align", aln]
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        fasta.LAST_TIMINGS.clear()
        if "csv" in case:
            assert _run_main(argv) == case["csv"]
            assert open(aln).read() == case["align"]
        else:
            from krisp_amd import amplicon
            from krisp_amd import krisp_fasta as KF
            groups, _ = KF.find_regions([files[f] for f in case["ingroup"]], [files[f] for f in case["outgroup"]], case["L"],
                                        case["R"], _amplicon(case), omit_soft=case["omit_soft"])
            assert canon_equal(sorted(amplicon.merged_lines(groups)), case["filtered_canon"])
        tms = [fasta.LAST_TIMINGS[q] for q in files.values() if q in fasta.LAST_TIMINGS]
        assert tms and all(bool(t.get("device_inflate")) == (dev == "1") for t in tms), tms
        if dev == "1":
            assert all(t.get("device_inflate_s", 0) > 0 and t["chunks"] >= 1 for t in tms), tms


def test_a_damaged_gzip_file_gets_the_host_paths_verdict(tmp_path, monkeypatch):
    """damage of every kind: the device uploads nothing, the host inflate says what the file is, the same exception type
    with the device path on and off"""
    from krisp_amd import krisp_fasta as KF
    case = [c for c in FC if c["name"] == "c1_25_1_2"][0]
    paths = _paths(case, tmp_path)
    names = case["ingroup"] + case["outgroup"]
    good = [open(paths[fn], "rb").read() for fn in names]
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_CHUNK", "4096")
    raw = good[1]
    damages = {"flip": raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 0x55]) + raw[len(raw) // 2 + 1:],
               "truncated": raw[:len(raw) - 300], "crc": raw[:-8] + bytes([raw[-8] ^ 1]) + raw[-7:],
               "isize": raw[:-4] + struct.pack("<I", int.from_bytes(raw[-4:], "little") + 7), "garbage": raw + b"garbage"}
    for what, b in damages.items():
        files = []
        for i, data in enumerate(good):
            q = str(tmp_path / f"{what}{i}.fa.gz")
            open(q, "wb").write(b if i == 1 else data)
            files.append(q)
        seen = []
        for dev in ("1", "0"):
            monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
            with pytest.raises(Exception) as ei:
                KF.find_regions(files[:2], files[2:], 25, 2, 28)
            seen.append(type(ei.value).__name__)
        assert seen[0] == seen[1], (what, seen)


def test_synthetic_genome_set_on_both_routes(tmp_path, monkeypatch):
    """4 x 5 Mbp related genomes (krisp_amd.synth) as plain gzip files, many chunks each: the same groups through the
    device inflate and the host's"""
    from krisp_amd import amplicon, fasta, synth
    from krisp_amd import krisp_fasta as KF
    fam = synth.family(21, 2, 2, 5_000_000, records=3, mu=0.01, snp_every=5000)
    files = []
    for i, (_, _, t) in enumerate(fam):
        recs = t.tobytes().split(b"\n")
        text = b"".join(b">r%d\n" % j + b"\n".join(r[k:k + 60] for k in range(0, len(r), 60)) + b"\n" for j, r in enumerate(recs))
        q = str(tmp_path / f"g{i}.fa.gz")
        open(q, "wb").write(_gzip(text, level=6))
        files.append(q)
    flags = [f for _, f, _ in fam]
    ing = [q for q, f in zip(files, flags) if f]
    outg = [q for q, f in zip(files, flags) if not f]
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_CHUNK", "65536")
    res = []
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        fasta.LAST_TIMINGS.clear()
        groups, _ = KF.find_regions(ing, outg, 25, 2, 28)
        res.append(sorted(amplicon.merged_lines(groups)))
        if dev == "1":
            tms = [fasta.LAST_TIMINGS[q] for q in files]
            assert all(t.get("device_inflate") and t["chunks_joined"] >= 2 for t in tms), tms
    assert res[0] == res[1] and len(res[0]) > 0


def test_a_tight_hbm_budget_sends_the_scratch_to_the_host(N, tmp_path):
    """a budget that holds the genome's upload but not the gunzip scratch (2 bytes per byte of text): the device path
    declines with nothing uploaded, and ingest_on_device reads the file through the host inflate -- the same bases"""
    from krisp_amd import fasta
    text = _fasta(12, 3_000_000)
    raw = _gzip(text, level=6)
    with N.Engine() as e:
        e.set_params(25, 1, 2, max_bases=len(text))
        want = e.upload_text(0, np.frombuffer(text, dtype=np.uint8), False)
        wb = e.fetch_bases(0, want[0]).copy()
        need = e.mem_info()["used"]
    q = str(tmp_path / "g.fa.gz")
    open(q, "wb").write(raw)
    with N.Engine(hbm_budget=need + len(text) // 2) as e:
        e.set_params(25, 1, 2, max_bases=len(text))
        e.upload_text(0, np.frombuffer(text, dtype=np.uint8), False)       # (the genome's own buffers: what the budget holds)
        assert e.upload_gzip(0, np.frombuffer(raw, dtype=np.uint8), chunk=65536) is None
        assert "scratch" in e.last_gzip[3], e.last_gzip
        obj = fasta.GzipFile(q, np.frombuffer(raw, dtype=np.uint8), len(text), 65536)
        n, rna, special = fasta.ingest_on_device(e, 0, obj, False, 25, False)
        assert n == want[0] and np.array_equal(e.fetch_bases(0, n), wb)


@pytest.mark.parametrize("name,flow", [("c1_25_1_2", "in_core"), ("c1_25_1_2", "batches"), ("c1_30_40_30", "in_core")])
def test_a_file_of_two_members_gets_the_host_paths_output(name, flow, tmp_path, monkeypatch):
    """`cat a.fa.gz b.fa.gz` with the smaller member last: read_text hands it to the device (its last ISIZE word is all it
    says), the device declines the second member, the host's text is longer than the plan -- the run plans again with that
    file on the host and gives what the host route gives, in the in-core, streaming and long-amplicon flows"""
    from krisp_amd import fasta
    case = [c for c in FC if c["name"] == name][0]
    files = dict(_gz_copies(case, tmp_path))
    first = case["ingroup"][0]
    with gzip.open(files[first], "rb") as f:
        data = f.read()
    cut = data.rfind(b"\n", 0, len(data) * 3 // 5) + 1      # (60 / 40: the last member smaller, its ISIZE still plausible)
    os.makedirs(tmp_path / "two_members")
    q = str(tmp_path / "two_members" / (first.split(".")[0] + ".fa.gz"))       # (the file's name is its label in the output)
    open(q, "wb").write(_gzip(data[:cut], level=6) + _gzip(data[cut:], level=6))
    assert gzip.decompress(open(q, "rb").read()) == data
    files[first] = q
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_CHUNK", "4096")
    monkeypatch.delenv("KRISP_DEVICE_INFLATE", raising=False)
    assert isinstance(fasta.read_text(q)[0], fasta.GzipFile)
    if flow == "batches":
        monkeypatch.setenv("KRISP_STREAM_BATCH", "2")
    aln = str(tmp_path / "a.txt")
    argv = [files[f] for f in case["ingroup"]] + (["--outgroup"] + [files[f] for f in case["outgroup"]] if case["outgroup"] else []) \
        + case.get("main_args", []) + ["--out_align", aln]
    outs = []
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        fasta._GUNZIP_HOST.clear()
        fasta.LAST_TIMINGS.clear()
        outs.append((_run_main(argv), open(aln).read()))
        if dev == "1":
            assert fasta._file_key(q) in fasta._GUNZIP_HOST
            assert not fasta.LAST_TIMINGS[q].get("device_inflate")
            others = [fasta.LAST_TIMINGS[p] for p in files.values() if p != q]
            assert others and all(t.get("device_inflate") for t in others), others
    assert outs[0] == outs[1]
    if "csv" in case:
        assert outs[0] == (case["csv"], case["align"])
