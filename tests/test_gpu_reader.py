"""The device's reader (kr_genome_upload_text, csrc/k_text.inc) at the sizes where its parallel parts change shape, against
the plain Python reader (oracle/krisp_oracle.py: the reference's line handling with str.strip(), its RNA rule) -- not
against another implementation of the same byte rule.  The line scan k_tx_scan1/2/3 runs Gs = min(1024,
ceil(lines / 2048)) workgroups of 256 threads, `per` lines a thread: line counts at and across the steps of both, runs of
blank lines longer than a workgroup's share (a workgroup that leaves the record state alone), headers as the last line of
a thread's run and of a workgroup's; '\\r\\n' and lone '\\r' at the 4096-byte tiles of k_tx_starts_*; first lines longer
than k_tx_firstline's 16 KB step; lines placed on k_tx_copy's 16384-byte boundaries; the RNA verdict of k_tx_stats1/2 and
k_tx_finish with its first U and first T far apart; str.strip()'s white space (29 characters, 19 of them above U+007F)
throughout.  The largest texts go through the device inflate of BGZF files too, and BGZF members with spare bytes in
front of their trailers are refused as Python's gzip refuses them."""
import gzip
import io
import os
import struct
import zlib

import numpy as np
import pytest

from krisp_amd import fasta
from oracle import krisp_oracle as O

pytestmark = pytest.mark.gpu

WHITE = [chr(c) for c in range(0x110000) if chr(c).isspace()]
INLINE_WHITE = [w for w in WHITE if w not in "\n\r"]       # (white space that does not end a line in either mode)
MAXB = 80 << 20


@pytest.fixture(scope="module")
def E():
    from krisp_amd import _native
    with _native.Engine() as e:
        e.set_params(25, 1, 2, max_bases=MAXB)
        yield e


def reference(text, universal, one_shot):
    """text -> (bases, records, special characters, rna, fasta) through the oracle's reader: text mode (universal
    newlines) or binary lines split on '\\n', decoded; str.strip(); the reference's FASTA and RNA rules"""
    if universal:
        lines = list(io.TextIOWrapper(io.BytesIO(text), encoding="utf-8", newline=None))
    else:
        lines = [ln.decode() for ln in io.BytesIO(text)]
    recs = O.parse_records(lines, one_shot=one_shot)
    rna = bool(O.detect_rna(recs))
    bases = fasta.to_bases([r.encode() for r in recs], rna)
    return bases, len(recs), int((~fasta._PLAIN[bases]).sum()), rna, bool(lines) and ">" in lines[0]


def check(e, text, modes=((0, 0), (0, 1), (1, 0), (1, 1)), what=""):
    for universal, one_shot in modes:
        want, nrec, special, rna, fa = reference(text, universal, one_shot)
        n, grec, gspecial, grna, gfa = e.upload_text(0, np.frombuffer(text, dtype=np.uint8), universal, one_shot)
        got = e.fetch_bases(0, n)
        tag = (what, universal, one_shot)
        assert n == len(want), tag
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"{tag}: first difference at output byte {at}: {got[at:at + 40].tobytes()!r} against "
                                 f"{want[at:at + 40].tobytes()!r}")
        assert (grec, gspecial, bool(grna), bool(gfa)) == (nrec, special, rna, fa), tag


def scan_shape(nlines):
    """(Gs, per) of the device's line scan for `nlines` lines (h_ingest.inc)"""
    gs = max(1, min(1024, (nlines + 2047) // 2048))
    return gs, -(-nlines // (gs * 256))


def _vocab(rng, n):
    """n short lines of every kind: headers, sequence lines, blank and white-space-only lines, white space of every kind
    at their ends and inside"""
    def pad():
        return "".join(rng.choice(INLINE_WHITE) for _ in range(int(rng.choice([0, 0, 0, 1, 2]))))
    out = []
    for i in range(n):
        kind = i % 8
        if kind == 0:
            body = ">" + "".join(rng.choice(list("ab >") + INLINE_WHITE) for _ in range(int(rng.integers(0, 5))))
        elif kind == 1:
            body = ""
        else:
            body = "".join(rng.choice(list("ACGTACGTacgtNU>") + INLINE_WHITE[:2] + INLINE_WHITE[-2:])
                           for _ in range(int(rng.integers(0, 10))))
        out.append((pad() + body + pad()).encode())
    return out


def _lines(seed, nlines, newlines=(b"\n",), p_header=0.05, p_blank=0.2):
    """nlines lines drawn from a vocabulary (vectorised: up to millions), joined by the given newline flavours"""
    rng = np.random.default_rng(seed)
    voc = _vocab(rng, 64)
    heads = [v for i, v in enumerate(voc) if i % 8 == 0]
    blanks = [v for i, v in enumerate(voc) if i % 8 == 1] + [b"", b" ", "　".encode(), b"\t\x1c"]
    seqs = [v for i, v in enumerate(voc) if i % 8 > 1]
    u = rng.random(nlines)
    kind = np.where(u < p_header, 0, np.where(u < p_header + p_blank, 1, 2))
    pick = rng.integers(0, 1 << 30, size=nlines)
    pools = (heads, blanks, seqs)
    lines = [pools[k][p % len(pools[k])] for k, p in zip(kind.tolist(), pick.tolist())]
    if len(newlines) == 1:
        return lines, newlines[0].join(lines) + newlines[0]
    nl = rng.integers(0, len(newlines), size=nlines).tolist()
    return lines, b"".join(ln + newlines[k] for ln, k in zip(lines, nl))


@pytest.mark.parametrize("nlines", [2047, 2048, 2049, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 3 * (1 << 21) + 5])
def test_device_reader_line_counts_at_the_scan_steps(E, nlines):
    """line counts at and across the steps of the scan's workgroups (2048 lines each up to 2^21 lines) and of its lines a
    thread (8, then more once Gs stops at 1024), FASTA and not, the first line consumed and not"""
    _, text = _lines(nlines, nlines)
    assert text.count(b"\n") == nlines
    rest = text[text.index(b"\n"):]
    check(E, b">h" + rest, modes=((0, 1), (1, 0)), what="fasta")
    # (the same lines under a first line without '>': one record a line)
    check(E, b"x" + rest, modes=((0, 0), (1, 1)), what="plain")


def _planted(seed, nlines, newlines):
    """adversarial lines with planted structure where the scan's threads and workgroups meet"""
    lines, _ = _lines(seed, nlines, p_header=0.02, p_blank=0.3)
    lines[0] = b">first"
    _, per = scan_shape(nlines)
    run = 2 * 256 * per + 10                    # blank lines: at least one whole workgroup's share (wg_f = 0) inside
    blank = [b"", b" ", " ".encode(), b"\x0b\x1f", "\xa0　".encode()]
    n = len(lines)
    for j in range(per - 1, n, 7 * per):        # a header as the last line of a thread's run ...
        lines[j] = b">t"
    for j in range(256 * per - 1, n, 256 * per):    # ... and of a workgroup's
        lines[j] = b">w \xe2\x80\x83"
    a = n // 5                                  # header, a run of blank lines, a sequence line
    lines[a] = b">planted"
    lines[a + 1:a + 1 + run] = [blank[i % len(blank)] for i in range(run)]
    lines[a + 1 + run] = b"ACGT"
    b = (3 * n) // 5                            # sequence line, a run of blank lines, sequence line
    lines[b] = b"GGGG"
    lines[b + 1:b + 1 + run] = [blank[i % len(blank)] for i in range(run)]
    lines[b + 1 + run] = b"CCCC"
    assert len(lines) == n
    rng = np.random.default_rng(seed + 1)
    nl = rng.integers(0, len(newlines), size=n).tolist()
    return b"".join(ln + newlines[k] for ln, k in zip(lines, nl))


@pytest.mark.parametrize("nlines,newlines", [(100_000, (b"\n",)), (1_000_000, (b"\n",)),
                                             (400_000, (b"\n", b"\r\n", b"\r")), (3 * (1 << 21) // 2, (b"\n",))],
                         ids=["1e5", "1e6", "4e5_mixed_newlines", "3e6"])
def test_device_reader_on_planted_structure(E, nlines, newlines):
    """adversarial texts of 10^5 - 3 x 10^6 lines with whole workgroups of blank lines between a header and a sequence
    line and between two sequence lines, headers as the last line of thread runs and workgroups"""
    check(E, _planted(nlines, nlines, newlines), what=str(nlines))


def test_device_reader_on_carriage_returns_at_tile_edges(E):
    """'\\r\\n' with the '\\r' at offset 4095 of a 4096-byte tile, a lone '\\r' ending a tile, every newline flavour"""
    rng = np.random.default_rng(7)
    m = 600
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=4096 * m)].copy()
    t[np.arange(60, len(t), 61)] = ord("\n")
    for k in range(m - 1):
        p = 4096 * k + 4095
        if k % 3 == 0:
            t[p], t[p + 1] = ord("\r"), ord("\n")
        elif k % 3 == 1:
            t[p], t[p + 1] = ord("\r"), ord("A")
        else:
            t[p - 1], t[p] = ord("\r"), ord("\r")
        if k % 5 == 0:
            t[p - 3:p] = np.frombuffer(b">hh", dtype=np.uint8)
    text = b">h\n" + t.tobytes()[3:]
    check(E, text, what="tiles")
    check(E, text.replace(b"\n", b"\r\n"), what="crlf")
    check(E, text.replace(b"\n", b"\r"), what="cr")


def test_device_reader_on_long_first_lines(E):
    """a first line longer than 16 KB with '>' after byte 16384 (FASTA), the same without '>' (one record a line, the
    first consumed or not), a text without a newline"""
    body = b"ACGT" * 9000
    for text in (body[:20000] + b" >x\nACGT\n\n>h\nGG\r\nTT", body + b"\r\nAC\n GT \n", body, body[:17000] + b">",
                 b"A" * 16384 + b">\n" + body, b"A" * 16383 + b"\r\nx>\nCC"):
        check(E, text, what=text[-12:])


def test_device_reader_on_copy_boundaries(E):
    """lines whose output place is a multiple of k_tx_copy's 16384 bytes, empty and white-space-only lines on that place,
    a record separator just in front of it"""
    pieces = [b">a"]
    pieces += [b"ACGTACGT" * 8] * 255 + [b"ACGTACG" * 9]                     # 16383 bytes of record a
    pieces += [b"", b" \t", b">b", b"", "　".encode(), b"C" * 64]       # separator at 16383, record b at 16384
    for k in range(2, 40):
        pieces += [b"T" * 64] * 255 + [b"G" * 63 if k % 2 else b"G" * 64, b"", b" "]
        if k % 4 == 0:
            pieces += [b">c", b""]
    text = b"\n".join(pieces) + b"\n"
    check(E, text, what="fasta")
    plain = b"\n".join([b"x"] + [b"A" * 16383] * 4 + [b""] * 3 + [b"C" * 16383, b"", b"G" * 16384, b" "]) + b"\n"
    check(E, plain, what="plain")


def test_device_reader_rna_verdict_across_workgroups(E):
    """the RNA verdict with the first U and the first T in different workgroups of k_tx_stats1: a first record of 3 MB
    all U, then T records; the first U before the first T but in the record that holds that T; U in the last record
    only; no T at all"""
    u = b"\n".join([b"U" * 80] * 40_000)
    acg = b"\n".join([b"ACGACG" * 13] * 20_000)
    cases = [b">a\n" + u + b"\n>b\nACGT\n>c\nTTTT\n",
             b">a\nGGU\n" + acg + b"\n" + b"T" * 80 + b"\n>b\nUUUU\n",
             b">a\n" + acg + b"\n>b\n" + acg + b"\n>c\nAAU\n",
             b">a\n" + acg + b"\n>b\n" + u + b"\n",
             b"x\n" + acg + b"\n" + u + b"\n" + b"T\n"]
    for i, text in enumerate(cases):
        check(E, text, what=f"rna{i}")


def _bgzf(data, block=65280, spare=b""):
    """bytes -> a BGZF file as bgzip writes it; `spare`: bytes put between every member's deflate stream and its trailer
    (BSIZE counts them)"""
    out = []
    for ch in [data[i:i + block] for i in range(0, len(data), block)] + [b""]:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        cd = co.compress(ch) + co.flush() + (spare if ch else b"")
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cd) + 25) + cd
                   + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch)))
    return b"".join(out)


def test_device_reader_after_bgzf_inflate(E):
    """the largest adversarial texts as BGZF files: inflated and parsed on the device (binary lines) against the oracle's
    reading of the .gz file"""
    for text in (_planted(1_000_000, 1_000_000, (b"\n", b"\r\n")), _lines(5, 1 << 21)[1]):
        raw = _bgzf(text)
        assert gzip.decompress(raw) == text
        for one_shot in (0, 1):
            want, nrec, special, rna, fa = reference(text, 0, one_shot)
            got = E.upload_bgzf(0, np.frombuffer(raw, dtype=np.uint8), one_shot=one_shot)
            assert got is not None, E.last_bgzf
            assert got[:5] == (len(want), nrec, special, rna, fa)
            assert np.array_equal(E.fetch_bases(0, got[0]), want)


@pytest.mark.parametrize("spare", [1, 3])
def test_bgzf_members_with_spare_bytes_before_the_trailer_are_refused(E, spare, tmp_path, monkeypatch):
    """a member whose BSIZE leaves bytes between the end of its deflate stream and its trailer: Python's gzip reads the
    trailer right after the stream and fails; so does the device (nothing uploaded, the member named), and
    ingest_on_device then reaches the host path's verdict -- the same error as with the device inflate off"""
    text = _lines(11, 20_000)[1]
    good = _bgzf(text, block=30000)
    assert E.upload_bgzf(0, np.frombuffer(good, dtype=np.uint8)) is not None
    raw = _bgzf(text, block=30000, spare=b"\x00\x07\x03"[:spare])
    with pytest.raises(Exception):
        gzip.decompress(raw)
    assert E.upload_bgzf(0, np.frombuffer(raw, dtype=np.uint8)) is None
    assert "member" in E.last_bgzf[3]
    path = str(tmp_path / "spare.fa.gz")
    with open(path, "wb") as f:
        f.write(raw)
    monkeypatch.setenv("KRISP_DEVICE_INFLATE_MIN", "0")
    seen, routes = [], []
    for dev in ("1", "0"):
        monkeypatch.setenv("KRISP_DEVICE_INFLATE", dev)
        with pytest.raises(Exception) as ei:
            t, universal = fasta.read_text(path)
            routes.append(type(t).__name__)
            fasta.ingest_on_device(E, 0, t, universal, 28, False)
        seen.append((type(ei.value).__name__, str(ei.value)))
    assert routes[0] == "BgzfFile"
    assert seen[0] == seen[1], seen
