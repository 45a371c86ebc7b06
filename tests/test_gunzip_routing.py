"""Which route read_text gives a `.gz` file (no GPU needed): one plain gzip member with enough text is only READ -- a
GzipFile the device inflates (kr_genome_upload_gzip) --, BGZF keeps its own route, KRISP_DEVICE_INFLATE=0 the host's; the
ABI declares the new entry."""
import gzip
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from krisp_amd import fasta  # noqa: E402


def _member(text, flags=0, extra=b"", name=b"", comment=b"", pad=0):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(text) + co.flush()
    flg = flags | (4 if extra else 0) | (8 if name else 0) | (16 if comment else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00" * 5 + b"\x03"
    if extra:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\x00"
    if comment:
        head += comment + b"\x00"
    if flg & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)) + b"\x00" * pad


def _bgzf(text, block=20000):
    out = []
    for i in list(range(0, len(text), block)) + [None]:
        ch = b"" if i is None else text[i:i + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        cd = co.compress(ch) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cd) + 25) + cd
                   + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch)))
    return b"".join(out)


TEXT = b">r1 x\n" + b"\n".join(b"ACGTTGCAAC" * 6 for _ in range(3000)) + b"\n>r2\n" + b"N" * 5000 + b"ACGT" * 500 + b"\n"


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    monkeypatch.delenv("KRISP_DEVICE_INFLATE", raising=False)
    monkeypatch.delenv("KRISP_DEVICE_GUNZIP_CHUNK", raising=False)
    monkeypatch.setenv("KRISP_DEVICE_INFLATE_MIN", "0")
    return monkeypatch


@pytest.mark.parametrize("kw", [dict(), dict(name=b"genome.fa"), dict(extra=b"XY\x02\x00ab", name=b"g", comment=b"note"),
                                dict(flags=2, name=b"g"), dict(flags=2, comment=b"only a comment")],
                         ids=["bare", "fname", "fextra_fcomment", "fhcrc", "fhcrc_fcomment"])
def test_a_plain_gzip_file_is_handed_to_the_device(env, tmp_path, kw):
    raw = _member(TEXT, **kw)
    assert gzip.decompress(raw) == TEXT
    p = tmp_path / "g.fa.gz"
    p.write_bytes(raw)
    got, universal = fasta.read_text(str(p))
    assert isinstance(got, fasta.GzipFile) and not universal
    assert len(got) == len(TEXT) and bytes(got.raw) == raw and got.chunk is None
    assert fasta.LAST_TIMINGS[str(p)]["device_inflate"] is True
    assert bytes(got.inflate()) == gzip.decompress(raw)


def test_the_chunk_size_can_be_forced(env, tmp_path):
    env.setenv("KRISP_DEVICE_GUNZIP_CHUNK", "16384")
    p = tmp_path / "g.fa.gz"
    p.write_bytes(_member(TEXT))
    got, _ = fasta.read_text(str(p))
    assert isinstance(got, fasta.GzipFile) and got.chunk == 16384


def test_bgzf_keeps_its_route(env, tmp_path):
    p = tmp_path / "b.fa.gz"
    p.write_bytes(_bgzf(TEXT))
    got, _ = fasta.read_text(str(p))
    assert type(got) is fasta.BgzfFile and len(got) == len(TEXT)
    env.setenv("KRISP_DEVICE_INFLATE_MIN", str(len(TEXT) + 1))        # (below its own threshold: the host, not the gunzip)
    got, _ = fasta.read_text(str(p))
    assert isinstance(got, np.ndarray) and bytes(got) == TEXT


def test_device_inflate_off_restores_the_host_route(env, tmp_path):
    env.setenv("KRISP_DEVICE_INFLATE", "0")
    for name, raw in (("g.fa.gz", _member(TEXT)), ("b.fa.gz", _bgzf(TEXT))):
        p = tmp_path / name
        p.write_bytes(raw)
        got, universal = fasta.read_text(str(p))
        assert isinstance(got, np.ndarray) and bytes(got) == TEXT and not universal
        assert not fasta.LAST_TIMINGS[str(p)].get("device_inflate")


def test_the_threshold_and_files_the_trailer_does_not_describe(env, tmp_path):
    p = tmp_path / "g.fa.gz"
    p.write_bytes(_member(TEXT))
    env.setenv("KRISP_DEVICE_GUNZIP_MIN", str(len(TEXT) + 1))
    assert isinstance(fasta.read_text(str(p))[0], np.ndarray)
    env.setenv("KRISP_DEVICE_GUNZIP_MIN", str(len(TEXT)))
    assert isinstance(fasta.read_text(str(p))[0], fasta.GzipFile)
    env.setenv("KRISP_DEVICE_GUNZIP_MIN", "0")
    # zero padding behind the trailer: the last word is no ISIZE -- the host path, which reads the file
    p.write_bytes(_member(TEXT, pad=64))
    got, _ = fasta.read_text(str(p))
    assert isinstance(got, np.ndarray) and bytes(got) == TEXT
    # a second member: the last member's ISIZE routes it; the device declines it, inflate() gives both members' text
    p.write_bytes(_member(TEXT) + _member(TEXT))
    got, _ = fasta.read_text(str(p))
    assert isinstance(got, fasta.GzipFile) and len(got) == len(TEXT)
    assert bytes(got.inflate()) == TEXT + TEXT
    # not gzip at all
    p.write_bytes(b"hello, not a gzip file at all" * 10)
    with pytest.raises(Exception):
        fasta.read_text(str(p))


def test_the_abi_declares_and_binds_the_gunzip_entry():
    from krisp_amd import _native
    header = open(os.path.join(ROOT, "include", "krisp_hip.h")).read()
    assert re.search(r"int64_t kr_genome_upload_gzip\(kr_ctx\*, int id, const uint8_t\* file, size_t n, size_t chunk, int one_shot, "
                     r"int64_t\* stats\);", header)
    assert "kr_genome_upload_gzip" in {name for name, _, _ in _native.SYMBOLS}
    assert hasattr(_native.Engine, "upload_gzip")


def test_a_file_whose_text_proved_longer_goes_to_the_host(env, tmp_path):
    """a file the device declined with a text longer than its last ISIZE word (several members) is remembered: read_text
    gives it to the host from then on, and a changed file is looked at afresh"""
    p = tmp_path / "g.fa.gz"
    p.write_bytes(_member(TEXT) + _member(TEXT))
    assert isinstance(fasta.read_text(str(p))[0], fasta.GzipFile)
    fasta._GUNZIP_HOST.add(fasta._file_key(str(p)))
    try:
        got, _ = fasta.read_text(str(p))
        assert isinstance(got, np.ndarray) and bytes(got) == TEXT + TEXT
        p.write_bytes(_member(TEXT + b">x\nAC\n"))
        assert isinstance(fasta.read_text(str(p))[0], fasta.GzipFile)
    finally:
        fasta._GUNZIP_HOST.clear()
    err = fasta.GzipTextLonger(str(p), 10, 20)
    assert err.filename == str(p) and "20" in str(err)
