"""kr_genome_upload_gzip alone: a FASTA text of `mb` MB as ONE plain gzip member (deflate level `level`; made side by side
as pigz makes it: pieces of 16 MB, each primed with the 32 KB in front of it, one stream) -> the device inflate + parse,
for every chunk size asked for (0: the library's choice), three times each; prints the upload's wall time, the inflate
inflate's own wall time (k_gz_find .. k_gz_crc and the host steps between them), chunks, chunks joined, the longest run of windows -- and the host path for the same
file (kr_read_file: the chunked inflate on the host threads, then kr_genome_upload_text).  Under
`rocprofv3 --kernel-trace --stats` the kernels show separately.  KRISP_GZ_LANES: active lanes per wave of k_gz_decode.
    python tools/gunzip_check.py [mb, default 1024] [level, default 1] [chunk[,chunk...], default 0]     (on the GPU box)"""
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from krisp_amd import _native  # noqa: E402

mb = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
level = int(sys.argv[2]) if len(sys.argv) > 2 else 1
chunks = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0]
rng = np.random.default_rng(1)
n = mb << 20
t0 = time.time()
body = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n, dtype=np.uint8)]
body[80::81] = 10
body[n // 3:n // 3 + (n >> 6)] = ord("N")           # (an N run of 1/64 of the text: a chunk that inflates 1000:1)
text = b">chr1 synthetic\n" + body.tobytes()
del body
PIECE = 16 << 20


def piece(i):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, *([text[i - 32768:i]] if i else []))
    last = i + PIECE >= len(text)
    return co.compress(text[i:i + PIECE]) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)


with ThreadPoolExecutor(16) as pool:
    deflate = b"".join(pool.map(piece, range(0, len(text), PIECE)))
raw = b"\x1f\x8b\x08\x08\x00\x00\x00\x00\x00\x03synthetic.fa\x00" + deflate + \
    (zlib.crc32(text) & 0xFFFFFFFF).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")
del deflate
arr = np.frombuffer(raw, dtype=np.uint8)
print(f"{len(text) / 1e6:.0f} MB of text, {len(raw) / 1e6:.0f} MB as one gzip member (level {level}), made in "
      f"{time.time() - t0:.0f} s; KRISP_GZ_LANES={os.environ.get('KRISP_GZ_LANES', '64')}", flush=True)
with _native.Engine() as eng:
    eng.set_params(25, 1, 2, max_bases=len(text))
    for ch in chunks:
        for rep in range(3):
            t1 = time.time()
            got = eng.upload_gzip(0, arr, chunk=ch)
            t2 = time.time()
            assert got is not None, eng.last_gzip
            print(f"chunk {ch or 'auto'} run {rep}: {got[0]:,} bases, {got[5]} chunks, {got[7]} joined, longest window run {got[8]}; "
                  f"upload + inflate + parse {t2 - t1:.3f} s, inflate wall time {got[6] / 1e3:.1f} ms = "
                  f"{len(text) / max(got[6], 1) / 1e3:.2f} GB/s of text", flush=True)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "synthetic.fa.gz")
        with open(path, "wb") as f:
            f.write(raw)
        for rep in range(2):
            t1 = time.time()
            host, universal, tm = _native.read_file(path)
            t2 = time.time()
            eng.upload_text(1, host, universal)
            t3 = time.time()
            print(f"host path run {rep}: read + inflate (host threads) {t2 - t1:.3f} s (inflate {tm.get('inflate_s', 0):.3f} s), "
                  f"upload + parse {t3 - t2:.3f} s, together {t3 - t1:.3f} s", flush=True)
            del host
