// h_inflate.inc -- part of krisp_hip.hip (one translation unit), HOST ONLY (no HIP call): a sequence file's bytes -> its
// text.  gzip members through libdeflate / zlib (BGZF members side by side), bz2 streams through libbz2 (the blocks of a
// stream found by their 48-bit marks, re-wrapped and decoded side by side), the file read itself (read_text).  Everything
// here parses untrusted files; it is split from h_ingest.inc (round 5) so that tests/native/asan_host.cpp builds exactly
// this code under AddressSanitizer + UBSan with stand-ins for the two pinned-memory calls (host_alloc, kr_host_free) and
// fuzzes it: truncated, bit-flipped and mark-spoofing inputs.  Needs before it: RawBuf's allocator (host_alloc /
// kr_host_free), g_last_error, h_pgzip.inc.
// ----------------------------------------------------------------------------
// ---- libdeflate through dlopen (the image ships the runtime library, not its header)
typedef void* (*ld_alloc_t)(void);
typedef void (*ld_free_t)(void*);
typedef int (*ld_gzip_ex_t)(void*, const void*, size_t, void*, size_t, size_t*, size_t*);
struct LibDeflate {
    ld_alloc_t alloc = nullptr;
    ld_free_t free_ = nullptr;
    ld_gzip_ex_t gzip_ex = nullptr;
    uint32_t (*crc32_)(uint32_t, const void*, size_t) = nullptr;
    bool ok = false;
    LibDeflate() {
        if (getenv("KRISP_NO_LIBDEFLATE")) return;
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libdeflate.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = (ld_alloc_t)dlsym(h, "libdeflate_alloc_decompressor");
        free_ = (ld_free_t)dlsym(h, "libdeflate_free_decompressor");
        gzip_ex = (ld_gzip_ex_t)dlsym(h, "libdeflate_gzip_decompress_ex");
        crc32_ = (uint32_t (*)(uint32_t, const void*, size_t))dlsym(h, "libdeflate_crc32");
        ok = alloc && free_ && gzip_ex;
    }
};
static LibDeflate& libdeflate() {
    static LibDeflate l;
    return l;
}

// a byte buffer that grows without zero-filling what it has not written yet and reports a failed allocation
// as `false` instead of throwing (nothing may unwind through the extern "C" boundary)
struct RawBuf {
    uint8_t* p = nullptr;
    size_t cap = 0, len = 0;
    bool pinned = false;        // allocate with host_alloc (pinned, device-visible): the block can be handed to the caller
    ~RawBuf() { drop(); }
    void drop() {
        if (p) { if (pinned) kr_host_free(p); else free(p); }
        p = nullptr;
        cap = 0;
    }
    bool reserve(size_t want) {
        if (want <= cap) return true;
        if (pinned) {
            uint8_t* q = (uint8_t*)host_alloc(want);
            if (!q) return false;
            if (len) memcpy(q, p, len);
            if (p) kr_host_free(p);
            p = q;
        } else {
            uint8_t* q = (uint8_t*)realloc(p, want);
            if (!q) return false;
            p = q;
        }
        cap = want;
        return true;
    }
    uint8_t* data() { return p; }
    size_t size() const { return cap; }
    bool resize(size_t want) { return reserve(want); }      // (the callers below only ever grow or trim the capacity they see)
    void swap(RawBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(len, o.len); std::swap(pinned, o.pinned); }
    uint8_t* detach() { uint8_t* q = p; p = nullptr; cap = len = 0; return q; }
};

// ---- host threads for independent pieces (BGZF members, bz2 streams, the chunks of a large gzip member): KRISP_INGEST_THREADS, default min(16, cores)
static unsigned ingest_threads() {
    const char* e = getenv("KRISP_INGEST_THREADS");
    unsigned n = e ? (unsigned)std::max(1, atoi(e)) : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    return std::min(n, 64u);
}

// all members of a gzip file -> out (grown as needed); returns 0 or a negative code
static int inflate_gzip(const uint8_t* in, size_t n, RawBuf& out, int64_t* members, int* used_libdeflate) {
    *members = 0;
    *used_libdeflate = 0;
    // ISIZE of the LAST member, modulo 2^32 -- a starting size only, and bounded by what deflate can expand to
    // (a truncated or hostile small file must not make us allocate 4 GiB before it is rejected)
    size_t guess = n >= 4 ? ((size_t)in[n - 4] | ((size_t)in[n - 3] << 8) | ((size_t)in[n - 2] << 16) | ((size_t)in[n - 1] << 24)) : 0;
    guess = std::min(guess, 64 * n + (1 << 16));
    if (guess < 4 * n) guess = 4 * n;
    if (!out.resize(guess + 64)) return KR_ERR_CAPACITY;
    size_t ipos = 0, opos = 0;
    // a large member goes to several threads first (h_pgzip.inc); "not done" there leaves it to the loops below.  1 taken,
    // 0 not, < 0 out of memory
    bool wide_ok = ingest_threads() > 1 && !(getenv("KRISP_PGZIP") && atoi(getenv("KRISP_PGZIP")) == 0);
    const char* emin = getenv("KRISP_PGZIP_MIN");
    const char* echunk = getenv("KRISP_PGZIP_CHUNK");
    const size_t wide_min = emin ? (size_t)std::max(0ll, atoll(emin)) : (size_t)8 << 20;
    // (chunks: four per thread, 1 .. 4 MB of compressed data -- a chunk's first megabyte or so of text decodes with markers)
    const size_t wide_chunk = echunk ? (size_t)std::max(65536ll, atoll(echunk))
                                     : std::min<size_t>((size_t)4 << 20, std::max<size_t>((size_t)1 << 20, n / (4 * (size_t)ingest_threads())));
    auto wide_member = [&]() -> int {
        if (!wide_ok || n - ipos < wide_min) return 0;
        PgzMember m;
        if (pgz_decode_member(in + ipos, n - ipos, ingest_threads(), wide_chunk, m) != 1) { wide_ok = false; return 0; }
        if (m.consumed * 2 < n - ipos) wide_ok = false;     // (many members: the chunks behind this one were decoded for nothing)
        out.len = opos;
        const double ta = pgz_now();
        if (opos + m.total + 64 > out.size() && !out.resize(opos + m.total + 64)) return KR_ERR_CAPACITY;
        const double tb = pgz_now();
        if (pgz_emit(m, out.data() + opos, ingest_threads(), libdeflate().ok ? libdeflate().crc32_ : nullptr) != 1) { wide_ok = false; return 0; }
        PGZ_SAY("pgzip: room for the text %.3f s, markers replaced + copied + checked %.3f s\n", tb - ta, pgz_now() - tb);
        ipos += m.consumed;
        opos += m.total;
        (*members)++;
        return 1;
    };
    LibDeflate& ld = libdeflate();
    if (ld.ok) {
        void* d = ld.alloc();
        if (d) {
            *used_libdeflate = 1;
            while (ipos < n) {
                // trailing zero padding after the last member is legal
                if (in[ipos] == 0) { ipos++; continue; }
                {
                    const int w = wide_member();
                    if (w < 0) { ld.free_(d); return w; }
                    if (w) continue;
                }
                size_t ain = 0, aout = 0;
                const int r = ld.gzip_ex(d, in + ipos, n - ipos, out.data() + opos, out.size() - opos, &ain, &aout);
                if (r == 3) {                      // LIBDEFLATE_INSUFFICIENT_SPACE: grow, retry this member
                    out.len = opos;               // (what is inflated so far moves with the buffer)
                    if (!out.resize(out.size() * 2 + (1 << 20))) { ld.free_(d); return KR_ERR_CAPACITY; }
                    continue;
                }
                if (r != 0) { ld.free_(d); return KR_ERR_PARAM; }
                ipos += ain;
                opos += aout;
                (*members)++;
            }
            ld.free_(d);
            out.len = opos;
            return KR_OK;
        }
    }
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return KR_ERR_PARAM;
    while (ipos < n) {
        if (in[ipos] == 0) { ipos++; continue; }
        {
            const int w = wide_member();
            if (w < 0) { inflateEnd(&zs); return w; }
            if (w) continue;
        }
        zs.next_in = (Bytef*)(in + ipos);
        zs.avail_in = (uInt)std::min<size_t>(n - ipos, 1u << 30);
        int r = Z_OK;
        while (r != Z_STREAM_END) {
            if (opos == out.size()) {
                out.len = opos;
                if (!out.resize(out.size() * 2 + (1 << 20))) { inflateEnd(&zs); return KR_ERR_CAPACITY; }
            }
            zs.next_out = out.data() + opos;
            zs.avail_out = (uInt)std::min<size_t>(out.size() - opos, 1u << 30);
            const uInt in_before = zs.avail_in;
            const size_t out_before = zs.avail_out;
            r = inflate(&zs, Z_NO_FLUSH);
            ipos += in_before - zs.avail_in;
            opos += out_before - zs.avail_out;
            if (r != Z_OK && r != Z_STREAM_END) { inflateEnd(&zs); return KR_ERR_PARAM; }
            if (zs.avail_in == 0 && r != Z_STREAM_END) {
                if (ipos >= n) { inflateEnd(&zs); return KR_ERR_PARAM; }     // truncated
                zs.next_in = (Bytef*)(in + ipos);
                zs.avail_in = (uInt)std::min<size_t>(n - ipos, 1u << 30);
            }
        }
        (*members)++;
        inflateReset(&zs);
    }
    inflateEnd(&zs);
    out.len = opos;
    return KR_OK;
}

#ifndef KR_SPAWN_DEFINED
#define KR_SPAWN_DEFINED
// start a host thread; false (nothing started) when the system has none to give (std::system_error: EAGAIN under a
// container's pid / thread limit).  The callers then do that thread's share themselves -- nothing may unwind through the
// extern "C" boundary, and a vector of joinable threads must not be destroyed by an exception (ADVICE r4).
extern "C++" {
template <class... A>
static bool kr_spawn(std::vector<std::thread>& th, A&&... a) {
    try {
        th.emplace_back(std::forward<A>(a)...);
        return true;
    } catch (const std::system_error&) {
        return false;
    } catch (const std::bad_alloc&) {
        return false;
    }
}
}   // extern "C++"
#endif
// fn(piece) for every piece in [0, n), on up to ingest_threads() threads; false when any call returned false
extern "C++" {
template <class F>
static bool parallel_pieces(size_t n, F fn) {
    const unsigned nt = (unsigned)std::min<size_t>(ingest_threads(), n);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++)
            if (!fn(i)) return false;
        return true;
    }
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    auto worker = [&]() {
        for (size_t i; ok.load(std::memory_order_relaxed) && (i = next.fetch_add(1)) < n;)
            if (!fn(i)) ok = false;
    };
    for (unsigned t = 0; t < nt; t++)
        if (!kr_spawn(th, worker)) break;           // (no more threads to be had: the ones started -- or this one -- take the pieces)
    if (th.size() < nt) worker();
    for (auto& x : th) x.join();
    return ok;
}
}   // extern "C++"

// ---- BGZF (bgzip; SAM spec 4.1): a gzip file whose members carry their own compressed length (extra subfield 'B' 'C',
// BSIZE = member length - 1) and hold <= 64 KiB each: the members are found by walking the headers, their output places
// by adding up the ISIZE words, and they inflate side by side.  Returns 1 done, 0 not a BGZF file (the caller inflates
// member by member), < 0 error.
static int inflate_bgzf(const uint8_t* in, size_t n, RawBuf& out, int64_t* members, int* used_libdeflate) {
    struct Mem { size_t at, len, oat; u32 isize; };
    std::vector<Mem> mem;
    size_t pos = 0, total = 0;
    while (pos < n) {
        if (n - pos < 28 || in[pos] != 0x1f || in[pos + 1] != 0x8b || in[pos + 2] != 8 || !(in[pos + 3] & 4)) return 0;
        const size_t xlen = in[pos + 10] | ((size_t)in[pos + 11] << 8);
        if (pos + 12 + xlen > n) return 0;
        size_t bsize = 0;
        for (size_t x = pos + 12; x + 4 <= pos + 12 + xlen;) {
            const size_t slen = in[x + 2] | ((size_t)in[x + 3] << 8);
            if (in[x] == 'B' && in[x + 1] == 'C' && slen == 2 && x + 6 <= pos + 12 + xlen) bsize = (in[x + 4] | ((size_t)in[x + 5] << 8)) + 1;
            x += 4 + slen;
        }
        if (bsize < 26 || pos + bsize > n) return 0;
        const uint8_t* t = in + pos + bsize - 4;
        const u32 isize = (u32)t[0] | ((u32)t[1] << 8) | ((u32)t[2] << 16) | ((u32)t[3] << 24);
        if (isize > (1u << 16)) return 0;
        mem.push_back(Mem{pos, bsize, total, isize});
        total += isize;
        pos += bsize;
    }
    if (mem.size() < 2) return 0;
    if (!out.resize(total + 64)) return KR_ERR_CAPACITY;
    LibDeflate& ld = libdeflate();
    const size_t per = 256;                     // members per piece (<= 16 MiB of text)
    const size_t npieces = (mem.size() + per - 1) / per;
    uint8_t* dst = out.data();
    const bool ok = parallel_pieces(npieces, [&](size_t pc) {
        const size_t m0 = pc * per, m1 = std::min(mem.size(), m0 + per);
        void* d = ld.ok ? ld.alloc() : nullptr;
        bool good = true;
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (!d && inflateInit2(&zs, 15 + 16) != Z_OK) return false;
        for (size_t m = m0; m < m1 && good; m++) {
            const Mem& M = mem[m];
            if (d) {
                size_t ain = 0, aout = 0;
                good = ld.gzip_ex(d, in + M.at, M.len, dst + M.oat, M.isize, &ain, &aout) == 0 && aout == M.isize && ain == M.len;
            } else {
                zs.next_in = (Bytef*)(in + M.at);
                zs.avail_in = (uInt)M.len;
                zs.next_out = dst + M.oat;
                zs.avail_out = M.isize;
                good = inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.avail_out == 0 && zs.avail_in == 0;
                inflateReset(&zs);
            }
        }
        if (d) ld.free_(d); else inflateEnd(&zs);
        return good;
    });
    if (!ok) return KR_ERR_PARAM;
    *members = (int64_t)mem.size();
    *used_libdeflate = ld.ok ? 1 : 0;
    out.len = total;
    return 1;
}

// ---- bz2: libbz2 through dlopen (the image ships the runtime library, not its header)
struct KrBzStream {                 // bz_stream of bzlib.h 1.0.x
    char* next_in; unsigned avail_in, total_in_lo32, total_in_hi32;
    char* next_out; unsigned avail_out, total_out_lo32, total_out_hi32;
    void* state;
    void* (*bzalloc)(void*, int, int);
    void (*bzfree)(void*, void*);
    void* opaque;
};
typedef int (*bz_init_t)(KrBzStream*, int, int);
typedef int (*bz_run_t)(KrBzStream*);
struct LibBz2 {
    bz_init_t init = nullptr;
    bz_run_t run = nullptr, end = nullptr;
    bool ok = false;
    LibBz2() {
        if (getenv("KRISP_NO_LIBBZ2")) return;
        void* h = dlopen("libbz2.so.1.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libbz2.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libbz2.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        init = (bz_init_t)dlsym(h, "BZ2_bzDecompressInit");
        run = (bz_run_t)dlsym(h, "BZ2_bzDecompress");
        end = (bz_run_t)dlsym(h, "BZ2_bzDecompressEnd");
        ok = init && run && end;
    }
};
static LibBz2& libbz2() {
    static LibBz2 l;
    return l;
}
// what stands at in[pos]?  1: a bzip2 stream ("BZh" + level, then the 48 bits of a block or -- an empty stream -- of the
// end); -1: the beginning of one, cut off by the end of the file (Python: "Compressed file ended before the end-of-stream
// marker was reached"); 0: no stream
static int bz_stream_at(const uint8_t* in, size_t n, size_t pos) {
    static const uint8_t blk[6] = {0x31, 0x41, 0x59, 0x26, 0x53, 0x59}, fin[6] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90};
    bool isb = true, isf = true;
    for (size_t k = 0; k < 10; k++) {
        if (pos + k >= n) return -1;                        // every byte there is fits a header
        const uint8_t c = in[pos + k];
        if (k < 3) { if (c != "BZh"[k]) return 0; }
        else if (k == 3) { if (c < '1' || c > '9') return 0; }
        else {
            isb = isb && c == blk[k - 4];
            isf = isf && c == fin[k - 4];
            if (!isb && !isf) return 0;
        }
    }
    return 1;
}
// the streams of in[0, n) one after the other into `out` (appended at out.len).  As Python's bz2 module reads a file
// (the reference reads .bz2 through fileinput.hook_compressed -> bz2.open; _compression.DecompressReader): the FIRST stream
// must be one; behind a complete stream, bytes that do not start another stream -- zeros, text, anything -- end the data
// and are ignored, with whatever follows them (ADVICE r4: `stream + "\0\0" + stream` is the first stream's text there,
// `stream + "XYZ"` is no error); a stream that starts and is cut or damaged is an error.
static int bunzip_range(const uint8_t* in, size_t n, RawBuf& out, int64_t* streams) {
    LibBz2& bz = libbz2();
    size_t ipos = 0;
    while (ipos < n) {
        if (*streams > 0) {
            const int at = bz_stream_at(in, n, ipos);
            if (at == 0) break;                                          // (trailing data behind a stream: ignored)
            if (at < 0) return KR_ERR_PARAM;                             // (a stream begins and the file ends)
        }
        KrBzStream zs;
        memset(&zs, 0, sizeof zs);
        if (bz.init(&zs, 0, 0) != 0) return KR_ERR_CAPACITY;
        int r = 0;
        while (r != 4 /* BZ_STREAM_END */) {
            if (out.cap - out.len < (1u << 16) && !out.reserve(out.cap * 2 + (1 << 20))) { bz.end(&zs); return KR_ERR_CAPACITY; }
            zs.next_in = (char*)(in + ipos);
            zs.avail_in = (unsigned)std::min<size_t>(n - ipos, 1u << 30);
            zs.next_out = (char*)out.p + out.len;
            zs.avail_out = (unsigned)std::min<size_t>(out.cap - out.len, 1u << 30);
            const unsigned in_before = zs.avail_in, out_before = zs.avail_out;
            r = bz.run(&zs);
            ipos += in_before - zs.avail_in;
            out.len += out_before - zs.avail_out;
            if (r != 0 /* BZ_OK */ && r != 4) { bz.end(&zs); return KR_ERR_PARAM; }
            if (r == 0 && ipos >= n && zs.avail_out != 0) { bz.end(&zs); return KR_ERR_PARAM; }     // truncated
        }
        bz.end(&zs);
        (*streams)++;
    }
    return KR_OK;
}
// ---- bz2 block by block.  A bzip2 stream is a chain of blocks (<= 900 kB of text each) that decode independently of
// each other and begin with 48 bits no compressor makes up by chance, 0x314159265359, on ANY bit; the stream ends with
// 0x177245385090 and the combined checksum of its blocks.  So: find both patterns on every bit of the file (host
// threads, a table look-up per byte), walk the headers to check that the patterns are the file's structure (stream header,
// blocks back to back, end mark, checksum, next stream on the next byte), wrap every block into a stream of its own
// ("BZh9", the block's bits moved to the byte boundary, the end mark, the block's checksum as the stream's) and let
// libbz2 decode the blocks side by side; the streams' combined checksums are checked from the blocks' own.  Anything that
// does not fit (a pattern inside compressed data: one in 2^48 positions; a damaged file) sends the file through the
// sequential decoder, whose verdict stands.
#define BZ_BLOCK_MAGIC 0x314159265359ull
#define BZ_END_MAGIC 0x177245385090ull
struct BzMark { size_t bit; int end; };
static void bz_find_marks(const uint8_t* in, size_t n, std::vector<BzMark>& marks) {
    // cand[k][b]: the (pattern, shift) pairs -- bit 8 * pattern + shift -- whose byte k + 1 is b (the bytes that lie
    // fully inside the 48 bits whatever the shift: bytes 1 .. 5 of the seven the pattern touches)
    static unsigned short cand[3][256];
    static std::once_flag once;
    std::call_once(once, []() {
        memset(cand, 0, sizeof cand);
        for (int pt = 0; pt < 2; pt++)
            for (int sh = 0; sh < 8; sh++) {
                const unsigned __int128 v = (unsigned __int128)(pt ? BZ_END_MAGIC : BZ_BLOCK_MAGIC) << (80 - 48 - sh);      // in 80 bits = 10 bytes, MSB first
                for (int k = 0; k < 3; k++) cand[k][(unsigned)(v >> (80 - 8 * (k + 2))) & 0xFF] |= (unsigned short)(1u << (8 * pt + sh));
            }
    });
    const size_t piece = (size_t)1 << 20;
    const size_t np = (n + piece - 1) / piece;
    std::vector<std::vector<BzMark>> found(np);
    (void)parallel_pieces(np, [&](size_t pc) {
        const size_t a = pc * piece, b = std::min(n, a + piece);
        for (size_t i = a; i < b && i + 7 <= n; i++) {
            unsigned m = cand[0][in[i + 1]] & cand[1][in[i + 2]] & cand[2][in[i + 3]];
            while (m) {
                const int bit = __builtin_ctz(m);
                m &= m - 1;
                const int pt = bit >> 3, sh = bit & 7;
                unsigned __int128 w = 0;
                for (int k = 0; k < 7; k++) w = (w << 8) | in[i + k];           // 56 bits
                if ((uint64_t)((w >> (8 - sh)) & 0xFFFFFFFFFFFFull) == (pt ? BZ_END_MAGIC : BZ_BLOCK_MAGIC)) found[pc].push_back(BzMark{i * 8 + (size_t)sh, pt});
            }
        }
        return true;
    });
    marks.clear();
    for (auto& f : found) marks.insert(marks.end(), f.begin(), f.end());
    std::sort(marks.begin(), marks.end(), [](const BzMark& x, const BzMark& y) { return x.bit < y.bit; });
}
static inline uint32_t bz_bits32(const uint8_t* in, size_t n, size_t bit) {       // 32 bits from `bit`, MSB first (0 behind the end)
    uint64_t w = 0;
    for (int k = 0; k < 5; k++) w = (w << 8) | ((bit >> 3) + (size_t)k < n ? in[(bit >> 3) + (size_t)k] : 0);
    return (uint32_t)(w >> (8 - (bit & 7)));
}
// 1 done, 0 not (the caller decodes sequentially), < 0 out of memory
static int inflate_bz2_blocks(const uint8_t* in, size_t n, RawBuf& out, int64_t* streams) {
    std::vector<BzMark> marks;
    bz_find_marks(in, n, marks);
    struct Blk { size_t a, b; uint32_t crc; };
    std::vector<Blk> blk;
    size_t byte = 0, mi = 0;
    int64_t ns = 0;
    while (byte < n) {
        if (ns > 0) {
            const int at = bz_stream_at(in, n, byte);
            if (at == 0) break;                                         // (trailing data behind a stream: ignored, as bunzip_range does)
            if (at < 0) return 0;                                       // (the sequential decoder says what that is)
        }
        if (byte + 4 > n || in[byte] != 'B' || in[byte + 1] != 'Z' || in[byte + 2] != 'h' || in[byte + 3] < '1' || in[byte + 3] > '9') return 0;
        size_t cur = (byte + 4) * 8;
        uint32_t combined = 0;
        for (;;) {
            while (mi < marks.size() && marks[mi].bit < cur) mi++;
            if (mi == marks.size() || marks[mi].bit != cur) return 0;
            if (marks[mi].end) {
                if (cur + 80 > n * 8 || bz_bits32(in, n, cur + 48) != combined) return 0;
                byte = (cur + 80 + 7) >> 3;
                ns++;
                break;
            }
            if (mi + 1 == marks.size()) return 0;           // a block with nothing behind it
            const uint32_t crc = bz_bits32(in, n, cur + 48);
            combined = ((combined << 1) | (combined >> 31)) ^ crc;
            blk.push_back(Blk{cur, marks[mi + 1].bit, crc});
            cur = marks[mi + 1].bit;
        }
    }
    if (blk.size() < 2) return 0;
    if (getenv("KRISP_PBZ2_DEBUG")) fprintf(stderr, "pbz2: %zu blocks in %lld stream(s), %zu marks\n", blk.size(), (long long)ns, marks.size());
    std::vector<RawBuf> part(blk.size());
    const bool ok = parallel_pieces(blk.size(), [&](size_t i) {
        const Blk& B = blk[i];
        const size_t nbits = B.b - B.a;
        std::vector<uint8_t> ms;
        try { ms.assign(4 + (nbits + 80 + 7) / 8 + 8, 0); } catch (...) { return false; }
        ms[0] = 'B'; ms[1] = 'Z'; ms[2] = 'h'; ms[3] = '9';
        const size_t s0 = B.a >> 3;
        const int sh = (int)(B.a & 7);
        const size_t whole = nbits >> 3;
        for (size_t k = 0; k < whole + 1; k++) {           // (one byte more than whole: its leading bits are the block's last)
            const unsigned hi = s0 + k < n ? in[s0 + k] : 0, lo = s0 + k + 1 < n ? in[s0 + k + 1] : 0;
            ms[4 + k] = (uint8_t)(((hi << 8 | lo) >> (8 - sh)) & 0xFF);
        }
        // the end mark and the checksum behind the block's last bit
        size_t at = 4 * 8 + nbits;
        ms[at >> 3] &= (uint8_t)(0xFF00u >> (at & 7));      // (keep the block's bits of that byte only)
        for (size_t k = (at >> 3) + 1; k < ms.size(); k++) ms[k] = 0;
        auto put = [&](uint64_t v, int bits) {
            for (int q = bits - 1; q >= 0; q--, at++)
                if ((v >> q) & 1) ms[at >> 3] |= (uint8_t)(0x80u >> (at & 7));
        };
        put(BZ_END_MAGIC, 48);
        put(B.crc, 32);
        const size_t len = (at + 7) >> 3;
        int64_t one = 0;
        if (!part[i].reserve(nbits / 8 * 5 + (1 << 16))) return false;
        return bunzip_range(ms.data(), len, part[i], &one) == KR_OK && one == 1;
    });
    if (!ok) {
        if (getenv("KRISP_PBZ2_DEBUG")) fprintf(stderr, "pbz2: a block did not decode\n");
        return 0;
    }
    size_t total = 0;
    std::vector<size_t> at(part.size());
    for (size_t i = 0; i < part.size(); i++) { at[i] = total; total += part[i].len; }
    if (!out.resize(total + 64)) return KR_ERR_CAPACITY;
    uint8_t* dst = out.data();
    (void)parallel_pieces(part.size(), [&](size_t i) { if (part[i].len) memcpy(dst + at[i], part[i].p, part[i].len); return true; });
    out.len = total;
    *streams = ns;
    return 1;
}

// all streams of a bz2 file -> out: block by block on the host threads when there are several, else (and whenever the
// block route declines) stream after stream through libbz2
static int inflate_bz2(const uint8_t* in, size_t n, RawBuf& out, int64_t* streams) {
    *streams = 0;
    if (!libbz2().ok) return KR_ERR_HOST;
    if (ingest_threads() > 1 && !(getenv("KRISP_PBZ2") && atoi(getenv("KRISP_PBZ2")) == 0)) {
        const int r = inflate_bz2_blocks(in, n, out, streams);
        if (r) return r < 0 ? r : KR_OK;
        *streams = 0;
    }
    if (!out.reserve(n * 5 + (1 << 16))) return KR_ERR_CAPACITY;
    out.len = 0;
    return bunzip_range(in, n, out, streams);
}

static inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// read `path` and inflate it (every gzip member): the file's text in `text` (len bytes).  times in microseconds.
// (text.pinned set by the caller: the text then lands in pinned memory directly -- inflated into it, or read into it)
static int64_t read_text(const char* path, RawBuf& text, bool* gz_out, double* t_read, double* t_inflate, int64_t* members,
                         int* used_ld) {
    const size_t plen = strlen(path);
    const bool gz = plen > 3 && strcmp(path + plen - 3, ".gz") == 0;
    const bool bz = plen > 4 && strcmp(path + plen - 4, ".bz2") == 0;
    *gz_out = gz || bz;                         // (a compressed stream is split on '\n' only: krisp_amd/fasta.py)
    if (bz && !libbz2().ok) return KR_ERR_HOST;
    const double t0 = now_us();
    FILE* f = fopen(path, "rb");
    if (!f) {
        g_last_error = std::string("cannot open ") + path + ": " + strerror(errno);
        return KR_ERR_PARAM;
    }
    RawBuf raw;
    raw.pinned = text.pinned && !gz && !bz;     // (a plain file is read straight into the block it is handed over in)
    {
        struct stat sb;
        size_t want = 1 << 16;
        if (fstat(fileno(f), &sb) == 0 && sb.st_size > 0) want = (size_t)sb.st_size + 1;
        for (;;) {
            if (!raw.reserve(std::max(want, raw.len + (1 << 16)))) {
                fclose(f);
                g_last_error = std::string("out of memory reading ") + path;
                return KR_ERR_CAPACITY;
            }
            const size_t r = fread(raw.p + raw.len, 1, raw.cap - raw.len, f);
            raw.len += r;
            if (r == 0) break;
            if (raw.len == raw.cap) want = raw.cap * 2;
        }
        fclose(f);
    }
    const double t1 = now_us();
    *members = 0;
    *used_ld = 0;
    if (gz) {
        int rc = inflate_bgzf(raw.p, raw.len, text, members, used_ld);
        if (rc == 0) rc = inflate_gzip(raw.p, raw.len, text, members, used_ld);
        else if (rc == 1) rc = KR_OK;
        if (rc) {
            g_last_error = (rc == KR_ERR_CAPACITY ? std::string("out of memory inflating ") : std::string("not a valid gzip file: ")) + path;
            return rc;
        }
    } else if (bz) {
        const int rc = inflate_bz2(raw.p, raw.len, text, members);
        if (rc) {
            g_last_error = (rc == KR_ERR_CAPACITY ? std::string("out of memory inflating ") : std::string("not a valid bz2 file: ")) + path;
            return rc;
        }
    } else {
        text.swap(raw);
    }
    *t_read = t1 - t0;
    *t_inflate = now_us() - t1;
    return (int64_t)text.len;
}

