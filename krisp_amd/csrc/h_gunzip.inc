// h_gunzip.inc -- part of krisp_hip.hip (one translation unit): ONE plain gzip member inflated ON THE DEVICE (k_gunzip.inc),
// then parsed there as kr_genome_upload_bgzf does it.  The host parses the gzip header, lines the chunks up between the
// two decode passes, draws the runs of the window kernel, and checks the trailer: CRC-32 (the segments' CRCs combined)
// and ISIZE.  Anything the device path does not take -- BGZF, a second member, data behind the trailer, >= 2^32 bytes, a
// chunk that does not decode, a join that does not meet, a checksum or length that differs, scratch that does not fit --
// returns KR_ERR_HOST with nothing uploaded: the caller reads the file through kr_read_file, whose verdict stands.
// ----------------------------------------------------------------------------
extern "C++" {
// CRC-32 algebra over GF(2) (the polynomial arithmetic zlib's crc32_combine rests on): a * b mod P, x^(2^k) mod P, and the
// CRC of A followed by B from crc(A), crc(B) and |B| as crc(A) * x^(8|B|) + crc(B)
static u32 gz_mulmodp(u32 a, u32 b) {
    u32 m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
static u32 gz_x8nmodp(u64 n) {          // x^(8 n) mod P
    u32 sq = 1u << 30;                  // x^1
    for (int k = 0; k < 3; k++) sq = gz_mulmodp(sq, sq);        // x^8
    u32 p = 1u << 31;                   // x^0
    while (n) {
        if (n & 1) p = gz_mulmodp(sq, p);
        sq = gz_mulmodp(sq, sq);
        n >>= 1;
    }
    return p;
}

// scratch of one call, given back when the call returns (ADVICE r6: kept, it pushed the streaming flow into smaller batches)
struct GzScratch {
    kr_ctx* c;
    DevBuf in, start, res, list, sym, win, chain, crc, bad;
    void drop() {
        DevBuf* all[] = {&in, &start, &res, &list, &sym, &win, &chain, &crc, &bad};
        bool any = false;
        for (DevBuf* b : all) any = any || b->p;
        if (any) (void)hipDeviceSynchronize();
        for (DevBuf* b : all) release(c, *b);
    }
    ~GzScratch() { drop(); }
};
}   // extern "C++"

// the length of the gzip header at file[0..n) (FEXTRA, FNAME, FCOMMENT, FHCRC -- the header CRC is skipped unchecked, as
// Python's gzip and libdeflate do), 0: not a gzip header; *bgzf: the extra field holds a BGZF 'BC' subfield
static size_t gz_header_len(const uint8_t* in, size_t n, bool* bgzf) {
    *bgzf = false;
    if (n < 18 || in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || (in[3] & 0xE0)) return 0;
    const int flg = in[3];
    size_t p = 10;
    if (flg & 4) {
        if (p + 2 > n) return 0;
        const size_t xlen = in[p] | ((size_t)in[p + 1] << 8);
        if (p + 2 + xlen > n) return 0;
        for (size_t x = p + 2; x + 4 <= p + 2 + xlen;) {
            const size_t slen = in[x + 2] | ((size_t)in[x + 3] << 8);
            if (in[x] == 'B' && in[x + 1] == 'C') *bgzf = true;
            x += 4 + slen;
        }
        p += 2 + xlen;
    }
    if (flg & 8) { while (p < n && in[p]) p++; p++; }
    if (flg & 16) { while (p < n && in[p]) p++; p++; }
    if (flg & 2) p += 2;
    return p + 8 <= n ? p : 0;
}

static size_t gz_default_chunk(size_t dn) {
    const char* e = getenv("KRISP_GZ_CHUNK");
    if (e && atoll(e) > 0) return (size_t)atoll(e);
    // (profiles/r07/gunzip_check_1024.log, 1 GB of text at level 1: 256 KB chunks 0.55 GB/s of text, 64 KB 0.49 -- their
    // windows wait on each other longer --, 1 MB 0.22 -- too few lanes)
    (void)dn;
    return (size_t)256 << 10;
}

int64_t kr_genome_upload_gzip(kr_ctx* c, int id, const uint8_t* file, size_t n, size_t chunk, int one_shot, int64_t* stats) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (!file && n) return fail(c, KR_ERR_PARAM, "kr_genome_upload_gzip: null file");
    if (stats) for (int i = 0; i < 8; i++) stats[i] = 0;
    if (n >= (1ull << 32) - 64) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: files of >= 2^32 bytes go through the host");
    bool bgzf = false;
    const size_t hlen = gz_header_len(file, n, &bgzf);
    if (!hlen) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: not a gzip header");
    if (bgzf) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: a BGZF file (kr_genome_upload_bgzf)");
    const uint8_t* const data = file + hlen;
    const u32 dn = (u32)(n - hlen);
    const size_t C = std::max<size_t>(chunk ? chunk : gz_default_chunk(dn), 4096);
    const u32 nch = (u32)std::max<size_t>(1, std::min<size_t>(dn / C, (size_t)1 << 20));
    const u32 cb = dn / nch;
    u32 act = BGZ_T;
    if (const char* e = getenv("KRISP_GZ_LANES")) act = (u32)std::min(std::max(atoi(e), 1), BGZ_T);
    HIPCHK(c, hipSetDevice(c->device));
    {
        // (a genome of this id may still be sorting out of tx_text: as kr_genome_upload_text)
        const auto seen = c->genomes.find(id);
        if (seen != c->genomes.end() && (seen->second.uploaded || seen->second.n_bases)) HIPCHK(c, hipDeviceSynchronize());
    }
    hipStream_t st = c->stream;
    GzScratch S{c};
    auto room = [&](DevBuf& b, size_t bytes) -> int {
        const int rc = ensure(c, b, bytes);
        return rc == KR_ERR_CAPACITY ? fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: the scratch does not fit (%s)", c->err.c_str()) : rc;
    };
    int rc;
    if ((rc = room(S.in, (size_t)dn + 64)) || (rc = room(S.start, ((size_t)nch + 1) * 8)) ||
        (rc = room(S.res, ((size_t)2 * nch + 1) * sizeof(GzRes))) || (rc = room(S.bad, 64)))
        return rc;
    uint8_t* din = (uint8_t*)S.in.p;
    u64* dstart = (u64*)S.start.p;
    GzRes* dres = (GzRes*)S.res.p;
    u32* dbad = (u32*)S.bad.p;
    HIPCHK(c, hipMemcpyAsync(din, data, dn, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(din + dn, 0, 64, st));
    HIPCHK(c, hipMemsetAsync(dstart, 0, 8, st));
    HIPCHK(c, hipMemsetAsync(dbad, 0, 64, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const double t0 = now_us();
    if (nch > 1) hipLaunchKernelGGL(k_gz_find, dim3(nch - 1), dim3(BGZ_T), 0, st, (const uint8_t*)din, dn, nch, cb, dstart);
    hipLaunchKernelGGL(k_gz_decode<1>, dim3((nch + act - 1) / act), dim3(BGZ_T), 0, st, (const uint8_t*)din, dn, (const u64*)dstart,
                       nch, act, (const u32*)nullptr, 0u, (const u64*)nullptr, dres, (unsigned short*)nullptr, (u32)((1ull << 32) - 65));
    std::vector<u64> hstart(nch);
    std::vector<GzRes> hres(nch);
    HIPCHK(c, hipMemcpyAsync(hstart.data(), dstart, (size_t)nch * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hres.data(), dres, (size_t)nch * sizeof(GzRes), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    // the line of chunks from the first to the final block; their places in the text (the scan of their lengths)
    std::vector<u32> path;
    std::vector<u64> off;
    u64 total = 0;
    for (u32 cur = 0;;) {
        const GzRes& R = hres[cur];
        if (R.status) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: chunk %u of %u does not decode (status %u)", cur, nch, R.status);
        path.push_back(cur);
        off.push_back(total);
        total += R.len;
        if (total >= (1ull << 32) - 64) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: texts of >= 2^32 bytes go through the host");
        if (R.final_) break;
        u32 nx = cur + 1;
        while (nx < nch && hstart[nx] != R.end) nx++;
        if (nx == nch) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: chunk %u ends at bit %llu where no chunk begins", cur, (unsigned long long)R.end);
        cur = nx;
    }
    const u32 npath = (u32)path.size();
    off.push_back(total);
    u32 found = 0;
    for (u32 i = 1; i < nch; i++) found += hstart[i] != GZ_NONE;
    // the trailer right behind the final block; zero padding behind it only
    const size_t tr = hlen + (size_t)((hres[path.back()].end + 7) >> 3);
    if (tr + 8 > n) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: the file ends inside the trailer");
    const u32 want_crc = (u32)file[tr] | ((u32)file[tr + 1] << 8) | ((u32)file[tr + 2] << 16) | ((u32)file[tr + 3] << 24);
    const u32 isize = (u32)file[tr + 4] | ((u32)file[tr + 5] << 8) | ((u32)file[tr + 6] << 16) | ((u32)file[tr + 7] << 24);
    for (size_t i = tr + 8; i < n; i++)
        if (file[i]) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: a second member or other data follows the trailer (byte %zu)", i);
    if ((u64)isize != total) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: %llu bytes of text, ISIZE %u", (unsigned long long)total, isize);
    // pass 2: the line's chunks write their symbols
    const u32 nseg = (u32)((total + GZ_SEG - 1) / GZ_SEG);
    if ((rc = room(S.list, (size_t)npath * 4 + ((size_t)npath + 1) * 8 + 64)) || (rc = room(S.sym, (size_t)total * 2 + 64)) ||
        (rc = room(S.win, (size_t)npath * GZ_WIN)) || (rc = room(S.chain, (size_t)npath * 8 + 64)) ||
        (rc = room(S.crc, (size_t)nseg * 4 + 64)) || (rc = room(c->tx_text, (size_t)total + 64)))
        return rc;
    u64* doff = (u64*)S.list.p;
    u32* dlist = (u32*)(doff + npath + 1);
    unsigned short* dsym = (unsigned short*)S.sym.p;
    HIPCHK(c, hipMemcpyAsync(doff, off.data(), ((size_t)npath + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dlist, path.data(), (size_t)npath * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gz_decode<2>, dim3((npath + act - 1) / act), dim3(BGZ_T), 0, st, (const uint8_t*)din, dn, (const u64*)dstart,
                       nch, act, (const u32*)dlist, npath, (const u64*)doff, dres, dsym, 0u);
    std::vector<GzRes> hres2(nch);
    HIPCHK(c, hipMemcpyAsync(hres2.data(), dres + nch, (size_t)nch * sizeof(GzRes), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    // the runs of the window kernel: chunk k's window needs the windows of the chunks that hold markers in the 32 KB in
    // front of it (k - 1, or further back behind short chunks); a chunk whose 32 KB in front hold none begins a run.
    // A run never reaches back behind its first chunk: a marker there would lie in the first chunk's 32 KB, too.
    std::vector<u32> chain;
    u32 longest = 0;
    for (u32 k = 1; k < npath; k++) {
        const GzRes& R2 = hres2[path[k]];
        if (R2.status || R2.len != hres[path[k]].len || R2.end != hres[path[k]].end)
            return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: chunk %u: second pass status %u", path[k], R2.status);
        const long long lo = (long long)off[k] - (long long)GZ_WIN;
        bool dep = false;
        for (u32 j = k; j-- > 0 && (long long)off[j + 1] > lo;) {
            const u32 lm = hres2[path[j]].lastmark;
            if (lm && (long long)(off[j] + lm - 1) >= lo) { dep = true; break; }
        }
        if (!dep || chain.empty()) { chain.push_back(k); chain.push_back(1); }
        else chain.back()++;
        longest = std::max(longest, chain.back());
    }
    if (hres2[0].status) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: chunk 0: second pass status %u", hres2[0].status);
    const u32 nchains = (u32)(chain.size() / 2);
    u32* dchain = (u32*)S.chain.p;
    u32* dcrc = (u32*)S.crc.p;
    if (nchains) {
        HIPCHK(c, hipMemcpyAsync(dchain, chain.data(), chain.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gz_window, dim3(nchains), dim3(256), 0, st, (const unsigned short*)dsym, (const u64*)doff, npath,
                           (const u32*)dchain, (uint8_t*)S.win.p, dbad);
    }
    if (total) {
        hipLaunchKernelGGL(k_gz_emit, dim3((u32)((total + 2047) / 2048)), dim3(256), 0, st, (const unsigned short*)dsym, (const u64*)doff,
                           npath, (const uint8_t*)S.win.p, total, (uint8_t*)c->tx_text.p, dbad);
        hipLaunchKernelGGL(k_gz_crc, dim3((nseg + BGZ_T - 1) / BGZ_T), dim3(BGZ_T), 0, st, (const uint8_t*)c->tx_text.p, total, nseg, dcrc);
    }
    std::vector<u32> crcs(nseg);
    u32 nbad = 0;
    if (nseg) HIPCHK(c, hipMemcpyAsync(crcs.data(), dcrc, (size_t)nseg * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&nbad, dbad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const double us = now_us() - t0;
    if (stats) { stats[4] = nch; stats[5] = npath - 1; stats[6] = longest; stats[7] = (int64_t)us; }
    if (nbad) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: %u markers name bytes in front of the member", nbad);
    u32 crc = 0;
    const u32 xseg = gz_x8nmodp(GZ_SEG);
    for (u32 s = 0; s < nseg; s++) {
        const u64 len = std::min<u64>(GZ_SEG, total - (u64)s * GZ_SEG);
        crc = gz_mulmodp(len == GZ_SEG ? xseg : gz_x8nmodp(len), crc) ^ crcs[s];
    }
    if (crc != want_crc) return fail(c, KR_ERR_HOST, "kr_genome_upload_gzip: CRC-32 %08x, trailer %08x", crc, want_crc);
    PGZ_SAY("gunzip: %u chunks of %u bytes, %u block starts found, %u on the line, %u window runs (longest %u), %.0f us\n", nch, cb,
            found, npath, nchains, longest, us);
    S.drop();                               // (the scratch goes before the parse needs its own buffers)
    const int64_t nb = upload_text_impl(c, id, nullptr, (size_t)total, 0, one_shot, stats, true);
    if (stats) { stats[4] = nch; stats[5] = npath - 1; stats[6] = longest; stats[7] = (int64_t)us; }
    return nb;
}
