// h_ingest.inc -- part of krisp_hip.hip (one translation unit): host: a sequence file -> upload buffer
// inside the library (SURVEY 8f rank 1; replaces kstream.py:458-479 fileinput + hook_compressed and
// kstream.py:556-583 parse for files): read, inflate, parse -- no Python object per line, no GIL
// (ctypes releases it: the host layer ingests several files at once and hands each genome to the
// GPU as soon as it is parsed) -- into PINNED host memory, from which kr_genome_upload copies by DMA
// without a staging copy.  gzip: libdeflate when the box has it (dlopen, ~2.5x zlib), else zlib;
// every member of a multi-member file in turn -- the members of a BGZF file (bgzip: every member says how long it is)
// side by side on host threads.  bz2 (round 4): libbz2 through dlopen, every stream of a multi-stream file (pbzip2), side
// by side on host threads when the stream boundaries check out; KR_ERR_HOST only when the box has no libbz2.
// ----------------------------------------------------------------------------
struct HostBlock { bool pinned; size_t bytes; unsigned devmask; };   // devmask: devices that copy (or copied) from the block
static std::mutex g_host_mu;
static std::map<void*, HostBlock> g_host_blocks;

static void* host_alloc(size_t bytes) {
    void* p = nullptr;
    bool pinned = false;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess)
        pinned = true;
    else {
        (void)hipGetLastError();
        p = malloc(bytes);
    }
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_blocks[p] = HostBlock{pinned, bytes, 0u};
    return p;
}

// is `p` inside a pinned block?  device >= 0: ... and that device is about to copy from it (kr_host_free waits for it)
static bool host_is_pinned(const void* p, int device) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_blocks.upper_bound((void*)p);
    if (it == g_host_blocks.begin()) return false;
    --it;
    const bool in = it->second.pinned && (const char*)p < (const char*)it->first + it->second.bytes;
    if (in && device >= 0 && device < 32) it->second.devmask |= 1u << device;
    return in;
}

void kr_host_free(void* p) {
    if (!p) return;
    HostBlock b{false, 0, 0u};
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_blocks.find(p);
        if (it == g_host_blocks.end()) return;
        b = it->second;
        g_host_blocks.erase(it);
    }
    if (b.pinned) {
        // a copy from this block may still be in flight, on another device than the caller's (krisp_fasta --devices drives one
        // context per device from its own thread): wait for every device that was handed the block
        int cur = 0;
        if (b.devmask && hipGetDevice(&cur) == hipSuccess) {
            for (int d = 0; d < 32; d++)
                if (((b.devmask >> d) & 1u) && hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
            (void)hipSetDevice(cur);
        }
        (void)hipHostFree(p);
    } else {
        free(p);
    }
}

#include "h_inflate.inc"     // libdeflate / zlib / libbz2 decoders, BGZF and bz2 block splitters, read_text (host only)

int64_t kr_ingest_file(const char* path, uint8_t** bases, int64_t* stats) {
    if (!path || !bases) return KR_ERR_PARAM;
    *bases = nullptr;
    RawBuf text;
    bool gz = false;
    double t_read = 0, t_inflate = 0;
    int64_t members = 0;
    int used_ld = 0;
    const int64_t nt = read_text(path, text, &gz, &t_read, &t_inflate, &members, &used_ld);
    if (nt < 0) return nt;
    const double t2 = now_us();
    uint8_t* out = (uint8_t*)host_alloc(text.len + 64);
    if (!out) return KR_ERR_CAPACITY;
    int64_t st4[4] = {0, 0, 0, 0};
    // .gz / .bz2 streams are split on '\n' only, plain files with universal newlines (krisp_amd/fasta.py)
    const int64_t n = kr_fasta_to_bases(text.p, text.len, gz ? 0 : 1, 1, out, text.len + 64, st4);
    if (n < 0) {
        kr_host_free(out);
        return n;
    }
    const double t3 = now_us();
    if (stats) {
        stats[0] = st4[0]; stats[1] = st4[1]; stats[2] = st4[2]; stats[3] = st4[3];
        stats[4] = (int64_t)t_read;             // read, microseconds
        stats[5] = (int64_t)t_inflate;          // inflate
        stats[6] = (int64_t)(t3 - t2);          // parse
        stats[7] = members | ((int64_t)used_ld << 32);
    }
    *bases = out;
    return n;
}

// ---- the same file with the PARSE on the device (SURVEY 8f rank 1: the host reads and inflates only).
// kr_read_file: the file's text in pinned host memory (free with kr_host_free); stats[4] read, [5] inflate microseconds,
// [7] members | libdeflate << 32, [3] = 1 when the text wants universal newlines (a plain file).
int64_t kr_read_file(const char* path, uint8_t** text_out, int64_t* stats) {
    if (!path || !text_out) return KR_ERR_PARAM;
    *text_out = nullptr;
    // (plain malloc'ed memory, not a pinned block: on these boxes -- tools/pinbench.hip -- pinning 50 MB costs 7-11 ms
    // and its release 4 ms, where the copy from pageable memory takes 1.5 ms against 1.0 ms from pinned)
    RawBuf text;
    bool gz = false;
    double t_read = 0, t_inflate = 0;
    int64_t members = 0;
    int used_ld = 0;
    const int64_t nt = read_text(path, text, &gz, &t_read, &t_inflate, &members, &used_ld);
    if (nt < 0) return nt;
    const double t2 = now_us();
    if (!text.p && !text.reserve(64)) return KR_ERR_CAPACITY;      // (an empty file still hands a block over)
    if (stats) {
        stats[0] = stats[1] = stats[2] = 0;
        stats[3] = gz ? 0 : 1;
        stats[4] = (int64_t)t_read;
        stats[5] = (int64_t)t_inflate;
        stats[6] = (int64_t)(now_us() - t2);
        stats[7] = members | ((int64_t)used_ld << 32);
    }
    const size_t cap = text.cap;
    uint8_t* out = text.detach();
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_blocks[out] = HostBlock{false, cap, 0u};      // (kr_host_free frees it)
    }
    *text_out = out;
    return nt;
}

// text -> genome `id`'s upload buffer, parsed on the device with the reference reader's semantics (k_text.inc;
// byte for byte what kr_fasta_to_bases writes), then as kr_genome_upload.  stats[0..3] = records, characters outside
// ACGTNacgtn, RNA (U mapped to T), FASTA.  Returns the number of bases (separators included).
static int64_t upload_text_impl(kr_ctx* c, int id, const uint8_t* text, size_t n, int universal_newlines, int one_shot,
                                int64_t* stats, bool resident);
int64_t kr_genome_upload_text(kr_ctx* c, int id, const uint8_t* text, size_t n, int universal_newlines, int one_shot,
                              int64_t* stats) {
    return upload_text_impl(c, id, text, n, universal_newlines, one_shot, stats, false);
}

// resident: the text lies in c->tx_text already (kr_genome_upload_bgzf inflated it there; the buffer holds n + 64 bytes)
static int64_t upload_text_impl(kr_ctx* c, int id, const uint8_t* text, size_t n, int universal_newlines, int one_shot,
                                int64_t* stats, bool resident) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (!text && n && !resident) return fail(c, KR_ERR_PARAM, "kr_genome_upload_text: null text");
    if (n >= (1ull << 32) - 64) return fail(c, KR_ERR_PARAM, "texts of >= 2^32 bytes are not supported");
    HIPCHK(c, hipSetDevice(c->device));
    const auto seen = c->genomes.find(id);
    const bool known = seen != c->genomes.end() && (seen->second.uploaded || seen->second.n_bases);     // (kr_reserve makes entries that were never uploaded)
    if (known) HIPCHK(c, hipDeviceSynchronize());
    Genome& G = c->genomes[id];
    G.id = id;
    G.sorted = G.finalized = G.ordered = G.coarse = G.hits_valid = false;
    coarse_pool_return(c, G);
    G.uploaded = false;
    G.count = -1;
    int rc;
    hipStream_t st = c->stream;
    const u32 nt = (u32)n;
    const u32 ntiles = (nt + TX_TILE - 1) / TX_TILE;
    if ((rc = ensure(c, G.bases, n + 64))) return rc;                  // (the parse only ever drops bytes)
    if ((rc = ensure(c, c->tx_text, n + 64))) return rc;
    if ((rc = ensure(c, c->tx_tile, ((size_t)ntiles + 4) * 4))) return rc;
    if ((rc = ensure(c, c->tx_tilepos, ((size_t)ntiles + 4) * 4))) return rc;
    const u32 nt2 = (ntiles + 2047) / 2048;
    if ((rc = ensure(c, c->tx_tsum, ((size_t)nt2 + 4) * 4))) return rc;
    if ((rc = ensure(c, c->tx_tpos, ((size_t)nt2 + 4) * 4))) return rc;
    if ((rc = ensure(c, c->tx_state, 64))) return rc;
    if (!G.up_done) HIPCHK(c, hipEventCreateWithFlags(&G.up_done, hipEventDisableTiming));
    TxState* ts = (TxState*)c->tx_state.p;
    u32 nlines = 0;
    volatile u32* mb = c->mbox + 8;
    if (n) {
        if (!resident) {
            hipStream_t cs = host_is_pinned(text, c->device) ? c->copy_stream : st;
            HIPCHK(c, hipMemcpyAsync(c->tx_text.p, text, n, hipMemcpyHostToDevice, cs));
            if (cs != st) {
                HIPCHK(c, hipEventRecord(G.up_done, cs));
                HIPCHK(c, hipStreamWaitEvent(st, G.up_done, 0));
            }
        }
        const uint8_t* dt = (const uint8_t*)c->tx_text.p;
        hipLaunchKernelGGL(k_tx_firstline, dim3(1), dim3(1024), 0, st, dt, nt, universal_newlines, ts);
        hipLaunchKernelGGL(k_tx_starts_count, dim3(ntiles), dim3(256), 0, st, dt, nt, universal_newlines, (u32*)c->tx_tile.p);
        launch_excl_scan(st, (const u32*)c->tx_tile.p, ntiles, (u32*)c->tx_tsum.p, (u32*)c->tx_tpos.p, (u32*)c->tx_tilepos.p);
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, (const u32*)c->tx_tilepos.p + ntiles, (const u32*)nullptr,
                           (const u32*)nullptr, (u32*)mb);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        nlines = mb[0];
    }
    u32 nout = 0, nrec = 0, special = 0, rna = 0, fasta = 0;
    if (nlines) {
        if ((rc = ensure(c, c->tx_lines, ((size_t)nlines + 4) * 4))) return rc;
        if ((rc = ensure(c, c->tx_ls, ((size_t)nlines + 4) * 4))) return rc;
        if ((rc = ensure(c, c->tx_ll, ((size_t)nlines + 4) * 4))) return rc;
        if ((rc = ensure(c, c->tx_op, (size_t)nlines + 16))) return rc;
        if ((rc = ensure(c, c->tx_outpos, ((size_t)nlines + 4) * 4))) return rc;
        const uint8_t* dt = (const uint8_t*)c->tx_text.p;
        hipLaunchKernelGGL(k_tx_starts_write, dim3(ntiles), dim3(256), 0, st, dt, nt, universal_newlines,
                           (const u32*)c->tx_tilepos.p, (u32*)c->tx_lines.p);
        hipLaunchKernelGGL(k_tx_lineinfo, dim3((nlines + 255) / 256), dim3(256), 0, st, dt, nt, (const u32*)c->tx_lines.p, nlines,
                           (const TxState*)ts, one_shot, (u32*)c->tx_ls.p, (u32*)c->tx_ll.p, (uint8_t*)c->tx_op.p);
        {
            // the scan over the lines (k_text.inc): G workgroups of TXS_T threads, a run of `per` lines per thread
            const u32 Gs = std::max<u32>(1u, std::min<u32>(TXS_GMAX, (nlines + 8 * TXS_T - 1) / (8 * TXS_T)));
            const u32 per = (u32)(((u64)nlines + (u64)Gs * TXS_T - 1) / ((u64)Gs * TXS_T));
            if ((rc = ensure(c, c->tx_scan, ((size_t)3 * Gs * TXS_T + 3 * Gs + 8) * 4))) return rc;
            u32* thr = (u32*)c->tx_scan.p;
            u32 *wg_f = thr + (size_t)3 * Gs * TXS_T, *wg_sep = wg_f + Gs, *wg_bytes = wg_sep + Gs;
            hipLaunchKernelGGL(k_tx_scan1, dim3(Gs), dim3(TXS_T), 0, st, (const uint8_t*)c->tx_op.p, nlines, per, wg_f);
            hipLaunchKernelGGL(k_tx_scan2, dim3(Gs), dim3(TXS_T), 0, st, (const u32*)c->tx_ll.p, (const uint8_t*)c->tx_op.p, nlines, per,
                               (const u32*)wg_f, thr, wg_sep, wg_bytes);
            hipLaunchKernelGGL(k_tx_scan3, dim3(Gs), dim3(TXS_T), 0, st, (const u32*)c->tx_ll.p, (uint8_t*)c->tx_op.p, nlines, per,
                               (const u32*)thr, (const u32*)wg_sep, (const u32*)wg_bytes, (u32*)c->tx_outpos.p, ts);
        }
        hipLaunchKernelGGL(k_tx_copy, dim3((nt + TX_OUT - 1) / TX_OUT), dim3(256), 0, st, dt, (const u32*)c->tx_ls.p,
                           (const u32*)c->tx_ll.p, (const uint8_t*)c->tx_op.p, (const u32*)c->tx_outpos.p, nlines,
                           (const TxState*)ts, (uint8_t*)G.bases.p);
        const u32 g2 = std::min<u32>((nt + 4095) / 4096, 2048u);
        hipLaunchKernelGGL(k_tx_stats1, dim3(g2), dim3(256), 0, st, (const uint8_t*)G.bases.p, ts);
        hipLaunchKernelGGL(k_tx_stats2, dim3(g2), dim3(256), 0, st, (const uint8_t*)G.bases.p, ts);
        hipLaunchKernelGGL(k_tx_finish, dim3(g2), dim3(256), 0, st, (uint8_t*)G.bases.p, ts);
        hipLaunchKernelGGL(k_tx_publish, dim3(1), dim3(64), 0, st, (const TxState*)ts, (u32*)mb);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        nout = mb[1]; nrec = mb[2]; special = mb[3]; rna = mb[4]; fasta = mb[5];
    }
    if (stats) { stats[0] = nrec; stats[1] = special; stats[2] = rna; stats[3] = fasta; }
    if (nout > c->max_bases) return fail(c, KR_ERR_PARAM, "genome of %u bases exceeds max_bases %zu", nout, c->max_bases);
    G.n_bases = nout;
    G.nwords = ((u64)nout + 31) / 32;
    HIPCHK(c, hipEventRecord(G.up_done, st));
    if ((rc = upload_finish(c, G, id, nout))) return rc;
    return (int64_t)nout;
}

// ---- a BGZF file inflated ON THE DEVICE (round 6; k_inflate.inc): the compressed bytes travel (a third of the text), every
// member is a lane of k_bgzf_inflate, the text lands where kr_genome_upload_text's copy would have put it and is parsed
// by the same kernels.  The host only walks the members' headers: magic, the BC subfield with the member's size, the
// trailer's CRC-32 and ISIZE.  A file that is not BGZF from its first byte to its last (plain gzip, another extra field,
// a member that overruns the file, more than 2^32 bytes of text) or ONE member the device could not inflate to its
// trailer's CRC-32 and length returns KR_ERR_HOST with nothing uploaded: the caller inflates the file on the host, as for
// any other `.gz`, and THAT path's verdict on the file stands (stats[5] = the first bad member, stats[6] = its status).
// stats[0..3] as kr_genome_upload_text, stats[4] = members, stats[7] = microseconds of the two inflate kernels.
int64_t kr_genome_upload_bgzf(kr_ctx* c, int id, const uint8_t* file, size_t n, int one_shot, int64_t* stats) {
    if (!c || !c->have_params) return fail(c, KR_ERR_STATE, "kr_set_params first");
    if (!file && n) return fail(c, KR_ERR_PARAM, "kr_genome_upload_bgzf: null file");
    if (n >= (1ull << 32) - 64) return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: files of >= 2^32 bytes go through the host");
    std::vector<BgzMember> tab;
    std::vector<u32> crcs;
    u64 total = 0;
    for (size_t at = 0; at < n;) {
        const uint8_t* h = file + at;
        if (n - at < 26 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4 || h[10] != 6 || h[11] != 0 || h[12] != 'B' ||
            h[13] != 'C' || h[14] != 2 || h[15] != 0)
            return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: not a BGZF member at byte %zu", at);
        const size_t bsize = (size_t)(h[16] | (h[17] << 8)) + 1;
        if (bsize < 26 || at + bsize > n) return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: member at byte %zu overruns the file", at);
        const uint8_t* t = h + bsize - 8;
        const u32 crc = (u32)t[0] | ((u32)t[1] << 8) | ((u32)t[2] << 16) | ((u32)t[3] << 24);
        const u32 isize = (u32)t[4] | ((u32)t[5] << 8) | ((u32)t[6] << 16) | ((u32)t[7] << 24);
        if (isize > 65536) return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: member at byte %zu says %u bytes of text", at, isize);
        tab.push_back(BgzMember{(u32)(at + 18), (u32)(bsize - 26), (u32)total, isize});
        crcs.push_back(crc);
        total += isize;
        if (total >= (1ull << 32) - 64) return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: texts of >= 2^32 bytes go through the host");
        at += bsize;
    }
    const u32 nmem = (u32)tab.size();
    HIPCHK(c, hipSetDevice(c->device));
    {
        // (a genome of this id may still be sorting out of the buffers below: as kr_genome_upload_text)
        const auto seen = c->genomes.find(id);
        if (seen != c->genomes.end() && (seen->second.uploaded || seen->second.n_bases)) HIPCHK(c, hipDeviceSynchronize());
    }
    int rc;
    hipStream_t st = c->stream;
    if ((rc = ensure(c, c->tx_text, (size_t)total + 64))) return rc;
    if ((rc = ensure(c, c->bgz_in, n + 64))) return rc;
    if ((rc = ensure(c, c->bgz_tab, (size_t)nmem * (sizeof(BgzMember) + 4) + 64))) return rc;
    if ((rc = ensure(c, c->bgz_stat, ((size_t)nmem + 4) * 4))) return rc;
    double us = 0;
    if (nmem) {
        uint8_t* din = (uint8_t*)c->bgz_in.p;
        BgzMember* dtab = (BgzMember*)c->bgz_tab.p;
        u32* dcrc = (u32*)(dtab + nmem);
        u32* dstat = (u32*)c->bgz_stat.p;
        HIPCHK(c, hipMemcpyAsync(din, file, n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(din + n, 0, 64, st));
        HIPCHK(c, hipMemcpyAsync(dtab, tab.data(), (size_t)nmem * sizeof(BgzMember), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(dcrc, crcs.data(), (size_t)nmem * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(dstat, 0, ((size_t)nmem + 4) * 4, st));
        const double t0 = now_us();
        const u32 grid = (nmem + BGZ_T - 1) / BGZ_T;
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZ_T), 0, st, (const uint8_t*)din, (const BgzMember*)dtab, nmem,
                           (uint8_t*)c->tx_text.p, dstat);
        hipLaunchKernelGGL(k_bgzf_crc, dim3(grid), dim3(BGZ_T), 0, st, (const uint8_t*)c->tx_text.p, (const BgzMember*)dtab,
                           (const u32*)dcrc, nmem, dstat, dstat + nmem);
        u32 nbad = 0;
        HIPCHK(c, hipMemcpyAsync(&nbad, dstat + nmem, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));         // (also: `tab`, `crcs` and the caller's `file` may go now)
        HIPCHK(c, hipGetLastError());
        us = now_us() - t0;
        if (nbad) {
            std::vector<u32> stv(nmem);
            HIPCHK(c, hipMemcpy(stv.data(), dstat, (size_t)nmem * 4, hipMemcpyDeviceToHost));
            u32 first = 0;
            while (first < nmem && stv[first] == 0) first++;
            if (stats) { stats[4] = nmem; stats[5] = first; stats[6] = first < nmem ? stv[first] : 0; stats[7] = (int64_t)us; }
            return fail(c, KR_ERR_HOST, "kr_genome_upload_bgzf: %u of %u members did not inflate to their trailers (first: member %u, status %u)",
                        nbad, nmem, first, first < nmem ? stv[first] : 0u);
        }
    }
    const int64_t nb = upload_text_impl(c, id, nullptr, (size_t)total, 0, one_shot, stats, true);
    if (stats) { stats[4] = nmem; stats[5] = stats[6] = 0; stats[7] = (int64_t)us; }
    return nb;
}

// the bases of an uploaded genome back to the host (the IUPAC side channel and the text cutting of long amplicons
// need them when the parse ran on the device)
int64_t kr_genome_fetch_bases(kr_ctx* c, int id, uint8_t* out, size_t cap) {
    if (!c) return KR_ERR_PARAM;
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    const size_t n = it->second.n_bases;
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "base buffer too small: %zu > %zu", n, cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(out, it->second.bases.p, n, hipMemcpyDeviceToHost));
    return (int64_t)n;
}
