// h_scan.inc -- part of krisp_hip.hip (one translation unit): the host side of what the locate, near-match and product
// passes share (k_scan.inc): the entry points' prologue, the launch geometry of a tile scan, the two-pass driver, the
// separator list, the seed table, the fetch of a result list and of its windows' text.  All three passes run in the locate
// context (kr_set_params_locate), one after the other on the context's stream: the per-tile counts, their offsets and the
// overflow flag are one set of scratch (loc.tcount, loc.toff, loc.flag).

static u32 loc_hash(const uint8_t* s, int m) {
    u32 h = 0;
    for (int i = 0; i < m; i++) h = h * LOC_HB + s[i];
    return h;
}

static u32 loc_pow(int e) {
    u32 r = 1;
    for (int i = 0; i < e; i++) r *= LOC_HB;
    return r;
}

// every entry point of the three passes begins here
static int scan_ctx(kr_ctx* c) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    return KR_OK;
}

// the uploaded genome `id` of a locate context whose table is ready (table_first: what to say when it is not)
static int scan_genome(kr_ctx* c, int id, bool table_ready, const char* table_first, const Genome** G) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    if (!table_ready) return fail(c, KR_ERR_STATE, "%s", table_first);
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    *G = &it->second;
    HIPCHK(c, hipSetDevice(c->device));
    return KR_OK;
}

// tiles of LOC_T * LOC_S window starts that hold the windows of `width` bases of n bases; *nw = the window starts
static u64 scan_tiles(u64 n, u64 width, u64* nw) {
    const u64 TP = (u64)LOC_T * LOC_S;
    *nw = n >= width ? n - width + 1 : 0;
    return (*nw + TP - 1) / TP;
}

// dynamic LDS of a tile scan: the bitmap, `head` bytes of the kernel's own (its block scan array, ...), the padded tile
// of windows of `width` bases
static size_t scan_lds_bytes(u32 width, u32 head) {
    const u32 tb = LOC_T * LOC_S + width - 1;
    return (size_t)LOC_BM_WORDS * 4 + head + (((tb + 16) + ((tb + 16) >> LOC_SH) * 4 + 15) & ~15u);
}

// a result list of n elements (n < 0: no scan yet) into the caller's buffer
static int64_t scan_fetch(kr_ctx* c, int64_t n, const char* scan_first, const char* noun, const DevBuf& src, void* out, size_t cap,
                          size_t elem) {
    if (n < 0) return fail(c, KR_ERR_STATE, "%s", scan_first);
    if ((size_t)n > cap) return fail(c, KR_ERR_CAPACITY, "%s buffer too small: %lld > %zu", noun, (long long)n, cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(out, src.p, (size_t)n * elem, hipMemcpyDeviceToHost));
    return n;
}

// a pair list (key, entry) -> the seed table on the device: slots that name the ranges of equal keys in the entry list,
// the membership bitmap, the entries' text.  -> the slots, or an error that names `who` and the n `unit`
static int64_t seed_table_build(kr_ctx* c, std::vector<std::pair<u64, u32>>& keyed, const std::vector<uint8_t>& text, DevBuf& table,
                                DevBuf& arena, DevBuf& list_buf, DevBuf& bitmap, const char* who, u64 n, const char* unit) {
    const u64 nk = keyed.size();
    std::vector<NearSlot> tab;
    std::vector<u32> list, bm;
    u64 slots = 1024;
    try {
        std::sort(keyed.begin(), keyed.end());
        u64 distinct = 0;
        for (u64 i = 0; i < nk; i++) distinct += i == 0 || keyed[i].first != keyed[i - 1].first;
        while (slots < 2 * distinct) slots <<= 1;
        tab.assign(slots, NearSlot{0, 0, NEAR_EMPTY});
        bm.assign(LOC_BM_WORDS, 0u);
        list.resize(nk + 1);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "%s: no host memory for the table of %llu %s", who, (unsigned long long)n, unit);
    }
    const u64 mask = slots - 1;
    for (u64 i = 0; i < nk;) {
        u64 j = i;
        for (; j < nk && keyed[j].first == keyed[i].first; j++) list[j] = keyed[j].second;
        const u64 key = keyed[i].first;
        u64 s = key & mask;
        while (tab[s].count != NEAR_EMPTY) s = (s + 1) & mask;
        tab[s].key = key;
        tab[s].start = (u32)i;                      // (nk < 2^28)
        tab[s].count = (u32)(j - i);
        const u32 b = (u32)(key >> (64 - LOC_BM_LOG));
        bm[b >> 5] |= 1u << (b & 31);
        i = j;
    }
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, table, slots * sizeof(NearSlot))) || (rc = ensure(c, arena, text.size())) ||
        (rc = ensure(c, list_buf, list.size() * 4)) || (rc = ensure(c, bitmap, (size_t)LOC_BM_WORDS * 4)))
        return fail(c, rc, "%s: the table of %llu %s does not fit the device (%s)", who, (unsigned long long)n, unit, c->err.c_str());
    HIPCHK(c, hipMemcpy(table.p, tab.data(), slots * sizeof(NearSlot), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(arena.p, text.data(), text.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(list_buf.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(bitmap.p, bm.data(), (size_t)LOC_BM_WORDS * 4, hipMemcpyHostToDevice));
    return (int64_t)slots;
}

#define SCAN_COUNT_ONLY 1           // a room() of scan_two_pass: the caller asked for the count, nothing is emitted

extern "C++" {    // (templates inside the translation unit's extern "C" block)
// persistent workgroups of a tile scan: what the device holds at once, the tiles at most
template <typename K>
static u32 scan_grid(kr_ctx* c, K kernel, size_t lds, u64 ntiles) {
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, LOC_T, lds) != hipSuccess || per < 1) {
        (void)hipGetLastError();
        per = 1;
    }
    const u32 grid = (u32)std::min<u64>(ntiles, c->scan_cap ? (u64)c->scan_cap : (u64)c->ncu * per);
    c->scan_dbg[0] = (int64_t)ntiles;
    c->scan_dbg[1] = grid;
    return grid;
}

// blocks of an element-stride launch over `blocks` blocks' worth of elements: 16 per CU at most (KR_SCAN_GRID: that many)
static u32 scan_stride_grid(kr_ctx* c, u64 blocks) {
    return (u32)std::min<u64>(blocks, c->scan_cap ? (u64)c->scan_cap : (u64)c->ncu * 16);
}

// a list made in two passes over nblocks tiles (or blocks): count(tcount, flag) launches the counting kernel,
// k_loc_offsets scans the counts, room(total) makes room for the list (-> KR_OK, an error, or SCAN_COUNT_ONLY),
// emit(tcount, toff, flag) launches the emitting kernel; the stream is idle on return.  over: what to say when a tile
// or the genome holds 2^32 or more (nullptr: a kernel with 32-bit counts, which has no flag)
template <typename C, typename R, typename E>
static int scan_two_pass(kr_ctx* c, u64 nblocks, const char* over, C&& count, R&& room, E&& emit, u64* total_out) {
    auto& l = c->loc;
    int rc;
    if ((rc = ensure(c, l.tcount, (nblocks + 1) * 4)) || (rc = ensure(c, l.toff, (nblocks + 1) * 8)) || (rc = ensure(c, l.flag, 16)))
        return rc;
    c->scan_dbg[2] = (int64_t)nblocks;
    hipStream_t st = c->stream;
    u32* tc = (u32*)l.tcount.p;
    u64* to = (u64*)l.toff.p;
    u32* fl = (u32*)l.flag.p;
    if (over) HIPCHK(c, hipMemsetAsync(fl, 0, 4, st));
    count(tc, fl);
    hipLaunchKernelGGL(k_loc_offsets, dim3(1), dim3(1024), 0, st, (const u32*)tc, nblocks, to);
    u64 total = 0;
    u32 flagged = 0;
    HIPCHK(c, hipMemcpyAsync(&total, to + nblocks, 8, hipMemcpyDeviceToHost, st));
    if (over) HIPCHK(c, hipMemcpyAsync(&flagged, fl, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (over && (flagged || total >= (1ull << 32))) return fail(c, KR_ERR_CAPACITY, "%s", over);
    *total_out = total;
    if (!total) return KR_OK;
    if ((rc = room(total))) return rc == SCAN_COUNT_ONLY ? KR_OK : rc;
    emit(tc, (const u64*)to, fl);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return KR_OK;
}

// the positions of the genome's record separators, ascending, into dst: room(total) sizes dst (scan_two_pass).  `who`
// names the entry point in the one refusal
template <typename R>
static int scan_seps(kr_ctx* c, const Genome& G, const char* who, DevBuf& dst, R&& room, u64* nseps) {
    const u64 n = G.n_bases, TB = (u64)LOC_T * LOC_SEP_BYTES;
    const u64 ntiles = (n + TB - 1) / TB;
    *nseps = 0;
    if (!ntiles) return KR_OK;
    if (ntiles >= (1ull << 31)) return fail(c, KR_ERR_PARAM, "%s: %llu bases", who, (unsigned long long)n);
    const uint8_t* b = (const uint8_t*)G.bases.p;
    return scan_two_pass(
        c, ntiles, nullptr,
        [&](u32* tc, u32*) {
            hipLaunchKernelGGL(k_loc_sep<false>, dim3((u32)ntiles), dim3(LOC_T), 0, c->stream, b, n, tc, (const u64*)nullptr,
                               (u64*)nullptr);
        },
        room,
        [&](u32* tc, const u64* to, u32*) {
            hipLaunchKernelGGL(k_loc_sep<true>, dim3((u32)ntiles), dim3(LOC_T), 0, c->stream, b, n, tc, to, (u64*)dst.p);
        },
        nseps);
}

// the text of the nhits windows of the latest scan (of genome gid; hits of type H on the device), k bytes a row
template <typename H>
static int64_t scan_windows(kr_ctx* c, int64_t nhits, int gid, const char* scan_first, const DevBuf& hits, DevBuf& dev_rows,
                            uint8_t* rows, size_t cap_bytes) {
    if (nhits < 0) return fail(c, KR_ERR_STATE, "%s", scan_first);
    if (!rows || !nhits) return nhits;
    auto it = c->genomes.find(gid);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d is gone", gid);
    const u64 bytes = (u64)nhits * c->loc.k;
    if (bytes > cap_bytes) return fail(c, KR_ERR_CAPACITY, "row buffer too small: %llu > %zu", (unsigned long long)bytes, cap_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, dev_rows, bytes))) return rc;
    const u32 grid = scan_stride_grid(c, (bytes + 255) / 256);
    hipLaunchKernelGGL(k_loc_cut<H>, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)it->second.bases.p, (const H*)hits.p,
                       (u64)nhits, (u32)c->loc.k, (uint8_t*)dev_rows.p);
    HIPCHK(c, hipMemcpyAsync(rows, dev_rows.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return nhits;
}
}  // extern "C++"
