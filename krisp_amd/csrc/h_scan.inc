// h_scan.inc -- part of krisp_hip.hip (one translation unit): the host side of what the six one-genome scans share
// (k_scan.inc): the locate pass and the five seed passes -- near matches, guide hits, bulged guide hits, flank products,
// primer products (the multiplex pass, h_multiplex.inc, is the primer pass's scan with a join of its own).  All run in the
// locate context (kr_set_params_locate), one after the other on the context's stream: the per-tile counts, their offsets and the overflow flag are one set of scratch (loc.tcount, loc.toff, loc.flag).
//   all six: scan_ctx / scan_genome (the entry points' prologue), scan_tiles, scan_lds_bytes, scan_grid / scan_stride_grid
//     (launch geometry), scan_two_pass (every list), scan_fetch; scan_seps (locate, products, primers); scan_windows (the
//     hits' text: locate, near matches, guide hits, bulges -- the pass's cut launch passed in)
//   the five seed passes: seed_pieces, seed_both_strands, seed_keys (pigeonhole pieces, the entries' text, their keys),
//     seed_table_build (kr_ctx::SeedTable); near_geom, near_scan_pairs (k_near_scan for near matches, guide hits, bulges);
//     pair_list_sort, pair_list_upload (kr_ctx::PairList of the product passes, whose common scan is h_products.inc's)

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

// every entry point of the six passes begins here
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

typedef std::vector<std::pair<u64, u32>> SeedKeys;      // (key, entry) of every piece of every entry

// the pigeonhole pieces of the first len letters of a text: piece j = the letters [off[j], off[j + 1]), NP = M + 1 of them;
// pw (or nullptr): LOC_HB^(length of piece j - 1), what a rolling hash takes off with the letter that leaves
static void seed_pieces(u32 len, u32 NP, u32* off, u32* pw) {
    for (u32 j = 0; j <= NP; j++) off[j] = (u32)((u64)j * len / NP);
    for (u32 j = 0; pw && j < NP; j++) pw[j] = loc_pow((int)(off[j + 1] - off[j]) - 1);
}

// two entries' text at f: the n letters of s, then their reverse complement
static void seed_both_strands(uint8_t* f, const uint8_t* s, size_t n) {
    for (size_t i = 0; i < n; i++) {
        f[i] = s[i];
        f[n + i] = loc_comp(s[n - 1 - i]);
    }
}

// the NP keys of entry e, whose text stands at t, under the piece numbers first, first + 1, ...
static void seed_keys(SeedKeys& keyed, const uint8_t* t, const u32* off, u32 NP, u32 first, u32 e) {
    for (u32 j = 0; j < NP; j++) keyed.emplace_back(near_key(first + j, loc_hash(t + off[j], (int)(off[j + 1] - off[j]))), e);
}

// the part of a NearGeom that the passes over k_near_scan fill alike (lo / hi, the conserved flanks, are the caller's)
static NearGeom near_geom(u32 k, u32 omit, u32 M) {
    NearGeom ng;
    memset(&ng, 0, sizeof ng);
    ng.k = k; ng.omit = omit; ng.M = M; ng.np = M + 1;
    seed_pieces(k, ng.np, ng.off, ng.pw);
    return ng;
}

// a pair list (key, entry) -> the seed table on the device: slots that name the ranges of equal keys in the entry list,
// the membership bitmap, the entries' text.  -> the slots, or an error that names `who` and the n `unit`; st.slots is the
// caller's to set (whether a refused table leaves the earlier one standing differs by pass)
static int64_t seed_table_build(kr_ctx* c, SeedKeys& keyed, const std::vector<uint8_t>& text, kr_ctx::SeedTable& st, const char* who,
                                u64 n, const char* unit) {
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
    if ((rc = ensure(c, st.table, slots * sizeof(NearSlot))) || (rc = ensure(c, st.arena, text.size())) ||
        (rc = ensure(c, st.list, list.size() * 4)) || (rc = ensure(c, st.bitmap, (size_t)LOC_BM_WORDS * 4)))
        return fail(c, rc, "%s: the table of %llu %s does not fit the device (%s)", who, (unsigned long long)n, unit, c->err.c_str());
    HIPCHK(c, hipMemcpy(st.table.p, tab.data(), slots * sizeof(NearSlot), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(st.arena.p, text.data(), text.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(st.list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(st.bitmap.p, bm.data(), (size_t)LOC_BM_WORDS * 4, hipMemcpyHostToDevice));
    return (int64_t)slots;
}

// the sorted pair list (pair_list_sort) onto the device; the refusal names `who` and its n texts, as the table's does
static int pair_list_upload(kr_ctx* c, kr_ctx::PairList& pl, const std::vector<u64>& pkeys, const std::vector<u32>& pidx, const char* who,
                            u64 n) {
    int rc;
    if ((rc = ensure(c, pl.pairkeys, pkeys.size() * 8)) || (rc = ensure(c, pl.pairidx, pidx.size() * 4)))
        return fail(c, rc, "%s: the table of %llu texts does not fit the device (%s)", who, (unsigned long long)n, c->err.c_str());
    HIPCHK(c, hipMemcpy(pl.pairkeys.p, pkeys.data(), pkeys.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pl.pairidx.p, pidx.data(), pidx.size() * 4, hipMemcpyHostToDevice));
    return KR_OK;
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

// the text of the nhits windows of the latest scan (of genome gid), `width` bytes a row: cut(genome, grid) launches the
// pass's cut kernel, blocks of 256 threads, from its hits into dev_rows
template <typename Cut>
static int64_t scan_windows(kr_ctx* c, int64_t nhits, int gid, const char* scan_first, u32 width, DevBuf& dev_rows, uint8_t* rows,
                            size_t cap_bytes, Cut&& cut) {
    if (nhits < 0) return fail(c, KR_ERR_STATE, "%s", scan_first);
    if (!rows || !nhits) return nhits;
    auto it = c->genomes.find(gid);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d is gone", gid);
    const u64 bytes = (u64)nhits * width;
    if (bytes > cap_bytes) return fail(c, KR_ERR_CAPACITY, "row buffer too small: %llu > %zu", (unsigned long long)bytes, cap_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, dev_rows, bytes))) return rc;
    cut(it->second, scan_stride_grid(c, (bytes + 255) / 256));
    HIPCHK(c, hipMemcpyAsync(rows, dev_rows.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return nhits;
}

// scan_windows' cut launch for the rows of k letters at hits of type H (locate, near matches, guide hits: pass state S)
template <typename H, typename S>
static auto scan_cut_k(kr_ctx* c, S& st) {
    return [c, &st](const Genome& G, u32 grid) {
        hipLaunchKernelGGL(k_loc_cut<H>, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)G.bases.p, (const H*)st.hits.p,
                           (u64)st.nhits, (u32)c->loc.k, (uint8_t*)st.rows.p);
    };
}

// k_near_scan over a seed pass's table: the pairs (entry, distance, position) of genome G into dst, in two passes.  room
// (total) makes room for what else the pass sizes by the pairs (KR_OK or ensure()'s error); over: what to say of 2^32 or
// more pairs; fit: the refusal of a list that does not fit, a format of the total (%llu) and the reason (%s)
template <u32 NP, typename R>
static int near_scan_pairs_np(kr_ctx* c, const Genome& G, const kr_ctx::SeedTable& st, const NearGeom& ng, u64 ntiles, DevBuf& dst,
                              R&& room, const char* over, const char* fit, u64* total_out) {
    const size_t lds = scan_lds_bytes(ng.k, LOC_T * 8);           // (a 64-bit scan array)
    const u32 grid = scan_grid(c, k_near_scan<NP, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_near_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, ng,
                           (const u32*)st.bitmap.p, (const NearSlot*)st.table.p, (u64)(st.slots - 1), (const u32*)st.list.p,
                           (const uint8_t*)st.arena.p, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, over, [&](u32* tc, u32* fl) { launch(k_near_scan<NP, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) {
            int rc = ensure(c, dst, total * sizeof(kr_near_hit));
            if (!rc) rc = room(total);
            return rc ? fail(c, rc, fit, (unsigned long long)total, c->err.c_str()) : KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_near_scan<NP, true>, tc, to, (kr_near_hit*)dst.p, fl); }, total_out);
}

template <typename R>
static int near_scan_pairs(kr_ctx* c, const Genome& G, const kr_ctx::SeedTable& st, const NearGeom& ng, u64 ntiles, DevBuf& dst, R&& room,
                           const char* over, const char* fit, u64* total_out) {
    switch (ng.np) {                // (the bulged pass takes M <= 2: it never reaches 4 pieces)
    case 1: return near_scan_pairs_np<1>(c, G, st, ng, ntiles, dst, room, over, fit, total_out);
    case 2: return near_scan_pairs_np<2>(c, G, st, ng, ntiles, dst, room, over, fit, total_out);
    case 3: return near_scan_pairs_np<3>(c, G, st, ng, ntiles, dst, room, over, fit, total_out);
    default: return near_scan_pairs_np<4>(c, G, st, ng, ntiles, dst, room, over, fit, total_out);
    }
}

// the pairs (left text, right text) of a product pass -> pkeys (left << 32 | right, ascending) and pidx (the pair's row
// in the caller's list), each with an element to spare.  A pair that names a text beyond nleft / nright or repeats another
// is refused under `who`; each(p, left, right) is the pass's own check of pair p (KR_OK or its refusal), made pair by pair
// behind the first.  Throws std::bad_alloc
template <typename F>
static int pair_list_sort(kr_ctx* c, const char* who, const u32* pairs, u64 npairs, u64 nleft, u64 nright, std::vector<u64>& pkeys,
                          std::vector<u32>& pidx, F&& each) {
    std::vector<std::pair<u64, u32>> pk;
    pk.reserve(npairs);
    for (u64 p = 0; p < npairs; p++) {
        const u32 li = pairs[2 * p], rj = pairs[2 * p + 1];
        int rc;
        if (li >= nleft || rj >= nright)
            return fail(c, KR_ERR_PARAM, "%s: pair %llu names text (%u, %u) of (%llu, %llu)", who, (unsigned long long)p, li, rj,
                        (unsigned long long)nleft, (unsigned long long)nright);
        if ((rc = each(p, li, rj))) return rc;
        pk.emplace_back(((u64)li << 32) | rj, (u32)p);
    }
    std::sort(pk.begin(), pk.end());
    for (u64 p = 1; p < npairs; p++)
        if (pk[p].first == pk[p - 1].first)
            return fail(c, KR_ERR_PARAM, "%s: pair %u repeats the texts of pair %u", who, pk[p].second, pk[p - 1].second);
    pkeys.resize(npairs + 1);
    pidx.resize(npairs + 1);
    for (u64 p = 0; p < npairs; p++) {
        pkeys[p] = pk[p].first;
        pidx[p] = pk[p].second;
    }
    return KR_OK;
}
}  // extern "C++"
