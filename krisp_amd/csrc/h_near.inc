// h_near.inc -- part of krisp_hip.hip (one translation unit): host side of the near-match pass (k_near.inc): the seed table of
// the targets, the scan of one genome, its hits and their windows.  The context is the locate context
// (kr_set_params_locate): one genome resident at a time, uploaded by the same entry points; kr_locate_seps lists its record
// separators.  Beside the genome live the entries' text (2 k bytes a target), the table (16 bytes a slot, >= 2 slots a
// distinct piece), the entry list (4 bytes per entry and piece), the bitmap, the per-tile counts and the hits.

int64_t kr_near_table(kr_ctx* c, const uint8_t* targets, uint64_t ntargets, int mismatches) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto& l = c->loc;
    auto& nr = c->near;
    const int k = l.k, M = mismatches;
    if (M < 0 || M >= NEAR_MAXP || M >= k)
        return fail(c, KR_ERR_PARAM, "kr_near_table: 0 <= mismatches <= %d and mismatches < L+D+R = %d (got %d)", NEAR_MAXP - 1, k, M);
    if (!targets && ntargets) return fail(c, KR_ERR_PARAM, "kr_near_table: null targets");
    if (ntargets >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_near_table: %llu targets (the limit is %u)", (unsigned long long)ntargets, (1u << 24) - 1);
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    for (u32 j = 0; j <= NP; j++) off[j] = (u32)((u64)j * k / NP);
    const u64 ne = 2 * ntargets, nk = ne * NP;
    std::vector<uint8_t> text;
    std::vector<std::pair<u64, u32>> keyed;
    std::vector<NearSlot> tab;
    std::vector<u32> list, bm;
    u64 slots = 1024;
    try {
        text.resize(ne * k + 16);
        for (u64 t = 0; t < ntargets; t++) {
            const uint8_t* s = targets + t * k;
            uint8_t* f = text.data() + 2 * t * k;
            for (int i = 0; i < k; i++) {
                f[i] = s[i];
                f[k + i] = loc_comp(s[k - 1 - i]);
            }
        }
        keyed.reserve(nk);
        for (u64 e = 0; e < ne; e++)
            for (u32 j = 0; j < NP; j++)
                keyed.emplace_back(near_key(j, loc_hash(text.data() + e * k + off[j], (int)(off[j + 1] - off[j]))), (u32)e);
        std::sort(keyed.begin(), keyed.end());
        u64 distinct = 0;
        for (u64 i = 0; i < nk; i++) distinct += i == 0 || keyed[i].first != keyed[i - 1].first;
        while (slots < 2 * distinct) slots <<= 1;
        tab.assign(slots, NearSlot{0, 0, NEAR_EMPTY});
        bm.assign(LOC_BM_WORDS, 0u);
        list.resize(nk + 1);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_near_table: no host memory for the table of %llu targets", (unsigned long long)ntargets);
    }
    const u64 mask = slots - 1;
    for (u64 i = 0; i < nk;) {
        u64 j = i;
        for (; j < nk && keyed[j].first == keyed[i].first; j++) list[j] = keyed[j].second;
        const u64 key = keyed[i].first;
        u64 s = key & mask;
        while (tab[s].count != NEAR_EMPTY) s = (s + 1) & mask;
        tab[s].key = key;
        tab[s].start = (u32)i;                      // (nk < 2^27)
        tab[s].count = (u32)(j - i);
        const u32 b = (u32)(key >> (64 - LOC_BM_LOG));
        bm[b >> 5] |= 1u << (b & 31);
        i = j;
    }
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, nr.table, slots * sizeof(NearSlot))) || (rc = ensure(c, nr.arena, text.size())) ||
        (rc = ensure(c, nr.list, list.size() * 4)) || (rc = ensure(c, nr.bitmap, (size_t)LOC_BM_WORDS * 4)) ||
        (rc = ensure(c, nr.flag, 16)))
        return fail(c, rc, "kr_near_table: the table of %llu targets does not fit the device (%s)", (unsigned long long)ntargets,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(nr.table.p, tab.data(), slots * sizeof(NearSlot), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(nr.arena.p, text.data(), text.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(nr.list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(nr.bitmap.p, bm.data(), (size_t)LOC_BM_WORDS * 4, hipMemcpyHostToDevice));
    nr.M = M;
    nr.ntargets = ntargets;
    nr.slots = slots;
    nr.nhits = -1;
    return (int64_t)slots;
}

static size_t near_lds_bytes(int k) {
    const u32 tb = LOC_T * LOC_S + k - 1;
    return (size_t)LOC_BM_WORDS * 4 + LOC_T * 8 + (((tb + 16) + ((tb + 16) >> LOC_SH) * 4 + 15) & ~15u);
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
template <u32 NP>
static int near_launch(kr_ctx* c, const Genome& G, const NearGeom& ng, u64 ntiles, u64* total_out) {
    auto& l = c->loc;
    auto& nr = c->near;
    const size_t lds = near_lds_bytes(l.k);
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_near_scan<NP, false>, LOC_T, lds) != hipSuccess || per < 1) {
        (void)hipGetLastError();
        per = 1;
    }
    const u64 grid = std::min<u64>(ntiles, (u64)c->ncu * per);
    hipStream_t st = c->stream;
    const uint8_t* b = (const uint8_t*)G.bases.p;
    const u64 n = G.n_bases;
    const u32* bm = (const u32*)nr.bitmap.p;
    const NearSlot* tab = (const NearSlot*)nr.table.p;
    const u32* li = (const u32*)nr.list.p;
    const uint8_t* ar = (const uint8_t*)nr.arena.p;
    u32* tc = (u32*)l.tcount.p;
    u64* to = (u64*)l.toff.p;
    u32* fl = (u32*)nr.flag.p;
    HIPCHK(c, hipMemsetAsync(fl, 0, 4, st));
    hipLaunchKernelGGL((k_near_scan<NP, false>), dim3((u32)grid), dim3(LOC_T), lds, st, b, n, ng, bm, tab, (u64)(nr.slots - 1), li, ar,
                       ntiles, tc, (const u64*)nullptr, (kr_near_hit*)nullptr, fl);
    hipLaunchKernelGGL(k_loc_offsets, dim3(1), dim3(1024), 0, st, (const u32*)tc, ntiles, to);
    u64 total = 0;
    u32 over = 0;
    HIPCHK(c, hipMemcpyAsync(&total, to + ntiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&over, fl, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (over || total >= (1ull << 32))
        return fail(c, KR_ERR_CAPACITY, "kr_near_scan: 2^32 or more near matches in one genome (fewer mismatches or targets)");
    if (total) {
        int rc;
        if ((rc = ensure(c, nr.hits, total * sizeof(kr_near_hit))))
            return fail(c, rc, "kr_near_scan: %llu near matches do not fit the device (%s)", (unsigned long long)total, c->err.c_str());
        hipLaunchKernelGGL((k_near_scan<NP, true>), dim3((u32)grid), dim3(LOC_T), lds, st, b, n, ng, bm, tab, (u64)(nr.slots - 1), li, ar,
                           ntiles, tc, (const u64*)to, (kr_near_hit*)nr.hits.p, fl);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
    }
    *total_out = total;
    return KR_OK;
}
}  // extern "C++"

int64_t kr_near_scan(kr_ctx* c, int id) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto& l = c->loc;
    auto& nr = c->near;
    if (!nr.slots) return fail(c, KR_ERR_STATE, "kr_near_table first");
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    const Genome& G = it->second;
    HIPCHK(c, hipSetDevice(c->device));
    nr.nhits = 0;
    nr.gid = id;
    const u64 n = G.n_bases, k = (u64)l.k;
    const u64 nw = n >= k ? n - k + 1 : 0;
    const u64 TP = (u64)LOC_T * LOC_S;
    const u64 ntiles = (nw + TP - 1) / TP;
    if (!ntiles || !nr.ntargets) return 0;
    int rc;
    if ((rc = ensure(c, l.tcount, (ntiles + 1) * 4)) || (rc = ensure(c, l.toff, (ntiles + 1) * 8))) return rc;
    NearGeom ng;
    memset(&ng, 0, sizeof ng);
    ng.k = (u32)l.k; ng.omit = (u32)l.omit; ng.M = (u32)nr.M; ng.np = (u32)nr.M + 1;
    ng.lo[0] = (u32)l.L; ng.hi[0] = (u32)(l.L + l.D);             // '+': the text as the target has it
    ng.lo[1] = (u32)l.R; ng.hi[1] = (u32)(l.R + l.D);             // '-': its reverse complement, the right flank first
    for (u32 j = 0; j <= ng.np; j++) ng.off[j] = (u32)((u64)j * l.k / ng.np);
    for (u32 j = 0; j < ng.np; j++) ng.pw[j] = loc_pow((int)(ng.off[j + 1] - ng.off[j]) - 1);
    u64 total = 0;
    switch (ng.np) {
    case 1: rc = near_launch<1>(c, G, ng, ntiles, &total); break;
    case 2: rc = near_launch<2>(c, G, ng, ntiles, &total); break;
    case 3: rc = near_launch<3>(c, G, ng, ntiles, &total); break;
    default: rc = near_launch<4>(c, G, ng, ntiles, &total); break;
    }
    if (rc) {
        nr.nhits = -1;
        return rc;
    }
    nr.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_near_fetch(kr_ctx* c, kr_near_hit* out, size_t cap) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    const int64_t n = c->near.nhits;
    if (n < 0) return fail(c, KR_ERR_STATE, "kr_near_scan first");
    if ((size_t)n > cap) return fail(c, KR_ERR_CAPACITY, "hit buffer too small: %lld > %zu", (long long)n, cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(out, c->near.hits.p, (size_t)n * sizeof(kr_near_hit), hipMemcpyDeviceToHost));
    return n;
}

int64_t kr_near_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto& nr = c->near;
    if (nr.nhits < 0) return fail(c, KR_ERR_STATE, "kr_near_scan first");
    if (!rows || !nr.nhits) return nr.nhits;
    auto it = c->genomes.find(nr.gid);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d is gone", nr.gid);
    const u64 bytes = (u64)nr.nhits * c->loc.k;
    if (bytes > cap_bytes) return fail(c, KR_ERR_CAPACITY, "row buffer too small: %llu > %zu", (unsigned long long)bytes, cap_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, nr.rows, bytes))) return rc;
    const u32 grid = (u32)std::min<u64>((bytes + 255) / 256, (u64)c->ncu * 16);
    hipLaunchKernelGGL(k_near_cut, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)it->second.bases.p,
                       (const kr_near_hit*)nr.hits.p, (u64)nr.nhits, (u32)c->loc.k, (uint8_t*)nr.rows.p);
    HIPCHK(c, hipMemcpyAsync(rows, nr.rows.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return nr.nhits;
}
