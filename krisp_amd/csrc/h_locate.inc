// h_locate.inc -- part of krisp_hip.hip (one translation unit): host side of the locate pass (k_locate.inc): a context that
// only uploads genomes, the flank table of the surviving groups, the scan of one genome, its record separators.
// One genome is resident at a time (the caller uploads the next under the same id); beside it live the table (16 bytes a
// slot, >= 2 slots a group), the flank text, the bitmap, the per-tile counts and the hits.

int kr_set_params_locate(kr_ctx* c, int L, int D, int R, int softmask_mode, size_t max_bases) {
    if (!c) return KR_ERR_PARAM;
    const int k = L + D + R;
    if (L < 0 || L > KR_WIDE_MAX_FLANK || R < 0 || R > KR_WIDE_MAX_FLANK || D < 0 || k < 1 || k > KR_WIDE_MAX_K)
        return fail(c, KR_ERR_PARAM, "locate needs 0 <= L, R <= %d and 1 <= L+D+R <= %d (got %d/%d/%d)", KR_WIDE_MAX_FLANK,
                    KR_WIDE_MAX_K, L, D, R);
    if (softmask_mode != KR_SOFT_MAP && softmask_mode != KR_SOFT_OMIT)
        return fail(c, KR_ERR_PARAM, "unknown softmask mode %d", softmask_mode);
    if (!c->genomes.empty()) return fail(c, KR_ERR_STATE, "kr_set_params_locate after genomes were uploaded");
    if (max_bases >= KR_MAX_BASES) return fail(c, KR_ERR_PARAM, "genomes of >= 2^33 bases are not supported");
    auto& l = c->loc;
    l.on = true;
    l.L = L; l.D = D; l.R = R; l.k = k;
    l.omit = softmask_mode == KR_SOFT_OMIT;
    l.ngroups = l.slots = 0;
    l.nhits = -1;
    c->near.slots = c->near.ntargets = 0;       // (a table of another geometry: kr_near_table again)
    c->near.nhits = -1;
    c->prod.slots = 0;                          // (likewise: kr_products_table again)
    c->prod.nsites = c->prod.nhits = -1;
    c->wide.on = false;
    c->max_bases = max_bases;
    c->have_params = true;
    return KR_OK;
}

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

int64_t kr_locate_table(kr_ctx* c, const uint8_t* flanks, uint64_t ngroups) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    if (!flanks && ngroups) return fail(c, KR_ERR_PARAM, "kr_locate_table: null flanks");
    if (ngroups >= LOC_EMPTY) return fail(c, KR_ERR_CAPACITY, "kr_locate_table: %llu groups (the limit is %u)",
                                          (unsigned long long)ngroups, LOC_EMPTY - 1);
    auto& l = c->loc;
    const int L = l.L, R = l.R, LR = L + R;
    u64 slots = 1024;
    while (slots < 2 * ngroups) slots <<= 1;
    std::vector<LocSlot> tab;
    std::vector<u32> bm;
    try {
        tab.assign(slots, LocSlot{0, LOC_EMPTY, 0});
        bm.assign(LOC_BM_WORDS, 0u);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_locate_table: no host memory for %llu slots", (unsigned long long)slots);
    }
    const u64 mask = slots - 1;
    for (u64 g = 0; g < ngroups; g++) {
        const uint8_t* f = flanks + g * LR;
        const u64 h = loc_mix(loc_hash(f, L), loc_hash(f + L, R));
        u64 i = h & mask;
        for (; tab[i].gid != LOC_EMPTY; i = (i + 1) & mask)
            if (tab[i].h == h && !memcmp(flanks + (u64)tab[i].gid * LR, f, LR))
                return fail(c, KR_ERR_PARAM, "kr_locate_table: group %llu repeats the flanks of group %u", (unsigned long long)g,
                            tab[i].gid);
        tab[i].h = h;
        tab[i].gid = (u32)g;
        const u32 b = (u32)(h >> (64 - LOC_BM_LOG));
        bm[b >> 5] |= 1u << (b & 31);
    }
    int rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, l.table, slots * sizeof(LocSlot))) || (rc = ensure(c, l.arena, ngroups * LR + 16)) ||
        (rc = ensure(c, l.bitmap, (size_t)LOC_BM_WORDS * 4)))
        return fail(c, rc, "kr_locate_table: the table of %llu groups does not fit the device (%s)", (unsigned long long)ngroups,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(l.table.p, tab.data(), slots * sizeof(LocSlot), hipMemcpyHostToDevice));
    if (ngroups * LR) HIPCHK(c, hipMemcpy(l.arena.p, flanks, ngroups * LR, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(l.bitmap.p, bm.data(), (size_t)LOC_BM_WORDS * 4, hipMemcpyHostToDevice));
    l.ngroups = ngroups;
    l.slots = slots;
    l.nhits = -1;
    return (int64_t)slots;
}

static size_t loc_lds_bytes(int k) {
    const u32 tb = LOC_T * LOC_S + k - 1;
    return (size_t)LOC_BM_WORDS * 4 + LOC_T * 4 + 256 + (((tb + 16) + ((tb + 16) >> LOC_SH) * 4 + 15) & ~15u);
}

int64_t kr_locate_scan(kr_ctx* c, int id) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto& l = c->loc;
    if (!l.slots) return fail(c, KR_ERR_STATE, "kr_locate_table first");
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    const Genome& G = it->second;
    HIPCHK(c, hipSetDevice(c->device));
    l.nhits = 0;
    l.gid = id;
    const u64 n = G.n_bases, k = (u64)l.k;
    const u64 nw = n >= k ? n - k + 1 : 0;
    const u64 TP = (u64)LOC_T * LOC_S;
    const u64 ntiles = (nw + TP - 1) / TP;
    if (!ntiles || !l.ngroups) return 0;
    int rc;
    if ((rc = ensure(c, l.tcount, (ntiles + 1) * 4)) || (rc = ensure(c, l.toff, (ntiles + 1) * 8))) return rc;
    LocGeom lg;
    lg.L = (u32)l.L; lg.D = (u32)l.D; lg.R = (u32)l.R; lg.k = (u32)l.k; lg.omit = (u32)l.omit;
    u32 inv = LOC_HB;
    for (int i = 0; i < 5; i++) inv *= 2u - LOC_HB * inv;         // Newton: LOC_HB * inv == 1 mod 2^32
    lg.binv = inv;
    lg.powL = l.L ? loc_pow(l.L - 1) : 0u;
    lg.powR = l.R ? loc_pow(l.R - 1) : 0u;
    const size_t lds = loc_lds_bytes(l.k);
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_loc_scan<false>, LOC_T, lds) != hipSuccess || per < 1) {
        (void)hipGetLastError();
        per = 1;
    }
    const u64 grid = std::min<u64>(ntiles, (u64)c->ncu * per);
    hipStream_t st = c->stream;
    const uint8_t* b = (const uint8_t*)G.bases.p;
    const u32* bm = (const u32*)l.bitmap.p;
    const LocSlot* tab = (const LocSlot*)l.table.p;
    const uint8_t* ar = (const uint8_t*)l.arena.p;
    u32* tc = (u32*)l.tcount.p;
    u64* to = (u64*)l.toff.p;
    hipLaunchKernelGGL(k_loc_scan<false>, dim3((u32)grid), dim3(LOC_T), lds, st, b, n, lg, bm, tab, (u64)(l.slots - 1), ar, ntiles,
                       tc, (const u64*)nullptr, (kr_loc_hit*)nullptr);
    hipLaunchKernelGGL(k_loc_offsets, dim3(1), dim3(1024), 0, st, (const u32*)tc, ntiles, to);
    u64 total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, to + ntiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (total) {
        if ((rc = ensure(c, l.hits, total * sizeof(kr_loc_hit))))
            return fail(c, rc, "kr_locate_scan: %llu hits of genome %d do not fit the device (%s)", (unsigned long long)total, id,
                        c->err.c_str());
        hipLaunchKernelGGL(k_loc_scan<true>, dim3((u32)grid), dim3(LOC_T), lds, st, b, n, lg, bm, tab, (u64)(l.slots - 1), ar,
                           ntiles, tc, (const u64*)to, (kr_loc_hit*)l.hits.p);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
    }
    l.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_locate_fetch(kr_ctx* c, kr_loc_hit* out, size_t cap) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    const int64_t n = c->loc.nhits;
    if (n < 0) return fail(c, KR_ERR_STATE, "kr_locate_scan first");
    if ((size_t)n > cap) return fail(c, KR_ERR_CAPACITY, "hit buffer too small: %lld > %zu", (long long)n, cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(out, c->loc.hits.p, (size_t)n * sizeof(kr_loc_hit), hipMemcpyDeviceToHost));
    return n;
}

int64_t kr_locate_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto& l = c->loc;
    if (l.nhits < 0) return fail(c, KR_ERR_STATE, "kr_locate_scan first");
    if (!rows || !l.nhits) return l.nhits;
    auto it = c->genomes.find(l.gid);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d is gone", l.gid);
    const u64 bytes = (u64)l.nhits * l.k;
    if (bytes > cap_bytes) return fail(c, KR_ERR_CAPACITY, "row buffer too small: %llu > %zu", (unsigned long long)bytes, cap_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, l.rows, bytes))) return rc;
    const u32 grid = (u32)std::min<u64>((bytes + 255) / 256, (u64)c->ncu * 16);
    hipLaunchKernelGGL(k_loc_cut, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)it->second.bases.p,
                       (const kr_loc_hit*)l.hits.p, (u64)l.nhits, (u32)l.k, (uint8_t*)l.rows.p);
    HIPCHK(c, hipMemcpyAsync(rows, l.rows.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return l.nhits;
}

int64_t kr_locate_seps(kr_ctx* c, int id, uint64_t* out, size_t cap) {
    if (!c || !c->loc.on) return fail(c, KR_ERR_STATE, "kr_set_params_locate first");
    auto it = c->genomes.find(id);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d not uploaded", id);
    const Genome& G = it->second;
    auto& l = c->loc;
    HIPCHK(c, hipSetDevice(c->device));
    const u64 n = G.n_bases, TB = (u64)LOC_T * LOC_SEP_BYTES;
    const u64 ntiles = (n + TB - 1) / TB;
    if (!ntiles) return 0;
    if (ntiles >= (1ull << 31)) return fail(c, KR_ERR_PARAM, "kr_locate_seps: %llu bases", (unsigned long long)n);
    int rc;
    if ((rc = ensure(c, l.tcount, (ntiles + 1) * 4)) || (rc = ensure(c, l.toff, (ntiles + 1) * 8))) return rc;
    hipStream_t st = c->stream;
    const uint8_t* b = (const uint8_t*)G.bases.p;
    u32* tc = (u32*)l.tcount.p;
    u64* to = (u64*)l.toff.p;
    hipLaunchKernelGGL(k_loc_sep<false>, dim3((u32)ntiles), dim3(LOC_T), 0, st, b, n, tc, (const u64*)nullptr, (u64*)nullptr);
    hipLaunchKernelGGL(k_loc_offsets, dim3(1), dim3(1024), 0, st, (const u32*)tc, ntiles, to);
    u64 total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, to + ntiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (!out || !total) return (int64_t)total;
    if (total > cap) return fail(c, KR_ERR_CAPACITY, "separator buffer too small: %llu > %zu", (unsigned long long)total, cap);
    if ((rc = ensure(c, l.seps, total * 8))) return rc;
    hipLaunchKernelGGL(k_loc_sep<true>, dim3((u32)ntiles), dim3(LOC_T), 0, st, b, n, tc, (const u64*)to, (u64*)l.seps.p);
    HIPCHK(c, hipMemcpyAsync(out, l.seps.p, total * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return (int64_t)total;
}
