// h_locate.inc -- part of krisp_hip.hip (one translation unit): host side of the locate pass (k_locate.inc): a context that
// only uploads genomes, the flank table of the surviving groups, the scan of one genome, its record separators.  What it
// shares with the five seed passes is h_scan.inc.
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
    coarse_pool_release(c);
    if (max_bases >= KR_MAX_BASES) return fail(c, KR_ERR_PARAM, "genomes of >= 2^33 bases are not supported");
    auto& l = c->loc;
    l.on = true;
    l.L = L; l.D = D; l.R = R; l.k = k;
    l.omit = softmask_mode == KR_SOFT_OMIT;
    l.ngroups = l.slots = 0;
    l.nhits = -1;
    // a table of another geometry (the primer pass: of another soft-mask mode) is no table: kr_*_table again
    c->near.reset(); c->ghit.reset(); c->gbulge.reset(); c->prod.reset(); c->prim.reset(); c->assay.reset(); c->mux.reset(); c->pclean.reset();
    c->wide.on = false;
    c->max_bases = max_bases;
    c->have_params = true;
    return KR_OK;
}

int64_t kr_locate_table(kr_ctx* c, const uint8_t* flanks, uint64_t ngroups) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
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

int64_t kr_locate_scan(kr_ctx* c, int id) {
    const Genome* G;
    int rc;
    if ((rc = scan_genome(c, id, c && c->loc.slots, "kr_locate_table first", &G))) return rc;
    auto& l = c->loc;
    l.nhits = 0;
    l.gid = id;
    u64 nw;
    const u64 n = G->n_bases, ntiles = scan_tiles(n, (u64)l.k, &nw);
    if (!ntiles || !l.ngroups) return 0;
    LocGeom lg;
    lg.L = (u32)l.L; lg.D = (u32)l.D; lg.R = (u32)l.R; lg.k = (u32)l.k; lg.omit = (u32)l.omit;
    u32 inv = LOC_HB;
    for (int i = 0; i < 5; i++) inv *= 2u - LOC_HB * inv;         // Newton: LOC_HB * inv == 1 mod 2^32
    lg.binv = inv;
    lg.powL = l.L ? loc_pow(l.L - 1) : 0u;
    lg.powR = l.R ? loc_pow(l.R - 1) : 0u;
    const size_t lds = scan_lds_bytes((u32)l.k, LOC_T * 4 + 256);     // (a 32-bit scan array, comp)
    const u32 grid = scan_grid(c, k_loc_scan<false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_loc_hit* out) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G->bases.p, n, lg, (const u32*)l.bitmap.p,
                           (const LocSlot*)l.table.p, (u64)(l.slots - 1), (const uint8_t*)l.arena.p, ntiles, tc, to, out);
    };
    u64 total = 0;
    rc = scan_two_pass(
        c, ntiles, nullptr, [&](u32* tc, u32*) { launch(k_loc_scan<false>, tc, nullptr, nullptr); },
        [&](u64 total) {
            const int rc = ensure(c, l.hits, total * sizeof(kr_loc_hit));
            return rc ? fail(c, rc, "kr_locate_scan: %llu hits of genome %d do not fit the device (%s)", (unsigned long long)total, id,
                             c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32*) { launch(k_loc_scan<true>, tc, to, (kr_loc_hit*)l.hits.p); }, &total);
    if (rc) return rc;
    l.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_locate_fetch(kr_ctx* c, kr_loc_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    return scan_fetch(c, c->loc.nhits, "kr_locate_scan first", "hit", c->loc.hits, out, cap, sizeof(kr_loc_hit));
}

int64_t kr_locate_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& l = c->loc;
    return scan_windows(c, l.nhits, l.gid, "kr_locate_scan first", (u32)l.k, l.rows, rows, cap_bytes, scan_cut_k<kr_loc_hit>(c, l));
}

int64_t kr_locate_seps(kr_ctx* c, int id, uint64_t* out, size_t cap) {
    const Genome* G;
    int rc;
    if ((rc = scan_genome(c, id, true, nullptr, &G))) return rc;
    auto& l = c->loc;
    u64 total = 0;
    rc = scan_seps(
        c, *G, "kr_locate_seps", l.seps,
        [&](u64 total) {
            if (!out) return SCAN_COUNT_ONLY;
            if (total > cap) return fail(c, KR_ERR_CAPACITY, "separator buffer too small: %llu > %zu", (unsigned long long)total, cap);
            return ensure(c, l.seps, total * 8);
        },
        &total);
    if (rc) return rc;
    if (out && total) HIPCHK(c, hipMemcpy(out, l.seps.p, total * 8, hipMemcpyDeviceToHost));
    return (int64_t)total;
}
