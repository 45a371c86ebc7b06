// h_assay.inc -- part of krisp_hip.hip (one translation unit): host side of the assay join (k_assay.inc): the link table,
// the join of the primer pass's products with the guide-hit pass's hits, its rows.  The context is the locate context of
// both passes (kr_set_params_locate with L+D+R = the protospacer length G); the state is kr_ctx::assay: the links (8 bytes
// each) and the assay hits (48 bytes each), sized by the largest join so far.  Which genome each list is of is the passes'
// own (prim.gid, ghit.gid); a new table of either pass drops its list (nhits < 0) and the links (assay.reset()), a new scan
// of either drops the join.  The two-pass driver and the fetch are h_scan.inc's.

int64_t kr_assay_table(kr_ctx* c, const uint32_t* links, uint64_t n) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& as = c->assay;
    if (!c->prim.seed.slots) return fail(c, KR_ERR_STATE, "kr_assay_table: kr_primers_table first");
    if (!c->ghit.seed.slots) return fail(c, KR_ERR_STATE, "kr_assay_table: kr_guide_hits_table first");
    if (!links && n) return fail(c, KR_ERR_PARAM, "kr_assay_table: null links");
    const u64 npairs = c->prim.plist.npairs, nguides = c->ghit.nguides;
    std::vector<u64> keys;
    try {
        keys.resize(n + 1);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_assay_table: no host memory for %llu links", (unsigned long long)n);
    }
    for (u64 i = 0; i < n; i++) {
        const u32 p = links[2 * i], g = links[2 * i + 1];
        if (p >= npairs || g >= nguides)
            return fail(c, KR_ERR_PARAM, "kr_assay_table: link %llu names (pair %u, guide %u) of (%llu, %llu)", (unsigned long long)i, p, g,
                        (unsigned long long)npairs, (unsigned long long)nguides);
        keys[i] = ((u64)p << 32) | g;
        if (i && keys[i] <= keys[i - 1])
            return fail(c, KR_ERR_PARAM, "kr_assay_table: link %llu does not lie behind link %llu (ascending, each once)",
                        (unsigned long long)i, (unsigned long long)(i - 1));
    }
    keys[n] = ~0ull;
    as.reset();                                     // (from here on the device's copy of an earlier table is written over)
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, as.links, keys.size() * 8)))
        return fail(c, rc, "kr_assay_table: %llu links do not fit the device (%s)", (unsigned long long)n, c->err.c_str());
    HIPCHK(c, hipMemcpy(as.links.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice));
    as.nlinks = n;
    as.on = true;
    return (int64_t)n;
}

int64_t kr_assay_join(kr_ctx* c, int id) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& as = c->assay;
    auto& pm = c->prim;
    auto& gh = c->ghit;
    as.nhits = -1;
    if (!as.on) return fail(c, KR_ERR_STATE, "kr_assay_join: kr_assay_table first");
    // (a new table of either pass left its list at nhits < 0, and dropped the links)
    if (pm.nhits < 0 || !pm.seed.slots) return fail(c, KR_ERR_STATE, "kr_assay_join: kr_primers_scan first");
    if (gh.nhits < 0 || !gh.seed.slots) return fail(c, KR_ERR_STATE, "kr_assay_join: kr_guide_hits_scan first");
    if (pm.gid != id || gh.gid != id)
        return fail(c, KR_ERR_STATE, "kr_assay_join: genome %d, but the products are of genome %d and the hits of genome %d", id, pm.gid,
                    gh.gid);
    const u64 np = (u64)pm.nhits, nh = (u64)gh.nhits;
    if (!np || !nh || !as.nlinks) {
        as.nhits = 0;
        return 0;
    }
    HIPCHK(c, hipSetDevice(c->device));
    AssayLists a;
    a.prods = (const kr_product_hit*)pm.hits.p;
    a.hits = (const kr_guide_hit*)gh.hits.p;
    a.plen = (const u32*)pm.plen.p;
    a.links = (const u64*)as.links.p;
    a.np = np; a.nh = nh; a.nl = as.nlinks;
    a.npairs = (u32)pm.plist.npairs;
    a.G = (u32)c->loc.k;
    const u64 nblocks = (np + LOC_T - 1) / LOC_T;                 // (np < 2^32: < 2^24 blocks)
    u64 total = 0;
    rc = scan_two_pass(
        c, nblocks, "kr_assay_join: 2^32 or more assay hits in one genome (fewer mismatches or a smaller max_product)",
        [&](u32* bc, u32* fl) {
            hipLaunchKernelGGL(k_assay_join<false>, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, a, bc, (const u64*)nullptr,
                               (kr_assay_hit*)nullptr, fl);
        },
        [&](u64 n) {
            const int rc = ensure(c, as.hits, n * sizeof(kr_assay_hit));
            return rc ? fail(c, rc, "kr_assay_join: %llu assay hits do not fit the device (%s)", (unsigned long long)n, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* bc, const u64* bo, u32* fl) {
            hipLaunchKernelGGL(k_assay_join<true>, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, a, bc, bo, (kr_assay_hit*)as.hits.p, fl);
        },
        &total);
    if (rc) return rc;
    as.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_assay_fetch(kr_ctx* c, kr_assay_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    if (c->assay.nhits >= 0 && !out) return c->assay.nhits;      // (the count alone)
    const int64_t n = scan_fetch(c, c->assay.nhits, "kr_assay_join first", "assay hit", c->assay.hits, out, cap, sizeof(kr_assay_hit));
    // the rows of one product position in (length, strand, pair, hit_pos, hit_strand, guide) order (the device lists them by
    // opening site, so positions ascend already: prod_sort_positions does the same for the products)
    auto less = [](const kr_assay_hit& x, const kr_assay_hit& y) {
        if (x.length != y.length) return x.length < y.length;
        if (x.strand != y.strand) return x.strand < y.strand;
        if (x.pair != y.pair) return x.pair < y.pair;
        if (x.hit_pos != y.hit_pos) return x.hit_pos < y.hit_pos;
        if (x.hit_strand != y.hit_strand) return x.hit_strand < y.hit_strand;
        return x.guide < y.guide;
    };
    for (int64_t i = 0; i < n;) {
        int64_t j = i + 1;
        while (j < n && out[j].pos == out[i].pos) j++;
        if (j - i > 1) std::sort(out + i, out + j, less);
        i = j;
    }
    return n;
}
