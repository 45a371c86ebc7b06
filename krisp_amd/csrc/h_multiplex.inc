// h_multiplex.inc -- part of krisp_hip.hip (one translation unit): host side of the multiplex pass (k_multiplex.inc, DESIGN
// §24): the seed table of a panel's oligos, the scan of one genome (separators, sites, records, the join of every opening
// with every closing site), its products, sites and tally.  The state is kr_ctx::mux, the primer pass's state once more:
// a kr_primers_* table, its lists and the assay links in the same context are not touched.  The table's entries, the site
// scan and what runs before the join are h_primers.inc's and h_products.inc's (prim_lengths, prim_entries, prim_sites,
// prod_scan_sites).  Beside the genome live the entries' text (2 bytes a letter) and offsets, the table, the entry list,
// the bitmap, the separators (8 bytes each), the sites (16 + 4 bytes each), the products (24 bytes each) and 2 T^2 counters.
#define MUX_MAX_TEXTS 128

int64_t kr_multiplex_table(kr_ctx* c, const uint8_t* text, const uint32_t* offsets, uint64_t ntexts, int mismatches, uint32_t max_product) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& mx = c->mux;
    const int M = mismatches;
    mx.seed.slots = 0;
    mx.nsites = mx.nhits = -1;
    if (M < 0 || M >= NEAR_MAXP)
        return fail(c, KR_ERR_PARAM, "kr_multiplex_table: 0 <= mismatches <= %d (got %d)", NEAR_MAXP - 1, M);
    if (ntexts < 1 || ntexts > MUX_MAX_TEXTS)
        return fail(c, KR_ERR_PARAM, "kr_multiplex_table: 1 .. %d texts are taken (got %llu)", MUX_MAX_TEXTS, (unsigned long long)ntexts);
    if (!text || !offsets) return fail(c, KR_ERR_PARAM, "kr_multiplex_table: null table");
    u32 smin, maxlen;
    if ((rc = prim_lengths(c, "kr_multiplex_table", offsets, ntexts, &smin, &maxlen))) return rc;
    // (with that bound every ordered pair of texts can form a product, and the join's max_product - smin cannot wrap)
    if ((u64)max_product < 2ull * maxlen)
        return fail(c, KR_ERR_PARAM, "kr_multiplex_table: max_product %u is shorter than twice the longest text (%u letters)", max_product,
                    maxlen);
    mx.M = M; mx.max_product = max_product; mx.nleft = ntexts; mx.nright = 0; mx.plist.npairs = 0;
    mx.smin = smin; mx.maxlen = maxlen;
    PrimGeom pg;
    prim_geom(c, mx, &pg);
    std::vector<uint8_t> arena;
    std::vector<u32> eoff;
    SeedKeys keyed;
    try {
        prim_entries(text, offsets, ntexts, pg, (u32)M + 1, arena, eoff, keyed);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_multiplex_table: no host memory for the table of %llu texts", (unsigned long long)ntexts);
    }
    const int64_t slots = seed_table_build(c, keyed, arena, mx.seed, "kr_multiplex_table", ntexts, "texts");
    if (slots < 0) return slots;
    if ((rc = ensure(c, mx.eoff, eoff.size() * 4)))
        return fail(c, rc, "kr_multiplex_table: the table of %llu texts does not fit the device (%s)", (unsigned long long)ntexts,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(mx.eoff.p, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice));
    mx.seed.slots = (u64)slots;
    return slots;
}

// the join of the ns sites on the device -> the number of products (h_products.inc's prod_join without a pair list)
static int mux_join(kr_ctx* c, const PrimGeom& pg, u64 ns, u64* total_out) {
    auto& mx = c->mux;
    *total_out = 0;
    if (!ns) return KR_OK;
    const u64 nblocks = (ns + LOC_T - 1) / LOC_T;                 // (ns < 2^32: < 2^24 blocks)
    auto launch = [&](auto kernel, u32* bc, const u64* bo, kr_multiplex_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, (const kr_product_site*)mx.sites.p, ns,
                           (const u32*)mx.rec.p, pg, (const u32*)mx.eoff.p, mx.max_product, bc, bo, out, fl);
    };
    return scan_two_pass(
        c, nblocks, "kr_multiplex_scan: 2^32 or more products in one genome (a smaller max_product, fewer mismatches or oligos)",
        [&](u32* bc, u32* fl) { launch(k_mux_join<false>, bc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, mx.hits, total * sizeof(kr_multiplex_hit));
            return rc ? fail(c, rc, "kr_multiplex_scan: %llu products do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* bc, const u64* bo, u32* fl) { launch(k_mux_join<true>, bc, bo, (kr_multiplex_hit*)mx.hits.p, fl); }, total_out);
}

int64_t kr_multiplex_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->mux.seed.slots, "kr_multiplex_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& mx = c->mux;
    mx.gid = id;
    PrimGeom pg;
    prim_geom(c, mx, &pg);
    auto sites = [&](u64 nw, u64 ntiles, u64* ns) {
        return prim_sites(c, G, mx, pg, nw, ntiles, "kr_multiplex_scan",
                          "kr_multiplex_scan: 2^32 or more primer sites in one genome (fewer mismatches or oligos)", ns);
    };
    u64 ns = 0, np = 0;
    if ((rc = prod_scan_sites(c, G, mx, pg.smin, "kr_multiplex_scan", sites, &ns))) return rc;
    if ((rc = mux_join(c, pg, ns, &np))) return rc;
    mx.nsites = (int64_t)ns;
    mx.nhits = (int64_t)np;
    return (int64_t)np;
}

// the products in (pos, length, fwd, rev) order: the device lists them by opening site, so positions ascend already
int64_t kr_multiplex_fetch(kr_ctx* c, kr_multiplex_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const auto& mx = c->mux;
    const int64_t n = scan_fetch(c, mx.nhits, "kr_multiplex_scan first", "product", mx.hits, out, cap, sizeof(kr_multiplex_hit));
    auto less = [](const kr_multiplex_hit& a, const kr_multiplex_hit& b) {
        if (a.length != b.length) return a.length < b.length;
        if (a.fwd != b.fwd) return a.fwd < b.fwd;
        return a.rev < b.rev;
    };
    for (int64_t i = 0; i < n;) {
        int64_t j = i + 1;
        while (j < n && out[j].pos == out[i].pos) j++;
        if (j - i > 1) std::sort(out + i, out + j, less);
        i = j;
    }
    return n;
}

int64_t kr_multiplex_sites(kr_ctx* c, kr_product_site* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const auto& mx = c->mux;
    if (mx.nsites >= 0 && !out) return mx.nsites;   // (the count alone)
    return scan_fetch(c, mx.nsites, "kr_multiplex_scan first", "site", mx.sites, out, cap, sizeof(kr_product_site));
}

// the products of the latest scan counted per ordered pair and clean ends (k_mux_tally): out[2 (a T + b) + clean]
int64_t kr_multiplex_tally(kr_ctx* c, uint32_t* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& mx = c->mux;
    if (mx.nhits < 0) return fail(c, KR_ERR_STATE, "kr_multiplex_scan first");
    const u64 T = mx.nleft, n = 2 * T * T;                         // (T <= 128: 32 768 counters at most)
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "kr_multiplex_tally: tally buffer too small: %llu > %zu", (unsigned long long)n, cap);
    if (!out) return fail(c, KR_ERR_PARAM, "kr_multiplex_tally: null argument");
    if (!mx.nhits) {
        memset(out, 0, n * sizeof(u32));
        return (int64_t)n;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, mx.tally, n * sizeof(u32)))) return rc;
    HIPCHK(c, hipMemsetAsync(mx.tally.p, 0, n * sizeof(u32), c->stream));
    const u64 nhits = (u64)mx.nhits;
    hipLaunchKernelGGL(k_mux_tally, dim3(scan_stride_grid(c, (nhits + 255) / 256)), dim3(256), 0, c->stream,
                       (const kr_multiplex_hit*)mx.hits.p, nhits, (u32)T, (u32*)mx.tally.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, mx.tally.p, n * sizeof(u32), hipMemcpyDeviceToHost));
    return (int64_t)n;
}
