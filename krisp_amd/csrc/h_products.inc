// h_products.inc -- part of krisp_hip.hip (one translation unit): host side of the product pass (k_products.inc): the seed
// table of the flank texts and the pair list, the scan of one genome (separators, sites, records, join), its products and
// sites.  The context is the locate context (kr_set_params_locate): one genome resident at a time.  Beside the genome live
// the entries' text (2 bytes a letter of a text), the table (16 bytes a slot, >= 2 slots a distinct piece), the entry list,
// the bitmap, the pair list (12 bytes a pair), the separators (8 bytes each), the sites (16 + 4 bytes each) and the
// products (24 bytes each).

static void prod_geom(const kr_ctx* c, ProdGeom* pg) {
    const auto& l = c->loc;
    const auto& pr = c->prod;
    memset(pg, 0, sizeof *pg);
    pg->len[0] = (u32)l.L; pg->len[1] = (u32)l.R;
    pg->omit = (u32)l.omit; pg->M = (u32)pr.M; pg->nleft2 = (u32)(2 * pr.nleft);
    pg->maxlen = std::max(pg->len[0], pg->len[1]);
    const u32 NP = (u32)pr.M + 1;
    for (int q = 0; q < 2; q++) {
        pg->end[q] = std::min<u32>(PROD_END, pg->len[q]);
        for (u32 j = 0; j <= NP; j++) pg->off[q][j] = (u32)((u64)j * pg->len[q] / NP);
        for (u32 j = 0; j < NP; j++) pg->pw[q][j] = loc_pow((int)(pg->off[q][j + 1] - pg->off[q][j]) - 1);
    }
}

int64_t kr_products_table(kr_ctx* c, const uint8_t* left, uint64_t nleft, const uint8_t* right, uint64_t nright,
                          const uint32_t* pairs, uint64_t npairs, int mismatches, uint32_t max_product) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& l = c->loc;
    auto& pr = c->prod;
    const int Le = l.L, Re = l.R, M = mismatches;
    if (M < 0 || M >= NEAR_MAXP || M >= std::min(Le, Re))
        return fail(c, KR_ERR_PARAM, "kr_products_table: 0 <= mismatches <= %d and mismatches < min(L, R) = %d (got %d)", NEAR_MAXP - 1,
                    std::min(Le, Re), M);
    if ((u64)max_product < (u64)Le + Re)
        return fail(c, KR_ERR_PARAM, "kr_products_table: max_product %u is shorter than the two flanks (%d + %d)", max_product, Le, Re);
    if ((!left && nleft) || (!right && nright) || (!pairs && npairs)) return fail(c, KR_ERR_PARAM, "kr_products_table: null table");
    if (nleft + nright >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_products_table: %llu flank texts (the limit is %u)", (unsigned long long)(nleft + nright),
                    (1u << 24) - 1);
    if (npairs >= LOC_EMPTY) return fail(c, KR_ERR_CAPACITY, "kr_products_table: %llu pairs (the limit is %u)",
                                         (unsigned long long)npairs, LOC_EMPTY - 1);
    pr.slots = 0;
    pr.nsites = pr.nhits = -1;
    pr.M = M; pr.max_product = max_product; pr.nleft = nleft; pr.nright = nright; pr.npairs = npairs;
    ProdGeom pg;
    prod_geom(c, &pg);
    const u32 NP = (u32)M + 1;
    const bool one = Le == Re;                      // one length class: the left and right entries share their keys
    const u64 ne = 2 * (nleft + nright), nk = ne * NP;
    std::vector<uint8_t> text;
    std::vector<std::pair<u64, u32>> keyed;
    std::vector<u32> pidx;
    std::vector<std::pair<u64, u32>> pk;
    try {
        text.resize(2 * (nleft * Le + nright * Re) + 16);
        for (u64 e = 0; e < ne; e += 2) {
            const bool lf = e < 2 * nleft;
            const int n = lf ? Le : Re;
            const uint8_t* s = lf ? left + (e >> 1) * Le : right + ((e >> 1) - nleft) * Re;
            uint8_t* f = text.data() + prod_text_at(pg, (u32)e);
            for (int i = 0; i < n; i++) {
                f[i] = s[i];
                f[n + i] = loc_comp(s[n - 1 - i]);
            }
        }
        keyed.reserve(nk);
        for (u64 e = 0; e < ne; e++) {
            const u32 q = prod_class(pg, (u32)e);
            for (u32 j = 0; j < NP; j++)
                keyed.emplace_back(near_key((one ? 0u : q) * NEAR_MAXP + j, loc_hash(text.data() + prod_text_at(pg, (u32)e) + pg.off[q][j],
                                                                                     (int)(pg.off[q][j + 1] - pg.off[q][j]))),
                                   (u32)e);
        }
        pk.reserve(npairs);
        for (u64 p = 0; p < npairs; p++) {
            if (pairs[2 * p] >= nleft || pairs[2 * p + 1] >= nright)
                return fail(c, KR_ERR_PARAM, "kr_products_table: pair %llu names text (%u, %u) of (%llu, %llu)", (unsigned long long)p,
                            pairs[2 * p], pairs[2 * p + 1], (unsigned long long)nleft, (unsigned long long)nright);
            pk.emplace_back(((u64)pairs[2 * p] << 32) | pairs[2 * p + 1], (u32)p);
        }
        std::sort(pk.begin(), pk.end());
        for (u64 p = 1; p < npairs; p++)
            if (pk[p].first == pk[p - 1].first)
                return fail(c, KR_ERR_PARAM, "kr_products_table: pair %u repeats the texts of pair %u", pk[p].second, pk[p - 1].second);
        pidx.resize(npairs + 1);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_products_table: no host memory for the table of %llu texts", (unsigned long long)(nleft + nright));
    }
    std::vector<u64> pkeys(npairs + 1);
    for (u64 p = 0; p < npairs; p++) {
        pkeys[p] = pk[p].first;
        pidx[p] = pk[p].second;
    }
    const int64_t slots = seed_table_build(c, keyed, text, pr.table, pr.arena, pr.list, pr.bitmap, "kr_products_table", nleft + nright,
                                           "texts");
    if (slots < 0) return slots;
    if ((rc = ensure(c, pr.pairkeys, pkeys.size() * 8)) || (rc = ensure(c, pr.pairidx, pidx.size() * 4)))
        return fail(c, rc, "kr_products_table: the table of %llu texts does not fit the device (%s)", (unsigned long long)(nleft + nright),
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(pr.pairkeys.p, pkeys.data(), pkeys.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pr.pairidx.p, pidx.data(), pidx.size() * 4, hipMemcpyHostToDevice));
    pr.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
template <u32 NP, u32 NC>
static int prod_sites_launch(kr_ctx* c, const Genome& G, const ProdGeom& pg, u64 nw, u64 ntiles, u64* total_out) {
    auto& pr = c->prod;
    const size_t lds = scan_lds_bytes(pg.maxlen, LOC_T * 8);      // (a 64-bit scan array)
    const u32 grid = scan_grid(c, k_prod_scan<NP, NC, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_product_site* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, pg,
                           (const u32*)pr.bitmap.p, (const NearSlot*)pr.table.p, (u64)(pr.slots - 1), (const u32*)pr.list.p,
                           (const uint8_t*)pr.arena.p, nw, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, "kr_products_scan: 2^32 or more primer sites in one genome (fewer mismatches or regions)",
        [&](u32* tc, u32* fl) { launch(k_prod_scan<NP, NC, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) -> int {
            int rc;
            if ((rc = ensure(c, pr.sites, total * sizeof(kr_product_site))) || (rc = ensure(c, pr.rec, total * 4)))
                return fail(c, rc, "kr_products_scan: %llu primer sites do not fit the device (%s)", (unsigned long long)total,
                            c->err.c_str());
            return KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_prod_scan<NP, NC, true>, tc, to, (kr_product_site*)pr.sites.p, fl); },
        total_out);
}
}  // extern "C++"

// the join of the sites on the device: -> the number of products
static int prod_join(kr_ctx* c, const ProdGeom& pg, u64 ns, u64* total_out) {
    auto& pr = c->prod;
    *total_out = 0;
    if (!ns || !pr.npairs) return KR_OK;
    const u64 nblocks = (ns + LOC_T - 1) / LOC_T;                 // (ns < 2^32: < 2^24 blocks)
    auto launch = [&](auto kernel, u32* bc, const u64* bo, kr_product_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, (const kr_product_site*)pr.sites.p, ns,
                           (const u32*)pr.rec.p, pg, (const u64*)pr.pairkeys.p, (const u32*)pr.pairidx.p, (u32)pr.npairs, pr.max_product,
                           bc, bo, out, fl);
    };
    return scan_two_pass(
        c, nblocks, "kr_products_scan: 2^32 or more products in one genome (a smaller max_product or fewer mismatches)",
        [&](u32* bc, u32* fl) { launch(k_prod_join<false>, bc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, pr.hits, total * sizeof(kr_product_hit));
            return rc ? fail(c, rc, "kr_products_scan: %llu products do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* bc, const u64* bo, u32* fl) { launch(k_prod_join<true>, bc, bo, (kr_product_hit*)pr.hits.p, fl); }, total_out);
}

int64_t kr_products_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->prod.slots, "kr_products_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& pr = c->prod;
    pr.nsites = pr.nhits = -1;
    ProdGeom pg;
    prod_geom(c, &pg);
    u64 nw;                                                       // window starts of the shorter class
    const u64 ntiles = scan_tiles(G.n_bases, std::min(pg.len[0], pg.len[1]), &nw);
    if (!ntiles || !(pr.nleft + pr.nright)) {
        pr.nsites = pr.nhits = 0;
        return 0;
    }
    u64 nseps = 0, ns = 0, np = 0;
    // (the pass's own list: k_prod_rec reads it, and a kr_locate_seps of the caller writes loc.seps)
    if ((rc = scan_seps(c, G, "kr_products_scan", pr.seps, [&](u64 total) { return ensure(c, pr.seps, total * 8); }, &nseps))) return rc;
    if (nseps >= (1ull << 32)) return fail(c, KR_ERR_CAPACITY, "kr_products_scan: 2^32 or more records in one genome");
    const bool one = pg.len[0] == pg.len[1];
    switch (pg.M + 1) {
    case 1: rc = one ? prod_sites_launch<1, 1>(c, G, pg, nw, ntiles, &ns) : prod_sites_launch<1, 2>(c, G, pg, nw, ntiles, &ns); break;
    case 2: rc = one ? prod_sites_launch<2, 1>(c, G, pg, nw, ntiles, &ns) : prod_sites_launch<2, 2>(c, G, pg, nw, ntiles, &ns); break;
    case 3: rc = one ? prod_sites_launch<3, 1>(c, G, pg, nw, ntiles, &ns) : prod_sites_launch<3, 2>(c, G, pg, nw, ntiles, &ns); break;
    default: rc = one ? prod_sites_launch<4, 1>(c, G, pg, nw, ntiles, &ns) : prod_sites_launch<4, 2>(c, G, pg, nw, ntiles, &ns); break;
    }
    if (rc) return rc;
    if (ns) {
        const u32 grid = scan_stride_grid(c, (ns + 255) / 256);
        hipLaunchKernelGGL(k_prod_rec, dim3(grid), dim3(256), 0, c->stream, (const kr_product_site*)pr.sites.p, ns,
                           (const u64*)pr.seps.p, nseps, (u32*)pr.rec.p);
        if ((rc = prod_join(c, pg, ns, &np))) return rc;
    }
    pr.nsites = (int64_t)ns;
    pr.nhits = (int64_t)np;
    return (int64_t)np;
}

// the products of one position in (length, strand, pair) order (kr_products_fetch, kr_primers_fetch: the device lists
// them by opening site -- position, then the sites' order there --, so positions ascend already)
static void prod_sort_positions(kr_product_hit* out, int64_t n) {
    auto less = [](const kr_product_hit& a, const kr_product_hit& b) {
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.length != b.length) return a.length < b.length;
        if (a.strand != b.strand) return a.strand < b.strand;
        return a.pair < b.pair;
    };
    for (int64_t i = 0; i < n;) {
        int64_t j = i + 1;
        while (j < n && out[j].pos == out[i].pos) j++;
        if (j - i > 1) std::sort(out + i, out + j, less);
        i = j;
    }
}

int64_t kr_products_fetch(kr_ctx* c, kr_product_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const int64_t n = scan_fetch(c, c->prod.nhits, "kr_products_scan first", "product", c->prod.hits, out, cap, sizeof(kr_product_hit));
    prod_sort_positions(out, n);
    return n;
}

int64_t kr_products_sites(kr_ctx* c, kr_product_site* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const int64_t n = c->prod.nsites;
    if (n >= 0 && !out) return n;                   // (the count alone)
    return scan_fetch(c, n, "kr_products_scan first", "site", c->prod.sites, out, cap, sizeof(kr_product_site));
}
