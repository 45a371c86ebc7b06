// h_products.inc -- part of krisp_hip.hip (one translation unit): host side of the product pass (k_products.inc): the seed
// table of the flank texts and the pair list, the scan of one genome (separators, sites, records, join), its products and
// sites.  The context is the locate context (kr_set_params_locate): one genome resident at a time.  Beside the genome live
// the entries' text (2 bytes a letter of a text), the table (16 bytes a slot, >= 2 slots a distinct piece), the entry list,
// the bitmap, the pair list (12 bytes a pair), the separators (8 bytes each), the sites (16 + 4 bytes each) and the
// products (24 bytes each).

// The primer-product pass (h_primers.inc) differs in its geometry, its kernels and one kernel argument more (eoff): the
// scan behind the prologue, the join, the fetch and the sites are here for both, over kr_ctx::Prod (kr_ctx::Prim's base).

static void prod_geom(const kr_ctx* c, ProdGeom* pg) {
    const auto& l = c->loc;
    const auto& pr = c->prod;
    memset(pg, 0, sizeof *pg);
    pg->len[0] = (u32)l.L; pg->len[1] = (u32)l.R;
    pg->omit = (u32)l.omit; pg->M = (u32)pr.M; pg->nleft2 = (u32)(2 * pr.nleft);
    pg->maxlen = std::max(pg->len[0], pg->len[1]);
    for (int q = 0; q < 2; q++) {
        pg->end[q] = std::min<u32>(PROD_END, pg->len[q]);
        seed_pieces(pg->len[q], (u32)pr.M + 1, pg->off[q], pg->pw[q]);
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
    pr.seed.slots = 0;
    pr.nsites = pr.nhits = -1;
    pr.M = M; pr.max_product = max_product; pr.nleft = nleft; pr.nright = nright; pr.plist.npairs = npairs;
    ProdGeom pg;
    prod_geom(c, &pg);
    const u32 NP = (u32)M + 1;
    const bool one = Le == Re;                      // one length class: the left and right entries share their keys
    const u64 ne = 2 * (nleft + nright);
    std::vector<uint8_t> text;
    SeedKeys keyed;
    std::vector<u64> pkeys;
    std::vector<u32> pidx;
    try {
        text.resize(2 * (nleft * Le + nright * Re) + 16);
        for (u64 e = 0; e < ne; e += 2) {
            const bool lf = e < 2 * nleft;
            seed_both_strands(text.data() + prod_text_at(pg, (u32)e), lf ? left + (e >> 1) * Le : right + ((e >> 1) - nleft) * Re,
                              (size_t)(lf ? Le : Re));
        }
        keyed.reserve(ne * NP);
        for (u64 e = 0; e < ne; e++) {
            const u32 q = prod_class(pg, (u32)e);
            seed_keys(keyed, text.data() + prod_text_at(pg, (u32)e), pg.off[q], NP, (one ? 0u : q) * NEAR_MAXP, (u32)e);
        }
        if ((rc = pair_list_sort(c, "kr_products_table", pairs, npairs, nleft, nright, pkeys, pidx, [](u64, u32, u32) { return KR_OK; })))
            return rc;
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_products_table: no host memory for the table of %llu texts", (unsigned long long)(nleft + nright));
    }
    const int64_t slots = seed_table_build(c, keyed, text, pr.seed, "kr_products_table", nleft + nright, "texts");
    if (slots < 0) return slots;
    if ((rc = pair_list_upload(c, pr.plist, pkeys, pidx, "kr_products_table", nleft + nright))) return rc;
    pr.seed.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (templates inside the translation unit's extern "C" block)
// the primer sites of genome G into st.sites, in two passes of the pass's scan kernels (count, emit) over its table.
// who: the scan's entry point; over: what to say of 2^32 or more sites; eoff...: the kernels' arguments between the
// entries' text and nw -- none, or the primer pass's offsets of the entries' text
template <typename Geom, typename KC, typename KE, typename... E>
static int prod_sites_launch(kr_ctx* c, const Genome& G, kr_ctx::Prod& st, const Geom& pg, u64 nw, u64 ntiles, const char* who,
                             const char* over, KC count, KE emit, u64* total_out, E... eoff) {
    const auto& sd = st.seed;
    const size_t lds = scan_lds_bytes(pg.maxlen, LOC_T * 8);      // (a 64-bit scan array)
    const u32 grid = scan_grid(c, count, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_product_site* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, pg,
                           (const u32*)sd.bitmap.p, (const NearSlot*)sd.table.p, (u64)(sd.slots - 1), (const u32*)sd.list.p,
                           (const uint8_t*)sd.arena.p, eoff..., nw, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, over, [&](u32* tc, u32* fl) { launch(count, tc, nullptr, nullptr, fl); },
        [&](u64 total) -> int {
            int rc;
            if ((rc = ensure(c, st.sites, total * sizeof(kr_product_site))) || (rc = ensure(c, st.rec, total * 4)))
                return fail(c, rc, "%s: %llu primer sites do not fit the device (%s)", who, (unsigned long long)total, c->err.c_str());
            return KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(emit, tc, to, (kr_product_site*)st.sites.p, fl); }, total_out);
}

// the join of the ns sites on the device (the pass's join kernels: count, emit; eoff...: their arguments between the
// geometry and the pair list) -> the number of products
template <typename Geom, typename KC, typename KE, typename... E>
static int prod_join(kr_ctx* c, kr_ctx::Prod& st, const Geom& pg, u64 ns, const char* who, KC count, KE emit, u64* total_out, E... eoff) {
    *total_out = 0;
    if (!ns || !st.plist.npairs) return KR_OK;
    const u64 nblocks = (ns + LOC_T - 1) / LOC_T;                 // (ns < 2^32: < 2^24 blocks)
    const std::string over = std::string(who) + ": 2^32 or more products in one genome (a smaller max_product or fewer mismatches)";
    auto launch = [&](auto kernel, u32* bc, const u64* bo, kr_product_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, (const kr_product_site*)st.sites.p, ns,
                           (const u32*)st.rec.p, pg, eoff..., (const u64*)st.plist.pairkeys.p, (const u32*)st.plist.pairidx.p,
                           (u32)st.plist.npairs, st.max_product, bc, bo, out, fl);
    };
    return scan_two_pass(
        c, nblocks, over.c_str(), [&](u32* bc, u32* fl) { launch(count, bc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, st.hits, total * sizeof(kr_product_hit));
            return rc ? fail(c, rc, "%s: %llu products do not fit the device (%s)", who, (unsigned long long)total, c->err.c_str()) : KR_OK;
        },
        [&](u32* bc, const u64* bo, u32* fl) { launch(emit, bc, bo, (kr_product_hit*)st.hits.p, fl); }, total_out);
}

// a product pass's scan behind scan_genome, up to its join: the windows of `width` bases (the shortest text's), the
// separators, the sites -- sites(nw, ntiles, &ns): the pass's choice of prod_sites_launch by its M -- and their records
// (launched: the join follows on the stream) -> *ns sites (*nseps_out: the genome's separators).  The pass's counts stand at
// -1 until its caller sets them
template <typename S>
static int prod_scan_sites(kr_ctx* c, const Genome& G, kr_ctx::Prod& st, u64 width, const char* who, S&& sites, u64* ns,
                           u64* nseps_out = nullptr) {
    int rc;
    st.nsites = st.nhits = -1;
    *ns = 0;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, width, &nw);
    if (!ntiles || !(st.nleft + st.nright)) return KR_OK;
    u64 nseps = 0;
    // (the pass's own list: k_prod_rec reads it, and a kr_locate_seps of the caller writes loc.seps)
    if ((rc = scan_seps(c, G, who, st.seps, [&](u64 total) { return ensure(c, st.seps, total * 8); }, &nseps))) return rc;
    if (nseps >= (1ull << 32)) return fail(c, KR_ERR_CAPACITY, "%s: 2^32 or more records in one genome", who);
    if (nseps_out) *nseps_out = nseps;
    if ((rc = sites(nw, ntiles, ns))) return rc;
    if (*ns) {
        const u32 grid = scan_stride_grid(c, (*ns + 255) / 256);
        hipLaunchKernelGGL(k_prod_rec, dim3(grid), dim3(256), 0, c->stream, (const kr_product_site*)st.sites.p, *ns,
                           (const u64*)st.seps.p, nseps, (u32*)st.rec.p);
    }
    return KR_OK;
}

// ... and with the join of the two passes that have a pair list (the pass's join kernels) -> the products
template <typename Geom, typename S, typename KC, typename KE, typename... E>
static int64_t prod_scan(kr_ctx* c, const Genome& G, kr_ctx::Prod& st, const Geom& pg, u64 width, const char* who, S&& sites, KC join_count,
                         KE join_emit, E... eoff) {
    int rc;
    u64 ns = 0, np = 0;
    if ((rc = prod_scan_sites(c, G, st, width, who, sites, &ns))) return rc;
    if (ns && (rc = prod_join(c, st, pg, ns, who, join_count, join_emit, &np, eoff...))) return rc;
    st.nsites = (int64_t)ns;
    st.nhits = (int64_t)np;
    return (int64_t)np;
}

template <u32 NP, u32 NC>
static int prod_sites_np(kr_ctx* c, const Genome& G, const ProdGeom& pg, u64 nw, u64 ntiles, u64* ns) {
    return prod_sites_launch(c, G, c->prod, pg, nw, ntiles, "kr_products_scan",
                             "kr_products_scan: 2^32 or more primer sites in one genome (fewer mismatches or regions)",
                             k_prod_scan<NP, NC, false>, k_prod_scan<NP, NC, true>, ns);
}
}  // extern "C++"

int64_t kr_products_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->prod.seed.slots, "kr_products_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    ProdGeom pg;
    prod_geom(c, &pg);
    const bool one = pg.len[0] == pg.len[1];
    auto sites = [&](u64 nw, u64 ntiles, u64* ns) {
        switch (pg.M + 1) {
        case 1: return one ? prod_sites_np<1, 1>(c, G, pg, nw, ntiles, ns) : prod_sites_np<1, 2>(c, G, pg, nw, ntiles, ns);
        case 2: return one ? prod_sites_np<2, 1>(c, G, pg, nw, ntiles, ns) : prod_sites_np<2, 2>(c, G, pg, nw, ntiles, ns);
        case 3: return one ? prod_sites_np<3, 1>(c, G, pg, nw, ntiles, ns) : prod_sites_np<3, 2>(c, G, pg, nw, ntiles, ns);
        default: return one ? prod_sites_np<4, 1>(c, G, pg, nw, ntiles, ns) : prod_sites_np<4, 2>(c, G, pg, nw, ntiles, ns);
        }
    };
    // (window starts of the shorter class)
    return prod_scan(c, G, c->prod, pg, std::min(pg.len[0], pg.len[1]), "kr_products_scan", sites, k_prod_join<false>, k_prod_join<true>);
}

// the products of one position in (length, strand, pair) order (prod_fetch: the device lists them by opening site --
// position, then the sites' order there --, so positions ascend already)
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

// kr_products_fetch and -- primers -- kr_primers_fetch
static int64_t prod_fetch(kr_ctx* c, bool primers, const char* scan_first, kr_product_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const kr_ctx::Prod& st = primers ? static_cast<const kr_ctx::Prod&>(c->prim) : c->prod;
    const int64_t n = scan_fetch(c, st.nhits, scan_first, "product", st.hits, out, cap, sizeof(kr_product_hit));
    prod_sort_positions(out, n);
    return n;
}

// kr_products_sites and -- primers -- kr_primers_sites
static int64_t prod_sites(kr_ctx* c, bool primers, const char* scan_first, kr_product_site* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const kr_ctx::Prod& st = primers ? static_cast<const kr_ctx::Prod&>(c->prim) : c->prod;
    if (st.nsites >= 0 && !out) return st.nsites;   // (the count alone)
    return scan_fetch(c, st.nsites, scan_first, "site", st.sites, out, cap, sizeof(kr_product_site));
}

int64_t kr_products_fetch(kr_ctx* c, kr_product_hit* out, size_t cap) { return prod_fetch(c, false, "kr_products_scan first", out, cap); }

int64_t kr_products_sites(kr_ctx* c, kr_product_site* out, size_t cap) { return prod_sites(c, false, "kr_products_scan first", out, cap); }
