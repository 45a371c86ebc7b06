// h_primers.inc -- part of krisp_hip.hip (one translation unit): host side of the primer-product pass (k_primers.inc): the
// seed table of primer texts of mixed lengths and the pair list, the scan of one genome (separators, sites, records, join),
// its products and sites.  The context is the locate context (kr_set_params_locate: only its soft-mask mode plays a part,
// the texts bring their own lengths): one genome resident at a time.  Beside the genome live the entries' text (2 bytes a
// letter of a text) and their offsets (8 bytes a text), the table (16 bytes a slot, >= 2 slots a distinct piece), the entry
// list (8 (M + 1) bytes a text), the bitmap, the pair list (12 bytes a pair), the separators (8 bytes each), the sites
// (16 + 4 bytes each) and the products (24 bytes each).
#define PRIM_MIN_LEN 10             // the lengths kr_design_table takes for a primer
#define PRIM_MAX_LEN 60

static void prim_geom(const kr_ctx* c, PrimGeom* pg) {
    const auto& pm = c->prim;
    memset(pg, 0, sizeof *pg);
    pg->smin = pm.smin; pg->maxlen = pm.maxlen;
    pg->omit = (u32)c->loc.omit; pg->M = (u32)pm.M; pg->nleft2 = (u32)(2 * pm.nleft);
    const u32 NP = (u32)pm.M + 1;
    for (u32 j = 0; j <= NP; j++) pg->off[j] = (u32)((u64)j * pg->smin / NP);
    for (u32 j = 0; j < NP; j++) pg->pw[j] = loc_pow((int)(pg->off[j + 1] - pg->off[j]) - 1);
}

int64_t kr_primers_table(kr_ctx* c, const uint8_t* text, const uint32_t* offsets, uint64_t nleft, uint64_t nright,
                         const uint32_t* pairs, uint64_t npairs, int mismatches, uint32_t max_product) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& pm = c->prim;
    const int M = mismatches;
    const u64 nt = nleft + nright;
    pm.slots = 0;
    pm.nsites = pm.nhits = -1;
    if (M < 0 || M >= NEAR_MAXP)
        return fail(c, KR_ERR_PARAM, "kr_primers_table: 0 <= mismatches <= %d (got %d)", NEAR_MAXP - 1, M);
    if ((nt && (!text || !offsets)) || (!pairs && npairs)) return fail(c, KR_ERR_PARAM, "kr_primers_table: null table");
    if (nt >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_primers_table: %llu primer texts (the limit is %u)", (unsigned long long)nt, (1u << 24) - 1);
    if (npairs >= LOC_EMPTY) return fail(c, KR_ERR_CAPACITY, "kr_primers_table: %llu pairs (the limit is %u)",
                                         (unsigned long long)npairs, LOC_EMPTY - 1);
    u32 smin = nt ? PRIM_MAX_LEN : PRIM_MIN_LEN, maxlen = PRIM_MIN_LEN;
    for (u64 t = 0; t < nt; t++) {
        const int64_t n = (int64_t)offsets[t + 1] - (int64_t)offsets[t];
        if (n < PRIM_MIN_LEN || n > PRIM_MAX_LEN)
            return fail(c, KR_ERR_PARAM, "kr_primers_table: text %llu has %lld letters (%d .. %d are taken)", (unsigned long long)t,
                        (long long)n, PRIM_MIN_LEN, PRIM_MAX_LEN);
        smin = std::min(smin, (u32)n);
        maxlen = std::max(maxlen, (u32)n);
    }
    pm.M = M; pm.max_product = max_product; pm.nleft = nleft; pm.nright = nright; pm.npairs = npairs;
    pm.smin = smin; pm.maxlen = maxlen;
    PrimGeom pg;
    prim_geom(c, &pg);
    const u32 NP = (u32)M + 1;
    const u64 ne = 2 * nt;
    std::vector<uint8_t> arena;
    std::vector<u32> eoff, pidx;
    std::vector<std::pair<u64, u32>> keyed, pk;
    std::vector<u64> pkeys;
    try {
        eoff.resize(ne + 1);
        u64 at = 0;
        for (u64 t = 0; t < nt; t++) {
            const u32 n = offsets[t + 1] - offsets[t];
            eoff[2 * t] = (u32)at;                  // (< 2^24 texts of <= 60 letters twice: < 2^31)
            eoff[2 * t + 1] = (u32)(at + n);
            at += 2 * (u64)n;
        }
        eoff[ne] = (u32)at;
        arena.resize(at + 16);
        for (u64 t = 0; t < nt; t++) {
            const u32 n = offsets[t + 1] - offsets[t];
            const uint8_t* s = text + (offsets[t] - offsets[0]);
            uint8_t* f = arena.data() + eoff[2 * t];
            for (u32 i = 0; i < n; i++) {
                f[i] = s[i];
                f[n + i] = loc_comp(s[n - 1 - i]);
            }
        }
        // every entry under the NP pieces of the first smin columns of its text as it reads on the forward strand
        keyed.reserve(ne * NP);
        for (u64 e = 0; e < ne; e++)
            for (u32 j = 0; j < NP; j++)
                keyed.emplace_back(near_key(j, loc_hash(arena.data() + eoff[e] + pg.off[j], (int)(pg.off[j + 1] - pg.off[j]))), (u32)e);
        pk.reserve(npairs);
        for (u64 p = 0; p < npairs; p++) {
            const u32 li = pairs[2 * p], rj = pairs[2 * p + 1];
            if (li >= nleft || rj >= nright)
                return fail(c, KR_ERR_PARAM, "kr_primers_table: pair %llu names text (%u, %u) of (%llu, %llu)", (unsigned long long)p, li,
                            rj, (unsigned long long)nleft, (unsigned long long)nright);
            const u32 n1 = offsets[li + 1] - offsets[li], n2 = offsets[nleft + rj + 1] - offsets[nleft + rj];
            if ((u64)max_product < (u64)n1 + n2)
                return fail(c, KR_ERR_PARAM, "kr_primers_table: max_product %u is shorter than the two texts of pair %llu (%u + %u)",
                            max_product, (unsigned long long)p, n1, n2);
            pk.emplace_back(((u64)li << 32) | rj, (u32)p);
        }
        std::sort(pk.begin(), pk.end());
        for (u64 p = 1; p < npairs; p++)
            if (pk[p].first == pk[p - 1].first)
                return fail(c, KR_ERR_PARAM, "kr_primers_table: pair %u repeats the texts of pair %u", pk[p].second, pk[p - 1].second);
        pidx.resize(npairs + 1);
        pkeys.resize(npairs + 1);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_primers_table: no host memory for the table of %llu texts", (unsigned long long)nt);
    }
    for (u64 p = 0; p < npairs; p++) {
        pkeys[p] = pk[p].first;
        pidx[p] = pk[p].second;
    }
    const int64_t slots = seed_table_build(c, keyed, arena, pm.table, pm.arena, pm.list, pm.bitmap, "kr_primers_table", nt, "texts");
    if (slots < 0) return slots;
    if ((rc = ensure(c, pm.eoff, eoff.size() * 4)) || (rc = ensure(c, pm.pairkeys, pkeys.size() * 8)) ||
        (rc = ensure(c, pm.pairidx, pidx.size() * 4)))
        return fail(c, rc, "kr_primers_table: the table of %llu texts does not fit the device (%s)", (unsigned long long)nt, c->err.c_str());
    HIPCHK(c, hipMemcpy(pm.eoff.p, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pm.pairkeys.p, pkeys.data(), pkeys.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pm.pairidx.p, pidx.data(), pidx.size() * 4, hipMemcpyHostToDevice));
    pm.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
template <u32 NP>
static int prim_sites_launch(kr_ctx* c, const Genome& G, const PrimGeom& pg, u64 nw, u64 ntiles, u64* total_out) {
    auto& pm = c->prim;
    const size_t lds = scan_lds_bytes(pg.maxlen, LOC_T * 8);      // (a 64-bit scan array)
    const u32 grid = scan_grid(c, k_prim_scan<NP, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_product_site* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, pg,
                           (const u32*)pm.bitmap.p, (const NearSlot*)pm.table.p, (u64)(pm.slots - 1), (const u32*)pm.list.p,
                           (const uint8_t*)pm.arena.p, (const u32*)pm.eoff.p, nw, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, "kr_primers_scan: 2^32 or more primer sites in one genome (fewer mismatches or pairs)",
        [&](u32* tc, u32* fl) { launch(k_prim_scan<NP, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) -> int {
            int rc;
            if ((rc = ensure(c, pm.sites, total * sizeof(kr_product_site))) || (rc = ensure(c, pm.rec, total * 4)))
                return fail(c, rc, "kr_primers_scan: %llu primer sites do not fit the device (%s)", (unsigned long long)total,
                            c->err.c_str());
            return KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_prim_scan<NP, true>, tc, to, (kr_product_site*)pm.sites.p, fl); },
        total_out);
}
}  // extern "C++"

// the join of the sites on the device: -> the number of products
static int prim_join(kr_ctx* c, const PrimGeom& pg, u64 ns, u64* total_out) {
    auto& pm = c->prim;
    *total_out = 0;
    if (!ns || !pm.npairs) return KR_OK;
    const u64 nblocks = (ns + LOC_T - 1) / LOC_T;                 // (ns < 2^32: < 2^24 blocks)
    auto launch = [&](auto kernel, u32* bc, const u64* bo, kr_product_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, (const kr_product_site*)pm.sites.p, ns,
                           (const u32*)pm.rec.p, pg, (const u32*)pm.eoff.p, (const u64*)pm.pairkeys.p, (const u32*)pm.pairidx.p,
                           (u32)pm.npairs, pm.max_product, bc, bo, out, fl);
    };
    return scan_two_pass(
        c, nblocks, "kr_primers_scan: 2^32 or more products in one genome (a smaller max_product or fewer mismatches)",
        [&](u32* bc, u32* fl) { launch(k_prim_join<false>, bc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, pm.hits, total * sizeof(kr_product_hit));
            return rc ? fail(c, rc, "kr_primers_scan: %llu products do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* bc, const u64* bo, u32* fl) { launch(k_prim_join<true>, bc, bo, (kr_product_hit*)pm.hits.p, fl); }, total_out);
}

int64_t kr_primers_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->prim.slots, "kr_primers_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& pm = c->prim;
    pm.nsites = pm.nhits = -1;
    PrimGeom pg;
    prim_geom(c, &pg);
    u64 nw;                                                       // window starts of the shortest text
    const u64 ntiles = scan_tiles(G.n_bases, pg.smin, &nw);
    if (!ntiles || !(pm.nleft + pm.nright)) {
        pm.nsites = pm.nhits = 0;
        return 0;
    }
    u64 nseps = 0, ns = 0, np = 0;
    // (the pass's own list: k_prod_rec reads it, and a kr_locate_seps of the caller writes loc.seps)
    if ((rc = scan_seps(c, G, "kr_primers_scan", pm.seps, [&](u64 total) { return ensure(c, pm.seps, total * 8); }, &nseps))) return rc;
    if (nseps >= (1ull << 32)) return fail(c, KR_ERR_CAPACITY, "kr_primers_scan: 2^32 or more records in one genome");
    switch (pg.M + 1) {
    case 1: rc = prim_sites_launch<1>(c, G, pg, nw, ntiles, &ns); break;
    case 2: rc = prim_sites_launch<2>(c, G, pg, nw, ntiles, &ns); break;
    case 3: rc = prim_sites_launch<3>(c, G, pg, nw, ntiles, &ns); break;
    default: rc = prim_sites_launch<4>(c, G, pg, nw, ntiles, &ns); break;
    }
    if (rc) return rc;
    if (ns) {
        const u32 grid = scan_stride_grid(c, (ns + 255) / 256);
        hipLaunchKernelGGL(k_prod_rec, dim3(grid), dim3(256), 0, c->stream, (const kr_product_site*)pm.sites.p, ns,
                           (const u64*)pm.seps.p, nseps, (u32*)pm.rec.p);
        if ((rc = prim_join(c, pg, ns, &np))) return rc;
    }
    pm.nsites = (int64_t)ns;
    pm.nhits = (int64_t)np;
    return (int64_t)np;
}

int64_t kr_primers_fetch(kr_ctx* c, kr_product_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const int64_t n = scan_fetch(c, c->prim.nhits, "kr_primers_scan first", "product", c->prim.hits, out, cap, sizeof(kr_product_hit));
    // the device lists them by opening site (position, then the sites' order there): positions ascend already, the
    // products of one position are put in (length, strand, pair) order here
    prod_sort_positions(out, n);
    return n;
}

int64_t kr_primers_sites(kr_ctx* c, kr_product_site* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const int64_t n = c->prim.nsites;
    if (n >= 0 && !out) return n;                   // (the count alone)
    return scan_fetch(c, n, "kr_primers_scan first", "site", c->prim.sites, out, cap, sizeof(kr_product_site));
}
