// h_panel_clean.inc -- part of krisp_hip.hip (one translation unit): host side of the clean panel selection
// (k_panel_clean.inc, DESIGN §26).  The state is kr_ctx::pclean: a table of ALL candidates' primer texts (the multiplex
// pass's table without its limit of 128 texts: prim_lengths, prim_entries, seed_table_build), the scan of one genome up to
// its sites and records (prod_scan_sites: no join, no product list), and the store that outlives a genome: every scan's
// sites (16 bytes each) and a running record number beside each (4 bytes).  kr_panel_run_clean is h_panel.inc's panel_run
// with the candidates' table rows, the texts' owners, and two or three more launches a round.

int64_t kr_panel_sites_table(kr_ctx* c, const uint8_t* text, const uint32_t* offsets, uint64_t ntexts, int mismatches, uint32_t max_product) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& pc = c->pclean;
    auto& tb = pc.tab;
    const int M = mismatches;
    pc.reset();
    if (M < 0 || M >= NEAR_MAXP)
        return fail(c, KR_ERR_PARAM, "kr_panel_sites_table: 0 <= mismatches <= %d (got %d)", NEAR_MAXP - 1, M);
    if (ntexts < 1 || ntexts >= (1ull << 24))
        return fail(c, KR_ERR_PARAM, "kr_panel_sites_table: 1 .. %u texts are taken (got %llu)", (1u << 24) - 1, (unsigned long long)ntexts);
    if (!text || !offsets) return fail(c, KR_ERR_PARAM, "kr_panel_sites_table: null table");
    u32 smin, maxlen;
    if ((rc = prim_lengths(c, "kr_panel_sites_table", offsets, ntexts, &smin, &maxlen))) return rc;
    // (with that bound the walks' max_product - smin and max_product - n cannot wrap)
    if ((u64)max_product < 2ull * maxlen)
        return fail(c, KR_ERR_PARAM, "kr_panel_sites_table: max_product %u is shorter than twice the longest text (%u letters)", max_product,
                    maxlen);
    tb.M = M; tb.max_product = max_product; tb.nleft = ntexts; tb.nright = 0; tb.plist.npairs = 0;
    tb.smin = smin; tb.maxlen = maxlen;
    PrimGeom pg;
    prim_geom(c, tb, &pg);
    std::vector<uint8_t> arena;
    std::vector<u32> eoff;
    SeedKeys keyed;
    try {
        prim_entries(text, offsets, ntexts, pg, (u32)M + 1, arena, eoff, keyed);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_panel_sites_table: no host memory for the table of %llu texts", (unsigned long long)ntexts);
    }
    const int64_t slots = seed_table_build(c, keyed, arena, tb.seed, "kr_panel_sites_table", ntexts, "texts");
    if (slots < 0) return slots;
    if ((rc = ensure(c, tb.eoff, eoff.size() * 4)))
        return fail(c, rc, "kr_panel_sites_table: the table of %llu texts does not fit the device (%s)", (unsigned long long)ntexts,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(tb.eoff.p, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice));
    tb.seed.slots = (u64)slots;
    return slots;
}

int64_t kr_panel_sites_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->pclean.tab.seed.slots, "kr_panel_sites_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& pc = c->pclean;
    auto& tb = pc.tab;
    tb.gid = id;
    PrimGeom pg;
    prim_geom(c, tb, &pg);
    auto sites = [&](u64 nw, u64 ntiles, u64* ns) {
        return prim_sites(c, G, tb, pg, nw, ntiles, "kr_panel_sites_scan",
                          "kr_panel_sites_scan: 2^32 or more primer sites in one genome (fewer mismatches or candidates)", ns);
    };
    u64 ns = 0, nseps = 0;
    if ((rc = prod_scan_sites(c, G, tb, pg.smin, "kr_panel_sites_scan", sites, &ns, &nseps))) return rc;
    const u64 n0 = pc.nstore, total = n0 + ns;
    if (total >= (1ull << 32))
        return fail(c, KR_ERR_CAPACITY, "kr_panel_sites_scan: %llu primer sites in the store (the limit is 2^32 - 1)", (unsigned long long)total);
    if (pc.units + nseps + 1 >= (1ull << 32))
        return fail(c, KR_ERR_CAPACITY, "kr_panel_sites_scan: 2^32 or more records in the scanned genomes");
    if (ns) {
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (the store grows through a copy on another stream)
        if ((rc = ensure_keep(c, pc.sites, total * sizeof(kr_product_site), n0 * sizeof(kr_product_site))) ||
            (rc = ensure_keep(c, pc.unit, total * 4, n0 * 4)))
            return fail(c, rc, "kr_panel_sites_scan: a store of %llu primer sites does not fit the device (%s)", (unsigned long long)total,
                        c->err.c_str());
        hipLaunchKernelGGL(k_pclean_append, dim3(scan_stride_grid(c, (ns + PCL_T - 1) / PCL_T)), dim3(PCL_T), 0, c->stream,
                           (const kr_product_site*)tb.sites.p, (const u32*)tb.rec.p, ns, (u32)pc.units, (kr_product_site*)pc.sites.p,
                           (u32*)pc.unit.p, n0);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    pc.nstore = total;
    pc.units += nseps + 1;
    tb.nsites = (int64_t)ns;
    return (int64_t)ns;
}

int64_t kr_panel_sites_fetch(kr_ctx* c, kr_product_site* out, uint32_t* unit, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    const auto& pc = c->pclean;
    if (!pc.tab.seed.slots) return fail(c, KR_ERR_STATE, "kr_panel_sites_table first");
    if (!out) return (int64_t)pc.nstore;            // (the count alone)
    if (!unit) return fail(c, KR_ERR_PARAM, "kr_panel_sites_fetch: null argument");
    if (pc.nstore > cap) return fail(c, KR_ERR_CAPACITY, "site buffer too small: %llu > %zu", (unsigned long long)pc.nstore, cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (pc.nstore) {
        HIPCHK(c, hipMemcpy(out, pc.sites.p, pc.nstore * sizeof(kr_product_site), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(unit, pc.unit.p, pc.nstore * 4, hipMemcpyDeviceToHost));
    }
    return (int64_t)pc.nstore;
}

static PcleanStore pclean_store(const kr_ctx* c) {
    const auto& pc = c->pclean;
    PcleanStore S;
    S.sites = (const kr_product_site*)pc.sites.p; S.unit = (const u32*)pc.unit.p; S.ns = pc.nstore;
    S.eoff = (const u32*)pc.tab.eoff.p; S.ne = (u32)(2 * pc.tab.nleft); S.smin = pc.tab.smin; S.max_product = pc.tab.max_product;
    return S;
}

static PcleanOwners pclean_owners(const kr_ctx* c, u64 nown) {
    const auto& pc = c->pclean;
    PcleanOwners O;
    O.ooff = (const u32*)pc.ooff.p; O.own = (const u32*)pc.own.p; O.T = (u32)pc.tab.nleft; O.nown = (u32)nown;
    return O;
}

// the owners of every text as a CSR (a candidate whose two primers share a text owns it once), the candidates' rows and the
// owners onto the device; k_pclean_self and the first member
static int pclean_before(kr_ctx* c, const uint32_t* texts, u64 ncand) {
    auto& pc = c->pclean;
    const u64 T = pc.tab.nleft;
    std::vector<u32> ooff, own;
    try {
        ooff.assign(T + 1, 0u);
        auto twice = [&](u64 i) { return texts[2 * i] != texts[2 * i + 1]; };
        for (u64 i = 0; i < ncand; i++) {
            ooff[texts[2 * i] + 1]++;
            if (twice(i)) ooff[texts[2 * i + 1] + 1]++;
        }
        for (u64 t = 0; t < T; t++) ooff[t + 1] += ooff[t];        // (ncand < 2^31: below 2^32)
        own.assign(std::max<u64>(ooff[T], 1), 0u);
        std::vector<u32> at(ooff.begin(), ooff.end() - 1);
        for (u64 i = 0; i < ncand; i++) {                           // (positions ascend within a text)
            own[at[texts[2 * i]]++] = (u32)i;
            if (twice(i)) own[at[texts[2 * i + 1]]++] = (u32)i;
        }
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_panel_run_clean: no host memory for the owners of %llu texts", (unsigned long long)T);
    }
    const u64 nown = ooff[T];
    int rc;
    if ((rc = ensure(c, pc.rows, ncand * 8)) || (rc = ensure(c, pc.ooff, ooff.size() * 4)) || (rc = ensure(c, pc.own, own.size() * 4)))
        return rc;
    HIPCHK(c, hipMemcpy(pc.rows.p, texts, ncand * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pc.ooff.p, ooff.data(), ooff.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pc.own.p, own.data(), own.size() * 4, hipMemcpyHostToDevice));
    pc.nown = nown;
    if (pc.nstore)
        hipLaunchKernelGGL(k_pclean_self, dim3(scan_stride_grid(c, (pc.nstore + PCL_T - 1) / PCL_T)), dim3(PCL_T), 0, c->stream,
                           pclean_store(c), pclean_owners(c, nown), (uint16_t*)c->panel.state.p, (u32)ncand);
    hipLaunchKernelGGL(k_pclean_next, dim3(1), dim3(PCL_T), 0, c->stream, (u32*)c->panel.pick.p, 0u, (const uint16_t*)c->panel.state.p,
                       (u32)ncand);
    return KR_OK;
}

static void pclean_round(kr_ctx* c, u32 r, u64 ncand) {
    auto& pc = c->pclean;
    if (pc.nstore)
        hipLaunchKernelGGL(k_pclean_cross, dim3(scan_stride_grid(c, (pc.nstore + PCL_T - 1) / PCL_T)), dim3(PCL_T), 0, c->stream,
                           pclean_store(c), pclean_owners(c, pc.nown), (const u32*)pc.rows.p, (const u32*)c->panel.pick.p, r,
                           (uint16_t*)c->panel.state.p, (u32)ncand);
    hipLaunchKernelGGL(k_pclean_next, dim3(1), dim3(PCL_T), 0, c->stream, (u32*)c->panel.pick.p, r + 1u, (const uint16_t*)c->panel.state.p,
                       (u32)ncand);
}

int64_t kr_panel_run_clean(kr_ctx* c, const uint8_t* templates, const uint16_t* pairs, const uint32_t* texts, uint64_t ncand, int W, int size) {
    if (!c || !c->design.on) return fail(c, KR_ERR_STATE, "kr_design_table first");
    c->panel.nmem = -1;
    if (!c->loc.on || !c->pclean.tab.seed.slots) return fail(c, KR_ERR_STATE, "kr_panel_sites_table first");
    if (ncand && !texts) return fail(c, KR_ERR_PARAM, "kr_panel_run_clean: null argument");
    if (ncand >= (1ull << 31))
        return fail(c, KR_ERR_CAPACITY, "kr_panel_run_clean: fewer than 2^31 candidates (got %llu)", (unsigned long long)ncand);
    const u64 T = c->pclean.tab.nleft;
    for (u64 i = 0; i < 2 * ncand; i++)
        if (texts[i] >= T)
            return fail(c, KR_ERR_PARAM, "kr_panel_run_clean: candidate %llu names text %u of a table of %llu", (unsigned long long)(i / 2),
                        texts[i], (unsigned long long)T);
    return panel_run(c, "kr_panel_run_clean", templates, pairs, ncand, W, size, texts);
}

// out[0] = the self-priming candidates, out[1 + j] = the candidates member j + 1 dropped as cross: counted from the fates
int64_t kr_panel_clean_drops(kr_ctx* c, uint32_t* out, size_t cap) {
    if (!c || c->panel.nmem < 0) return fail(c, KR_ERR_STATE, "kr_panel_run_clean first");
    const auto& p = c->panel;
    const size_t n = 1 + (size_t)p.nmem;
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "drop buffer too small: %zu > %zu", n, cap);
    if (!out) return fail(c, KR_ERR_PARAM, "kr_panel_clean_drops: null argument");
    memset(out, 0, n * sizeof(uint32_t));
    for (u64 i = 0; i < p.ncand; i++) {
        const unsigned fate = p.fates[2 * i], by = p.fates[2 * i + 1];
        if (fate == PCLEAN_FATE_SELF) out[0]++;
        else if (fate == PCLEAN_FATE_CROSS && by >= 1 && by <= (unsigned)p.nmem) out[by]++;
    }
    return (int64_t)n;
}
