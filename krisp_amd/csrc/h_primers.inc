// h_primers.inc -- part of krisp_hip.hip (one translation unit): host side of the primer-product pass (k_primers.inc): the
// seed table of primer texts of mixed lengths and the pair list, the scan of one genome (separators, sites, records, join),
// its products and sites.  The context is the locate context (kr_set_params_locate: only its soft-mask mode plays a part,
// the texts bring their own lengths): one genome resident at a time.  Beside the genome live the entries' text (2 bytes a
// letter of a text) and their offsets (8 bytes a text), the table (16 bytes a slot, >= 2 slots a distinct piece), the entry
// list (8 (M + 1) bytes a text), the bitmap, the pair list (12 bytes a pair), the separators (8 bytes each), the sites
// (16 + 4 bytes each), the products (24 bytes each) and kr_primers_tally's counters (32 bytes a pair).  The scan behind the prologue, the join, the fetch and the sites are
// h_products.inc's (prod_scan, prod_fetch, prod_sites), with this pass's kernels and the entries' offsets.
#define PRIM_MIN_LEN 10             // the lengths kr_design_table takes for a primer
#define PRIM_MAX_LEN 60

// (pm: the primer pass's state, or the multiplex pass's -- h_multiplex.inc)
static void prim_geom(const kr_ctx* c, const kr_ctx::Prim& pm, PrimGeom* pg) {
    memset(pg, 0, sizeof *pg);
    pg->smin = pm.smin; pg->maxlen = pm.maxlen;
    pg->omit = (u32)c->loc.omit; pg->M = (u32)pm.M; pg->nleft2 = (u32)(2 * pm.nleft);
    seed_pieces(pg->smin, (u32)pm.M + 1, pg->off, pg->pw);
}

// the lengths of the nt texts of a table of `who`: 10 .. 60 letters each -> the shortest and the longest
static int prim_lengths(kr_ctx* c, const char* who, const uint32_t* offsets, u64 nt, u32* smin_out, u32* maxlen_out) {
    u32 smin = nt ? PRIM_MAX_LEN : PRIM_MIN_LEN, maxlen = PRIM_MIN_LEN;
    for (u64 t = 0; t < nt; t++) {
        const int64_t n = (int64_t)offsets[t + 1] - (int64_t)offsets[t];
        if (n < PRIM_MIN_LEN || n > PRIM_MAX_LEN)
            return fail(c, KR_ERR_PARAM, "%s: text %llu has %lld letters (%d .. %d are taken)", who, (unsigned long long)t, (long long)n,
                        PRIM_MIN_LEN, PRIM_MAX_LEN);
        smin = std::min(smin, (u32)n);
        maxlen = std::max(maxlen, (u32)n);
    }
    *smin_out = smin; *maxlen_out = maxlen;
    return KR_OK;
}

// the 2 nt entries of nt texts: their offsets (eoff), their text (arena: text t, then its reverse complement) and every
// entry's keys under the NP pieces of the first smin columns of its text as it reads on the forward strand.  Throws
// std::bad_alloc
static void prim_entries(const uint8_t* text, const uint32_t* offsets, u64 nt, const PrimGeom& pg, u32 NP, std::vector<uint8_t>& arena,
                         std::vector<u32>& eoff, SeedKeys& keyed) {
    const u64 ne = 2 * nt;
    eoff.resize(ne + 1);
    u64 at = 0;
    for (u64 t = 0; t < nt; t++) {
        const u32 n = offsets[t + 1] - offsets[t];
        eoff[2 * t] = (u32)at;                      // (< 2^24 texts of <= 60 letters twice: < 2^31)
        eoff[2 * t + 1] = (u32)(at + n);
        at += 2 * (u64)n;
    }
    eoff[ne] = (u32)at;
    arena.resize(at + 16);
    for (u64 t = 0; t < nt; t++)
        seed_both_strands(arena.data() + eoff[2 * t], text + (offsets[t] - offsets[0]), offsets[t + 1] - offsets[t]);
    keyed.reserve(ne * NP);
    for (u64 e = 0; e < ne; e++) seed_keys(keyed, arena.data() + eoff[e], pg.off, NP, 0, (u32)e);
}

int64_t kr_primers_table(kr_ctx* c, const uint8_t* text, const uint32_t* offsets, uint64_t nleft, uint64_t nright,
                         const uint32_t* pairs, uint64_t npairs, int mismatches, uint32_t max_product) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& pm = c->prim;
    const int M = mismatches;
    const u64 nt = nleft + nright;
    pm.seed.slots = 0;
    pm.nsites = pm.nhits = -1;
    c->assay.reset();                               // (its links name this table's pairs)
    if (M < 0 || M >= NEAR_MAXP)
        return fail(c, KR_ERR_PARAM, "kr_primers_table: 0 <= mismatches <= %d (got %d)", NEAR_MAXP - 1, M);
    if ((nt && (!text || !offsets)) || (!pairs && npairs)) return fail(c, KR_ERR_PARAM, "kr_primers_table: null table");
    if (nt >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_primers_table: %llu primer texts (the limit is %u)", (unsigned long long)nt, (1u << 24) - 1);
    if (npairs >= LOC_EMPTY) return fail(c, KR_ERR_CAPACITY, "kr_primers_table: %llu pairs (the limit is %u)",
                                         (unsigned long long)npairs, LOC_EMPTY - 1);
    u32 smin, maxlen;
    if ((rc = prim_lengths(c, "kr_primers_table", offsets, nt, &smin, &maxlen))) return rc;
    pm.M = M; pm.max_product = max_product; pm.nleft = nleft; pm.nright = nright; pm.plist.npairs = npairs;
    pm.smin = smin; pm.maxlen = maxlen;
    PrimGeom pg;
    prim_geom(c, pm, &pg);
    const u32 NP = (u32)M + 1;
    std::vector<uint8_t> arena;
    std::vector<u32> eoff, pidx, plen;
    SeedKeys keyed;
    std::vector<u64> pkeys;
    try {
        prim_entries(text, offsets, nt, pg, NP, arena, eoff, keyed);
        plen.assign(npairs + 1, 0u);
        rc = pair_list_sort(c, "kr_primers_table", pairs, npairs, nleft, nright, pkeys, pidx, [&](u64 p, u32 li, u32 rj) {
            const u32 n1 = offsets[li + 1] - offsets[li], n2 = offsets[nleft + rj + 1] - offsets[nleft + rj];
            plen[p] = n1 | (n2 << 16);
            if ((u64)max_product < (u64)n1 + n2)
                return fail(c, KR_ERR_PARAM, "kr_primers_table: max_product %u is shorter than the two texts of pair %llu (%u + %u)",
                            max_product, (unsigned long long)p, n1, n2);
            return (int)KR_OK;
        });
        if (rc) return rc;
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_primers_table: no host memory for the table of %llu texts", (unsigned long long)nt);
    }
    const int64_t slots = seed_table_build(c, keyed, arena, pm.seed, "kr_primers_table", nt, "texts");
    if (slots < 0) return slots;
    if ((rc = ensure(c, pm.eoff, eoff.size() * 4)) || (rc = ensure(c, pm.plen, plen.size() * 4)))
        return fail(c, rc, "kr_primers_table: the table of %llu texts does not fit the device (%s)", (unsigned long long)nt, c->err.c_str());
    if ((rc = pair_list_upload(c, pm.plist, pkeys, pidx, "kr_primers_table", nt))) return rc;
    HIPCHK(c, hipMemcpy(pm.eoff.p, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(pm.plen.p, plen.data(), plen.size() * 4, hipMemcpyHostToDevice));
    pm.seed.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
// the sites of genome G against the table of st (the primer pass's or the multiplex pass's), by its number of pieces
template <u32 NP>
static int prim_sites_np(kr_ctx* c, const Genome& G, kr_ctx::Prim& st, const PrimGeom& pg, u64 nw, u64 ntiles, const char* who,
                         const char* over, u64* ns) {
    return prod_sites_launch(c, G, st, pg, nw, ntiles, who, over, k_prim_scan<NP, false>, k_prim_scan<NP, true>, ns, (const u32*)st.eoff.p);
}
}  // extern "C++"

static int prim_sites(kr_ctx* c, const Genome& G, kr_ctx::Prim& st, const PrimGeom& pg, u64 nw, u64 ntiles, const char* who,
                      const char* over, u64* ns) {
    switch (pg.M + 1) {
    case 1: return prim_sites_np<1>(c, G, st, pg, nw, ntiles, who, over, ns);
    case 2: return prim_sites_np<2>(c, G, st, pg, nw, ntiles, who, over, ns);
    case 3: return prim_sites_np<3>(c, G, st, pg, nw, ntiles, who, over, ns);
    default: return prim_sites_np<4>(c, G, st, pg, nw, ntiles, who, over, ns);
    }
}

int64_t kr_primers_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->prim.seed.slots, "kr_primers_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    c->prim.gid = id;
    c->assay.nhits = -1;                            // (a join of the earlier list is no join of this one)
    PrimGeom pg;
    prim_geom(c, c->prim, &pg);
    auto sites = [&](u64 nw, u64 ntiles, u64* ns) {
        return prim_sites(c, G, c->prim, pg, nw, ntiles, "kr_primers_scan",
                          "kr_primers_scan: 2^32 or more primer sites in one genome (fewer mismatches or pairs)", ns);
    };
    // (window starts of the shortest text)
    return prod_scan(c, G, c->prim, pg, pg.smin, "kr_primers_scan", sites, k_prim_join<false>, k_prim_join<true>, (const u32*)c->prim.eoff.p);
}

int64_t kr_primers_fetch(kr_ctx* c, kr_product_hit* out, size_t cap) { return prod_fetch(c, true, "kr_primers_scan first", out, cap); }

int64_t kr_primers_sites(kr_ctx* c, kr_product_site* out, size_t cap) { return prod_sites(c, true, "kr_primers_scan first", out, cap); }

// the products of the latest scan counted per pair (k_prim_tally): out[8 p + m] = pair p's products with m mismatches in
// their two sites together, out[8 p + 7] = those without a mismatch at either 3' end; 8 npairs counters
int64_t kr_primers_tally(kr_ctx* c, uint32_t* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& pm = c->prim;
    if (pm.nhits < 0) return fail(c, KR_ERR_STATE, "kr_primers_scan first");
    const u64 npairs = pm.plist.npairs, n = 8 * npairs;
    if (npairs >= (1ull << 29)) return fail(c, KR_ERR_CAPACITY, "kr_primers_tally: %llu pairs (the counters' index has 32 bits)", (unsigned long long)npairs);
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "kr_primers_tally: tally buffer too small: %llu > %zu", (unsigned long long)n, cap);
    if (!n) return 0;
    if (!out) return fail(c, KR_ERR_PARAM, "kr_primers_tally: null argument");
    if (!pm.nhits) {
        memset(out, 0, n * sizeof(u32));
        return (int64_t)n;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, pm.pair_tally, n * sizeof(u32)))) return rc;
    HIPCHK(c, hipMemsetAsync(pm.pair_tally.p, 0, n * sizeof(u32), c->stream));
    const u64 nhits = (u64)pm.nhits;
    hipLaunchKernelGGL(k_prim_tally, dim3(scan_stride_grid(c, (nhits + 255) / 256)), dim3(256), 0, c->stream,
                       (const kr_product_hit*)pm.hits.p, nhits, (u32)npairs, (u32*)pm.pair_tally.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, pm.pair_tally.p, n * sizeof(u32), hipMemcpyDeviceToHost));
    return (int64_t)n;
}
