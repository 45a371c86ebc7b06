// h_guide_hits.inc -- part of krisp_hip.hip (one translation unit): host side of the guide-hit pass (k_guide_hits.inc): the
// seed table of the guides' protospacers, the scan of one genome, its hits and their windows.  The context is the locate
// context (kr_set_params_locate with L+D+R = the protospacer length G; only k and the soft-mask mode play a part), the
// table's build, the two-pass driver and the fetches are h_scan.inc's.  The pass keeps a state of its own (kr_ctx::ghit):
// a near-match table of the same context and this one do not disturb each other.  Beside the table it holds three lists
// for the context's life, sized by the largest scan so far: the scan's pairs (16 bytes each), the hits (24) and, once
// need_pam was on, the kept hits (24); and, once kr_guide_hits_tally was asked, 16 bytes of counters a guide.

#define GHIT_MIN_SIZE 12            // protospacer lengths the pass takes (the guide pass's: kr_guides_table)
#define GHIT_MAX_SIZE 40
#define GHIT_MAX_MOTIF 8

// a motif in IUPAC letters (either case, U as T; NULL = none) -> its 4-bit base sets, letter j in bits [4 j, 4 j + 4)
static int ghit_motif_sets(kr_ctx* c, const char* name, const char* motif, u32* sets, u32* len) {
    static const char letters[] = "ACGTURYSWKMBDHVN";
    static const u32 set_of[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    *sets = *len = 0;
    if (!motif) return KR_OK;
    const size_t m = strnlen(motif, GHIT_MAX_MOTIF + 1);
    if (m > GHIT_MAX_MOTIF) return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: %s has more than %d letters", name, GHIT_MAX_MOTIF);
    for (size_t j = 0; j < m; j++) {
        const char ch = motif[j] >= 'a' && motif[j] <= 'z' ? (char)(motif[j] - 32) : motif[j];
        const char* at = strchr(letters, ch);       // (ch is not 0: j < strnlen)
        if (!at) return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: letter %zu of %s is no letter of the IUPAC code", j + 1, name);
        *sets |= set_of[at - letters] << (4 * j);
    }
    *len = (u32)m;
    return KR_OK;
}

// what kr_guide_hits_table and kr_guide_bulges_table (`who`) check alike, in the order both had it: the motifs -> *gm, fewer
// than `limit` guides, texts of k letters in A, C, G, T.  (A motif's refusal names kr_guide_hits_table for either: legacy)
static int guide_table_prologue(kr_ctx* c, const char* who, const uint8_t* texts, u64 nguides, int k, u64 limit, const char* pam5,
                                const char* pam3, GhitMotifs* gm) {
    int rc;
    if ((rc = ghit_motif_sets(c, "pam5", pam5, &gm->sets5, &gm->a)) || (rc = ghit_motif_sets(c, "pam3", pam3, &gm->sets3, &gm->b))) return rc;
    if (nguides >= limit)
        return fail(c, KR_ERR_CAPACITY, "%s: %llu guides (the limit is %u)", who, (unsigned long long)nguides, (u32)limit - 1);
    for (u64 i = 0; i < nguides * (u64)k; i++) {
        const uint8_t ch = texts[i];
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T')
            return fail(c, KR_ERR_PARAM, "%s: guide %llu holds a byte that is none of A, C, G, T (0x%02x)", who,
                        (unsigned long long)(i / (u64)k), ch);
    }
    return KR_OK;
}

int64_t kr_guide_hits_table(kr_ctx* c, const uint8_t* texts, uint64_t nguides, int mismatches, const char* pam5, const char* pam3,
                            int need_pam) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& l = c->loc;
    auto& gh = c->ghit;
    const int k = l.k, M = mismatches;
    if (k < GHIT_MIN_SIZE || k > GHIT_MAX_SIZE)
        return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: %d <= L+D+R <= %d, the protospacer's length (got %d)", GHIT_MIN_SIZE,
                    GHIT_MAX_SIZE, k);
    if (M < 0 || M >= NEAR_MAXP) return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: 0 <= mismatches <= %d (got %d)", NEAR_MAXP - 1, M);
    if (!texts && nguides) return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: null texts");
    GhitMotifs gm;
    if ((rc = guide_table_prologue(c, "kr_guide_hits_table", texts, nguides, k, 1ull << 24, pam5, pam3, &gm))) return rc;
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    seed_pieces((u32)k, NP, off, nullptr);
    const u64 ne = 2 * nguides;
    std::vector<uint8_t> text;
    SeedKeys keyed;
    try {
        text.resize(ne * k + 16);                   // entry 2 i = text i, entry 2 i + 1 = its reverse complement
        for (u64 t = 0; t < nguides; t++) seed_both_strands(text.data() + 2 * t * k, texts + t * k, (size_t)k);
        keyed.reserve(ne * NP);
        for (u64 e = 0; e < ne; e++) seed_keys(keyed, text.data() + e * k, off, NP, 0, (u32)e);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_guide_hits_table: no host memory for the table of %llu guides", (unsigned long long)nguides);
    }
    gh.seed.slots = 0;                              // (from here on the device's copy of an earlier table is written over)
    gh.nhits = -1;
    c->assay.reset();                               // (its links name this table's guides)
    const int64_t slots = seed_table_build(c, keyed, text, gh.seed, "kr_guide_hits_table", nguides, "guides");
    if (slots < 0) return slots;
    gh.M = M;
    gh.gm = gm;
    gh.need = need_pam ? 1u : 0u;
    gh.nguides = nguides;
    gh.seed.slots = (u64)slots;
    return slots;
}

// the per-hit step over the *total pairs of the scan (k_ghit_finish: gh.pairs -> gh.hits), then -- with need_pam -- the hits with both motifs beside
// them, in their order (k_ghit_keep, into gh.kept; the two lists change places): *total = what is left
static int ghit_finish_hits(kr_ctx* c, const Genome& G, u64* total) {
    auto& gh = c->ghit;
    const u64 nhits = *total;
    const u32 grid = scan_stride_grid(c, (nhits + 255) / 256);
    hipLaunchKernelGGL(k_ghit_finish, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases,
                       (const uint8_t*)gh.seed.arena.p, (u32)c->loc.k, (u32)c->loc.omit, gh.gm, (u32)gh.nguides, (const kr_near_hit*)gh.pairs.p,
                       (kr_guide_hit*)gh.hits.p, nhits);
    if (!gh.need) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        return KR_OK;
    }
    const u64 nblocks = (nhits + LOC_T - 1) / LOC_T;               // (< 2^24: nhits < 2^32)
    const kr_guide_hit* all = (const kr_guide_hit*)gh.hits.p;
    const int rc = scan_two_pass(
        c, nblocks, nullptr,
        [&](u32* tc, u32*) {
            hipLaunchKernelGGL(k_ghit_keep<false>, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, all, nhits, tc, (const u64*)nullptr,
                               (kr_guide_hit*)nullptr);
        },
        [&](u64 kept) {
            const int rc = ensure(c, gh.kept, kept * sizeof(kr_guide_hit));
            return rc ? fail(c, rc, "kr_guide_hits_scan: %llu hits do not fit the device (%s)", (unsigned long long)kept, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32*) {
            hipLaunchKernelGGL(k_ghit_keep<true>, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, all, nhits, tc, to,
                               (kr_guide_hit*)gh.kept.p);
        },
        total);
    if (rc) return rc;
    if (*total) std::swap(gh.hits, gh.kept);
    return KR_OK;
}

int64_t kr_guide_hits_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    // (KR_ERR_PARAM where the other passes answer KR_ERR_STATE: deliberate, callers hold the code)
    if (!c->ghit.seed.slots) return fail(c, KR_ERR_PARAM, "kr_guide_hits_scan: kr_guide_hits_table first");
    if ((rc = scan_genome(c, id, true, "kr_guide_hits_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& gh = c->ghit;
    gh.nhits = 0;
    gh.gid = id;
    c->assay.nhits = -1;                            // (a join of the earlier list is no join of this one)
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)l.k, &nw);
    if (!ntiles || !gh.nguides) return 0;
    NearGeom ng = near_geom((u32)l.k, (u32)l.omit, (u32)gh.M);
    ng.hi[0] = ng.hi[1] = (u32)l.k;                               // no flank: every column lies inside [0, k)
    u64 total = 0;
    // the near pass's scan kernels over the guides' table: the pairs (guide, strand, distance, position) into gh.pairs
    rc = near_scan_pairs(c, G, gh.seed, ng, ntiles, gh.pairs, [&](u64 n) { return ensure(c, gh.hits, n * sizeof(kr_guide_hit)); },
                         "kr_guide_hits_scan: 2^32 or more hits in one genome (fewer mismatches or guides)",
                         "kr_guide_hits_scan: %llu hits do not fit the device (%s)", &total);
    if (!rc && total) rc = ghit_finish_hits(c, G, &total);
    if (rc) {
        gh.nhits = -1;
        return rc;
    }
    gh.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_guide_hits_fetch(kr_ctx* c, kr_guide_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    return scan_fetch(c, c->ghit.nhits, "kr_guide_hits_scan first", "hit", c->ghit.hits, out, cap, sizeof(kr_guide_hit));
}

int64_t kr_guide_hits_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& gh = c->ghit;
    return scan_windows(c, gh.nhits, gh.gid, "kr_guide_hits_scan first", (u32)c->loc.k, gh.rows, rows, cap_bytes, scan_cut_k<kr_guide_hit>(c, gh));
}

// the hits of the latest scan counted per guide and distance (k_ghit_tally): out[4 guide + m], 4 nguides counters
int64_t kr_guide_hits_tally(kr_ctx* c, uint32_t* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& gh = c->ghit;
    if (gh.nhits < 0) return fail(c, KR_ERR_STATE, "kr_guide_hits_scan first");
    const u64 n = 4 * gh.nguides;                                  // (< 2^26: the table holds fewer than 2^24 guides)
    if (n > cap) return fail(c, KR_ERR_CAPACITY, "kr_guide_hits_tally: tally buffer too small: %llu > %zu", (unsigned long long)n, cap);
    if (!n) return 0;
    if (!out) return fail(c, KR_ERR_PARAM, "kr_guide_hits_tally: null argument");
    if (!gh.nhits) {
        memset(out, 0, n * sizeof(u32));
        return (int64_t)n;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, gh.tally, n * sizeof(u32)))) return rc;
    HIPCHK(c, hipMemsetAsync(gh.tally.p, 0, n * sizeof(u32), c->stream));
    const u64 nhits = (u64)gh.nhits;
    hipLaunchKernelGGL(k_ghit_tally, dim3(scan_stride_grid(c, (nhits + 255) / 256)), dim3(256), 0, c->stream, (const kr_guide_hit*)gh.hits.p,
                       nhits, (u32)gh.nguides, (u32*)gh.tally.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, gh.tally.p, n * sizeof(u32), hipMemcpyDeviceToHost));
    return (int64_t)n;
}
