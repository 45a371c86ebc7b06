// h_guide_hits.inc -- part of krisp_hip.hip (one translation unit): host side of the guide-hit pass (k_guide_hits.inc): the
// seed table of the guides' protospacers, the scan of one genome, its hits and their windows.  The context is the locate
// context (kr_set_params_locate with L+D+R = the protospacer length G; only k and the soft-mask mode play a part), the
// table's build, the two-pass driver and the fetches are h_scan.inc's.  The pass keeps a state of its own (kr_ctx::ghit):
// a near-match table of the same context and this one do not disturb each other.  Beside the table it holds three lists
// for the context's life, sized by the largest scan so far: the scan's pairs (16 bytes each), the hits (24) and, once
// need_pam was on, the kept hits (24).

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
    u32 sets5, a, sets3, b;
    if ((rc = ghit_motif_sets(c, "pam5", pam5, &sets5, &a)) || (rc = ghit_motif_sets(c, "pam3", pam3, &sets3, &b))) return rc;
    if (nguides >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_guide_hits_table: %llu guides (the limit is %u)", (unsigned long long)nguides, (1u << 24) - 1);
    for (u64 i = 0; i < nguides * (u64)k; i++) {
        const uint8_t ch = texts[i];
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T')
            return fail(c, KR_ERR_PARAM, "kr_guide_hits_table: guide %llu holds a byte that is none of A, C, G, T (0x%02x)",
                        (unsigned long long)(i / (u64)k), ch);
    }
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    for (u32 j = 0; j <= NP; j++) off[j] = (u32)((u64)j * k / NP);
    const u64 ne = 2 * nguides, nk = ne * NP;
    std::vector<uint8_t> text;
    std::vector<std::pair<u64, u32>> keyed;
    try {
        // entry 2 i = text i, entry 2 i + 1 = its reverse complement
        text.resize(ne * k + 16);
        for (u64 t = 0; t < nguides; t++) {
            const uint8_t* s = texts + t * k;
            uint8_t* f = text.data() + 2 * t * k;
            for (int i = 0; i < k; i++) {
                f[i] = s[i];
                f[k + i] = loc_comp(s[k - 1 - i]);
            }
        }
        keyed.reserve(nk);
        for (u64 e = 0; e < ne; e++)
            for (u32 j = 0; j < NP; j++)
                keyed.emplace_back(near_key(j, loc_hash(text.data() + e * k + off[j], (int)(off[j + 1] - off[j]))), (u32)e);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_guide_hits_table: no host memory for the table of %llu guides", (unsigned long long)nguides);
    }
    gh.slots = 0;                                   // (from here on the device's copy of an earlier table is written over)
    gh.nhits = -1;
    const int64_t slots = seed_table_build(c, keyed, text, gh.table, gh.arena, gh.list, gh.bitmap, "kr_guide_hits_table", nguides, "guides");
    if (slots < 0) return slots;
    gh.M = M;
    gh.sets5 = sets5; gh.a = a; gh.sets3 = sets3; gh.b = b;
    gh.need = need_pam ? 1u : 0u;
    gh.nguides = nguides;
    gh.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
// the near pass's scan kernels over the guides' table: the pairs (guide, strand, distance, position) into gh.pairs
template <u32 NP>
static int ghit_launch(kr_ctx* c, const Genome& G, const NearGeom& ng, u64 ntiles, u64* total_out) {
    auto& gh = c->ghit;
    const size_t lds = scan_lds_bytes(ng.k, LOC_T * 8);           // (a 64-bit scan array: the near pass's expression)
    const u32 grid = scan_grid(c, k_near_scan<NP, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_near_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, ng,
                           (const u32*)gh.bitmap.p, (const NearSlot*)gh.table.p, (u64)(gh.slots - 1), (const u32*)gh.list.p,
                           (const uint8_t*)gh.arena.p, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, "kr_guide_hits_scan: 2^32 or more hits in one genome (fewer mismatches or guides)",
        [&](u32* tc, u32* fl) { launch(k_near_scan<NP, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) {
            int rc = ensure(c, gh.pairs, total * sizeof(kr_near_hit));
            if (!rc) rc = ensure(c, gh.hits, total * sizeof(kr_guide_hit));
            return rc ? fail(c, rc, "kr_guide_hits_scan: %llu hits do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_near_scan<NP, true>, tc, to, (kr_near_hit*)gh.pairs.p, fl); }, total_out);
}
}  // extern "C++"

// the per-hit step over the *total pairs of the scan (k_ghit_finish: gh.pairs -> gh.hits), then -- with need_pam -- the hits with both motifs beside
// them, in their order (k_ghit_keep, into gh.kept; the two lists change places): *total = what is left
static int ghit_finish_hits(kr_ctx* c, const Genome& G, u64* total) {
    auto& gh = c->ghit;
    const u64 nhits = *total;
    const GhitMotifs gm = {gh.sets5, gh.a, gh.sets3, gh.b};
    const u32 grid = scan_stride_grid(c, (nhits + 255) / 256);
    hipLaunchKernelGGL(k_ghit_finish, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases,
                       (const uint8_t*)gh.arena.p, (u32)c->loc.k, (u32)c->loc.omit, gm, (u32)gh.nguides, (const kr_near_hit*)gh.pairs.p,
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
    if (!c->ghit.slots) return fail(c, KR_ERR_PARAM, "kr_guide_hits_scan: kr_guide_hits_table first");
    if ((rc = scan_genome(c, id, true, "kr_guide_hits_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& gh = c->ghit;
    gh.nhits = 0;
    gh.gid = id;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)l.k, &nw);
    if (!ntiles || !gh.nguides) return 0;
    NearGeom ng;
    memset(&ng, 0, sizeof ng);
    ng.k = (u32)l.k; ng.omit = (u32)l.omit; ng.M = (u32)gh.M; ng.np = (u32)gh.M + 1;
    ng.lo[0] = ng.lo[1] = 0; ng.hi[0] = ng.hi[1] = (u32)l.k;     // no flank: every column lies inside
    for (u32 j = 0; j <= ng.np; j++) ng.off[j] = (u32)((u64)j * l.k / ng.np);
    for (u32 j = 0; j < ng.np; j++) ng.pw[j] = loc_pow((int)(ng.off[j + 1] - ng.off[j]) - 1);
    u64 total = 0;
    switch (ng.np) {
    case 1: rc = ghit_launch<1>(c, G, ng, ntiles, &total); break;
    case 2: rc = ghit_launch<2>(c, G, ng, ntiles, &total); break;
    case 3: rc = ghit_launch<3>(c, G, ng, ntiles, &total); break;
    default: rc = ghit_launch<4>(c, G, ng, ntiles, &total); break;
    }
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
    return scan_windows<kr_guide_hit>(c, gh.nhits, gh.gid, "kr_guide_hits_scan first", gh.hits, gh.rows, rows, cap_bytes);
}
