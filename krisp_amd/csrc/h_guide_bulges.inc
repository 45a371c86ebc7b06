// h_guide_bulges.inc -- part of krisp_hip.hip (one translation unit): host side of the bulged guide-hit pass
// (k_guide_bulges.inc): the seed table of the guides' halves, the scan of one genome, its hits and their windows.  The
// context is the guide-hit pass's (the locate context with L+D+R = the protospacer length G); the uploaded genome does not
// depend on the window length, so the near scan runs over it with k = h, the halves' length.  The pass keeps a state of its
// own (kr_ctx::gbulge) beside kr_ctx::ghit: neither disturbs the other.  Beside the seed table it holds the entries' whole
// text and, sized by the largest scan so far, the scan's pairs (16 bytes each) and the hits (32).

#define GBULGE_MAX 2                // the largest bulge
#define GBULGE_MIN_SIZE 20          // the shortest protospacer: halves of h >= 9 letters
#define GBULGE_MAX_M 2              // the most mismatches: seed pieces of >= 3 letters

int64_t kr_guide_bulges_table(kr_ctx* c, const uint8_t* texts, uint64_t nguides, int mismatches, int bulges, const char* pam5,
                              const char* pam3, int need_pam) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& l = c->loc;
    auto& gb = c->gbulge;
    const int G = l.k, M = mismatches, B = bulges;
    // (a shorter guide or a looser distance leaves seed pieces of one or two letters, which lie at nearly every window)
    if (G < GBULGE_MIN_SIZE || G > GHIT_MAX_SIZE)
        return fail(c, KR_ERR_PARAM, "kr_guide_bulges_table: %d <= L+D+R <= %d, the protospacer's length (got %d)", GBULGE_MIN_SIZE,
                    GHIT_MAX_SIZE, G);
    if (M < 0 || M > GBULGE_MAX_M) return fail(c, KR_ERR_PARAM, "kr_guide_bulges_table: 0 <= mismatches <= %d (got %d)", GBULGE_MAX_M, M);
    if (B < 1 || B > GBULGE_MAX) return fail(c, KR_ERR_PARAM, "kr_guide_bulges_table: 1 <= bulges <= %d (got %d)", GBULGE_MAX, B);
    if (!texts && nguides) return fail(c, KR_ERR_PARAM, "kr_guide_bulges_table: null texts");
    GhitMotifs gm;
    if ((rc = guide_table_prologue(c, "kr_guide_bulges_table", texts, nguides, G, 1ull << 23, pam5, pam3, &gm))) return rc;
    // the halves: h letters, so short that every cut leaves one of them whole (2 h <= G - b + 1 for every b <= B); h >= 9
    // letters hold the M + 1 <= 3 seed pieces
    const int h = (G - B) / 2;
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    seed_pieces((u32)h, NP, off, nullptr);
    const u64 nt = 2 * nguides, ne = 2 * nt;                      // half texts, their entries
    std::vector<uint8_t> halves, whole;
    SeedKeys keyed;
    try {
        // seed text 2 g = guide g's first h letters, 2 g + 1 = its last h; seed entry 2 t = text t, 2 t + 1 = its reverse
        // complement.  whole: entry 2 g = guide g, 2 g + 1 = its reverse complement (the step's texts)
        halves.resize(ne * h + 16);
        whole.resize(nt * G + 16);
        for (u64 g = 0; g < nguides; g++) {
            const uint8_t* s = texts + g * G;
            seed_both_strands(whole.data() + 2 * g * G, s, (size_t)G);
            seed_both_strands(halves.data() + 4 * g * h, s, (size_t)h);
            seed_both_strands(halves.data() + (4 * g + 2) * h, s + (G - h), (size_t)h);
        }
        keyed.reserve(ne * NP);
        for (u64 e = 0; e < ne; e++) seed_keys(keyed, halves.data() + e * h, off, NP, 0, (u32)e);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_guide_bulges_table: no host memory for the table of %llu guides", (unsigned long long)nguides);
    }
    gb.seed.slots = 0;                              // (from here on the device's copy of an earlier table is written over)
    gb.nhits = -1;
    const int64_t slots = seed_table_build(c, keyed, halves, gb.seed, "kr_guide_bulges_table", nguides, "guides");
    if (slots < 0) return slots;
    if ((rc = ensure(c, gb.texts, whole.size())))
        return fail(c, rc, "kr_guide_bulges_table: the table of %llu guides does not fit the device (%s)", (unsigned long long)nguides,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(gb.texts.p, whole.data(), whole.size(), hipMemcpyHostToDevice));
    gb.M = M;
    gb.B = B;
    gb.h = (u32)h;
    gb.gm = gm;
    gb.need = need_pam ? 1u : 0u;
    gb.nguides = nguides;
    gb.seed.slots = (u64)slots;
    return slots;
}

// the per-pair step over the scan's *total pairs (k_gbulge_extend: gb.pairs -> gb.hits): *total = the rows
static int gbulge_extend(kr_ctx* c, const Genome& G, u64* total) {
    auto& gb = c->gbulge;
    const u64 npairs = *total;
    GbulgeGeom gg;
    gg.G = (u32)c->loc.k; gg.h = gb.h; gg.B = (u32)gb.B; gg.M = (u32)gb.M; gg.omit = (u32)c->loc.omit; gg.need = gb.need;
    gg.nhalves = (u32)(2 * gb.nguides);
    gg.gm = gb.gm;
    const u64 nblocks = (npairs + LOC_T - 1) / LOC_T;              // (< 2^24: npairs < 2^32)
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_guide_bulge_hit* out) {
        hipLaunchKernelGGL(kernel, dim3((u32)nblocks), dim3(LOC_T), 0, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases,
                           (const uint8_t*)gb.texts.p, gg, (const kr_near_hit*)gb.pairs.p, npairs, tc, to, out);
    };
    return scan_two_pass(
        c, nblocks, "kr_guide_bulges_scan: 2^32 or more hits in one genome (fewer mismatches or guides)",
        [&](u32* tc, u32*) { launch(k_gbulge_extend<false>, tc, nullptr, nullptr); },
        [&](u64 rows) {
            const int rc = ensure(c, gb.hits, rows * sizeof(kr_guide_bulge_hit));
            return rc ? fail(c, rc, "kr_guide_bulges_scan: %llu hits do not fit the device (%s)", (unsigned long long)rows, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32*) { launch(k_gbulge_extend<true>, tc, to, (kr_guide_bulge_hit*)gb.hits.p); }, total);
}

int64_t kr_guide_bulges_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    // (KR_ERR_PARAM where the other passes answer KR_ERR_STATE: deliberate, callers hold the code)
    if (!c->gbulge.seed.slots) return fail(c, KR_ERR_PARAM, "kr_guide_bulges_scan: kr_guide_bulges_table first");
    if ((rc = scan_genome(c, id, true, "kr_guide_bulges_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& gb = c->gbulge;
    gb.nhits = 0;
    gb.gid = id;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)gb.h, &nw);
    if (!ntiles || !gb.nguides) return 0;
    NearGeom ng = near_geom(gb.h, (u32)l.omit, (u32)gb.M);
    ng.hi[0] = ng.hi[1] = gb.h;                                   // no flank: every column lies inside [0, h)
    u64 total = 0;
    // the near pass's scan kernels over the halves' table: the pairs (half text, strand, distance, position) into gb.pairs
    rc = near_scan_pairs(c, G, gb.seed, ng, ntiles, gb.pairs, [](u64) { return KR_OK; },
                         "kr_guide_bulges_scan: 2^32 or more hits in one genome (fewer mismatches or guides)",
                         "kr_guide_bulges_scan: %llu hits do not fit the device (%s)", &total);
    if (!rc && total) rc = gbulge_extend(c, G, &total);
    if (rc) {
        gb.nhits = -1;
        return rc;
    }
    gb.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_guide_bulges_fetch(kr_ctx* c, kr_guide_bulge_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    return scan_fetch(c, c->gbulge.nhits, "kr_guide_bulges_scan first", "hit", c->gbulge.hits, out, cap, sizeof(kr_guide_bulge_hit));
}

int64_t kr_guide_bulges_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& gb = c->gbulge;
    const u32 W = (u32)(c->loc.k + gb.B);
    return scan_windows(c, gb.nhits, gb.gid, "kr_guide_bulges_scan first", W, gb.rows, rows, cap_bytes, [&](const Genome& G, u32 grid) {
        hipLaunchKernelGGL(k_gbulge_cut, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases,
                           (const kr_guide_bulge_hit*)gb.hits.p, (u64)gb.nhits, W, (uint8_t*)gb.rows.p);
    });
}
