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
    u32 sets5, a, sets3, b;
    if ((rc = ghit_motif_sets(c, "pam5", pam5, &sets5, &a)) || (rc = ghit_motif_sets(c, "pam3", pam3, &sets3, &b))) return rc;
    if (nguides >= (1ull << 23))
        return fail(c, KR_ERR_CAPACITY, "kr_guide_bulges_table: %llu guides (the limit is %u)", (unsigned long long)nguides, (1u << 23) - 1);
    for (u64 i = 0; i < nguides * (u64)G; i++) {
        const uint8_t ch = texts[i];
        if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T')
            return fail(c, KR_ERR_PARAM, "kr_guide_bulges_table: guide %llu holds a byte that is none of A, C, G, T (0x%02x)",
                        (unsigned long long)(i / (u64)G), ch);
    }
    // the halves: h letters, so short that every cut leaves one of them whole (2 h <= G - b + 1 for every b <= B); h >= 9
    // letters hold the M + 1 <= 3 seed pieces
    const int h = (G - B) / 2;
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    for (u32 j = 0; j <= NP; j++) off[j] = (u32)((u64)j * h / NP);
    const u64 nt = 2 * nguides, ne = 2 * nt, nk = ne * NP;        // half texts, their entries, the keys
    std::vector<uint8_t> halves, whole;
    std::vector<std::pair<u64, u32>> keyed;
    try {
        // seed text 2 g = guide g's first h letters, 2 g + 1 = its last h; seed entry 2 t = text t, 2 t + 1 = its reverse
        // complement.  whole: entry 2 g = guide g, 2 g + 1 = its reverse complement (the step's texts)
        halves.resize(ne * h + 16);
        whole.resize(nt * G + 16);
        for (u64 g = 0; g < nguides; g++) {
            const uint8_t* s = texts + g * G;
            uint8_t* w = whole.data() + 2 * g * G;
            for (int i = 0; i < G; i++) {
                w[i] = s[i];
                w[G + i] = loc_comp(s[G - 1 - i]);
            }
            for (u32 half = 0; half < 2; half++) {
                const uint8_t* t = s + (half ? G - h : 0);
                uint8_t* f = halves.data() + 2 * (2 * g + half) * h;
                for (int i = 0; i < h; i++) {
                    f[i] = t[i];
                    f[h + i] = loc_comp(t[h - 1 - i]);
                }
            }
        }
        keyed.reserve(nk);
        for (u64 e = 0; e < ne; e++)
            for (u32 j = 0; j < NP; j++)
                keyed.emplace_back(near_key(j, loc_hash(halves.data() + e * h + off[j], (int)(off[j + 1] - off[j]))), (u32)e);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_guide_bulges_table: no host memory for the table of %llu guides", (unsigned long long)nguides);
    }
    gb.slots = 0;                                   // (from here on the device's copy of an earlier table is written over)
    gb.nhits = -1;
    const int64_t slots = seed_table_build(c, keyed, halves, gb.table, gb.arena, gb.list, gb.bitmap, "kr_guide_bulges_table", nguides, "guides");
    if (slots < 0) return slots;
    if ((rc = ensure(c, gb.texts, whole.size())))
        return fail(c, rc, "kr_guide_bulges_table: the table of %llu guides does not fit the device (%s)", (unsigned long long)nguides,
                    c->err.c_str());
    HIPCHK(c, hipMemcpy(gb.texts.p, whole.data(), whole.size(), hipMemcpyHostToDevice));
    gb.M = M;
    gb.B = B;
    gb.h = (u32)h;
    gb.sets5 = sets5; gb.a = a; gb.sets3 = sets3; gb.b = b;
    gb.need = need_pam ? 1u : 0u;
    gb.nguides = nguides;
    gb.slots = (u64)slots;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
// the near pass's scan kernels over the halves' table: the pairs (half text, strand, distance, position) into gb.pairs
template <u32 NP>
static int gbulge_launch(kr_ctx* c, const Genome& G, const NearGeom& ng, u64 ntiles, u64* total_out) {
    auto& gb = c->gbulge;
    const size_t lds = scan_lds_bytes(ng.k, LOC_T * 8);           // (a 64-bit scan array: the near pass's expression)
    const u32 grid = scan_grid(c, k_near_scan<NP, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_near_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, ng,
                           (const u32*)gb.bitmap.p, (const NearSlot*)gb.table.p, (u64)(gb.slots - 1), (const u32*)gb.list.p,
                           (const uint8_t*)gb.arena.p, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, "kr_guide_bulges_scan: 2^32 or more hits in one genome (fewer mismatches or guides)",
        [&](u32* tc, u32* fl) { launch(k_near_scan<NP, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, gb.pairs, total * sizeof(kr_near_hit));
            return rc ? fail(c, rc, "kr_guide_bulges_scan: %llu hits do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_near_scan<NP, true>, tc, to, (kr_near_hit*)gb.pairs.p, fl); }, total_out);
}
}  // extern "C++"

// the per-pair step over the scan's *total pairs (k_gbulge_extend: gb.pairs -> gb.hits): *total = the rows
static int gbulge_extend(kr_ctx* c, const Genome& G, u64* total) {
    auto& gb = c->gbulge;
    const u64 npairs = *total;
    GbulgeGeom gg;
    gg.G = (u32)c->loc.k; gg.h = gb.h; gg.B = (u32)gb.B; gg.M = (u32)gb.M; gg.omit = (u32)c->loc.omit; gg.need = gb.need;
    gg.nhalves = (u32)(2 * gb.nguides);
    gg.gm = {gb.sets5, gb.a, gb.sets3, gb.b};
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
    if (!c->gbulge.slots) return fail(c, KR_ERR_PARAM, "kr_guide_bulges_scan: kr_guide_bulges_table first");
    if ((rc = scan_genome(c, id, true, "kr_guide_bulges_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& gb = c->gbulge;
    gb.nhits = 0;
    gb.gid = id;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)gb.h, &nw);
    if (!ntiles || !gb.nguides) return 0;
    NearGeom ng;
    memset(&ng, 0, sizeof ng);
    ng.k = gb.h; ng.omit = (u32)l.omit; ng.M = (u32)gb.M; ng.np = (u32)gb.M + 1;
    ng.lo[0] = ng.lo[1] = 0; ng.hi[0] = ng.hi[1] = gb.h;         // no flank: every column lies inside
    for (u32 j = 0; j <= ng.np; j++) ng.off[j] = (u32)((u64)j * gb.h / ng.np);
    for (u32 j = 0; j < ng.np; j++) ng.pw[j] = loc_pow((int)(ng.off[j + 1] - ng.off[j]) - 1);
    u64 total = 0;
    switch (ng.np) {
    case 1: rc = gbulge_launch<1>(c, G, ng, ntiles, &total); break;
    case 2: rc = gbulge_launch<2>(c, G, ng, ntiles, &total); break;
    default: rc = gbulge_launch<3>(c, G, ng, ntiles, &total); break;
    }
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
    const int64_t nhits = gb.nhits;
    if (nhits < 0) return fail(c, KR_ERR_STATE, "kr_guide_bulges_scan first");
    if (!rows || !nhits) return nhits;
    auto it = c->genomes.find(gb.gid);
    if (it == c->genomes.end() || !it->second.uploaded) return fail(c, KR_ERR_STATE, "genome %d is gone", gb.gid);
    const u32 W = (u32)(c->loc.k + gb.B);
    const u64 bytes = (u64)nhits * W;
    if (bytes > cap_bytes) return fail(c, KR_ERR_CAPACITY, "row buffer too small: %llu > %zu", (unsigned long long)bytes, cap_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure(c, gb.rows, bytes))) return rc;
    const u32 grid = scan_stride_grid(c, (bytes + 255) / 256);
    hipLaunchKernelGGL(k_gbulge_cut, dim3(grid), dim3(256), 0, c->stream, (const uint8_t*)it->second.bases.p, (u64)it->second.n_bases,
                       (const kr_guide_bulge_hit*)gb.hits.p, (u64)nhits, W, (uint8_t*)gb.rows.p);
    HIPCHK(c, hipMemcpyAsync(rows, gb.rows.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return nhits;
}
