// h_near.inc -- part of krisp_hip.hip (one translation unit): host side of the near-match pass (k_near.inc): the seed table of
// the targets, the scan of one genome, its hits and their windows.  The context is the locate context
// (kr_set_params_locate): one genome resident at a time, uploaded by the same entry points; kr_locate_seps lists its record
// separators; the table's build, the two-pass driver and the fetches are h_scan.inc's.  Beside the genome live the
// entries' text (2 k bytes a target), the table (16 bytes a slot, >= 2 slots a distinct piece), the entry list (4 bytes per entry and piece), the bitmap, the per-tile counts and the hits.

int64_t kr_near_table(kr_ctx* c, const uint8_t* targets, uint64_t ntargets, int mismatches) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& l = c->loc;
    auto& nr = c->near;
    const int k = l.k, M = mismatches;
    if (M < 0 || M >= NEAR_MAXP || M >= k)
        return fail(c, KR_ERR_PARAM, "kr_near_table: 0 <= mismatches <= %d and mismatches < L+D+R = %d (got %d)", NEAR_MAXP - 1, k, M);
    if (!targets && ntargets) return fail(c, KR_ERR_PARAM, "kr_near_table: null targets");
    if (ntargets >= (1ull << 24))
        return fail(c, KR_ERR_CAPACITY, "kr_near_table: %llu targets (the limit is %u)", (unsigned long long)ntargets, (1u << 24) - 1);
    const u32 NP = (u32)M + 1;
    u32 off[NEAR_MAXP + 1] = {0, 0, 0, 0, 0};
    for (u32 j = 0; j <= NP; j++) off[j] = (u32)((u64)j * k / NP);
    const u64 ne = 2 * ntargets, nk = ne * NP;
    std::vector<uint8_t> text;
    std::vector<std::pair<u64, u32>> keyed;
    try {
        text.resize(ne * k + 16);
        for (u64 t = 0; t < ntargets; t++) {
            const uint8_t* s = targets + t * k;
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
        return fail(c, KR_ERR_CAPACITY, "kr_near_table: no host memory for the table of %llu targets", (unsigned long long)ntargets);
    }
    const int64_t slots = seed_table_build(c, keyed, text, nr.table, nr.arena, nr.list, nr.bitmap, "kr_near_table", ntargets, "targets");
    if (slots < 0) return slots;
    nr.M = M;
    nr.ntargets = ntargets;
    nr.slots = (u64)slots;
    nr.nhits = -1;
    return slots;
}

extern "C++" {    // (a template inside the translation unit's extern "C" block)
template <u32 NP>
static int near_launch(kr_ctx* c, const Genome& G, const NearGeom& ng, u64 ntiles, u64* total_out) {
    auto& nr = c->near;
    const size_t lds = scan_lds_bytes(ng.k, LOC_T * 8);           // (a 64-bit scan array)
    const u32 grid = scan_grid(c, k_near_scan<NP, false>, lds, ntiles);
    auto launch = [&](auto kernel, u32* tc, const u64* to, kr_near_hit* out, u32* fl) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(LOC_T), lds, c->stream, (const uint8_t*)G.bases.p, (u64)G.n_bases, ng,
                           (const u32*)nr.bitmap.p, (const NearSlot*)nr.table.p, (u64)(nr.slots - 1), (const u32*)nr.list.p,
                           (const uint8_t*)nr.arena.p, ntiles, tc, to, out, fl);
    };
    return scan_two_pass(
        c, ntiles, "kr_near_scan: 2^32 or more near matches in one genome (fewer mismatches or targets)",
        [&](u32* tc, u32* fl) { launch(k_near_scan<NP, false>, tc, nullptr, nullptr, fl); },
        [&](u64 total) {
            const int rc = ensure(c, nr.hits, total * sizeof(kr_near_hit));
            return rc ? fail(c, rc, "kr_near_scan: %llu near matches do not fit the device (%s)", (unsigned long long)total, c->err.c_str())
                      : KR_OK;
        },
        [&](u32* tc, const u64* to, u32* fl) { launch(k_near_scan<NP, true>, tc, to, (kr_near_hit*)nr.hits.p, fl); }, total_out);
}
}  // extern "C++"

int64_t kr_near_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->near.slots, "kr_near_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& nr = c->near;
    nr.nhits = 0;
    nr.gid = id;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)l.k, &nw);
    if (!ntiles || !nr.ntargets) return 0;
    NearGeom ng;
    memset(&ng, 0, sizeof ng);
    ng.k = (u32)l.k; ng.omit = (u32)l.omit; ng.M = (u32)nr.M; ng.np = (u32)nr.M + 1;
    ng.lo[0] = (u32)l.L; ng.hi[0] = (u32)(l.L + l.D);             // '+': the text as the target has it
    ng.lo[1] = (u32)l.R; ng.hi[1] = (u32)(l.R + l.D);             // '-': its reverse complement, the right flank first
    for (u32 j = 0; j <= ng.np; j++) ng.off[j] = (u32)((u64)j * l.k / ng.np);
    for (u32 j = 0; j < ng.np; j++) ng.pw[j] = loc_pow((int)(ng.off[j + 1] - ng.off[j]) - 1);
    u64 total = 0;
    switch (ng.np) {
    case 1: rc = near_launch<1>(c, G, ng, ntiles, &total); break;
    case 2: rc = near_launch<2>(c, G, ng, ntiles, &total); break;
    case 3: rc = near_launch<3>(c, G, ng, ntiles, &total); break;
    default: rc = near_launch<4>(c, G, ng, ntiles, &total); break;
    }
    if (rc) {
        nr.nhits = -1;
        return rc;
    }
    nr.nhits = (int64_t)total;
    return (int64_t)total;
}

int64_t kr_near_fetch(kr_ctx* c, kr_near_hit* out, size_t cap) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    return scan_fetch(c, c->near.nhits, "kr_near_scan first", "hit", c->near.hits, out, cap, sizeof(kr_near_hit));
}

int64_t kr_near_windows(kr_ctx* c, uint8_t* rows, size_t cap_bytes) {
    int rc;
    if ((rc = scan_ctx(c))) return rc;
    auto& nr = c->near;
    return scan_windows<kr_near_hit>(c, nr.nhits, nr.gid, "kr_near_scan first", nr.hits, nr.rows, rows, cap_bytes);
}
