// h_near.inc -- part of krisp_hip.hip (one translation unit): host side of the near-match pass (k_near.inc): the seed table of
// the targets, the scan of one genome, its hits and their windows.  The context is the locate context
// (kr_set_params_locate): one genome resident at a time, uploaded by the same entry points; kr_locate_seps lists its record
// separators; the entries' text and keys, the table's build, the scan's launcher (near_scan_pairs), the two-pass driver
// and the fetches are h_scan.inc's.  Beside the genome live the entries' text (2 k bytes a target), the table (16 bytes a
// slot, >= 2 slots a distinct piece), the entry list (4 bytes per entry and piece), the bitmap, the per-tile counts and the hits.

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
    seed_pieces((u32)k, NP, off, nullptr);
    const u64 ne = 2 * ntargets;
    std::vector<uint8_t> text;
    SeedKeys keyed;
    try {
        text.resize(ne * k + 16);                   // entry 2 t = target t, entry 2 t + 1 = its reverse complement
        for (u64 t = 0; t < ntargets; t++) seed_both_strands(text.data() + 2 * t * k, targets + t * k, (size_t)k);
        keyed.reserve(ne * NP);
        for (u64 e = 0; e < ne; e++) seed_keys(keyed, text.data() + e * k, off, NP, 0, (u32)e);
    } catch (const std::bad_alloc&) {
        return fail(c, KR_ERR_CAPACITY, "kr_near_table: no host memory for the table of %llu targets", (unsigned long long)ntargets);
    }
    // (a refused table leaves the earlier one standing: the slots change with a table that is whole)
    const int64_t slots = seed_table_build(c, keyed, text, nr.seed, "kr_near_table", ntargets, "targets");
    if (slots < 0) return slots;
    nr.M = M;
    nr.ntargets = ntargets;
    nr.seed.slots = (u64)slots;
    nr.nhits = -1;
    return slots;
}

int64_t kr_near_scan(kr_ctx* c, int id) {
    const Genome* Gp;
    int rc;
    if ((rc = scan_genome(c, id, c && c->near.seed.slots, "kr_near_table first", &Gp))) return rc;
    const Genome& G = *Gp;
    auto& l = c->loc;
    auto& nr = c->near;
    nr.nhits = 0;
    nr.gid = id;
    u64 nw;
    const u64 ntiles = scan_tiles(G.n_bases, (u64)l.k, &nw);
    if (!ntiles || !nr.ntargets) return 0;
    NearGeom ng = near_geom((u32)l.k, (u32)l.omit, (u32)nr.M);
    ng.lo[0] = (u32)l.L; ng.hi[0] = (u32)(l.L + l.D);             // '+': the text as the target has it
    ng.lo[1] = (u32)l.R; ng.hi[1] = (u32)(l.R + l.D);             // '-': its reverse complement, the right flank first
    u64 total = 0;
    rc = near_scan_pairs(c, G, nr.seed, ng, ntiles, nr.hits, [](u64) { return KR_OK; },
                         "kr_near_scan: 2^32 or more near matches in one genome (fewer mismatches or targets)",
                         "kr_near_scan: %llu near matches do not fit the device (%s)", &total);
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
    return scan_windows(c, nr.nhits, nr.gid, "kr_near_scan first", (u32)c->loc.k, nr.rows, rows, cap_bytes, scan_cut_k<kr_near_hit>(c, nr));
}
