// k_near.inc -- part of krisp_hip.hip (one translation unit): the near-match pass (--out_near): every window of a genome within
// Hamming distance M of a target (an ingroup window of a diagnostic region), on both strands.  The host driver is h_near.inc;
// the context and the genome on the device are the locate pass's; the tile layout, the staging, the seed table's slots and
// probe, the count / emit epilogue and the cut of the windows' text are k_scan.inc's.
//
// Pigeonhole seeds: the k columns are cut into NP = M + 1 pieces at fixed offsets (piece j = columns [off[j], off[j + 1])); a
// window within distance M of a text equals it in at least one piece.  The host lists every target and its reverse complement
// (an "entry": 2 * target + strand, its text in the arena) under the key (piece, 32-bit polynomial hash of the piece's bytes);
// a slot of the open-addressing table names the RANGE of the entry list with that key (a region's targets share their flank
// pieces, regions overlap).  Forward hashes only: the reverse strand is in the table.
//
// A workgroup stages a tile as k_loc_scan does (LOC_T * LOC_S window starts + k - 1 bases, 16-byte loads, bad bytes as '\n',
// upper case, 4 bytes of padding per LOC_S); a thread owns LOC_S consecutive starts and rolls the index of the last bad byte
// and NP hashes.  A valid window whose piece key has its bit set in the LDS copy of the membership bitmap probes the table;
// every entry of the slot's range is compared with the window byte by byte (bytes, not 2-bit codes: IUPAC letters are
// letters), which gives the mismatches per piece, their sum, and those in the conserved flanks.  A (window, entry) pair
// within M is emitted by the FIRST piece in which the two are equal, and by no other: once, whatever collides in the hash.
//
// Pass 1 (EMIT = false) counts per tile, k_loc_offsets scans, pass 2 (EMIT = true) revisits the tiles with hits and writes
// them at their tile's offset: position order, then piece, then the entry list's order.  No atomics: the same bytes on
// every run.  (The host orders the table's rows by target and strand afterwards; a row is unique in (target, pos, strand).)
struct NearGeom {
    u32 k, omit, np, M;
    u32 lo[2], hi[2];               // strand s: column c lies in a conserved flank when c < lo[s] or c >= hi[s]
    u32 off[NEAR_MAXP + 1];         // piece j = columns [off[j], off[j + 1])
    u32 pw[NEAR_MAXP];              // LOC_HB^(length of piece j - 1)
};

// window p of the tile against entry e, found through piece `via`: on_hit(entry, mismatches, flank mismatches) when the
// distance is <= M and `via` is the first piece without a mismatch
template <u32 NP, typename F>
__device__ inline void near_check(const NearGeom& ng, const uint8_t* tile, const uint8_t* __restrict__ arena, u32 p, u32 e, u32 via,
                                  F&& on_hit) {
    const uint8_t* f = arena + (u64)e * ng.k;
    const u32 lo = ng.lo[e & 1u], hi = ng.hi[e & 1u];
    u32 mm = 0, fm = 0;
#pragma unroll
    for (u32 j = 0; j < NP; j++) {
        u32 pm = 0;
        #pragma unroll 1
        for (u32 c = ng.off[j]; c < ng.off[j + 1]; c++) {
            const u32 ne = tile[loc_at(p + c)] != f[c];
            pm += ne;
            fm += ne & (u32)(c < lo || c >= hi);
        }
        mm += pm;
        if (j < via && pm == 0) return;             // an earlier piece is equal too: that piece emits the pair
        if (j == via && pm != 0) return;            // (a hash collision)
        if (mm > ng.M) return;
    }
    on_hit(e, mm, fm);
}

// one thread's window starts [s, e) of the staged tile: on_hit(p, entry, mismatches, flank mismatches)
template <u32 NP, typename F>
__device__ inline void near_roll(const NearGeom& ng, const uint8_t* tile, const u32* bm, const NearSlot* __restrict__ table, u64 tmask,
                                 const u32* __restrict__ list, const uint8_t* __restrict__ arena, u32 s, u32 e, F&& on_hit) {
    if (s >= e) return;
    const u32 k = ng.k;
    u32 h[NP];
#pragma unroll
    for (u32 j = 0; j < NP; j++) {
        u32 x = 0;
        #pragma unroll 1
        for (u32 c = ng.off[j]; c < ng.off[j + 1]; c++) x = x * LOC_HB + tile[loc_at(s + c)];
        h[j] = x;
    }
    int bad = -1;                   // the last bad byte in [s, s + k)
    #pragma unroll 1
    for (u32 j = k; j-- > 0;)
        if (tile[loc_at(s + j)] == '\n') { bad = (int)(s + j); break; }
    for (u32 p = s;; p++) {
        if (bad < (int)p) {
#pragma unroll
            for (u32 j = 0; j < NP; j++)
                seed_probe(bm, table, tmask, list, near_key(j, h[j]), [&](u32 en) {
                    near_check<NP>(ng, tile, arena, p, en, j, [&](u32 en, u32 mm, u32 fm) { on_hit(p, en, mm, fm); });
                });
        }
        if (p + 1 >= e) break;
        // slide to p + 1: the byte that leaves piece j + 1 enters piece j
        u32 out = tile[loc_at(p)];
#pragma unroll
        for (u32 j = 0; j < NP; j++) {
            const u32 in = tile[loc_at(p + ng.off[j + 1])];
            h[j] = (h[j] - out * ng.pw[j]) * LOC_HB + in;
            out = in;
        }
        if (out == '\n') bad = (int)(p + k);        // (the last piece's new byte is byte p + k)
    }
}

// the near scan: persistent workgroups over tiles of LOC_T * LOC_S window starts.  EMIT = false: tcount[tile] = hits (a tile
// with 2^32 or more sets *overflow); EMIT = true: the hits of the tiles with any, at toff[tile] (k_loc_offsets)
template <u32 NP, bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_near_scan(const uint8_t* __restrict__ bases, u64 n, NearGeom ng,
                                                     const u32* __restrict__ bitmap, const NearSlot* __restrict__ table, u64 tmask,
                                                     const u32* __restrict__ list, const uint8_t* __restrict__ arena, u64 ntiles,
                                                     u32* __restrict__ tcount, const u64* __restrict__ toff,
                                                     kr_near_hit* __restrict__ out, u32* __restrict__ overflow) {
    extern __shared__ __align__(16) u32 near_lds[];
    u32* bm = near_lds;                                           // LOC_BM_WORDS
    u64* scan = (u64*)(bm + LOC_BM_WORDS);                        // LOC_T
    uint8_t* tile = (uint8_t*)(scan + LOC_T);                     // loc_at(LOC_T * LOC_S + k - 1) bytes
    scan_load_bitmap(bm, bitmap);
    const u64 nw = n >= ng.k ? n - ng.k + 1 : 0;                  // window starts of the genome
    const u32 TP = LOC_T * LOC_S;
    for (u64 tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        if (EMIT && tcount[tl] == 0) continue;                    // (workgroup-uniform)
        const u64 t0 = tl * TP;
        scan_stage_tile(bases, n, t0, TP + ng.k - 1, ng.omit, tile);
        u32 s, e;
        scan_lane_starts(nw, t0, &s, &e);
        u64 cnt = 0;
        near_roll<NP>(ng, tile, bm, table, tmask, list, arena, s, e, [&](u32, u32, u32, u32) { cnt++; });
        kr_near_hit* o = out + scan_epilogue<EMIT>(cnt, scan, tl, tcount, toff, overflow);
        if (!EMIT) continue;
        near_roll<NP>(ng, tile, bm, table, tmask, list, arena, s, e, [&](u32 p, u32 en, u32 mm, u32 fm) {
            kr_near_hit hit;
            hit.target = en >> 1;
            hit.strand = (uint8_t)(en & 1u);
            hit.mismatches = (uint8_t)mm;
            hit.flank_mismatches = (uint8_t)fm;
            hit.pad = 0;
            hit.pos = t0 + p;
            *o++ = hit;
        });
    }
}
