// k_locate.inc -- part of krisp_hip.hip (one translation unit): the locate pass (--out_locations): where the windows of the
// surviving groups lie in a genome.  The host driver is h_locate.inc.
//
// A genome's bases are scanned once, from the device's copy (no sort).  A workgroup stages a tile of LOC_T * LOC_S window
// starts plus k - 1 bases of overlap in LDS (16-byte loads, coalesced; separators, N / n and -- under omit-soft -- lower
// case become '\n', the rest upper case); a thread then owns LOC_S consecutive starts and rolls, from LDS:
//   * the index of the last bad byte at or before the window's end (the window holds none when it lies before the start);
//   * four 32-bit polynomial hashes: the forward strand's left and right flank, and the reverse complement's left flank
//     (the complements of the window's last L bases, read backwards) and right flank (of its first R bases, backwards).
// (left, right) hashes to 64 bits (loc_mix); a valid window whose hash has its bit set in the LDS copy of the membership
// bitmap probes the global open-addressing table, and a slot with the same 64-bit hash is checked base by base against
// the flank text (the arena): a hash collision never yields a row.  Bytes are hashed, not 2-bit codes, so packed and
// wide geometries and windows that hold IUPAC letters take the same path.
//
// Pass 1 (EMIT = false) counts the hits per tile; k_loc_offsets scans the counts; pass 2 (EMIT = true) revisits the tiles
// that hold hits and writes them at their tile's offset in position order, '+' before '-' at one position: no atomics,
// the same bytes on every run.  The staging, the block scan, the count / emit epilogue, k_loc_offsets, k_loc_sep (the record
// separators, listed the same way) and k_loc_cut are k_scan.inc's: the near-match and product passes use them too.
struct LocGeom {
    u32 L, D, R, k, omit;
    u32 binv;                       // LOC_HB^-1 mod 2^32
    u32 powL, powR;                 // LOC_HB^(L-1), LOC_HB^(R-1) (0 for an empty flank)
};

struct LocSlot {                    // one slot of the flank table: the 64-bit hash of (left, right) and the group
    u64 h;
    u32 gid, pad;
};

// the hash table's verdict on one window strand: the group, or LOC_EMPTY
__device__ inline u32 loc_probe(u64 h, const LocSlot* __restrict__ table, u64 tmask, const uint8_t* __restrict__ arena,
                                const LocGeom& lg, const uint8_t* tile, const uint8_t* comp, u32 p, bool rc) {
    const u32 LR = lg.L + lg.R;
    for (u64 i = h & tmask;; i = (i + 1) & tmask) {
        const LocSlot e = table[i];
        if (e.gid == LOC_EMPTY) return LOC_EMPTY;
        if (e.h != h) continue;
        const uint8_t* f = arena + (u64)e.gid * LR;
        bool same = true;
        if (!rc) {
            #pragma unroll 1
            for (u32 j = 0; j < lg.L && same; j++) same = tile[loc_at(p + j)] == f[j];
            #pragma unroll 1
            for (u32 j = 0; j < lg.R && same; j++) same = tile[loc_at(p + lg.L + lg.D + j)] == f[lg.L + j];
        } else {
            #pragma unroll 1
            for (u32 j = 0; j < lg.L && same; j++) same = comp[tile[loc_at(p + lg.k - 1 - j)]] == f[j];
            #pragma unroll 1
            for (u32 j = 0; j < lg.R && same; j++) same = comp[tile[loc_at(p + lg.R - 1 - j)]] == f[lg.L + j];
        }
        if (same) return e.gid;     // (the flank pairs of the groups are distinct: h_locate.inc refuses a repeat)
    }
}

// one thread's window starts [s, e) of the staged tile: on_hit(p, strand, group) in position order, '+' first
template <typename F>
__device__ inline void loc_roll(const LocGeom& lg, const uint8_t* tile, const uint8_t* comp, const u32* bm,
                                const LocSlot* __restrict__ table, u64 tmask, const uint8_t* __restrict__ arena, u32 s, u32 e,
                                F&& on_hit) {
    if (s >= e) return;
    const u32 L = lg.L, R = lg.R, k = lg.k, RO = lg.L + lg.D;
    u32 hfl = 0, hfr = 0, grl = 0, grr = 0;
    #pragma unroll 1
    for (u32 j = 0; j < L; j++) hfl = hfl * LOC_HB + tile[loc_at(s + j)];
    #pragma unroll 1
    for (u32 j = 0; j < R; j++) hfr = hfr * LOC_HB + tile[loc_at(s + RO + j)];
    #pragma unroll 1
    for (u32 j = L; j-- > 0;) grl = grl * LOC_HB + comp[tile[loc_at(s + k - L + j)]];
    #pragma unroll 1
    for (u32 j = R; j-- > 0;) grr = grr * LOC_HB + comp[tile[loc_at(s + j)]];
    int bad = -1;                   // the last bad byte in [s, s + k)
    #pragma unroll 1
    for (u32 j = k; j-- > 0;)
        if (tile[loc_at(s + j)] == '\n') { bad = (int)(s + j); break; }
    for (u32 p = s;; p++) {
        if (bad < (int)p) {
            const u64 hf = loc_mix(hfl, hfr), hr = loc_mix(grl, grr);
            if (scan_bm_test(bm, hf)) {
                const u32 g = loc_probe(hf, table, tmask, arena, lg, tile, comp, p, false);
                if (g != LOC_EMPTY) on_hit(p, 0u, g);
            }
            if (scan_bm_test(bm, hr)) {
                const u32 g = loc_probe(hr, table, tmask, arena, lg, tile, comp, p, true);
                if (g != LOC_EMPTY) on_hit(p, 1u, g);
            }
        }
        if (p + 1 >= e) break;
        // slide to p + 1: byte p + k enters the window
        const u32 in = tile[loc_at(p + k)];
        if (in == '\n') bad = (int)(p + k);
        if (L) {
            hfl = (hfl - tile[loc_at(p)] * lg.powL) * LOC_HB + tile[loc_at(p + L)];
            grl = (grl - comp[tile[loc_at(p + k - L)]]) * lg.binv + comp[in] * lg.powL;
        }
        if (R) {
            hfr = (hfr - tile[loc_at(p + RO)] * lg.powR) * LOC_HB + in;
            grr = (grr - comp[tile[loc_at(p)]]) * lg.binv + comp[tile[loc_at(p + R)]] * lg.powR;
        }
    }
}

// the locate scan: persistent workgroups over tiles of LOC_T * LOC_S window starts.  EMIT = false: tcount[tile] = hits;
// EMIT = true: the hits of the tiles with any, at toff[tile] (k_loc_offsets), as kr_loc_hit
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_loc_scan(const uint8_t* __restrict__ bases, u64 n, LocGeom lg,
                                                    const u32* __restrict__ bitmap, const LocSlot* __restrict__ table, u64 tmask,
                                                    const uint8_t* __restrict__ arena, u64 ntiles, u32* __restrict__ tcount,
                                                    const u64* __restrict__ toff, kr_loc_hit* __restrict__ out) {
    extern __shared__ __align__(16) u32 loc_lds[];
    u32* bm = loc_lds;                                            // LOC_BM_WORDS
    u32* scan = bm + LOC_BM_WORDS;                                // LOC_T
    uint8_t* comp = (uint8_t*)(scan + LOC_T);                     // 256
    uint8_t* tile = comp + 256;                                   // loc_at(LOC_T * LOC_S + k - 1) bytes
    scan_load_bitmap(bm, bitmap);
    comp[threadIdx.x] = loc_comp((uint8_t)threadIdx.x);
    const u64 nw = n >= lg.k ? n - lg.k + 1 : 0;                  // window starts of the genome
    const u32 TP = LOC_T * LOC_S;
    for (u64 tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        if (EMIT && tcount[tl] == 0) continue;                    // (workgroup-uniform)
        const u64 t0 = tl * TP;
        scan_stage_tile(bases, n, t0, TP + lg.k - 1, lg.omit, tile);
        u32 s, e;
        scan_lane_starts(nw, t0, &s, &e);
        u32 cnt = 0;
        loc_roll(lg, tile, comp, bm, table, tmask, arena, s, e, [&](u32, u32, u32) { cnt++; });
        kr_loc_hit* o = out + scan_epilogue<EMIT>(cnt, scan, tl, tcount, toff, nullptr);
        if (!EMIT) continue;
        loc_roll(lg, tile, comp, bm, table, tmask, arena, s, e, [&](u32 p, u32 strand, u32 g) {
            kr_loc_hit hit;
            hit.group = g;
            hit.strand = strand;
            hit.pos = t0 + p;
            *o++ = hit;
        });
    }
}
