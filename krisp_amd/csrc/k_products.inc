// k_products.inc -- part of krisp_hip.hip (one translation unit): the product pass (--out_products): in-silico PCR of the
// regions' conserved flanks against a genome.  The host driver is h_products.inc; the context and the genome on the device
// are the locate pass's; the tile layout, the staging, the seed table's slots and probe, the count / emit epilogue and the
// separator kernels are k_scan.inc's.
//
// Entries: every distinct left flank text A (len[0] letters) gives entry 2 i (A) and 2 i + 1 (rc(A)); every distinct right
// flank text B (len[1] letters) gives entry nleft2 + 2 j (B) and nleft2 + 2 j + 1 (rc(B)), nleft2 = twice the left texts.
// A SITE is a valid window of an entry's length within Hamming distance M of its text.  Pigeonhole seeds as in k_near.inc,
// per length class: the columns of a class are cut into NP = M + 1 pieces, an entry is listed under (class, piece, 32-bit
// hash of the piece); with NC = 1 (both flanks of one length) there is one class and half the hashes.
//
// k_prod_scan stages a tile as k_loc_scan does, with max(len) - 1 bases of overhang; a thread owns LOC_S starts and rolls,
// per class, the last bad byte and NP hashes.  A (window, entry) pair within M is emitted by the FIRST equal piece only.
// Count per tile, k_loc_offsets, emit on a second visit: sites in position order, at one position by class, piece and list
// order.  k_prod_rec gives every site its record (the separators before it).  k_prod_join: a thread per OPENING site (A, or
// rc(B)) walks the following sites of its record up to max_product and pairs it with every CLOSING site (B, or rc(A)) whose
// (left, right) texts are a region's pair: count per block, k_loc_offsets, emit.  No atomics: the same bytes on every run.
#define PROD_END 5                  // columns at the primer's 3' end that the end mismatches count

struct ProdGeom {
    u32 len[2];                     // letters of a left / right flank text
    u32 end[2];                     // min(PROD_END, len)
    u32 omit, M, nleft2, maxlen;
    u32 off[2][NEAR_MAXP + 1];      // class c, piece j = columns [off[c][j], off[c][j + 1])
    u32 pw[2][NEAR_MAXP];           // LOC_HB^(length of the piece - 1)
};

__host__ __device__ inline u32 prod_class(const ProdGeom& pg, u32 e) { return e >= pg.nleft2 ? 1u : 0u; }
__host__ __device__ inline u64 prod_text_at(const ProdGeom& pg, u32 e) {
    return e < pg.nleft2 ? (u64)e * pg.len[0] : (u64)pg.nleft2 * pg.len[0] + (u64)(e - pg.nleft2) * pg.len[1];
}
// the 3' end of the primer lies in the LAST columns of A and of rc(B) as the text reads, in the FIRST of B and of rc(A)
__host__ __device__ inline bool prod_end_last(const ProdGeom& pg, u32 e) { return ((e < pg.nleft2) ? 1u : 0u) != (e & 1u); }
__host__ __device__ inline bool prod_opening(const ProdGeom& pg, u32 e) { return prod_end_last(pg, e); }

// window p of the tile against entry e (class c), found through piece `via`: on_hit(entry, mismatches, end mismatches)
template <u32 NP, typename F>
__device__ inline void prod_check(const ProdGeom& pg, const uint8_t* tile, const uint8_t* __restrict__ arena, u32 p, u32 e, u32 via,
                                  F&& on_hit) {
    const u32 c = prod_class(pg, e);
    const uint8_t* f = arena + prod_text_at(pg, e);
    const u32 n = pg.len[c];
    const bool last = prod_end_last(pg, e);
    const u32 elo = last ? n - pg.end[c] : 0u, ehi = last ? n : pg.end[c];
    u32 mm = 0, em = 0;
#pragma unroll
    for (u32 j = 0; j < NP; j++) {
        u32 pm = 0;
        #pragma unroll 1
        for (u32 q = pg.off[c][j]; q < pg.off[c][j + 1]; q++) {
            const u32 ne = tile[loc_at(p + q)] != f[q];
            pm += ne;
            em += ne & (u32)(q >= elo && q < ehi);
        }
        mm += pm;
        if (j < via && pm == 0) return;             // an earlier piece is equal too: that piece emits the pair
        if (j == via && pm != 0) return;            // (a hash collision)
        if (mm > pg.M) return;
    }
    on_hit(e, mm, em);
}

// one thread's window starts [s, e) of the staged tile: on_hit(p, entry, mismatches, end mismatches), position order
template <u32 NP, u32 NC, typename F>
__device__ inline void prod_roll(const ProdGeom& pg, const uint8_t* tile, const u32* bm, const NearSlot* __restrict__ table, u64 tmask,
                                 const u32* __restrict__ list, const uint8_t* __restrict__ arena, u32 s, u32 e, F&& on_hit) {
    if (s >= e) return;
    u32 h[NC][NP];
    int bad[NC];                    // the last bad byte in [s, s + len[c])
#pragma unroll
    for (u32 c = 0; c < NC; c++) {
#pragma unroll
        for (u32 j = 0; j < NP; j++) {
            u32 x = 0;
            #pragma unroll 1
            for (u32 q = pg.off[c][j]; q < pg.off[c][j + 1]; q++) x = x * LOC_HB + tile[loc_at(s + q)];
            h[c][j] = x;
        }
        bad[c] = -1;
        #pragma unroll 1
        for (u32 j = pg.len[c]; j-- > 0;)
            if (tile[loc_at(s + j)] == '\n') { bad[c] = (int)(s + j); break; }
    }
    for (u32 p = s;; p++) {
#pragma unroll
        for (u32 c = 0; c < NC; c++) {
            if (bad[c] < (int)p) {
#pragma unroll
                for (u32 j = 0; j < NP; j++)
                    // (entries of another class under the key -- NC == 1 lists both kinds under class 0 -- are of the
                    // same length by construction)
                    seed_probe(bm, table, tmask, list, near_key(c * NEAR_MAXP + j, h[c][j]), [&](u32 en) {
                        prod_check<NP>(pg, tile, arena, p, en, j, [&](u32 en, u32 mm, u32 em) { on_hit(p, en, mm, em); });
                    });
            }
        }
        if (p + 1 >= e) break;
        // slide to p + 1: the byte that leaves piece j + 1 enters piece j
        const u32 first = tile[loc_at(p)];
#pragma unroll
        for (u32 c = 0; c < NC; c++) {
            u32 out = first;
#pragma unroll
            for (u32 j = 0; j < NP; j++) {
                const u32 in = tile[loc_at(p + pg.off[c][j + 1])];
                h[c][j] = (h[c][j] - out * pg.pw[c][j]) * LOC_HB + in;
                out = in;
            }
            if (out == '\n') bad[c] = (int)(p + pg.len[c]);       // (the last piece's new byte is byte p + len[c])
        }
    }
}

// the site scan: persistent workgroups over tiles of LOC_T * LOC_S window starts (starts of the SHORTER class: a window of
// the longer one that runs past the genome's end holds a staged '\n').  EMIT = false: tcount[tile] = sites (a tile with 2^32
// or more sets *overflow); EMIT = true: the sites of the tiles with any, at toff[tile] (k_loc_offsets)
template <u32 NP, u32 NC, bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_prod_scan(const uint8_t* __restrict__ bases, u64 n, ProdGeom pg,
                                                     const u32* __restrict__ bitmap, const NearSlot* __restrict__ table, u64 tmask,
                                                     const u32* __restrict__ list, const uint8_t* __restrict__ arena, u64 nw,
                                                     u64 ntiles, u32* __restrict__ tcount, const u64* __restrict__ toff,
                                                     kr_product_site* __restrict__ out, u32* __restrict__ overflow) {
    extern __shared__ __align__(16) u32 prod_lds[];
    u32* bm = prod_lds;                                           // LOC_BM_WORDS
    u64* scan = (u64*)(bm + LOC_BM_WORDS);                        // LOC_T
    uint8_t* tile = (uint8_t*)(scan + LOC_T);                     // loc_at(LOC_T * LOC_S + maxlen - 1) bytes
    scan_load_bitmap(bm, bitmap);
    const u32 TP = LOC_T * LOC_S;
    for (u64 tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        if (EMIT && tcount[tl] == 0) continue;                    // (workgroup-uniform)
        const u64 t0 = tl * TP;
        scan_stage_tile(bases, n, t0, TP + pg.maxlen - 1, pg.omit, tile);
        u32 s, e;
        scan_lane_starts(nw, t0, &s, &e);
        u64 cnt = 0;
        prod_roll<NP, NC>(pg, tile, bm, table, tmask, list, arena, s, e, [&](u32, u32, u32, u32) { cnt++; });
        kr_product_site* o = out + scan_epilogue<EMIT>(cnt, scan, tl, tcount, toff, overflow);
        if (!EMIT) continue;
        prod_roll<NP, NC>(pg, tile, bm, table, tmask, list, arena, s, e, [&](u32 p, u32 en, u32 mm, u32 em) {
            kr_product_site site;
            site.pos = t0 + p;
            site.entry = en;
            site.mismatches = (uint8_t)mm;
            site.end_mismatches = (uint8_t)em;
            site.pad = 0;
            *o++ = site;
        });
    }
}

// rec[i] = the record of site i: the separators before its position (seps ascending)
__global__ __launch_bounds__(256) void k_prod_rec(const kr_product_site* __restrict__ sites, u64 ns, const u64* __restrict__ seps,
                                                  u64 nseps, u32* __restrict__ rec) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < ns; i += (u64)gridDim.x * 256) {
        const u64 pos = sites[i].pos;
        u64 lo = 0, hi = nseps;
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if (seps[mid] < pos) lo = mid + 1; else hi = mid;
        }
        rec[i] = (u32)lo;
    }
}

// the region of (left text, right text), or LOC_EMPTY: keys ascending
__device__ inline u32 prod_pair(const u64* __restrict__ keys, const u32* __restrict__ idx, u32 npairs, u32 li, u32 rj) {
    const u64 key = ((u64)li << 32) | rj;
    u32 lo = 0, hi = npairs;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < npairs && keys[lo] == key ? idx[lo] : LOC_EMPTY;
}

// the products of opening site i: on_hit(closing site's index, the closing site, pair)
template <typename F>
__device__ inline void prod_walk(const ProdGeom& pg, const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                 const u64* __restrict__ keys, const u32* __restrict__ idx, u32 npairs, u32 max_product, u64 i,
                                 F&& on_hit) {
    const kr_product_site a = sites[i];
    if (!prod_opening(pg, a.entry)) return;
    const bool plus = a.entry < pg.nleft2;                        // A ... B; otherwise rc(B) ... rc(A)
    const u32 n1 = pg.len[plus ? 0 : 1], n2 = pg.len[plus ? 1 : 0];
    const u64 first = a.pos + n1, last = a.pos + max_product - n2;   // (max_product >= n1 + n2: the host refuses less)
    const u32 r = rec[i];
    for (u64 j = i + 1; j < ns; j++) {
        const kr_product_site b = sites[j];
        if (b.pos > last || rec[j] != r) break;
        if (b.pos < first) continue;
        // the closing site on this strand: B as written after A, rc(A) after rc(B)
        if ((b.entry < pg.nleft2) == plus || (b.entry & 1u) == (plus ? 1u : 0u)) continue;
        const u32 li = (plus ? a.entry : b.entry) >> 1, rj = ((plus ? b.entry : a.entry) - pg.nleft2) >> 1;
        const u32 pr = prod_pair(keys, idx, npairs, li, rj);
        if (pr != LOC_EMPTY) on_hit(b, pr, plus, n2);
    }
}

// the join: a thread per site, a workgroup per LOC_T sites.  EMIT = false: bcount[block] = products (2^32 or more in a
// block set *overflow); EMIT = true: the products of the blocks with any, at boff[block], in the opening sites' order
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_prod_join(const kr_product_site* __restrict__ sites, u64 ns, const u32* __restrict__ rec,
                                                     ProdGeom pg, const u64* __restrict__ keys, const u32* __restrict__ idx, u32 npairs,
                                                     u32 max_product, u32* __restrict__ bcount, const u64* __restrict__ boff,
                                                     kr_product_hit* __restrict__ out, u32* __restrict__ overflow) {
    __shared__ u64 scan[LOC_T];
    const u64 bl = blockIdx.x;
    if (EMIT && bcount[bl] == 0) return;                          // (workgroup-uniform)
    const u64 i = bl * LOC_T + threadIdx.x;
    u64 cnt = 0;
    if (i < ns)
        prod_walk(pg, sites, ns, rec, keys, idx, npairs, max_product, i, [&](const kr_product_site&, u32, bool, u32) { cnt++; });
    kr_product_hit* o = out + scan_epilogue<EMIT>(cnt, scan, bl, bcount, boff, overflow);
    if (!EMIT || i >= ns) return;
    const kr_product_site a = sites[i];
    prod_walk(pg, sites, ns, rec, keys, idx, npairs, max_product, i, [&](const kr_product_site& b, u32 pr, bool plus, u32 n2) {
        const kr_product_site& lf = plus ? a : b;                 // the site of the left flank's text (A or rc(A))
        const kr_product_site& rt = plus ? b : a;
        kr_product_hit hit;
        hit.pos = a.pos;
        hit.length = (u32)(b.pos + n2 - a.pos);
        hit.pair = pr;
        hit.strand = plus ? 0 : 1;
        hit.left_mm = lf.mismatches;
        hit.right_mm = rt.mismatches;
        hit.left_end_mm = lf.end_mismatches;
        hit.right_end_mm = rt.end_mismatches;
        hit.pad[0] = hit.pad[1] = hit.pad[2] = 0;
        *o++ = hit;
    });
}
