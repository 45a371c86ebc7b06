// k_near.inc -- part of krisp_hip.hip (one translation unit): the near-match pass (--out_near): every window of a genome within
// Hamming distance M of a target (an ingroup window of a diagnostic region), on both strands.  The host driver is h_near.inc;
// the context, the genome on the device, the separator list and the tile layout are the locate pass's (k_locate.inc).
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
#define NEAR_MAXP 4                 // pieces at most: M <= 3
#define NEAR_EMPTY 0u               // a free slot has no entries

struct NearGeom {
    u32 k, omit, np, M;
    u32 lo[2], hi[2];               // strand s: column c lies in a conserved flank when c < lo[s] or c >= hi[s]
    u32 off[NEAR_MAXP + 1];         // piece j = columns [off[j], off[j + 1])
    u32 pw[NEAR_MAXP];              // LOC_HB^(length of piece j - 1)
};

struct NearSlot {                   // the entries whose piece has this key: list[start, start + count)
    u64 key;
    u32 start, count;
};

__host__ __device__ inline u64 near_key(u32 piece, u32 h) { return loc_mix(piece * 0x85EBCA6Bu + 1u, h); }

// exclusive prefix sum of one u64 per thread over the workgroup; *total = the sum
__device__ inline u64 near_block_scan(u64 v, u64* sh, u64* total) {
    const u32 t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (u32 d = 1; d < LOC_T; d <<= 1) {
        const u64 a = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const u64 incl = sh[t];
    *total = sh[LOC_T - 1];
    __syncthreads();
    return incl - v;
}

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

template <u32 NP, typename F>
__device__ inline void near_probe(const NearGeom& ng, const uint8_t* tile, const u32* bm, const NearSlot* __restrict__ table, u64 tmask,
                                  const u32* __restrict__ list, const uint8_t* __restrict__ arena, u32 p, u32 piece, u32 h, F&& on_hit) {
    const u64 key = near_key(piece, h);
    const u32 b = (u32)(key >> (64 - LOC_BM_LOG));
    if (!((bm[b >> 5] >> (b & 31)) & 1u)) return;
    for (u64 i = key & tmask;; i = (i + 1) & tmask) {
        const NearSlot s = table[i];
        if (s.count == NEAR_EMPTY) return;
        if (s.key != key) continue;
        #pragma unroll 1
        for (u32 q = 0; q < s.count; q++) near_check<NP>(ng, tile, arena, p, list[s.start + q], piece, on_hit);
        return;                                     // (a key has one slot)
    }
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
                near_probe<NP>(ng, tile, bm, table, tmask, list, arena, p, j, h[j],
                               [&](u32 en, u32 mm, u32 fm) { on_hit(p, en, mm, fm); });
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
    const u32 t = threadIdx.x;
    for (u32 i = t; i < LOC_BM_WORDS / 4; i += LOC_T) ((uint4*)bm)[i] = ((const uint4*)bitmap)[i];
    const u64 nw = n >= ng.k ? n - ng.k + 1 : 0;                  // window starts of the genome
    const u32 TP = LOC_T * LOC_S;
    const u32 tb = TP + ng.k - 1;                                 // bytes a tile reads
    u32* tile32 = (u32*)tile;
    for (u64 tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        if (EMIT && tcount[tl] == 0) continue;                    // (workgroup-uniform)
        const u64 t0 = tl * TP;
        __syncthreads();                                          // (the previous tile's readers are done)
        for (u32 c = t; c * 16 < tb; c += LOC_T) {
            const u64 g = t0 + (u64)c * 16;
            u32 w[4];
            if (g + 16 <= n) {
                const uint4 v = *(const uint4*)(bases + g);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
#pragma unroll
                for (u32 q = 0; q < 4; q++) {
                    u32 x = 0;
                    for (u32 b = 0; b < 4; b++) {
                        const u64 i = g + 4 * q + b;
                        x |= (u32)(i < n ? bases[i] : (uint8_t)'\n') << (8 * b);
                    }
                    w[q] = x;
                }
            }
#pragma unroll
            for (u32 q = 0; q < 4; q++) {
                u32 x = 0;
                for (u32 b = 0; b < 4; b++) x |= loc_stage_byte((w[q] >> (8 * b)) & 0xFFu, ng.omit) << (8 * b);
                tile32[loc_at(c * 16 + 4 * q) >> 2] = x;
            }
        }
        __syncthreads();
        const u32 np = (u32)min((u64)TP, nw - t0);               // window starts of this tile
        const u32 s = min(t * LOC_S, np), e = min(s + LOC_S, np);
        u64 cnt = 0;
        near_roll<NP>(ng, tile, bm, table, tmask, list, arena, s, e, [&](u32, u32, u32, u32) { cnt++; });
        u64 total;
        const u64 before = near_block_scan(cnt, scan, &total);
        if (!EMIT) {
            if (t == 0) {
                if (total >> 32) *overflow = 1u;
                tcount[tl] = (total >> 32) ? 0u : (u32)total;
            }
            continue;
        }
        kr_near_hit* o = out + toff[tl] + before;
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

// the text of the hits' windows, a row of k bytes per hit: upper case, the reverse complement for strand 1 (k_loc_cut's rows)
__global__ __launch_bounds__(256) void k_near_cut(const uint8_t* __restrict__ bases, const kr_near_hit* __restrict__ hits, u64 nhits,
                                                  u32 k, uint8_t* __restrict__ rows) {
    const u64 total = nhits * k;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
        const u64 h = i / k;
        const u32 j = (u32)(i - h * k);
        const kr_near_hit e = hits[h];
        u32 b = bases[e.pos + (e.strand ? k - 1 - j : j)];
        if (b >= 'a' && b <= 'z') b -= 32;
        rows[i] = e.strand ? loc_comp((uint8_t)b) : (uint8_t)b;
    }
}
