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
// the same bytes on every run.  k_loc_sep lists the positions of the record separators the same way (count / scan / emit).
#define LOC_T 256                   // threads per workgroup
#define LOC_S 64                    // window starts per thread (a power of two: LDS addressing below)
#define LOC_SH 6                    // log2(LOC_S)
#define LOC_BM_LOG 18               // membership bitmap: 2^18 bits = 32 KB of LDS (3 workgroups per CU with the tile)
#define LOC_BM_WORDS (1u << (LOC_BM_LOG - 5))
#define LOC_EMPTY 0xFFFFFFFFu
#define LOC_HB 0x9E3779B1u          // hash multiplier (odd: invertible modulo 2^32)
#define LOC_SEP_BYTES 64            // k_loc_sep: bytes per thread

struct LocGeom {
    u32 L, D, R, k, omit;
    u32 binv;                       // LOC_HB^-1 mod 2^32
    u32 powL, powR;                 // LOC_HB^(L-1), LOC_HB^(R-1) (0 for an empty flank)
};

struct LocSlot {                    // one slot of the flank table: the 64-bit hash of (left, right) and the group
    u64 h;
    u32 gid, pad;
};

__host__ __device__ inline u64 loc_mix(u32 hl, u32 hr) {
    u64 x = ((u64)hl << 32) | hr;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// COMP_MAP (kstream.py:11-18) on upper-case bytes; every other byte maps to itself (it is '\n' after staging, or a
// character the reference refuses before a group exists)
__host__ __device__ inline uint8_t loc_comp(uint8_t b) {
    switch (b) {
    case 'A': return 'T'; case 'T': return 'A'; case 'G': return 'C'; case 'C': return 'G';
    case 'R': return 'Y'; case 'Y': return 'R'; case 'M': return 'K'; case 'K': return 'M';
    case 'B': return 'V'; case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D';
    default: return b;             // S, W, N and the rest
    }
}

__device__ inline u32 loc_stage_byte(u32 b, u32 omit) {
    const bool lower = b >= 'a' && b <= 'z';
    if (b == '\n' || b == 'N' || b == 'n' || (omit && lower)) return '\n';
    return lower ? b - 32 : b;
}

// byte p of the tile in LDS: 4 bytes of padding after every LOC_S (a thread's bytes start on distinct banks)
__device__ inline u32 loc_at(u32 p) { return p + ((p >> LOC_SH) << 2); }

// exclusive prefix sum of one u32 per thread over the workgroup; *total = the sum
__device__ inline u32 loc_block_scan(u32 v, u32* sh, u32* total) {
    const u32 t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (u32 d = 1; d < LOC_T; d <<= 1) {
        const u32 a = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const u32 incl = sh[t];
    *total = sh[LOC_T - 1];
    __syncthreads();
    return incl - v;
}

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
            const u32 bf = (u32)(hf >> (64 - LOC_BM_LOG)), br = (u32)(hr >> (64 - LOC_BM_LOG));
            if ((bm[bf >> 5] >> (bf & 31)) & 1u) {
                const u32 g = loc_probe(hf, table, tmask, arena, lg, tile, comp, p, false);
                if (g != LOC_EMPTY) on_hit(p, 0u, g);
            }
            if ((bm[br >> 5] >> (br & 31)) & 1u) {
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
    const u32 t = threadIdx.x;
    for (u32 i = t; i < LOC_BM_WORDS / 4; i += LOC_T) ((uint4*)bm)[i] = ((const uint4*)bitmap)[i];
    comp[t] = loc_comp((uint8_t)t);
    const u64 nw = n >= lg.k ? n - lg.k + 1 : 0;                  // window starts of the genome
    const u32 TP = LOC_T * LOC_S;
    const u32 tb = TP + lg.k - 1;                                 // bytes a tile reads
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
                for (u32 b = 0; b < 4; b++) x |= loc_stage_byte((w[q] >> (8 * b)) & 0xFFu, lg.omit) << (8 * b);
                tile32[loc_at(c * 16 + 4 * q) >> 2] = x;
            }
        }
        __syncthreads();
        const u32 np = (u32)min((u64)TP, nw - t0);               // window starts of this tile
        const u32 s = min(t * LOC_S, np), e = min(s + LOC_S, np);
        u32 cnt = 0;
        loc_roll(lg, tile, comp, bm, table, tmask, arena, s, e, [&](u32, u32, u32) { cnt++; });
        u32 total;
        const u32 before = loc_block_scan(cnt, scan, &total);
        if (!EMIT) {
            if (t == 0) tcount[tl] = total;
            continue;
        }
        kr_loc_hit* o = out + toff[tl] + before;
        loc_roll(lg, tile, comp, bm, table, tmask, arena, s, e, [&](u32 p, u32 strand, u32 g) {
            kr_loc_hit hit;
            hit.group = g;
            hit.strand = strand;
            hit.pos = t0 + p;
            *o++ = hit;
        });
    }
}

// exclusive offsets of per-tile counts (one workgroup of 1024 threads, a contiguous run of tiles each): off[n] = the total
__global__ __launch_bounds__(1024) void k_loc_offsets(const u32* __restrict__ cnt, u64 n, u64* __restrict__ off) {
    __shared__ u64 sh[1024];
    const u32 t = threadIdx.x;
    const u64 per = (n + 1023) / 1024, lo = min(n, t * per), hi = min(n, lo + per);
    u64 sum = 0;
    for (u64 i = lo; i < hi; i++) sum += cnt[i];
    sh[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024; d <<= 1) {
        const u64 a = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    u64 run = sh[t] - sum;
    for (u64 i = lo; i < hi; i++) {
        off[i] = run;
        run += cnt[i];
    }
    if (t == 1023) off[n] = sh[1023];
}

// the positions of the record separators ('\n') of n bases: a workgroup per LOC_T * LOC_SEP_BYTES bytes, a thread per
// LOC_SEP_BYTES; EMIT = false: cnt[tile]; EMIT = true: the positions, ascending, at off[tile]
template <bool EMIT>
__global__ __launch_bounds__(LOC_T) void k_loc_sep(const uint8_t* __restrict__ bases, u64 n, u32* __restrict__ cnt,
                                                   const u64* __restrict__ off, u64* __restrict__ out) {
    __shared__ u32 scan[LOC_T];
    const u32 t = threadIdx.x;
    const u64 tl = blockIdx.x;
    if (EMIT && cnt[tl] == 0) return;                             // (workgroup-uniform)
    const u64 g = (tl * LOC_T + t) * LOC_SEP_BYTES;
    u32 w[LOC_SEP_BYTES / 4];
    if (g + LOC_SEP_BYTES <= n) {
#pragma unroll
        for (u32 q = 0; q < LOC_SEP_BYTES / 16; q++) {
            const uint4 v = *(const uint4*)(bases + g + 16 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (u32 q = 0; q < LOC_SEP_BYTES / 4; q++) {
            u32 x = 0;
            for (u32 b = 0; b < 4; b++) {
                const u64 i = g + 4 * q + b;
                x |= (u32)(i < n ? bases[i] : (uint8_t)0) << (8 * b);
            }
            w[q] = x;
        }
    }
    u32 c = 0;
#pragma unroll
    for (u32 q = 0; q < LOC_SEP_BYTES / 4; q++) {
        // (bytes equal to '\n': the zero bytes of w ^ 0x0a0a0a0a, counted exactly)
        const u32 x = w[q] ^ 0x0A0A0A0Au;
        const u32 z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
        c += __popc(z);
    }
    u32 total;
    const u32 before = loc_block_scan(c, scan, &total);
    if (!EMIT) {
        if (t == 0) cnt[tl] = total;
        return;
    }
    u64* o = out + off[tl] + before;
#pragma unroll
    for (u32 q = 0; q < LOC_SEP_BYTES / 4; q++)
        for (u32 b = 0; b < 4; b++)
            if (((w[q] >> (8 * b)) & 0xFFu) == '\n') *o++ = g + 4 * q + b;
}

// the text of the hits' windows, a row of k bytes per hit: upper case, the reverse complement for strand 1 (what the
// alignment lists for the genome; the host writes U for T in an RNA genome)
__global__ __launch_bounds__(256) void k_loc_cut(const uint8_t* __restrict__ bases, const kr_loc_hit* __restrict__ hits, u64 nhits,
                                                 u32 k, uint8_t* __restrict__ rows) {
    const u64 total = nhits * k;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
        const u64 h = i / k;
        const u32 j = (u32)(i - h * k);
        const kr_loc_hit e = hits[h];
        u32 b = bases[e.pos + (e.strand ? k - 1 - j : j)];
        if (b >= 'a' && b <= 'z') b -= 32;
        rows[i] = e.strand ? loc_comp((uint8_t)b) : (uint8_t)b;
    }
}
