// k_scan.inc -- part of krisp_hip.hip (one translation unit): what the three passes that scan one genome at a time against a
// small table share on the device: the locate pass (k_locate.inc), the near-match pass (k_near.inc) and the product pass
// (k_products.inc).  The host side of the same is h_scan.inc.
//
// A genome's bases are scanned once, from the device's copy (no sort).  A workgroup stages a tile of LOC_T * LOC_S window
// starts plus an overhang (the longest window - 1) in LDS (scan_stage_tile: 16-byte loads, coalesced; separators, N / n
// and -- under omit-soft -- lower case become '\n', the rest upper case); a thread then owns LOC_S consecutive starts and
// rolls its pass's hashes from LDS.  A hash whose bit is set in the LDS copy of the pass's membership bitmap (scan_bm_test)
// probes the pass's open-addressing table in global memory; the seed passes share the table's form (NearSlot, seed_probe).
//
// Every list is made in two passes (scan_epilogue): EMIT = false counts per tile (or block), k_loc_offsets scans the counts,
// EMIT = true revisits the tiles that hold any and writes at the tile's offset, each lane after the lanes before it: no
// atomics, the same bytes on every run.  k_loc_sep lists the positions of the record separators that way, k_loc_cut cuts
// the text of the hits' windows.
#define LOC_T 256                   // threads per workgroup
#define LOC_S 64                    // window starts per thread (a power of two: LDS addressing below)
#define LOC_SH 6                    // log2(LOC_S)
#define LOC_BM_LOG 18               // membership bitmap: 2^18 bits = 32 KB of LDS (3 workgroups per CU with the tile)
#define LOC_BM_WORDS (1u << (LOC_BM_LOG - 5))
#define LOC_EMPTY 0xFFFFFFFFu
#define LOC_HB 0x9E3779B1u          // hash multiplier (odd: invertible modulo 2^32)
#define LOC_SEP_BYTES 64            // k_loc_sep: bytes per thread
#define NEAR_MAXP 4                 // seed pieces at most: M <= 3
#define NEAR_EMPTY 0u               // a free seed slot has no entries

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

// the workgroup stages bytes [t0, t0 + tb) of the n bases as its tile (bytes past the genome's end are '\n'); the tile
// is ready on return
__device__ inline void scan_stage_tile(const uint8_t* __restrict__ bases, u64 n, u64 t0, u32 tb, u32 omit, uint8_t* tile) {
    u32* tile32 = (u32*)tile;
    __syncthreads();                                              // (the previous tile's readers are done)
    for (u32 c = threadIdx.x; c * 16 < tb; c += LOC_T) {
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
            for (u32 b = 0; b < 4; b++) x |= loc_stage_byte((w[q] >> (8 * b)) & 0xFFu, omit) << (8 * b);
            tile32[loc_at(c * 16 + 4 * q) >> 2] = x;
        }
    }
    __syncthreads();
}

// the workgroup copies a pass's membership bitmap to LDS (visible after the next barrier: scan_stage_tile has one)
__device__ inline void scan_load_bitmap(u32* bm, const u32* __restrict__ bitmap) {
    for (u32 i = threadIdx.x; i < LOC_BM_WORDS / 4; i += LOC_T) ((uint4*)bm)[i] = ((const uint4*)bitmap)[i];
}

// the window starts [*s, *e) of the tile at t0 that this lane owns, of the genome's nw
__device__ inline void scan_lane_starts(u64 nw, u64 t0, u32* s, u32* e) {
    const u32 np = (u32)min((u64)(LOC_T * LOC_S), nw - t0);     // window starts of this tile
    *s = min(threadIdx.x * LOC_S, np);
    *e = min(*s + LOC_S, np);
}

// the bit of a 64-bit hash in the LDS copy of a membership bitmap
__device__ inline bool scan_bm_test(const u32* bm, u64 h) {
    const u32 b = (u32)(h >> (64 - LOC_BM_LOG));
    return (bm[b >> 5] >> (b & 31)) & 1u;
}

// exclusive prefix sum of one value per thread over the workgroup; *total = the sum
template <typename T>
__device__ inline T block_scan(T v, T* sh, T* total) {
    const u32 t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (u32 d = 1; d < LOC_T; d <<= 1) {
        const T a = t >= d ? sh[t - d] : (T)0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const T incl = sh[t];
    *total = sh[LOC_T - 1];
    __syncthreads();
    return incl - v;
}

// what follows a lane's counting in a two-pass kernel, for tile (or block) tl.  EMIT = false: tcount[tl] = the lanes' sum;
// a 64-bit sum of 2^32 or more sets *overflow instead (a 32-bit count has no flag).  EMIT = true: -> where the lane's
// output starts: the tile's offset (k_loc_offsets) plus what the lanes before it write
template <bool EMIT, typename T>
__device__ inline u64 scan_epilogue(T cnt, T* sh, u64 tl, u32* __restrict__ tcount, const u64* __restrict__ toff, u32* overflow) {
    T total;
    const T before = block_scan(cnt, sh, &total);
    if constexpr (EMIT) {
        return toff[tl] + before;
    } else {
        if (threadIdx.x == 0) {
            if constexpr (sizeof(T) > 4) {
                if (total >> 32) *overflow = 1u;
                tcount[tl] = (total >> 32) ? 0u : (u32)total;
            } else {
                tcount[tl] = total;
            }
        }
        return 0;
    }
}

// a wavefront's 64 neighbouring list elements counted by key (the tallies of the guide-hit and the multiplex pass): a run
// of equal keys among them is one integer add of its length by its first lane; key ~0 = not counted.  Every lane of the
// wavefront calls it (the shuffle and the ballot are whole)
__device__ inline void tally_runs(u32 key, u32 lane, u32* __restrict__ tally) {
    const u32 prev = (u32)__shfl_up((int)key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const u64 heads = __ballot(head);
    if (head && key != ~0u) {
        const u64 later = lane == 63 ? 0ull : heads >> (lane + 1);          // the heads behind this one
        atomicAdd(tally + key, later ? (u32)__ffsll((long long)later) : 64u - lane);
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
    u64* o = out + scan_epilogue<EMIT>(c, scan, tl, cnt, off, nullptr);
    if (!EMIT) return;
#pragma unroll
    for (u32 q = 0; q < LOC_SEP_BYTES / 4; q++)
        for (u32 b = 0; b < 4; b++)
            if (((w[q] >> (8 * b)) & 0xFFu) == '\n') *o++ = g + 4 * q + b;
}

// the seed table of the near-match and product passes: a slot names the entries whose piece has this key,
// list[start, start + count) (h_scan.inc: seed_table_build)
struct NearSlot {
    u64 key;
    u32 start, count;
};

__host__ __device__ inline u64 near_key(u32 piece, u32 h) { return loc_mix(piece * 0x85EBCA6Bu + 1u, h); }

// fn(entry) for every entry listed under the key, in the list's order (the pass checks each: the key is a hash)
template <typename F>
__device__ inline void seed_probe(const u32* bm, const NearSlot* __restrict__ table, u64 tmask, const u32* __restrict__ list, u64 key,
                                  F&& fn) {
    if (!scan_bm_test(bm, key)) return;
    for (u64 i = key & tmask;; i = (i + 1) & tmask) {
        const NearSlot s = table[i];
        if (s.count == NEAR_EMPTY) return;
        if (s.key != key) continue;
        #pragma unroll 1
        for (u32 q = 0; q < s.count; q++) fn(list[s.start + q]);
        return;                                     // (a key has one slot)
    }
}

// the text of the hits' windows (H: kr_loc_hit, kr_near_hit), a row of k bytes per hit: upper case, the reverse
// complement for strand 1 (what the alignment lists for the genome; the host writes U for T in an RNA genome)
template <typename H>
__global__ __launch_bounds__(256) void k_loc_cut(const uint8_t* __restrict__ bases, const H* __restrict__ hits, u64 nhits, u32 k,
                                                 uint8_t* __restrict__ rows) {
    const u64 total = nhits * k;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
        const u64 h = i / k;
        const u32 j = (u32)(i - h * k);
        const H e = hits[h];
        u32 b = bases[e.pos + (e.strand ? k - 1 - j : j)];
        if (b >= 'a' && b <= 'z') b -= 32;
        rows[i] = e.strand ? loc_comp((uint8_t)b) : (uint8_t)b;
    }
}
