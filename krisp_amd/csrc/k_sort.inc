// k_sort.inc -- part of krisp_hip.hip (one translation unit): K1-K4, Kb: pack, histograms, pass 1 of the wide path, pass 2, chunk table, merge fallback (pass 1 of packed windows and the LDS sort: k_sort2.inc)
// ----------------------------------------------------------------------------
// K1  ASCII -> 2-bit codes (32 bases / u64, MSB first) + bad bits (32 / u32, MSB first)
// ----------------------------------------------------------------------------
// allow: bit c set = base code c (A C G T = 0 1 2 3) may occur in a k-mer (kstream's --allow reduced to
// the letters the device carries; 15 = all)
// Four bases at a time (one dword of text, the first base in the low byte), all four lanes of the dword in
// parallel: the code from bits 1-2 of the letter, validity by exact byte compares against A C G T, the 2-bit codes
// and the bad bits gathered by shifts.  (One base at a time cost ~18 instructions per base and made this kernel,
// which moves 1.2 bytes per base, compute-bound at 36 us per 50 Mbp; this is ~9.)
__device__ __forceinline__ u32 bytes_equal(u32 v, u32 k4) {       // 0x80 in every byte of v that equals k4's
    const u32 z = v ^ k4;
    return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
}
__device__ __forceinline__ void pack4(u32 w, int omit, u32 allow, u32& code8, u32& bad4) {
    const u32 up = w & 0xDFDFDFDFu;
    u32 x = (up >> 1) & 0x03030303u;
    x ^= (x >> 1) & 0x01010101u;                                  // A C G T -> 0 1 2 3
    u32 ok = bytes_equal(up, 0x41414141u) | bytes_equal(up, 0x43434343u) | bytes_equal(up, 0x47474747u) |
             bytes_equal(up, 0x54545454u);
    if (omit) ok &= ~((w & 0x20202020u) << 2);                    // lower case: soft-masked, dropped under --omit-soft
    if (allow != 15u) {
#pragma unroll
        for (u32 c = 0; c < 4; c++)
            if (!((allow >> c) & 1u)) ok &= ~bytes_equal(x, c * 0x01010101u);
    }
    x &= (ok >> 7) | (ok >> 6);                                   // a bad base packs as code 0
    code8 = ((x << 6) | (x >> 4) | (x >> 14) | (x >> 24)) & 0xFFu;
    const u32 nb = ~ok & 0x80808080u;
    bad4 = ((nb >> 4) | (nb >> 13) | (nb >> 22) | (nb >> 31)) & 0xFu;
}

__global__ void k_pack(const uint8_t* __restrict__ bases, u64 n, u64* __restrict__ codes,
                       u32* __restrict__ bad, u64 nwords_padded, int omit, u32 allow) {
    u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 stride = (u64)gridDim.x * blockDim.x;
    for (; w < nwords_padded; w += stride) {
        u64 base = w * 32;
        u64 c = 0;
        u32 bd = 0;
        if (base + 32 <= n) {
            const uint4* p = reinterpret_cast<const uint4*>(bases + base);
            uint4 v0 = p[0], v1 = p[1];
            u32 wd[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            u32 hi = 0, lo = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                u32 c8, b4;
                pack4(wd[q], omit, allow, c8, b4);
                if (q < 4) hi |= c8 << (24 - 8 * q); else lo |= c8 << (56 - 8 * q);
                bd |= b4 << (28 - 4 * q);
            }
            c = ((u64)hi << 32) | lo;
        } else {
            for (int q = 0; q < 32; q++) {
                u32 code = 0;
                bool ok = false;
                if (base + q < n) {
                    u32 ch = bases[base + q];
                    u32 up = ch & 0xDF;
                    code = (up >> 1) & 3;
                    code ^= code >> 1;
                    ok = (up == 'A') | (up == 'C') | (up == 'G') | (up == 'T');
                    if (omit) ok = ok & (ch == up);
                    ok = ok & ((allow >> code) & 1u);
                }
                c = (c << 2) | (ok ? code : 0);
                bd = (bd << 1) | (ok ? 0u : 1u);
            }
        }
        codes[w] = c;
        bad[w] = bd;
    }
}


// ---- a whole code word at a time (k_hist8 cheap path, k_hist16): all 32 window starts with
// compile-time bit offsets.  sf = c0:c1 (the window's first bases start at bit 2 j), sr = the same
// string shifted so that the window's LAST `nbase` bases start at bit 2 j; `invalid` bit 31 - j:
// window j holds a bad base (OR of the k bad bits from j on, smeared once per word).
template <int OFF>
__device__ __forceinline__ u32 bits128(const u32 (&w)[5]) {      // 32 bits from bit offset OFF (MSB first)
    constexpr int q = OFF >> 5, r = OFF & 31;
    return r ? __funnelshift_l(w[q + 1], w[q], r) : w[q];
}
__device__ __forceinline__ u32 word_invalid(u32 b0, u32 b1, int k) {
    u64 R = ((u64)b0 << 32) | b1;
    for (int span = 1; span < k;) {
        const int st = span < k - span ? span : k - span;
        R |= R << st;
        span += st;
    }
    return (u32)(R >> 32);
}
// reverse complement of the 16 bases of a dword: bit reversal of the complement, then the two bits of every base
// swapped back
__device__ __forceinline__ u32 revcomp16(u32 x) {
    const u32 y = __brev(~x);
    return ((y & 0xAAAAAAAAu) >> 1) | ((y & 0x55555555u) << 1);
}
// sf = the 64 bases c0:c1 (window J's first bases start at bit 2 J); rv = their reverse complement
// R = revcomp(c1) : revcomp(c0) shifted left by 66 - 2 k bits: window J = bases [J, J + k) of c0:c1, its reverse
// key = bases [64 - J - k, 64 - J) of R, which starts at bit 128 - 2 J - 2 k of R, i.e. at bit 62 - 2 J of rv
__device__ __forceinline__ void word_revstring(u64 c0, u64 c1, int k, u32 (&sf)[5], u32 (&rv)[5]) {
    sf[0] = (u32)(c0 >> 32); sf[1] = (u32)c0; sf[2] = (u32)(c1 >> 32); sf[3] = (u32)c1; sf[4] = 0;
    const u64 r0 = ((u64)revcomp16((u32)c1) << 32) | revcomp16((u32)(c1 >> 32));
    const u64 r1 = ((u64)revcomp16((u32)c0) << 32) | revcomp16((u32)(c0 >> 32));
    const int sl = 66 - 2 * k;                   // 2 .. 64 for k <= 32
    u64 q0, q1;
    if (sl >= 64) { q0 = r1; q1 = 0; }
    else { q0 = (r0 << sl) | (r1 >> (64 - sl)); q1 = r1 << sl; }
    rv[0] = (u32)(q0 >> 32); rv[1] = (u32)q0; rv[2] = (u32)(q1 >> 32); rv[3] = (u32)q1; rv[4] = 0;
}

// the slice test and the pass-1 digit from those 16 bits
__device__ __forceinline__ bool top16_in_slice(u32 t16, const Geom& g, u32& d1) {
    if (g.sbits && (t16 >> (16 - g.sbits)) != g.slice) return false;
    d1 = (t16 >> (8 - g.sbits)) & 0xFFu;
    return true;
}

// (rv: the reverse complement of the word string, shifted so that the reverse key of window J starts at bit
// 62 - 2 J -- word_revstring below; one funnel shift per window instead of complement + bit reversal + pair swap)
template <int J>
__device__ __forceinline__ void hist8_window(const u32 (&sf)[5], const u32 (&rv)[5], u32 invalid, const Geom& g,
                                             u32* lhist) {
    if ((invalid >> (31 - J)) & 1u) return;
    const u32 tf = bits128<2 * J>(sf) >> 16;              // top 16 bits of the forward key
    const u32 tr = bits128<62 - 2 * J>(rv) >> 16;         // ... of the reverse key
    u32 d1;
    if (top16_in_slice(tf, g, d1)) atomicAdd(&lhist[d1], 1u);
    if (top16_in_slice(tr, g, d1)) atomicAdd(&lhist[d1], 1u);
}
template <int... J>
__device__ __forceinline__ void hist8_word(std::integer_sequence<int, J...>, const u32 (&sf)[5], const u32 (&sr)[5],
                                           u32 invalid, const Geom& g, u32* lhist) {
    (hist8_window<J>(sf, sr, invalid, g, lhist), ...);
}

// one strand (WIDE = 3; co_strand.inc): the forward key alone, counted by the digit both of the window's records share --
// the key's high word is the window's first 16 bases (`left` fills it: the FAST geometries)
template <int J>
__device__ __forceinline__ void hist8_window_fwd(const u32 (&sf)[5], u32 invalid, const CoStrand& S, u32* lhist) {
    if ((invalid >> (31 - J)) & 1u) return;
    atomicAdd(&lhist[cs_digit(S, (u64)bits128<2 * J>(sf) << 32)], 1u);
}
template <int... J>
__device__ __forceinline__ void hist8_word_fwd(std::integer_sequence<int, J...>, const u32 (&sf)[5], u32 invalid,
                                               const CoStrand& S, u32* lhist) {
    (hist8_window_fwd<J>(sf, invalid, S, lhist), ...);
}

template <int WIDE>
__global__ __launch_bounds__(P1_T) void k_hist8(const u64* __restrict__ codes, const u32* __restrict__ bad,
                                               u64 nwords, u32* __restrict__ partial8, Geom g) {
    __shared__ u32 lhist[256];
    if (threadIdx.x < 256) lhist[threadIdx.x] = 0;
    __syncthreads();
    u64 wpw = (nwords + NWG - 1) / NWG;
    u64 w0 = (u64)blockIdx.x * wpw;
    u64 w1 = w0 + wpw < nwords ? w0 + wpw : nwords;
    const bool cheap = g.L >= 8;
    for (u64 w = w0 + threadIdx.x; w < w1; w += P1_T) {
        u32 b0 = bad[w], b1 = bad[w + 1];
        if (b0 == 0xFFFFFFFFu) continue;
        u64 c0 = codes[w], c1 = codes[w + 1];
        if (WIDE == 3) {
            const CoStrand S = cs_make(g.L, g.R);
            const u32 sf[5] = {(u32)(c0 >> 32), (u32)c0, (u32)(c1 >> 32), (u32)c1, 0u};
            hist8_word_fwd(std::make_integer_sequence<int, 32>{}, sf, word_invalid(b0, b1, g.k), S, lhist);
            continue;
        }
        if (WIDE == 2) {
#pragma unroll 4
            for (int j = 0; j < 32; j++) {
                u64 k1;
                if (window_key_single(c0, c1, b0, b1, j, g, k1) && slice_key(k1, g))
                    atomicAdd(&lhist[(u32)(k1 >> 56)], 1u);
            }
            continue;
        }
        if (cheap) {
            u32 sf[5], rv[5];
            word_revstring(c0, c1, g.k, sf, rv);
            hist8_word(std::make_integer_sequence<int, 32>{}, sf, rv, word_invalid(b0, b1, g.k), g, lhist);
        } else {
#pragma unroll 4
            for (int j = 0; j < 32; j++) {
                u64 kf, kr;
                if (!window_keys(c0, c1, b0, b1, j, g, kf, kr)) continue;
                if (slice_key(kf, g)) atomicAdd(&lhist[(u32)(kf >> 56)], 1u);
                if (slice_key(kr, g)) atomicAdd(&lhist[(u32)(kr >> 56)], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) partial8[P8(blockIdx.x, threadIdx.x)] = lhist[threadIdx.x];
}

// the same histogram for WIDE windows (wide_keys<WM>, k_keys.inc): a lane per window start, consecutive lanes =
// consecutive starts (the composite keys a wave leaves in the per-window cache are then one contiguous kilobyte,
// and the dictionary look-ups of 64 windows are in flight together)
#ifndef H8W_PPT
#define H8W_PPT 4           // positions a thread looks up per tile of k_hist8w's canonical form (independent chains in flight)
#endif
#define H8W_HALO 512        // k - flank length up to which k_hist8w shares its canonical look-ups through LDS (< H8W_PPT x P1_T)
template <int WM>
__global__ __launch_bounds__(P1_T) void k_hist8w(const u64* __restrict__ codes, const u32* __restrict__ bad,
                                                u64 nwords, u32* __restrict__ partial8, Geom g) {
    __shared__ u32 lhist[256];
    __shared__ u32 lcount;
    if (threadIdx.x < 256) lhist[threadIdx.x] = 0;
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    const u64 wpw = (nwords + NWG - 1) / NWG;
    const u64 w0 = (u64)blockIdx.x * wpw;
    const u64 w1 = w0 + wpw < nwords ? w0 + wpw : nwords;
    if (WM == 2 && g.wshare && g.wfl[0].np == 1 && g.wfl[0].d[0].canon && g.wk - g.wfl[0].len <= H8W_HALO) {
        // Round 6 (VERDICT r5 item 3): composite keys through a CANONICAL flank dictionary.  A window needs the id of its
        // left flank (the len bases at pos) and the id of the reverse complement of its last len bases (at pos + halo); one
        // look-up of the canonical form of the len bases at p yields BOTH ids of position p (canon_ids), so a tile of P1_T
        // window starts makes P1_T + halo look-ups -- each shared through LDS by the window that starts at p and the window
        // that ends there -- instead of 2 P1_T (configs[2], 32/60/32: 604 random sectors per 512 windows instead of 1024).
        // A tile = H8W_PPT x P1_T positions, one look-up each, H8W_PPT of them per thread and independent of each other (the
        // look-up is a chain of dependent reads -- bucket bounds, two or three probes -- and the kernel is bound by how many
        // such chains are in flight, not by their bytes: first form of this code, one position per thread and the halo's
        // look-ups on top, ran no faster than two look-ups per window); the tile's first H8W_PPT x P1_T - halo window
        // starts are composed from it, the next tile starts there.
        __shared__ u32 sF[H8W_PPT * P1_T], sR[H8W_PPT * P1_T];
        const FlankRank& F = g.wfl[0];
        const int len = F.len, halo = g.wk - len;
        const u32 tid = threadIdx.x;
        const u32 TP = H8W_PPT * P1_T, TW = TP - (u32)halo;          // positions looked up / windows composed per tile
        for (u64 base = w0 * 32; base < w1 * 32; base += TW) {
            u32 idf[H8W_PPT], idr[H8W_PPT];
#pragma unroll
            for (int q = 0; q < H8W_PPT; q++) {
                const u64 p = base + tid + q * P1_T;
                idf[q] = idr[q] = ~0u;
                // (past the genome's last word come PAD_WORDS all-bad words: no look-up there)
                if ((p >> 5) < nwords && range_valid(bad, p, len) && !canon_ids(codes, p + g.woff[0], len, F.d[0], idf[q], idr[q]))
                    idf[q] = idr[q] = ~0u;
            }
#pragma unroll
            for (int q = 0; q < H8W_PPT; q++) {
                sF[tid + q * P1_T] = idf[q];
                sR[tid + q * P1_T] = idr[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < H8W_PPT; q++) {
                const u32 t = tid + q * P1_T;
                const u64 pos = base + t;
                if (t < TW && pos < w1 * 32) {
                    const u32 a = sF[t], b = sR[t + halo];
                    u64 kf = ~0ull, kr = 0;
                    const bool ok = a != ~0u && b != ~0u && range_valid(bad, pos, g.wk);
                    if (ok) {
                        kf = ((u64)min(a, b) << g.wshL) | ((u64)max(a, b) << g.wshR);
                        kr = (a > b ? 1ull : 0ull) | (a == b ? 2ull : 0ull);
                    }
                    if (g.wcmode == 1) {
                        ulonglong2 v;
                        v.x = kf;
                        v.y = kr;
                        *reinterpret_cast<ulonglong2*>(g.wcache + 2 * pos) = v;
                    } else if (g.wcmode == 3 && ok) {
                        // (the key list, Geom.wlcnt: this workgroup's segment)
                        const u32 at = atomicAdd(&lcount, 1u);
                        if (at < g.wlcap) {
                            ulonglong2 v;
                            v.x = kf;
                            v.y = (pos << 2) | kr;
                            *reinterpret_cast<ulonglong2*>(g.wcache + 2 * ((u64)blockIdx.x * g.wlcap + at)) = v;
                        }
                    }
                    if (ok && slice_key(kf, g)) atomicAdd(&lhist[(u32)(kf >> 56)], 1u);
                }
            }
            __syncthreads();
        }
        __syncthreads();
        if (threadIdx.x < 256) partial8[P8(blockIdx.x, threadIdx.x)] = lhist[threadIdx.x];
        if (threadIdx.x == 0 && g.wcmode == 3) g.wlcnt[blockIdx.x] = lcount;
        return;
    }
    for (u64 pos = w0 * 32 + threadIdx.x; pos < w1 * 32; pos += P1_T) {
        if (bad[pos >> 5] == 0xFFFFFFFFu) continue;
        u64 kf, kr;
        const u32 m = wide_keys<WM>(codes, bad, pos, g, kf, kr);
        if ((m & 1) && slice_key(kf, g)) atomicAdd(&lhist[(u32)(kf >> 56)], 1u);
        if ((m & 2) && slice_key(kr, g)) atomicAdd(&lhist[(u32)(kr >> 56)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256) partial8[P8(blockIdx.x, threadIdx.x)] = lhist[threadIdx.x];
}

// ----------------------------------------------------------------------------
// block-wide exclusive scan helper (blockDim.x <= 1024, multiple of 64)
// ----------------------------------------------------------------------------
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* lds_waves /* >= 17 u32 */, u32& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const u32 x = wave_incl_scan(v);
    if (lane == 63) lds_waves[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int i = 0; i < nw; i++) { u32 t = lds_waves[i]; lds_waves[i] = run; run += t; }
        lds_waves[16] = run;
    }
    __syncthreads();
    u32 res = lds_waves[wave] + x - v;
    total = lds_waves[16];
    __syncthreads();
    return res;
}

// ----------------------------------------------------------------------------
// K2b  (single workgroup, 256 threads) thread d walks column d of partial8[NWG][256]:
// in place exclusive prefix over the workgroups (= that workgroup's private pass-1
// cursor offset inside bucket d), then a scan over d gives the bucket bases.
// ----------------------------------------------------------------------------
// (a) one workgroup per top-byte column d: exclusive prefix over the NWG persistent
//     workgroups, in place (= each workgroup's private pass-1 cursor offset), column total out
__global__ __launch_bounds__(256) void k_reduce8a(u32* __restrict__ partial8, u32* __restrict__ tot) {
    __shared__ u32 waves[17];
    const u32 d = blockIdx.x;
    constexpr u32 PER = NWG / 256;
    static_assert(PER % 4 == 0, "k_reduce8a reads 16 bytes at a time");
    uint4* col = reinterpret_cast<uint4*>(partial8 + P8(threadIdx.x * PER, d));      // (column-major: PER consecutive words)
    u32 v[PER];
    u32 sum = 0;
#pragma unroll
    for (u32 q = 0; q < PER / 4; q++) {
        const uint4 x = col[q];
        v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        sum += x.x + x.y + x.z + x.w;
    }
    u32 total;
    u32 ex = block_excl_scan(sum, waves, total);
#pragma unroll
    for (u32 q = 0; q < PER / 4; q++) {
        uint4 x;
        x.x = ex; ex += v[4 * q];
        x.y = ex; ex += v[4 * q + 1];
        x.z = ex; ex += v[4 * q + 2];
        x.w = ex; ex += v[4 * q + 3];
        col[q] = x;
    }
    if (threadIdx.x == 0) tot[d] = total;
}

// (b) bucket bases, the first pass-2 tile of every bucket and the tile table: tiledesc[t] = key range of tile t
//     (tiles of `tile` keys never straddle a pass-1 bucket), empty for the tiles past the last one (pass 2 launches
//     ntmax workgroups).  EVERY workgroup scans the 256 column totals for itself (two block scans in LDS, a microsecond)
//     and then takes 256 tiles, a binary search in LDS per thread; workgroup 0 also leaves the bases and first tiles
//     in memory for the kernels that follow.
//     (Round 3: one workgroup used to do all of this, 6000 descriptors from 1024 threads, 18 us; a version that made
//     the bases in the last workgroup of (a) paid a device-wide fence per workgroup, 25 us; pass 2 looking its
//     range up itself lost 5 % of its own time.)
// (offs != nullptr: the totals are the differences of 256 ascending offsets, the last bucket ending at `nlast` -- the
// pass-1 buckets of a key-space slice, whose offsets k_hist16_off made for the whole genome)
__global__ __launch_bounds__(256) void k_reduce8b(const u32* __restrict__ tot, u32* __restrict__ base1,
                                                  u32* __restrict__ tp, u32 tile, u32 ntmax, uint2* __restrict__ tiledesc,
                                                  const u32* __restrict__ offs, u32 nlast) {
    __shared__ u32 waves[17];
    __shared__ u32 s_b1[260], s_tp[260];
    const u32 colsum = offs ? (threadIdx.x == 255 ? nlast : offs[threadIdx.x + 1]) - offs[threadIdx.x] : tot[threadIdx.x];
    u32 btotal, ttotal;
    const u32 bex = block_excl_scan(colsum, waves, btotal);
    const u32 t0 = block_excl_scan(tile ? (colsum + tile - 1) / tile : 0u, waves, ttotal);
    s_b1[threadIdx.x] = bex;
    s_tp[threadIdx.x] = t0;
    if (threadIdx.x == 0) { s_b1[256] = btotal; s_tp[256] = ttotal; }
    if (blockIdx.x == 0) {
        base1[threadIdx.x] = bex;
        tp[threadIdx.x] = t0;
        if (threadIdx.x == 0) { base1[256] = btotal; tp[256] = ttotal; }
    }
    __syncthreads();
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntmax) return;
    uint2 d = make_uint2(0, 0);
    if (t < s_tp[256]) {
        u32 lo = 0, hi = 256;                            // largest d with tp[d] <= t (then tp[d + 1] > t)
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_tp[mid] <= t) lo = mid; else hi = mid;
        }
        const u32 s = s_b1[lo] + (t - s_tp[lo]) * tile;
        d = make_uint2(s, min(s_b1[lo + 1], s + tile));
    }
    tiledesc[t] = d;
}

// ----------------------------------------------------------------------------
// generic single-workgroup exclusive scan: out[0..n] (n+1 entries), out[n] = total
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_scan(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
    __shared__ u32 waves[17];
    // thread-contiguous slices of a multiple of 4 elements (in / out are 16-byte aligned)
    const u32 per = ((n + 1023) / 1024 + 3) & ~3u;
    const u32 s0 = threadIdx.x * per;
    const u32 s1 = s0 + per < n ? s0 + per : n;
    u32 s = 0;
    for (u32 i = s0; i < s1; i += 4) {
        if (i + 4 <= n) {
            uint4 v = *reinterpret_cast<const uint4*>(in + i);
            s += v.x + v.y + v.z + v.w;
        } else {
            for (u32 q = i; q < s1; q++) s += in[q];
        }
    }
    u32 total;
    u32 ex = block_excl_scan(s, waves, total);
    for (u32 i = s0; i < s1; i += 4) {
        if (i + 4 <= n) {
            uint4 v = *reinterpret_cast<const uint4*>(in + i);
            uint4 o;
            o.x = ex; ex += v.x;
            o.y = ex; ex += v.y;
            o.z = ex; ex += v.z;
            o.w = ex; ex += v.w;
            *reinterpret_cast<uint4*>(out + i) = o;
        } else {
            for (u32 q = i; q < s1; q++) { u32 v = in[q]; out[q] = ex; ex += v; }
        }
    }
    if (threadIdx.x == 0) out[n] = total;
}

// ----------------------------------------------------------------------------
// K3w  pass 1 of the WIDE path (windows longer than one key: the key generator reads the codes,
// the dictionaries and the composite-key cache from global memory, data-dependent loads inside
// the tile).  Partition by the top 8 bits, LDS-staged so that global stores are coalesced runs.
// Same word ranges as k_hist8, so the workgroup's private cursors (base1[d] + its column
// prefix) are exact: no global atomics.  Per tile of P1_WORDS code words: generate the keys, rank
// them per digit with LDS atomics, scan the 256 digit counts, stage the keys digit-sorted in LDS,
// copy the runs out.  (Packed windows: k_scatter1p, k_sort2.inc.)
// ----------------------------------------------------------------------------
// (WM = 2, composite keys through the dictionaries for eight window starts per thread with no cache to read them from --
// flanks of more than 32 bases only --, is compiled for 2 waves per SIMD: at 128 VGPRs it spills)
template <int WM>
__global__ __launch_bounds__(P1_T, WM == 2 ? 2 : P1_OCC) void k_scatter1w(const u64* __restrict__ codes, const u32* __restrict__ bad,
                                                            u64 nwords, const u32* __restrict__ base1,
                                                            const u64* __restrict__ base64,
                                                            const u32* __restrict__ rowoff, u64* __restrict__ dst, Geom g) {
    __shared__ __attribute__((aligned(16))) u64 stage[P1_STAGE];
    __shared__ u64 cur[256];      // (64 bit: the slice pre-partition of a >= 2 Gbp genome exceeds 2^32 keys)
    __shared__ u32 cnt[256];
    __shared__ u64 delta[256];
    __shared__ u32 waves[17];
    const u32 tid = threadIdx.x;
    if (tid < 256) cur[tid] = (base64 ? base64[tid] : (u64)base1[tid]) + rowoff[P8(blockIdx.x, tid)];
    u64 wpw = (nwords + NWG - 1) / NWG;
    u64 w0 = (u64)blockIdx.x * wpw;
    u64 w1 = w0 + wpw < nwords ? w0 + wpw : nwords;
    for (u64 wt = w0; wt < w1; wt += P1_WORDS) {
        u64 key[P1_KPT];
        u32 r[P1_KPT];
        u32 vm = 0;
        if (tid < 256) cnt[tid] = 0;
        // window starts of the tile: consecutive lanes take consecutive starts (coalesced reads of the
        // composite-key cache; the order of the keys inside a tile is free)
#pragma unroll
        for (int jj = 0; jj < P1_PPT; jj++) {
            const u64 pos = wt * 32 + (u64)jj * P1_T + tid;
            if (pos < w1 * 32 && bad[pos >> 5] != 0xFFFFFFFFu) {
                u64 kf, kr;
                const u32 m = wide_keys<WM>(codes, bad, pos, g, kf, kr);
                if ((m & 1) && slice_key(kf, g)) { key[2 * jj] = kf; vm |= 1u << (2 * jj); }
                if ((m & 2) && slice_key(kr, g)) { key[2 * jj + 1] = kr; vm |= 2u << (2 * jj); }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < P1_KPT; q++)
            if ((vm >> q) & 1) r[q] = atomicAdd(&cnt[(u32)(key[q] >> 56)], 1u);
        __syncthreads();
        u32 c = tid < 256 ? cnt[tid] : 0, total;
        u32 ex = block_excl_scan(c, waves, total);
        if (tid < 256) {
            cnt[tid] = ex;
            delta[tid] = cur[tid] - ex;
            cur[tid] += c;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < P1_KPT; q++)
            if ((vm >> q) & 1) stage[cnt[(u32)(key[q] >> 56)] + r[q]] = key[q];
        __syncthreads();
        for (u32 p = tid; p < total; p += P1_T) {
            u64 k2 = stage[p];
            dst[p + delta[(u32)(k2 >> 56)]] = k2;
        }
        __syncthreads();
    }
}

// K3l  the same pass over the key LIST of Geom.wlcnt (round 6): workgroup w takes the keys IT listed in k_hist8w -- its
// segment of wcache --, so its private cursors are the ones its counts made.  Tiles of P1_KPT keys per thread.
__global__ __launch_bounds__(P1_T, P1_OCC) void k_scatter1l(const u32* __restrict__ base1, const u64* __restrict__ base64,
                                                            const u32* __restrict__ rowoff, u64* __restrict__ dst, Geom g) {
    __shared__ __attribute__((aligned(16))) u64 stage[P1_STAGE];
    __shared__ u64 cur[256];
    __shared__ u32 cnt[256];
    __shared__ u64 delta[256];
    __shared__ u32 waves[17];
    const u32 tid = threadIdx.x;
    if (tid < 256) cur[tid] = (base64 ? base64[tid] : (u64)base1[tid]) + rowoff[P8(blockIdx.x, tid)];
    const u32 nseg = min(g.wlcnt[blockIdx.x], g.wlcap);
    const ulonglong2* __restrict__ seg = reinterpret_cast<const ulonglong2*>(g.wcache) + (u64)blockIdx.x * g.wlcap;
    for (u32 t0 = 0; t0 < nseg; t0 += P1_KPT * P1_T) {
        u64 key[P1_KPT];
        u32 r[P1_KPT];
        u32 vm = 0;
        if (tid < 256) cnt[tid] = 0;
#pragma unroll
        for (int q = 0; q < P1_KPT; q++) {
            const u32 i = t0 + (u32)q * P1_T + tid;
            if (i < nseg) {
                u64 k1 = seg[i].x;
                if (slice_key(k1, g)) { key[q] = k1; vm |= 1u << q; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < P1_KPT; q++)
            if ((vm >> q) & 1) r[q] = atomicAdd(&cnt[(u32)(key[q] >> 56)], 1u);
        __syncthreads();
        u32 c = tid < 256 ? cnt[tid] : 0, total;
        u32 ex = block_excl_scan(c, waves, total);
        if (tid < 256) {
            cnt[tid] = ex;
            delta[tid] = cur[tid] - ex;
            cur[tid] += c;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < P1_KPT; q++)
            if ((vm >> q) & 1) stage[cnt[(u32)(key[q] >> 56)] + r[q]] = key[q];
        __syncthreads();
        for (u32 p = tid; p < total; p += P1_T) {
            u64 k2 = stage[p];
            dst[p + delta[(u32)(k2 >> 56)]] = k2;
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------
// K3k  sliced genomes: "pass 0" partitions ALL keys of a genome once by their top byte
// (k_hist8 / k_scatter1 on absolute keys, 64-bit bucket bases from k_bases64) -- a slice is a
// run of 2^(8 - sbits) such buckets, i.e. one contiguous region -- and every slice then takes
// its pass 1 from that region instead of regenerating all windows of the genome:
// k_hist8k / k_scatter1kp (k_sort2.inc) = k_hist8 / k_scatter1p with keys read (and made relative)
// instead of generated.  Same workgroup ranges in both, so the private cursors stay exact.
// ----------------------------------------------------------------------------
__global__ void k_bases64(const u32* __restrict__ tot, u64* __restrict__ base64) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        u64 run = 0;
        for (int d = 0; d < 256; d++) { base64[d] = run; run += tot[d]; }
        base64[256] = run;
    }
}

// Round 4: a slice's pass 1 without a counting pass over its keys.  Pass 0 partitions by the slice alone (the top 2 sb
// bits); a slice's region is then split by the top byte of the RELATIVE key -- top 8 + 2 sb absolute bits in all,
// (slice, top byte) -- with k_scatter2 itself:
// the counts of those bins come from the codes, ONE k_hist16 launch per genome (<= 65536 bins: one partition), and a tile
// reserves its runs with an atomic per non-empty bin, as the unsliced route's pass 2 does.  (Round 3 read every slice
// once more just to count its top byte per workgroup, k_hist8k: 27 of configs[4]'s 267 ms.)
//   k_bases_rel      rel[q] = keys of the pass-0 buckets of q's slice in front of bucket q: the bucket's place inside the
//                    slice's pass-1 output, what k_hist16_off adds to the bins of bucket q
//   (a slice's region of the pass-0 array is ONE bucket whose tiles k_scatter2 cuts from its length; the totals of its 256
//   pass-1 buckets are differences of those offsets: k_reduce8b reads them there -- no table kernel per slice)
__global__ __launch_bounds__(256) void k_bases_rel(const u32* __restrict__ tot, u32 per, u32* __restrict__ rel) {
    const u32 q = threadIdx.x;
    u32 sum = 0;
    for (u32 j = q - q % per; j < q; j++) sum += tot[j];
    rel[q] = sum;
    if (q == 0) rel[256] = 0;
}
#define P1K_TILE (P1_T * P1_KPT)      // keys per tile of the from-keys kernels (= P1_STAGE)

__global__ __launch_bounds__(P1_T) void k_hist8k(const u64* __restrict__ src, u64 n, int sbits,
                                                u32* __restrict__ partial8) {
    __shared__ u32 lhist[256];
    if (threadIdx.x < 256) lhist[threadIdx.x] = 0;
    __syncthreads();
    const u64 per = ((n + NWG - 1) / NWG + P1K_TILE - 1) / P1K_TILE * P1K_TILE;
    const u64 k0 = (u64)blockIdx.x * per;
    const u64 k1 = k0 + per < n ? k0 + per : n;
    if (k0 < k1) {
        // 4 x 16-byte buffer loads in flight per lane (8 keys); lanes past the range read 0 and are not counted
        const u32 nk = (u32)(k1 - k0);
        const bufrsrc rs = make_rsrc(src + k0, nk * 8);
        for (u32 base = 0; base < nk; base += 8 * P1_T) {
            u32x4 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (base + q * 2 * P1_T + 2 * threadIdx.x) * 8, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32 i = base + q * 2 * P1_T + 2 * threadIdx.x;
                if (i < nk) atomicAdd(&lhist[(u32)((pair_lo(v[q]) << sbits) >> 56)], 1u);
                if (i + 1 < nk) atomicAdd(&lhist[(u32)((pair_hi(v[q]) << sbits) >> 56)], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 256) partial8[P8(blockIdx.x, threadIdx.x)] = lhist[threadIdx.x];
}

// ----------------------------------------------------------------------------
// K3h  the FINE bucket histogram (top b bits of every key) straight from the codes: the top
// bits of both strands' keys come from the first / last bases of the window without building
// the key (valid when they lie inside `left`: 2 L >= b), so pass 2 needs no histogram pass
// over the pass-1 output (k_hist2 reads 8 bytes per key; this reads 0.19 bytes per key per
// partition).  One workgroup per (word range, partition of 32768 bins): 128 KB of LDS counters.
//   k_hist16        partial16[range][2^b]
//   k_hist16_sum    hist16[2^b] = sum over the ranges      (then k_scan -> off[])
// ----------------------------------------------------------------------------
#define H16_BINS 65536u      // bins of one partition: 16-bit counters, two per LDS word (128 KB)
#define H16_T 1024
#define H16_EXC_CAP 8192u    // (range, bin) pairs with >= 65536 keys: at most N / 65536 <= 2^29 / 2^16 of them exist

// Round 3: the counters are 16 bits wide, so ONE partition holds 65536 bins and a workgroup decodes every window
// of its range once where it used to decode it once per 32768 bins (fan-out 2^16: twice; the kernel is bound by
// that decoding, ~20 vector instructions per window and strand).  16 bits are enough unless one bin of one range
// collects 65536 keys (a satellite); the workgroup knows a bound before it starts -- its range is H16_SUB ranges of
// k_hist8, whose per-range counts by top byte are in memory (prefix-summed by k_reduce8a) -- and a range over
// that bound counts with 32-bit counters in two passes over half the bins, as before.  Partial counts leave as
// 16 bits + a list of the rare (range, bin, high part) exceptions.
// FAST = one partition, 16-bit counters, every bin in range (fan-out <= 2^16 and no crowded range: the usual case):
// no test per key.  rv = the reverse complement of the whole word string, shifted so that the reverse key of window
// J starts at bit 62 - 2 J: one funnel shift per window instead of complement + bit reversal + pair swap.
template <int J, bool FAST>
__device__ __forceinline__ void hist16_window(const u32 (&sf)[5], const u32 (&rv)[5], u32 invalid, int nb,
                                              int pbits, u32 part, u32 lo, u32 nbp, u32 pk, u32* h) {
    if ((invalid >> (31 - J)) & 1u) return;
    const u32 tf = bits128<2 * J>(sf) >> (32 - nb);                 // top nb bits of the forward key
    const u32 tr = bits128<62 - 2 * J>(rv) >> (32 - nb);            // top nb bits of the reverse key
    if (FAST) {
        atomicAdd(&h[tf >> 1], 1u << ((tf & 1u) << 4));
        atomicAdd(&h[tr >> 1], 1u << ((tr & 1u) << 4));
        return;
    }
    // (pk = 1: two 16-bit counters per word; pk = 0: one 32-bit counter)
    const u32 xf = (tf & (H16_BINS - 1)) - lo, xr = (tr & (H16_BINS - 1)) - lo;
    if ((pbits ? tf >> 16 : 0u) == part && xf < nbp) atomicAdd(&h[xf >> pk], 1u << ((xf & pk) << 4));
    if ((pbits ? tr >> 16 : 0u) == part && xr < nbp) atomicAdd(&h[xr >> pk], 1u << ((xr & pk) << 4));
}

template <bool FAST, int... J>
__device__ __forceinline__ void hist16_word(std::integer_sequence<int, J...>, const u32 (&sf)[5], const u32 (&rv)[5],
                                            u32 invalid, int nb, int pbits, u32 part, u32 lo, u32 nbp, u32 pk, u32* h) {
    (hist16_window<J, FAST>(sf, rv, invalid, nb, pbits, part, lo, nbp, pk, h), ...);
}

// colpre = k_hist8's per-range counts by top byte, prefix-summed over the ranges by k_reduce8a; coltot = the column totals
__global__ __launch_bounds__(H16_T) void k_hist16(const u64* __restrict__ codes, const u32* __restrict__ bad,
                                                 u64 nwords, const u32* __restrict__ colpre, const u32* __restrict__ coltot,
                                                 unsigned short* __restrict__ partial16, u32* __restrict__ exc, int k, int nb) {
    __shared__ u32 h[H16_BINS / 2];
    __shared__ u32 s_max;
    const u32 tid = threadIdx.x;
    const u32 nbins = 1u << nb;
    const u32 pbins = nbins < H16_BINS ? nbins : H16_BINS;     // bins of this partition
    const u32 part = blockIdx.y;                               // partition = value of the bits above the low 16
    const int pbits = nb > 16 ? nb - 16 : 0;
    // this workgroup's words = H16_SUB word ranges of k_hist8 (same arithmetic there and in k_scatter1p)
    const u32 sub = NWG / gridDim.x;
    const u64 wpw = (nwords + NWG - 1) / NWG;
    const u64 w0 = (u64)blockIdx.x * sub * wpw;
    const u64 w1 = w0 + sub * wpw < nwords ? w0 + sub * wpw : nwords;
    if (tid == 0) s_max = 0;
    __syncthreads();
    if (tid < 256) {
        const u32 r0 = blockIdx.x * sub, r1 = r0 + sub;
        const u32 a = colpre[P8(r0, tid)], b2 = r1 < NWG ? colpre[P8(r1, tid)] : coltot[tid];
        atomicMax(&s_max, b2 - a);
    }
    __syncthreads();
    const u32 pk = s_max <= 65535u ? 1u : 0u;                  // no bin of this range can pass 65535: 16-bit counters
    const u32 npass = (pk || pbins <= H16_BINS / 2) ? 1u : 2u;
    const u32 nbp = pbins / npass;
    const bool fast = pk && pbits == 0;
    for (u32 pass = 0; pass < npass; pass++) {
        const u32 lo = pass * nbp;
        for (u32 i = tid; i < H16_BINS / 2; i += H16_T) h[i] = 0;
        __syncthreads();
        for (u64 w = w0 + tid; w < w1; w += H16_T) {
            const u32 b0 = bad[w], b1 = bad[w + 1];
            if (b0 == 0xFFFFFFFFu) continue;
            const u64 c0 = codes[w], c1 = codes[w + 1];
            const u32 invalid = word_invalid(b0, b1, k);
            u32 sf[5], rv[5];
            word_revstring(c0, c1, k, sf, rv);
            if (fast) hist16_word<true>(std::make_integer_sequence<int, 32>{}, sf, rv, invalid, nb, pbits, part, lo, nbp, pk, h);
            else hist16_word<false>(std::make_integer_sequence<int, 32>{}, sf, rv, invalid, nb, pbits, part, lo, nbp, pk, h);
        }
        __syncthreads();
        unsigned short* out = partial16 + (u64)blockIdx.x * nbins + (u64)part * H16_BINS + lo;
        for (u32 i = tid; i < nbp; i += H16_T) {
            const u32 v = pk ? ((h[i >> 1] >> ((i & 1u) << 4)) & 0xFFFFu) : h[i];
            out[i] = (unsigned short)v;
            if (v > 0xFFFFu) {
                const u32 e = atomicAdd(&exc[0], 1u);
                if (e < H16_EXC_CAP) { exc[1 + 3 * e] = blockIdx.x; exc[2 + 3 * e] = part * H16_BINS + lo + i; exc[3 + 3 * e] = v >> 16; }
            }
        }
        __syncthreads();
    }
}

// one workgroup per pass-1 bucket d: sum over the ranges, scan inside the bucket, add the bucket base of
// k_reduce8b -> off[].  1024 threads = (pairs of adjacent bins, read as one 32-bit word) x (groups of ranges): every
// thread sums its group's ranges for its pair, the groups meet in LDS.
__global__ __launch_bounds__(1024) void k_hist16_off(const unsigned short* __restrict__ partial16, u32 nranges, int b,
                                                    const u32* __restrict__ exc, const u32* __restrict__ base1,
                                                    u32* __restrict__ off, u32* __restrict__ cursor) {
    __shared__ u32 waves[17];
    __shared__ u32 acc[1024];
    const u32 nb2 = 1u << (b - 8), nbins = 1u << b;
    const u32 d1 = blockIdx.x, tid = threadIdx.x;
    for (u32 i = tid; i < nb2; i += 1024) acc[i] = 0;
    __syncthreads();
    const u32 npair = nb2 / 2;                       // (b >= 9: nb2 >= 2)
    const u32 ngrp = 1024 / npair < nranges ? 1024 / npair : nranges;
    const u32 pr = tid % npair, grp = tid / npair;
    if (grp < ngrp) {
        const u32* row = reinterpret_cast<const u32*>(partial16) + (d1 * nb2) / 2 + pr;      // (4-byte aligned: nb2 is even)
        u32 lo = 0, hi = 0;
        for (u32 r = grp; r < nranges; r += ngrp) {
            const u32 v = row[(u64)r * (nbins / 2)];
            lo += v & 0xFFFFu;
            hi += v >> 16;
        }
        atomicAdd(&acc[2 * pr], lo);
        atomicAdd(&acc[2 * pr + 1], hi);
    }
    __syncthreads();
    const u32 bin = tid;
    u32 sum = 0;
    if (bin < nb2) {
        const u32 fine = d1 * nb2 + bin;
        sum = acc[bin];
        const u32 ne = min(exc[0], H16_EXC_CAP);                // (counts beyond 16 bits: rare, listed)
        for (u32 e = 0; e < ne; e++)
            if (exc[2 + 3 * e] == fine) sum += exc[3 + 3 * e] << 16;
    }
    u32 total;
    const u32 ex = block_excl_scan(sum, waves, total);
    if (bin < nb2) {
        off[d1 * nb2 + bin] = base1[d1] + ex;
        cursor[d1 * nb2 + bin] = base1[d1] + ex;         // pass 2 reserves its runs from here
    }
    if (d1 == 255 && bin == 0) off[nbins] = base1[256];
}

// ----------------------------------------------------------------------------
// K4  pass 2 = segmented partition of the pass-1 buckets by the next b-8 bits, in
// tiles of P2_TILE keys that never straddle a bucket (tp / tiledesc from k_reduce8b):
//   k_hist2    per-tile digit counts (LDS histogram)           -> tilehist[tile][bin]
//   k_scan2    per bucket: bin totals -> fine offsets off[], per-tile bin bases (in place)
//   k_scatter2 per tile: rank, scan, stage digit-sorted in LDS, coalesced runs out
// No global atomics, any number of workgroups per CU.
// ----------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_hist2(const u64* __restrict__ src, const uint2* __restrict__ tiledesc,
                                               u32* __restrict__ tilehist, int b) {
    __shared__ u32 h[1024];
    const u32 tile = blockIdx.x;
    const uint2 td = tiledesc[tile];
    const u32 s = td.x, e = td.y;
    if (s >= e) return;
    const u32 nb2 = 1u << (b - 8);
    const int rb = 64 - b;
    for (u32 i = threadIdx.x; i < nb2; i += T) h[i] = 0;
    __syncthreads();
    u64 key[P2_KPT];
    {   // (two keys per lane and load, as k_scatter2 reads them)
        const bufrsrc rs = make_rsrc(src + s, (e - s) * 8);
#pragma unroll
        for (int q = 0; q < (int)P2_KPT / 2; q++) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (2 * q * T + 2 * threadIdx.x) * 8, 0, 0);
            key[2 * q] = pair_lo(v);
            key[2 * q + 1] = pair_hi(v);
        }
    }
#pragma unroll
    for (int q = 0; q < (int)P2_KPT; q++) {
        u32 i = s + (q >> 1) * 2 * T + 2 * threadIdx.x + (q & 1);
        if (i < e) atomicAdd(&h[(u32)(key[q] >> rb) & (nb2 - 1)], 1u);
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < nb2; i += T) tilehist[(u64)tile * nb2 + i] = h[i];
}

__global__ __launch_bounds__(1024) void k_scan2(u32* __restrict__ tilehist, const u32* __restrict__ base1,
                                                const u32* __restrict__ tp, u32* __restrict__ off, int b) {
    __shared__ u32 waves[17];
    const u32 nb2 = 1u << (b - 8);
    const u32 d1 = blockIdx.x, bin = threadIdx.x;
    const u32 t0 = tp[d1], t1 = tp[d1 + 1];
    u32 tot = 0;
    if (bin < nb2) {
        u32 t = t0;
        for (; t + 8 <= t1; t += 8) {
            u32 v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = tilehist[(u64)(t + q) * nb2 + bin];
#pragma unroll
            for (int q = 0; q < 8; q++) tot += v[q];
        }
        for (; t < t1; t++) tot += tilehist[(u64)t * nb2 + bin];
    }
    u32 total;
    u32 ex = block_excl_scan(tot, waves, total);
    u32 run = base1[d1] + ex;
    if (bin < nb2) {
        off[d1 * nb2 + bin] = run;
        u32 t = t0;
        for (; t + 8 <= t1; t += 8) {
            u32 v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = tilehist[(u64)(t + q) * nb2 + bin];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                tilehist[(u64)(t + q) * nb2 + bin] = run;
                run += v[q];
            }
        }
        for (; t < t1; t++) {
            u32 v = tilehist[(u64)t * nb2 + bin];
            tilehist[(u64)t * nb2 + bin] = run;
            run += v;
        }
    }
    if (d1 == 255 && bin == 0) off[256u * nb2] = base1[256];
}

// `cursor` != nullptr: the fine offsets are known up front (k_hist16) and a tile reserves its
// place in every fine bucket with one global atomic per non-empty bin (the order of the tiles
// inside a fine bucket is free: k_localsort sorts it); else the per-tile bases of k_scan2.
// shl > 0 (pass 1 of a key-space slice, straight from the slice's region of the pass-0 array): the keys are made relative
// on the way (key << shl) and partitioned by their top byte; the bins of slice s are cursor[s << 8 ...].
#ifndef P2_ABL
#define P2_ABL 0            // tools/p2bench.hip only (timing of the kernel's parts, results wrong): 1 no global stores, 2 no ranking
#endif                      // atomics, 4 no staging writes, 8 no loads
static_assert(!(P2_ABL & (2 | 4 | 8)) || (P2_ABL & 1), "a part that decides the keys' places is only taken out together with the global stores");
template <int T>
__global__ __launch_bounds__(T) void k_scatter2(const u64* __restrict__ src, u64* __restrict__ dst,
                                                   const uint2* __restrict__ tiledesc,
                                                   const u32* __restrict__ tilehist, u32* __restrict__ cursor, int b, int shl,
                                                   u32 region_n) {
    __shared__ __attribute__((aligned(16))) u64 stage[T * P2_KPT];
    __shared__ u32 cnt[1024 + 2];
    __shared__ u32 delta[1024 + 2];
    __shared__ u32 waves[17];
    // tiles are walked from the last to the first: k_hist2 has just streamed the same keys in
    // ascending order, so its tail is what the 256 MiB Infinity Cache still holds; and the
    // fine buckets written last (low ones) are the ones k_localsort reads first
#ifndef P2_NO_XCD
    // workgroups b and b + 8 share an XCD (round-robin placement, speed only): give every XCD one contiguous
    // eighth of the tiles, so that the runs that meet in a 128-byte line come from ONE L2 (k_scatter2 -3.5 %, A/B in
    // one box; the same remap of pass 1's window ranges showed nothing beyond the run-to-run spread)
    const u32 G8 = gridDim.x, q8 = G8 / 8, r8 = G8 % 8, x8 = blockIdx.x % 8, i8 = blockIdx.x / 8;
    const u32 lin = (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + i8;
    const u32 tile = G8 - 1 - lin;
#else
    const u32 tile = gridDim.x - 1 - blockIdx.x;
#endif
    // (slice mode: the region is ONE bucket, its tiles are cut from its length: no table)
    const uint2 td = shl ? make_uint2(min(tile * (u32)(T * P2_KPT), region_n), min((tile + 1) * (u32)(T * P2_KPT), region_n))
                         : tiledesc[tile];
    const u32 s = td.x, e = td.y;
    if (s >= e) return;
    const u32 tid = threadIdx.x;
    // (shl: the whole tile lies in one slice, whose 256 bins -- the top byte of the relative key -- start at slice << 8)
    const u32 nb2 = shl ? 256u : 1u << (b - 8);
    const int rb = shl ? 56 : 64 - b;
    u64 key[P2_KPT];
    u32 r[P2_KPT];
    // two keys per lane and load (16 bytes; the descriptor's range check zeroes the lanes past the tile):
    // element 2 q + h of a thread is key s + 2 q T + 2 tid + h
    {
        const bufrsrc rs = make_rsrc(src + s, (e - s) * 8);
#pragma unroll
        for (int q = 0; q < (int)P2_KPT / 2; q++) {
            u32x4 v;
            if (P2_ABL & 8) { v.x = tid * 2654435761u + q; v.y = (tid ^ (q * 40503u)) * 2246822519u; v.z = v.x * 3u; v.w = v.y + 77u * q; }
            else v = __builtin_amdgcn_raw_buffer_load_b128(rs, (2 * q * T + 2 * tid) * 8, 0, KR_P2_LD_AUX);
            key[2 * q] = pair_lo(v) << shl;
            key[2 * q + 1] = pair_hi(v) << shl;
        }
    }
#define P2_IDX(q) (s + ((q) >> 1) * 2 * T + 2 * tid + ((q) & 1))
    // this thread scans the 1024 / T bins [BPT tid, BPT tid + BPT) (nb2 <= 1024); with one bin per
    // thread the second one is a dummy past the table
    constexpr u32 BPT = 1024 / T;
    const u32 bin0 = BPT * tid, bin1 = BPT == 2 ? 2 * tid + 1 : 1024 + (tid & 1);
    u32 tb0 = 0, tb1 = 0;
    if (!cursor) {
        tb0 = bin0 < nb2 ? tilehist[(u64)tile * nb2 + bin0] : 0;
        tb1 = (BPT == 2 && bin1 < nb2) ? tilehist[(u64)tile * nb2 + bin1] : 0;
    }
    cnt[bin0] = 0;
    cnt[bin1] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (int)P2_KPT; q++) {
        u32 i = P2_IDX(q);
        if (P2_ABL & 2) r[q] = (u32)q;
        else if (i < e) r[q] = atomicAdd(&cnt[(u32)(key[q] >> rb) & (nb2 - 1)], 1u);
    }
    __syncthreads();
    u32 c0 = cnt[bin0], c1 = cnt[bin1], total;
    if (cursor && !(P2_ABL & 1)) {
        const u32 d1 = shl ? (u32)(src[s] >> (64 - shl)) : (u32)(src[s] >> 56);     // the tile's slice / pass-1 bucket
        if (c0) tb0 = atomicAdd(&cursor[d1 * nb2 + bin0], c0);
        if (BPT == 2 && c1) tb1 = atomicAdd(&cursor[d1 * nb2 + bin1], c1);
    }
    u32 ex = block_excl_scan(c0 + c1, waves, total);
    cnt[bin0] = ex;
    cnt[bin1] = ex + c0;
    delta[bin0] = tb0 - ex;
    delta[bin1] = tb1 - (ex + c0);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (int)P2_KPT; q++) {
        u32 i = P2_IDX(q);
        if (P2_ABL & 4) asm volatile("" ::"v"(key[q]), "v"(r[q]));
        else if (i < e) stage[(cnt[(u32)(key[q] >> rb) & (nb2 - 1)] + r[q]) & (P2_ABL ? T * P2_KPT - 1 : ~0u)] = key[q];
    }
#undef P2_IDX
    __syncthreads();
    const u32 nt = e - s;
#pragma unroll
    for (int q = 0; q < (int)P2_KPT; q++) {
        u32 p = q * T + tid;
        if (p < nt) {
            u64 k2 = stage[p];
            if (P2_ABL & 1) asm volatile("" ::"v"(k2), "v"(delta[(u32)(k2 >> rb) & (nb2 - 1)]));
            else if (KR_P2_ST_NT) __builtin_nontemporal_store(k2, &dst[p + delta[(u32)(k2 >> rb) & (nb2 - 1)]]);
            else dst[p + delta[(u32)(k2 >> rb) & (nb2 - 1)]] = k2;
        }
    }
}

// ----------------------------------------------------------------------------
// K4b  chunk table of the LDS sort and of the intersection: chunk j = the fine buckets whose
// start offset lies in [j T, (j + 1) T), one 16-byte descriptor {first key, end key, first
// bucket, end bucket} per chunk (all zero for an empty chunk).  One thread per chunk: two binary
// searches in off[0 .. nb] (first bucket whose start is >= j T; off[nb] = the key count).  Also
// clears the oversized-bucket counter of the sort that follows.  (One launch; it used to be a
// fill, a kernel over the buckets, a kernel over the chunks and a second fill.)
// ----------------------------------------------------------------------------
__device__ __forceinline__ u32 first_bucket_from(const u32* __restrict__ off, u32 nb, u64 v) {
    u32 l = 0, r = nb + 1;                     // smallest f in [0, nb] with off[f] >= v, nb when there is none
    while (l < r) {
        const u32 mid = l + ((r - l) >> 1);
        if ((u64)off[mid] < v) l = mid + 1; else r = mid;
    }
    return l < nb ? l : nb;
}

__global__ void k_chunk_table(const u32* __restrict__ off, u32 nb, u32 nchunks, uint4* __restrict__ desc,
                              u32* __restrict__ ovf_count, u32* __restrict__ h16_exc) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0 && ovf_count) { ovf_count[0] = 0; ovf_count[1] = 0; ovf_count[2] = 0; ovf_count[3] = 0; }
    if (j == 0 && h16_exc) h16_exc[0] = 0;             // (k_hist16's exception list: read by k_hist16_off before this launch)
    if (j >= nchunks) return;
    const u32 lo = first_bucket_from(off, nb, (u64)j * LS_T);
    const u32 hi = first_bucket_from(off, nb, (u64)(j + 1) * LS_T);
    uint4 d = make_uint4(0, 0, 0, 0);
    if (lo < hi) d = make_uint4(off[lo], off[hi], lo, hi);
    desc[j] = d;
}

// ----------------------------------------------------------------------------
// Ko  keys in STREAM order (kstream without --sort, kstream.py:327-405: the k-mers as the windows
// come, a window's reverse complement right after it): per tile of 2048 window starts the number of
// keys (k_order_count), a scan of the tile totals, then the keys written in order (k_order_emit).
// ----------------------------------------------------------------------------
__device__ __forceinline__ u32 order_keys(const u64* __restrict__ codes, const u32* __restrict__ bad, u64 pos, u64 npos,
                                          const Geom& g, u64& k0, u64& k1) {
    if (pos >= npos) return 0;
    const u64 w = pos >> 5;
    const int j = (int)(pos & 31);
    const u64 c0 = codes[w], c1 = codes[w + 1];
    const u32 b0 = bad[w], b1 = bad[w + 1];
    if (g.strands) return window_key_single(c0, c1, b0, b1, j, g, k0) ? 1u : 0u;
    return window_keys(c0, c1, b0, b1, j, g, k0, k1) ? 2u : 0u;
}

__global__ __launch_bounds__(256) void k_order_count(const u64* __restrict__ codes, const u32* __restrict__ bad, u64 npos,
                                                     Geom g, u32* __restrict__ tsum) {
    __shared__ u32 waves[17];
    u32 cnt = 0;
    for (int q = 0; q < 8; q++) {
        u64 k0, k1;
        cnt += order_keys(codes, bad, (u64)blockIdx.x * 2048 + threadIdx.x * 8 + q, npos, g, k0, k1);
    }
    u32 total;
    (void)block_excl_scan(cnt, waves, total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_order_emit(const u64* __restrict__ codes, const u32* __restrict__ bad, u64 npos,
                                                    Geom g, const u64* __restrict__ tpos, u64* __restrict__ out) {
    __shared__ u32 waves[17];
    // (count, scan, then generate again and store as the keys come: a private array filled at a running index
    // lives in scratch memory)
    u32 cnt = 0;
    for (int q = 0; q < 8; q++) {
        u64 k0 = 0, k1 = 0;
        cnt += order_keys(codes, bad, (u64)blockIdx.x * 2048 + threadIdx.x * 8 + q, npos, g, k0, k1);
    }
    u32 total;
    const u32 ex = block_excl_scan(cnt, waves, total);
    u64* o = out + tpos[blockIdx.x] + ex;
    for (int q = 0; q < 8; q++) {
        u64 k0 = 0, k1 = 0;
        const u32 m = order_keys(codes, bad, (u64)blockIdx.x * 2048 + threadIdx.x * 8 + q, npos, g, k0, k1);
        if (m >= 1) *o++ = k0;
        if (m == 2) *o++ = k1;
    }
}

// exclusive scan of u32 tile totals into u64 positions (one workgroup; the totals of a 3 Gbp genome fit)
__global__ __launch_bounds__(1024) void k_scan64(const u32* __restrict__ in, u64* __restrict__ out, u32 n) {
    __shared__ u64 part[1024];
    const u32 per = (n + 1023) / 1024;
    const u32 s0 = threadIdx.x * per, s1 = s0 + per < n ? s0 + per : n;
    u64 s = 0;
    for (u32 i = s0; i < s1; i++) s += in[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        for (int i = 0; i < 1024; i++) { const u64 t = part[i]; part[i] = run; run += t; }
        out[n] = run;
    }
    __syncthreads();
    u64 ex = part[threadIdx.x];
    for (u32 i = s0; i < s1; i++) { out[i] = ex; ex += in[i]; }
}

// property check for full-size runs: number of adjacent pairs out of order
__global__ void k_count_inversions(const u64* __restrict__ keys, u64 n, u64* __restrict__ out) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 stride = (u64)gridDim.x * blockDim.x;
    u32 bad = 0;
    for (; i + 1 < n; i += stride) bad += keys[i] > keys[i + 1];
    if (bad) atomicAdd(out, (u64)bad);
}

// fine bucket offsets of an already sorted key array: off[f] = lower_bound(f << rb)
__global__ void k_offsets_from_sorted(const u64* __restrict__ keys, u32 n, u32 nb, int rb, u32* __restrict__ off) {
    u32 f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > nb) return;
    if (f == nb) { off[f] = n; return; }
    const u64 target = (u64)f << rb;
    u32 l = 0, r = n;
    while (l < r) {
        u32 mid = l + ((r - l) >> 1);
        if (keys[mid] < target) l = mid + 1; else r = mid;
    }
    off[f] = l;
}

// (K5, the LDS sort of one chunk: k_localsort2 in k_sort2.inc.)  16-bit counter of sub-bin i:
__device__ __forceinline__ u32 cnt16_get(const u32* c, u32 i) {
    u32 w = c[i >> 1];
    return (i & 1) ? (w >> 16) : (w & 0xFFFFu);
}

// ----------------------------------------------------------------------------
// Kb  fallback for fine buckets that do not fit the LDS sort (poly-A, satellites, tandem
// repeats): their 4096-key tiles are sorted by k_localsort itself (descriptor list of
// tiles), then merged pairwise -- run length doubling each round -- by a merge-path kernel:
// one workgroup per 2048 output keys finds its two input ranges by binary search, stages
// them in LDS, every thread merges 8 outputs.  Source -> scratch, then copied back.
// segs[i] = {start, end, first global tile of the segment, 0}
// ----------------------------------------------------------------------------
#define MG_T 256
#define MG_VT 8
#define MG_TILE (MG_T * MG_VT)

__device__ __forceinline__ u32 merge_path(const u64* A, u32 na, const u64* B, u32 nb, u32 diag) {
    u32 lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi) {
        u32 mid = (lo + hi) >> 1;
        if (A[mid] <= B[diag - mid - 1]) lo = mid + 1; else hi = mid;
    }
    return lo;      // number of A elements among the first `diag` merged (ties: A first)
}

__global__ __launch_bounds__(MG_T) void k_seg_merge(const u64* __restrict__ src, u64* __restrict__ dst,
                                                    const uint4* __restrict__ segs, u32 nseg, u32 run) {
    __shared__ __attribute__((aligned(16))) u64 L[MG_TILE];
    __shared__ u32 sh[4];
    const u32 tile = blockIdx.x;
    u32 lo = 0, hi = nseg;                      // last segment whose first tile is <= tile
    while (hi - lo > 1) {
        u32 mid = (lo + hi) >> 1;
        if (segs[mid].z <= tile) lo = mid; else hi = mid;
    }
    const uint4 sg = segs[lo];
    const u32 len = sg.y - sg.x;
    const u32 o0 = (tile - sg.z) * MG_TILE;
    if (o0 >= len) return;
    const u32 o1 = min(o0 + MG_TILE, len);
    const u32 base = (o0 / (2 * run)) * (2 * run);
    const u32 amid = min(base + run, len), bend = min(base + 2 * run, len);
    const u64* A = src + sg.x + base;
    const u64* B = src + sg.x + amid;
    const u32 na = amid - base, nb = bend - amid;
    if (threadIdx.x == 0) {
        sh[0] = merge_path(A, na, B, nb, o0 - base);
        sh[1] = merge_path(A, na, B, nb, o1 - base);
    }
    __syncthreads();
    const u32 a0 = sh[0], a1 = sh[1];
    const u32 b0 = (o0 - base) - a0, b1 = (o1 - base) - a1;
    const u32 ca = a1 - a0, cb = b1 - b0;
    for (u32 i = threadIdx.x; i < ca; i += MG_T) L[i] = A[a0 + i];
    for (u32 i = threadIdx.x; i < cb; i += MG_T) L[ca + i] = B[b0 + i];
    __syncthreads();
    const u64* LA = L;
    const u64* LB = L + ca;
    const u32 total = ca + cb;
    const u32 d = min(threadIdx.x * MG_VT, total);
    u32 ia = merge_path(LA, ca, LB, cb, d);
    u32 ib = d - ia;
    u64* out = dst + sg.x + o0;
#pragma unroll
    for (int q = 0; q < MG_VT; q++) {
        u32 o = d + q;
        if (o < total) {
            bool takeA = ib >= cb || (ia < ca && LA[ia] <= LB[ib]);
            out[o] = takeA ? LA[ia] : LB[ib];
            ia += takeA;
            ib += !takeA;
        }
    }
}

__global__ void k_seg_copy(const u64* __restrict__ src, u64* __restrict__ dst, const uint4* __restrict__ segs,
                           u32 nseg) {
    const u32 tile = blockIdx.x;
    u32 lo = 0, hi = nseg;
    while (hi - lo > 1) {
        u32 mid = (lo + hi) >> 1;
        if (segs[mid].z <= tile) lo = mid; else hi = mid;
    }
    const uint4 sg = segs[lo];
    const u32 len = sg.y - sg.x;
    const u32 o0 = (tile - sg.z) * MG_TILE;
    for (u32 i = o0 + threadIdx.x; i < min(o0 + MG_TILE, len); i += blockDim.x) dst[sg.x + i] = src[sg.x + i];
}
