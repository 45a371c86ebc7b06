// k_sort2.inc -- part of krisp_hip.hip (one translation unit): pass 1 and the LDS sort as persistent,
// software-pipelined kernels.
//
// Why these exist (round 2, profiles/r02/): the first versions read their keys with predicated
// loads (`i < e ? src[i] : 0`).  hipcc turns each into an exec-masked branch around the load and,
// unable to count memory operations across divergent control flow, waits with `s_waitcnt
// vmcnt(0)` at the first use of ANY loaded value -- which also waits for every store still in
// flight (CDNA4 counts loads and stores in one in-order counter) and for the "prefetched" loads of
// the next tile.  The ISA of round 1 shows exactly that: no load was ever in flight across a tile,
// and every tile start waited for the acknowledgement of the previous tile's stores.  Here:
//   * every global access inside a persistent loop is a raw BUFFER load / store whose range check
//     does the predication in hardware (an out-of-range lane reads 0 / is dropped): straight-line
//     code, so the compiler's counted `vmcnt(N)` leaves the newer operations in flight;
//   * loads are 16 bytes per lane;
//   * the next tile's keys are loaded into a second register set while the current tile is ranked,
//     staged and stored (loop unrolled by two: sets A / B, no register copies);
//   * no vector-memory operation sits in rarely taken branches or loops of dynamic length between
//     a prefetch and its first use (the waits stay exact).
// Measured (profiles/r02/ab_pipelined.log, same box, interleaved): k_localsort2 0.39 ms per 10^8 keys
// against 0.52 ms; pass 1 unchanged (0.30 ms) and a pass 2 built the same way 7 % SLOWER than the
// one-tile-per-workgroup k_scatter2 (kept): the two scatters are bound by the number of 128-byte
// line requests of their runs, which start on any 8-byte boundary (tools/membench.hip: 512-byte
// runs 4.0 TB/s misaligned, 5.4 TB/s line-aligned; 256-byte runs 3.5 / 5.4), not by latency.
// ----------------------------------------------------------------------------
// (vector types, buffer descriptors, opaque_tid, pair_lo / pair_hi, buf_store_u64: k_keys.inc)
// block-wide exclusive scan with ONE barrier inside (the caller separates uses of `waves` by its
// own barriers): wave scan by shuffles, wave totals through LDS, every thread sums the totals of
// the waves before its own.  NW = waves per workgroup.
template <int NW>
__device__ __forceinline__ u32 block_excl_scan1(u32 v, u32* lds_waves /* NW u32 */, u32& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 x = wave_incl_scan(v);
    if (lane == 63) lds_waves[wave] = x;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const u32 t = lds_waves[i];
        before += i < wave ? t : 0u;
        tot += t;
    }
    total = tot;
    return before + x - v;
}

// ----------------------------------------------------------------------------
// K5  LDS sort of one chunk (<= LS_CAP keys), in place in global memory.  Same algorithm as
// before (order-preserving 4096-way sub-binning with 16-bit LDS counters, block scan, placement,
// rank-by-counting inside each sub-bin; crowded sub-bins switch the chunk to a bitonic network;
// an oversized bucket is reported for the merge fallback), restructured:
//   * 16-byte buffer loads, the next chunk's keys in flight in a second register set;
//   * counters and the crowded flag ping-pong between chunks, the scan has one barrier:
//     4 barriers per chunk instead of 9;
//   * the stores of a chunk are 8 straight-line buffer stores (out-of-range offsets for empty
//     slots), the bitonic path ends in the same stores;
//   * oversized buckets are noted in LDS and reported after the loop.
// ----------------------------------------------------------------------------
#define LS2_PAIRS (LS_CAP / 2 / LS_THREADS)       // 16-byte loads per thread and chunk
#define LS2_NW (LS_THREADS / 64)
#ifndef LS2_OCC
#define LS2_OCC 6          // waves per SIMD: 3 workgroups of 512 threads per CU (<= 80 VGPRs, 3 x 49 KB LDS)
#endif
#define LS2_OVL 64          // oversized buckets one workgroup can note (more: whole-array fallback)

struct LsRegs { u32x4 q[LS2_PAIRS]; };

__device__ __forceinline__ void ls2_issue(LsRegs& r, const u64* keys, uint4 d) {
    const u32 tid = opaque_tid();
    const u32 m = min(d.y - d.x, LS_CAP);
    const bufrsrc rs = make_rsrc(keys + d.x, ((m + 1) & ~1u) * 8);      // (the arrays have two keys of slack)
#pragma unroll
    for (int i = 0; i < (int)LS2_PAIRS; i++)
        r.q[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + i * LS_THREADS) * 16, 0, KR_LS_LD_AUX);
    __builtin_amdgcn_sched_barrier(0);        // issued here, before anything of the current chunk
}

// element e (0 .. 2 LS2_PAIRS - 1) of the register set = key at chunk position 2 (tid + (e / 2) LS_THREADS) + (e & 1)
#define LS2_KEY(r, e) (((e) & 1) ? pair_hi((r).q[(e) >> 1]) : pair_lo((r).q[(e) >> 1]))
#define LS2_POS(e) (2u * (tid + ((e) >> 1) * LS_THREADS) + ((e) & 1))
#define LS2_HI(r, e) (((e) & 1) ? (r).q[(e) >> 1].w : (r).q[(e) >> 1].y)

__device__ __forceinline__ void ls2_process(const LsRegs& R, u64* keys, const u32* __restrict__ off, uint4 d, int rb,
                                            u64* S, u32* cnt, u32* cnt_next, u32* waves, u32* flag, u32* flag_next,
                                            uint4* ovl, u32* novl) {
    const u32 tid = opaque_tid();
    u32 s = d.x, e = d.y, lo = d.z, hi = d.w;
    u32 m = e - s;
    if (m > LS_CAP) {               // the chunk's last bucket is oversized: the merge fallback sorts it
        const u32 last = hi - 1;
        const u32 ls = off[last];
        if (tid == 0) {
            const u32 idx = *novl;
            if (idx < LS2_OVL) ovl[idx] = make_uint4(ls, e, last, 0);
            *novl = idx + 1;
        }
        hi = last;
        e = ls;
        m = e - s;
    }
    const u32 nbk = hi - lo;
    const int clog = nbk <= 1 ? 0 : 32 - __clz((int)(nbk - 1));
    // the sub-bin of a key from its HIGH word alone: the chunk's first key value lo << rb has no low word (rb >= 46)
    // and the field starts at bit rb + clog - 12 >= 34: one subtraction and one shift of 32 bits instead of 64
    const int sh32 = rb + clog - LS_NB_LOG - 32;
    const u32 klo_hi = lo << (rb - 32);
    // ---- count into the sub-bins (two 16-bit counters per word); a key's arrival number inside
    //      its sub-bin is kept in 16 bits (two per register), the sub-bin is recomputed from the key
#define LS2_SUB(q) ((LS2_HI(R, q) - klo_hi) >> sh32)
    u32 rp[LS2_PAIRS];
#pragma unroll
    for (int q = 0; q < 2 * (int)LS2_PAIRS; q++) {
        if ((q & 1) == 0) rp[q >> 1] = 0;
        if (LS2_POS(q) < m) {
            const u32 sub = LS2_SUB(q);
            const u32 old = atomicAdd(&cnt[sub >> 1], (sub & 1) ? 0x10000u : 1u);
            rp[q >> 1] |= ((sub & 1) ? (old >> 16) : (old & 0xFFFFu)) << (16 * (q & 1));
        }
    }
    __syncthreads();
    // ---- exclusive scan of the counters: thread t owns LS_WPT consecutive words
    {
        u32 w[LS_WPT];
        u32 sum = 0, mx = 0;
#pragma unroll
        for (int q = 0; q < LS_WPT; q++) {
            w[q] = cnt[tid * LS_WPT + q];
            const u32 a = w[q] & 0xFFFFu, c2 = w[q] >> 16;
            sum += a + c2;
            mx = max(mx, max(a, c2));
        }
        if (mx > LS_BIN_LIMIT) atomicMax(flag, mx);
        u32 total;
        u32 ex = block_excl_scan1<LS2_NW>(sum, waves, total);       // (one barrier inside)
#pragma unroll
        for (int q = 0; q < LS_WPT; q++) {
            const u32 a = w[q] & 0xFFFFu, c2 = w[q] >> 16;
            const u32 lo16 = ex;
            ex += a;
            const u32 hi16 = ex;
            ex += c2;
            cnt[tid * LS_WPT + q] = lo16 | (hi16 << 16);
            cnt_next[tid * LS_WPT + q] = 0;                         // the next chunk counts into the other array
        }
        if (tid == 0) {
            *flag_next = 0;
            cnt[LS_NB / 2] = m;                                     // (the end of the last sub-bin: no test for it below)
        }
    }
    __syncthreads();
    // ---- placement
#pragma unroll
    for (int q = 0; q < 2 * (int)LS2_PAIRS; q++)
        if (LS2_POS(q) < m) S[reinterpret_cast<const unsigned short*>(cnt)[LS2_SUB(q)] + ((rp[q >> 1] >> (16 * (q & 1))) & 0xFFFFu)] = LS2_KEY(R, q);
#undef LS2_SUB
    __syncthreads();
    // ---- rank inside the sub-bins, keys walked in PLACED order (lanes of a wave rank neighbours:
    //      adjacent LDS reads, stores inside one or two 512-byte runs); a crowded chunk runs the
    //      bitonic network over S instead and stores it as it lies.  Both forms end in the same
    //      2 LS2_PAIRS unconditional buffer stores (empty slots: out-of-range offsets).
    //      The stores are ONE common sequence behind both forms: the compiler's count of the
    //      operations in flight takes the minimum over all paths of the control-flow graph, so
    //      stores duplicated into the two branches would count as "maybe none".
    u64 kk[2 * LS2_PAIRS];
    u32 rk[2 * LS2_PAIRS];
    if (*flag <= LS_BIN_LIMIT) {
#pragma unroll
        for (int q = 0; q < 2 * (int)LS2_PAIRS; q++) {
            const u32 p = tid + q * LS_THREADS;
            kk[q] = 0;
            rk[q] = 0;
            if (p < m) {
                kk[q] = S[p];
                const u32 sb = ((u32)(kk[q] >> 32) - klo_hi) >> sh32;
                const unsigned short* c16 = reinterpret_cast<const unsigned short*>(cnt);
                const u32 b0 = c16[sb], b1 = c16[sb + 1];
                // rank = keys of the sub-bin in front of this one in (key, place) order: of those placed before it
                // the ones <= it, of those placed behind it the ones < it (two loops, one compare per key each)
                u32 rank = b0;
#ifndef LS2_NORANK          // (timing experiment: without the loops the keys leave in placed order)
                for (u32 t = b0; t < p; t++) rank += S[t] <= kk[q];
                for (u32 t = p + 1; t < b1; t++) rank += S[t] < kk[q];
#else
                rank = p + (b1 & 0);
#endif
                rk[q] = rank;
            }
        }
    } else {
        u32 np = 1;
        while (np < m) np <<= 1;
        for (u32 p = m + tid; p < np; p += LS_THREADS) S[p] = ~0ull;
        __syncthreads();
        for (u32 k2 = 2; k2 <= np; k2 <<= 1) {
            for (u32 jj = k2 >> 1; jj > 0; jj >>= 1) {
                for (u32 t = tid; t < np / 2; t += LS_THREADS) {
                    const u32 i0 = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
                    const u32 i1 = i0 | jj;
                    const bool up = (i0 & k2) == 0;
                    const u64 a = S[i0], c2 = S[i1];
                    if ((a > c2) == up) { S[i0] = c2; S[i1] = a; }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int q = 0; q < 2 * (int)LS2_PAIRS; q++) {
            const u32 p = tid + q * LS_THREADS;
            kk[q] = S[p < m ? p : 0];
            rk[q] = p;
        }
    }
    const bufrsrc ws = make_rsrc(keys + s, m * 8);
#pragma unroll
    for (int q = 0; q < 2 * (int)LS2_PAIRS; q++) {
        const u32 p = tid + q * LS_THREADS;
        buf_store_u64<KR_LS_ST_AUX>(kk[q], ws, p < m ? rk[q] * 8 : BUF_OOB);
    }
    // no barrier here: the next chunk counts into the other counter array, and it writes S only
    // after three of its own barriers, which every thread reaches after its reads above
}

__global__ __launch_bounds__(LS_THREADS, LS2_OCC) void k_localsort2(u64* keys, const u32* __restrict__ off,
                                                                    const uint4* __restrict__ desc, u32 nchunks, int b,
                                                                    u32* __restrict__ ovf_count,
                                                                    uint4* __restrict__ ovf_list) {
    __shared__ __attribute__((aligned(16))) u64 S[LS_CAP];
    __shared__ __attribute__((aligned(16))) u32 cnt[2][LS_NB / 2 + 4];      // (+ the sentinel behind the last sub-bin)
    __shared__ u32 waves[LS2_NW];
    __shared__ u32 flag[2];
    __shared__ uint4 ovl[LS2_OVL];
    __shared__ u32 novl;
    const u32 tid = threadIdx.x;
    const u32 G = gridDim.x;
    const int rb = 64 - b;
    // descriptor of chunk jj, all zero (an empty chunk) past the last one.  (Loaded from a clamped
    // index and then masked: a select between the table and a zero constant would put that
    // constant into scratch memory.)
    auto chunk = [&](u32 jj) {
        uint4 dd = desc[jj < nchunks ? jj : nchunks - 1];
        const u32 keep = jj < nchunks ? ~0u : 0u;
        dd.x &= keep; dd.y &= keep; dd.z &= keep; dd.w &= keep;
        return dd;
    };
    for (u32 i = tid; i < LS_NB / 2; i += LS_THREADS) cnt[0][i] = 0;
    if (tid == 0) { flag[0] = 0; flag[1] = 0; novl = 0; }
    u32 j = blockIdx.x;
    uint4 d0 = chunk(j);
    uint4 d1 = chunk(j + G);
    LsRegs A, B;
    ls2_issue(A, keys, d0);
    // equalise the memory-operation history of the loop's two entries (first iteration / back
    // edge), so that the counted wait for A does not also wait for the previous chunk's stores:
    // as many dropped stores here as ls2_process issues
    {
        const bufrsrc none = make_rsrc(keys, 0);
#pragma unroll
        for (int q = 0; q < 2 * (int)LS2_PAIRS; q++) buf_store_u64(0, none, 64u * q);     // (distinct, non-adjacent offsets: else they are merged or widened)
    }
    __syncthreads();
    for (; j < nchunks; j += 2 * G) {
        const uint4 d2 = chunk(j + 2 * G);
        ls2_issue(B, keys, d1);
        ls2_process(A, keys, off, d0, rb, S, cnt[0], cnt[1], waves, &flag[0], &flag[1], ovl, &novl);
        const uint4 d3 = chunk(j + 3 * G);
        ls2_issue(A, keys, d2);
        ls2_process(B, keys, off, d1, rb, S, cnt[1], cnt[0], waves, &flag[1], &flag[0], ovl, &novl);
        d0 = d2;
        d1 = d3;
    }
    __syncthreads();
    if (tid == 0 && novl) {
        const u32 n = novl;
        if (n > LS2_OVL) {
            atomicAdd(ovf_count, OVF_MAX + 1u);            // more than this list holds: whole-array fallback
        } else {
            const u32 idx = atomicAdd(ovf_count, n);
            for (u32 i = 0; i < n; i++)
                if (idx + i < OVF_MAX) ovf_list[idx + i] = ovl[i];
        }
    }
}

// ----------------------------------------------------------------------------
// K3  pass 1, software-pipelined: same tiles, ranges and private cursors as k_scatter1 (no global
// atomics); the code words of the next tile are in flight while the current one is ranked, staged
// and stored, and the stores are straight-line (buffer stores; BIG = 1, the pass 0 of sliced
// genomes whose output exceeds the 4 GiB a buffer descriptor spans: plain stores, the rare empty
// slot written to the spare key behind the array).  WIDE: 0 both strands, 2 one key per window.
// ----------------------------------------------------------------------------
struct P1Regs { u32x4 c; u32x2 b; };

template <int TPW = P1_TPW>
__device__ __forceinline__ void p1_issue(P1Regs& r, bufrsrc cs, bufrsrc bs, u64 wt) {
    const u32 w = (u32)wt + opaque_tid() / TPW;
    r.c = __builtin_amdgcn_raw_buffer_load_b128(cs, w * 8, 0, 0);       // codes[w], codes[w + 1]
    r.b = __builtin_amdgcn_raw_buffer_load_b64(bs, w * 4, 0, 0);        // bad[w], bad[w + 1]
    __builtin_amdgcn_sched_barrier(0);
}

// BIG (the pass 0 of a sliced genome): the digit is the top P0_DIGIT_BITS bits of the key -- the slice alone, so that a
// tile leaves 4^sb runs four times as long as 256 would be (configs[4]: pass 0 wrote 96 GB at 2.6 TB/s by the top byte);
// the kernel runs with g.sbits = 0 (absolute keys, no slice test), g.slice carries the digit width.
#define P0_DIGIT_BITS(g) ((int)(g).slice)

// FAST (both strands, no field rotation, `left` fills the key's high word -- layout_key's 32-bit form; every krisp_fasta
// geometry with L >= 16): the P1_PPT windows of a thread start 2 bits apart in the word string, so the string is shifted
// to the thread's first window ONCE (three dwords of the forward string, three of word_revstring's reverse string) and
// a window's two keys are four funnel shifts by compile-time amounts + the layout -- instead of, per window, a 128-bit
// shift by a run-time amount, complement + bit reversal + pair swap, and the top mask (which the field masks of the
// layout imply: every field's source bits lie inside the window).  ~24 vector instructions per window against ~64
// (ISA of round 5; k_scatter1p is bound by them: with its stores dropped it ran at 0.74 of its time).
__device__ __forceinline__ void p1_fast_keys(u64 c0, u64 c1, u32 b0, u32 b1, const Geom& g, u64 (&key)[P1_KPT], u32& vm) {
    static_assert(P1_PPT <= 16, "a thread's windows must start inside one dword of the shifted strings");
    const u32 q = opaque_tid() % P1_TPW;
    const int cs = 2 * P1_PPT * (int)q;                      // bit offset of the thread's first window in c0:c1 (< 64)
    const u64 f01 = cs ? (c0 << cs) | (c1 >> (64 - cs)) : c0;
    const u32 f0 = (u32)(f01 >> 32), f1 = (u32)f01, f2 = (u32)((c1 << cs) >> 32);
    // the reverse string (word_revstring): the reverse key of window J starts at bit 62 - 2 J; shifted so that the
    // thread's LAST window starts at bit 0, window jj of the thread at bit 2 (P1_PPT - 1 - jj)
    u32 sf[5], rv[5];
    word_revstring(c0, c1, g.k, sf, rv);
    (void)sf;
    const u64 q0 = ((u64)rv[0] << 32) | rv[1], q1 = ((u64)rv[2] << 32) | rv[3];
    const int ro = 64 - 2 * P1_PPT * ((int)q + 1);           // 62 - 2 (first window + P1_PPT - 1): 0 .. 62, even
    const u64 y01 = ro ? (q0 << ro) | (q1 >> (64 - ro)) : q0;
    const u32 y0 = (u32)(y01 >> 32), y1 = (u32)y01, y2 = (u32)((q1 << ro) >> 32);
    const u64 B = (((u64)b0 << 32) | b1) << (P1_PPT * q);     // bad bits from the thread's first window on
    const u32 bh = (u32)(B >> 32), bl = (u32)B;
    const u32 mLh = (u32)(g.mL >> 32), mLl = (u32)g.mL, mRl = (u32)g.mR, mDl = (u32)g.mD;
    const u32 sR = (u32)g.sR & 31u, sD = (u32)g.sD & 31u, vsh = 32u - (u32)g.k;
#pragma unroll
    for (int jj = 0; jj < P1_PPT; jj++) {
        const u32 bm = __funnelshift_l(bl, bh, jj);
        const u32 fh = __funnelshift_l(f1, f0, 2 * jj), fl = __funnelshift_l(f2, f1, 2 * jj);
        const u32 rh = __funnelshift_l(y1, y0, 2 * (P1_PPT - 1 - jj)), rl = __funnelshift_l(y2, y1, 2 * (P1_PPT - 1 - jj));
        key[2 * jj] = ((u64)(fh & mLh) << 32) | ((fl & mLl) | ((fl << sR) & mRl) | ((fl >> sD) & mDl));
        key[2 * jj + 1] = ((u64)(rh & mLh) << 32) | ((rl & mLl) | ((rl << sR) & mRl) | ((rl >> sD) & mDl));
        vm |= (bm >> vsh) == 0u ? 3u << (2 * jj) : 0u;
    }
}

// ONE (a coarse genome whose forward strand answers for both: co_strand.inc): the forward keys alone, 32 windows per pair
// of threads, so a tile is twice the code words and still P1_STAGE keys
#define P1_ONE_TPW (P1_TPW / 2)
#define P1_ONE_PPT (2 * P1_PPT)
__device__ __forceinline__ void p1_fast_keys_fwd(u64 c0, u64 c1, u32 b0, u32 b1, const Geom& g, u64 (&key)[P1_KPT], u32& vm) {
    static_assert(P1_ONE_PPT <= 16 && P1_ONE_PPT == P1_KPT, "a thread's windows must start inside one dword of the shifted string");
    const u32 q = opaque_tid() % P1_ONE_TPW;
    const int cs = 2 * P1_ONE_PPT * (int)q;                  // bit offset of the thread's first window in c0:c1 (< 64)
    const u64 f01 = cs ? (c0 << cs) | (c1 >> (64 - cs)) : c0;
    const u32 f0 = (u32)(f01 >> 32), f1 = (u32)f01, f2 = (u32)((c1 << cs) >> 32);
    const u64 B = (((u64)b0 << 32) | b1) << (P1_ONE_PPT * q);
    const u32 bh = (u32)(B >> 32), bl = (u32)B;
    const u32 mLh = (u32)(g.mL >> 32), mLl = (u32)g.mL, mRl = (u32)g.mR, mDl = (u32)g.mD;
    const u32 sR = (u32)g.sR & 31u, sD = (u32)g.sD & 31u, vsh = 32u - (u32)g.k;
#pragma unroll
    for (int jj = 0; jj < P1_ONE_PPT; jj++) {
        const u32 bm = __funnelshift_l(bl, bh, jj);
        const u32 fh = __funnelshift_l(f1, f0, 2 * jj), fl = __funnelshift_l(f2, f1, 2 * jj);
        key[jj] = ((u64)(fh & mLh) << 32) | ((fl & mLl) | ((fl << sR) & mRl) | ((fl >> sD) & mDl));
        vm |= (bm >> vsh) == 0u ? 1u << jj : 0u;
    }
}

template <int WIDE, int BIG, int FAST = 0, int ONE = 0>
__device__ __forceinline__ void p1_tile(const P1Regs& R, u64 wt, u64 w1, const Geom& g, bufrsrc ds, u64* dst,
                                        u64 sink, u64* stage, u64* cur, u32* cnt, u32* cnt_next, u64* delta,
                                        u32* waves) {
    const u32 tid = opaque_tid();
    const int dsh = BIG ? 64 - P0_DIGIT_BITS(g) : 56;
    const u64 w = wt + tid / (ONE ? P1_ONE_TPW : P1_TPW);
    const int j0 = (tid % P1_TPW) * P1_PPT;
    const CoStrand S = cs_make(ONE ? g.L : 5, ONE ? g.R : 0);       // (ONE: the digit is co_strand.inc's; else unused)
    auto digit = [&](u64 k) { return ONE ? cs_digit(S, k) : (u32)(k >> dsh); };
    u64 key[P1_KPT];
    u32 rp[P1_KPT / 2];         // a key's arrival number inside its digit: 16 bits, two per register
    u32 vm = 0;
#pragma unroll
    for (int q = 0; q < P1_KPT; q++) { key[q] = 0; if ((q & 1) == 0) rp[q >> 1] = 0; }
    if (w < w1) {
        const u32 b0 = R.b.x, b1 = R.b.y;
        if (b0 != 0xFFFFFFFFu) {
            const u64 c0 = pair_lo(R.c), c1 = pair_hi(R.c);
            if (ONE) {
                p1_fast_keys_fwd(c0, c1, b0, b1, g, key, vm);
            } else if (FAST) {
                p1_fast_keys(c0, c1, b0, b1, g, key, vm);
            } else if (WIDE == 2) {
#pragma unroll
                for (int jj = 0; jj < P1_PPT; jj++) {
                    u64 k1;
                    if (window_key_single(c0, c1, b0, b1, j0 + jj, g, k1)) {
                        key[2 * jj] = k1;
                        vm |= 1u << (2 * jj);
                    }
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < P1_PPT; jj++) {
                    u64 kf, kr;
                    // (no slice test: this kernel makes the absolute keys of a whole genome -- the one sort unit, or the
                    // pass 0 of a sliced genome --, g.sbits = 0 in every launch: h_core.inc)
                    if (window_keys(c0, c1, b0, b1, j0 + jj, g, kf, kr)) {
                        key[2 * jj] = kf;
                        key[2 * jj + 1] = kr;
                        vm |= 3u << (2 * jj);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < P1_KPT; q++)
        if ((vm >> q) & 1) rp[q >> 1] |= atomicAdd(&cnt[digit(key[q])], 1u) << (16 * (q & 1));
    __syncthreads();
    const u32 c = tid < 256 ? cnt[tid] : 0;
    u32 total;
    const u32 ex = block_excl_scan1<P1_T / 64>(c, waves, total);         // (one barrier inside)
    if (tid < 256) {
        cnt[tid] = ex;
        delta[tid] = cur[tid] - ex;
        cur[tid] += c;
        cnt_next[tid] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < P1_KPT; q++)
        if ((vm >> q) & 1) stage[cnt[digit(key[q])] + ((rp[q >> 1] >> (16 * (q & 1))) & 0xFFFFu)] = key[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < P1_KPT; q++) {
        const u32 p = q * P1_T + tid;
        const u64 k2 = stage[p];
        const u64 o = p + delta[digit(k2)];
        if (BIG) dst[p < total ? o : sink] = k2;
        else buf_store_u64<KR_P1_ST_AUX>(k2, ds, p < total ? (u32)o * 8 : BUF_OOB);
    }
}

template <int WIDE, int BIG, int FAST = 0, int ONE = 0>
__global__ __launch_bounds__(P1_T, P1_OCC) void k_scatter1p(const u64* __restrict__ codes, const u32* __restrict__ bad,
                                                            u64 nwords, const u32* __restrict__ base1,
                                                            const u64* __restrict__ base64,
                                                            const u32* __restrict__ rowoff, u64* dst, u64 dst_keys,
                                                            Geom g) {
    __shared__ __attribute__((aligned(16))) u64 stage[P1_STAGE];
    __shared__ u64 cur[256];      // (64 bit: the slice pre-partition of a >= 2 Gbp genome exceeds 2^32 keys)
    __shared__ u32 cnt[2][256];
    __shared__ u64 delta[256];
    __shared__ u32 waves[P1_T / 64];
    const u32 tid = threadIdx.x;
    if (tid < 256) {
        if (BIG) {
            // bucket `tid` of the pass 0 = the `per` top-byte columns of k_hist8 that share its top bits: its place is
            // the base of the first of them, this workgroup's place inside it the sum of its places in each
            const u32 per = 256u >> P0_DIGIT_BITS(g);
            u64 at = 0;
            if (tid * per < 256u) {
                at = base64[tid * per];
                for (u32 j = 0; j < per; j++) at += rowoff[P8(blockIdx.x, tid * per + j)];
            }
            cur[tid] = at;
        } else {
            cur[tid] = (u64)base1[tid] + rowoff[P8(blockIdx.x, tid)];
        }
        cnt[0][tid] = 0;
    }
    const u64 wpw = (nwords + NWG - 1) / NWG;
    const u64 w0 = (u64)blockIdx.x * wpw;
    const u64 w1 = w0 + wpw < nwords ? w0 + wpw : nwords;
    const bufrsrc cs = make_rsrc(codes, (u32)(nwords + PAD_WORDS) * 8);
    const bufrsrc bs = make_rsrc(bad, (u32)(nwords + PAD_WORDS) * 4);
    const bufrsrc ds = make_rsrc(dst, BIG ? 0u : (u32)dst_keys * 8);
    const u64 sink = dst_keys + 1;            // (the arrays have two keys of slack)
    constexpr int TPW = ONE ? P1_ONE_TPW : P1_TPW;
    constexpr u64 WORDS = P1_T / TPW;         // code words of a tile
    P1Regs A, B;
    p1_issue<TPW>(A, cs, bs, w0);
    {   // equalise the memory-operation history of the loop's two entries (see k_localsort2)
        const bufrsrc none = make_rsrc(dst, 0);
#pragma unroll
        for (int q = 0; q < P1_KPT; q++) buf_store_u64(0, none, 64u * q);     // (distinct, non-adjacent offsets: else they are merged or widened)
    }
    __syncthreads();
    for (u64 wt = w0; wt < w1; wt += 2 * WORDS) {
        p1_issue<TPW>(B, cs, bs, wt + WORDS);
        p1_tile<WIDE, BIG, FAST, ONE>(A, wt, w1, g, ds, dst, sink, stage, cur, cnt[0], cnt[1], delta, waves);
        p1_issue<TPW>(A, cs, bs, wt + 2 * WORDS);
        p1_tile<WIDE, BIG, FAST, ONE>(B, wt + WORDS, w1, g, ds, dst, sink, stage, cur, cnt[1], cnt[0], delta, waves);
    }
}

// ----------------------------------------------------------------------------
// K3k  pass 1 of one key-space slice from its region of the pass-0 array (keys read and made
// relative instead of generated), pipelined the same way: the next tile's keys in a second
// register set.
// ----------------------------------------------------------------------------
struct P1kRegs { u32x4 q[P1_KPT / 2]; };

__device__ __forceinline__ void p1k_issue(P1kRegs& r, const u64* src, u64 t0, u64 k1) {
    const u32 tid = opaque_tid();
    const u32 n = t0 < k1 ? (u32)min((u64)P1K_TILE, k1 - t0) : 0u;
    const bufrsrc rs = make_rsrc(src + (t0 < k1 ? t0 : 0), ((n + 1) & ~1u) * 8);
#pragma unroll
    for (int i = 0; i < P1_KPT / 2; i++)
        r.q[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + i * P1_T) * 16, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
}
#define P1K_KEY(r, e) ((((e) & 1) ? pair_hi((r).q[(e) >> 1]) : pair_lo((r).q[(e) >> 1])) << sbits)
#define P1K_POS(e) (2u * (tid + ((e) >> 1) * P1_T) + ((e) & 1))

__device__ __forceinline__ void p1k_tile(const P1kRegs& R, u64 t0, u64 k1, int sbits, bufrsrc ds, u64* stage, u32* cur,
                                         u32* cnt, u32* cnt_next, u32* delta, u32* waves) {
    const u32 tid = opaque_tid();
    const u32 nt = t0 < k1 ? (u32)min((u64)P1K_TILE, k1 - t0) : 0u;
    u32 rp[P1_KPT / 2];
#pragma unroll
    for (int q = 0; q < P1_KPT; q++) {
        if ((q & 1) == 0) rp[q >> 1] = 0;
        if (P1K_POS(q) < nt) rp[q >> 1] |= atomicAdd(&cnt[(u32)(P1K_KEY(R, q) >> 56)], 1u) << (16 * (q & 1));
    }
    __syncthreads();
    const u32 c = tid < 256 ? cnt[tid] : 0;
    u32 total;
    const u32 ex = block_excl_scan1<P1_T / 64>(c, waves, total);
    if (tid < 256) {
        cnt[tid] = ex;
        delta[tid] = cur[tid] - ex;
        cur[tid] += c;
        cnt_next[tid] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < P1_KPT; q++)
        if (P1K_POS(q) < nt)
            stage[cnt[(u32)(P1K_KEY(R, q) >> 56)] + ((rp[q >> 1] >> (16 * (q & 1))) & 0xFFFFu)] = P1K_KEY(R, q);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < P1_KPT; q++) {
        const u32 p = q * P1_T + tid;
        const u64 k2 = stage[p];
        const u32 o = p + delta[(u32)(k2 >> 56)];
        buf_store_u64(k2, ds, p < nt ? o * 8 : BUF_OOB);
    }
}

__global__ __launch_bounds__(P1_T, P1_OCC) void k_scatter1kp(const u64* __restrict__ src, u64 n, int sbits,
                                                             const u32* __restrict__ base1,
                                                             const u32* __restrict__ rowoff, u64* dst, u32 dst_keys) {
    __shared__ __attribute__((aligned(16))) u64 stage[P1_STAGE];
    __shared__ u32 cur[256];
    __shared__ u32 cnt[2][256];
    __shared__ u32 delta[256];
    __shared__ u32 waves[P1_T / 64];
    const u32 tid = threadIdx.x;
    if (tid < 256) {
        cur[tid] = base1[tid] + rowoff[P8(blockIdx.x, tid)];
        cnt[0][tid] = 0;
    }
    const u64 per = ((n + NWG - 1) / NWG + P1K_TILE - 1) / P1K_TILE * P1K_TILE;
    const u64 k0 = (u64)blockIdx.x * per;
    const u64 k1 = k0 + per < n ? k0 + per : n;
    const bufrsrc ds = make_rsrc(dst, dst_keys * 8);
    P1kRegs A, B;
    p1k_issue(A, src, k0, k1);
    {
        const bufrsrc none = make_rsrc(dst, 0);
#pragma unroll
        for (int q = 0; q < P1_KPT; q++) buf_store_u64(0, none, 64u * q);     // (distinct, non-adjacent offsets: else they are merged or widened)
    }
    __syncthreads();
    for (u64 t0 = k0; t0 < k1; t0 += 2 * (u64)P1K_TILE) {
        p1k_issue(B, src, t0 + P1K_TILE, k1);
        p1k_tile(A, t0, k1, sbits, ds, stage, cur, cnt[0], cnt[1], delta, waves);
        p1k_issue(A, src, t0 + 2 * (u64)P1K_TILE, k1);
        p1k_tile(B, t0 + P1K_TILE, k1, sbits, ds, stage, cur, cnt[1], cnt[0], delta, waves);
    }
}
