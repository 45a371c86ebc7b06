// k_intersect3.inc -- part of krisp_hip.hip (one translation unit): K6 as a persistent, software-pipelined kernel.
//
// Why (round 3, profiles/r03/isect_ablate_r02_kernel.log): k_intersect<0> spent 1.38 ms per 4 x 10^8 keys where the
// bytes need 0.5 ms.  With the streaming switched off the anchor set-up alone took 0.58 ms (1.4 TB/s over its 0.8 GB),
// with the probes switched off 0.99 ms: one workgroup per chunk walks a chain of dependent round trips per sub-tile
// (boundary search -> anchor keys -> compaction (2 barriers) -> sub-bin fill -> stream ranges -> first batch ...), eight
// barriers long, and four such workgroups per CU do not hide it.  Here:
//   * an ITEM is 2^mlog whole fine buckets (<= 4 T anchor keys, T = threads of the workgroup, both chosen by the host
//     from the bucket statistics): no boundary search; the item's sub-bins are a fixed bit field of the prefix
//     (bits [sh, sh + 11): the bits right below the item's common top bits), so a key's bin needs no first / last
//     head, no clamp and no compare;
//   * no compaction of the anchor's prefixes: slot p of the item IS anchor key p (heads[p] = its prefix); the rare
//     later member of a run of equal prefixes hands its diagnostic columns to the run's first slot and retires, a
//     look-up always lands on the first slot of a run;
//   * the workgroup is persistent and every global read is one stream of BATCHES (4 T keys: two 16-byte buffer loads
//     per lane; the anchor's keys of an item, then every other genome's keys of the same buckets, then the next
//     item's anchor ...) walked by a uniform state machine: batch t + 1 is in flight in a second register set while
//     batch t is processed, across genomes and across items; the bucket offsets of the NEXT item are loaded while the
//     current one is set up, so no wave ever waits for an offset it then needs for an address;
//   * five barriers per item (heads written | bin scan | bins published | probes done | survivor scan) instead of nine.
// Items whose anchor run exceeds 4 T keys (skew) are listed and handled by k_intersect afterwards (item-list mode);
// 2 * LRrel < b, one genome, KR_OPT_GENERIC_INTERSECT: k_intersect as before.
// ----------------------------------------------------------------------------
#ifndef I3_NB_LOG
#define I3_NB_LOG 11
#endif
#define I3_NB (1u << I3_NB_LOG)         // sub-bins per item (16-bit counters, two per word)
#define I3_MAXT 512
#define I3_WMAX (I3_NB / 2 / 256)   // counter words per thread in the scan at the smallest workgroup (256 threads)
#define I3_SLOTS (4 * I3_MAXT)
#define I3_OVF_CAP 1024u     // oversized items one launch can list (and the grid of the launch that takes them)
#define I3_OVF_LAUNCH I3_OVF_CAP
#ifndef I3_ABL
#define I3_ABL 0           // (timing experiments only: parts of the kernel compiled out, results wrong)
#endif
#ifndef I3_OCC0
#define I3_OCC0 6           // waves per SIMD the compact format is compiled for (8: 64 VGPRs with spills; 6: 70 VGPRs, 7 waves fit)
#endif

struct Isect3Args {
    const u64* keys[MAXG];
    const u32* off[MAXG];
    u32 ingroup_bits;
    int n, anchor;
    u32 nb;           // fine buckets of the grid
    int mlog;         // an item = 2^mlog buckets
    u32 nitems;
    int sh;           // sub-bin of a prefix = (prefix >> sh) & (I3_NB - 1)
    kr_cand* tmp;     // survivors of item i at tmp[offA[first bucket of i] ...]
    u32* itemcnt;     // survivors per item
    u32* ovf;         // [0] = number of oversized items, [1 ...] = their numbers
    u32 ovf_cap;
    int apply_filter;
    int p0;           // k_intersect3t: lowest bit of the prefix (64 - 2 LRrel)
};

struct I3Regs { u32x4 q[2]; };
// element e (0..3) of a register set = key (2 (tid + (e / 2) T) + (e & 1)) of the batch
#define I3_KEY(r, e) (((e) & 1) ? pair_hi((r).q[(e) >> 1]) : pair_lo((r).q[(e) >> 1]))
#define I3_POS(e) (2u * (tid + ((e) >> 1) * T) + ((e) & 1))

// where the stream of batches stands: all fields wave-uniform
struct I3State {
    u32 it;       // item
    int g;        // -1: the anchor's keys of the item (heads are built from them), else the genome streamed
    u32 i0, e;    // the batch = keys [i0, min(i0 + 4 T, e)) of that genome
    u32 par;      // slot of rng[] holding the item's ranges
    u32 over;     // the item's anchor run exceeds 4 T keys: nothing is loaded or probed, the item is listed
};

__device__ __forceinline__ u32 i3_uni(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
// sub-bin of a prefix: bits [sh, sh + I3_NB_LOG), sh >= 35 always (sh >= 64 - b + mlog - I3_NB_LOG, b <= 18): one
// bit-field extract from the high word
__device__ __forceinline__ u32 i3_bin(u64 pre, int sh) { return __builtin_amdgcn_ubfe((u32)(pre >> 32), (u32)(sh - 32), I3_NB_LOG); }

// the batch after `st` (rng[par][g] = key range of genome g in the item's buckets)
__device__ __forceinline__ void i3_advance(I3State& st, const Isect3Args& a, const uint2 (*rng)[MAXG], u32 S, u32 G) {
    int g2 = st.g + 1;
    if (g2 == a.anchor) g2++;
    if (st.g >= 0 && st.i0 + S < st.e) {
        st.i0 += S;
    } else if (g2 < a.n) {
        const uint2 r = rng[st.par][g2];
        st.g = g2;
        st.i0 = i3_uni(r.x);
        st.e = st.over ? st.i0 : i3_uni(r.y);
    } else {
        st.it += G;
        st.par ^= 1u;
        st.g = -1;
        const uint2 r = rng[st.par][a.anchor];
        const u32 s = i3_uni(r.x), e = i3_uni(r.y);
        st.over = (e - s > S) ? 1u : 0u;
        st.i0 = s;
        st.e = st.over ? s : e;
    }
    if (st.it >= a.nitems) { st.i0 = 0; st.e = 0; st.over = 0; }
    // (stated once more for the compiler: every field is wave-uniform, the branches on them are scalar)
    st.it = i3_uni(st.it); st.g = (int)i3_uni((u32)st.g); st.i0 = i3_uni(st.i0); st.e = i3_uni(st.e);
    st.par = i3_uni(st.par); st.over = i3_uni(st.over);
}

__device__ __forceinline__ void i3_issue(I3Regs& r, const Isect3Args& a, const u64* const* keyp, const I3State& st, u32 T) {
    const u32 tid = opaque_tid();
    const u32 S = 4 * T;
    const u32 m = min(st.e - st.i0, S);
    // (the pointer table lives in LDS: indexed from the kernel arguments it is a vector load from memory and
    // a wait for every load in flight in front of each batch)
    const u64 kp = (u64)keyp[st.g < 0 ? a.anchor : st.g];
    const u64* base = (const u64*)(((u64)i3_uni((u32)(kp >> 32)) << 32) | i3_uni((u32)kp)) + st.i0;
    const bufrsrc rs = make_rsrc(base, ((m + 1) & ~1u) * 8);        // (the arrays have two keys of slack)
    r.q[0] = __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, 0, KR_IS_LD_AUX);
    r.q[1] = __builtin_amdgcn_raw_buffer_load_b128(rs, (tid + T) * 16, 0, KR_IS_LD_AUX);
    __builtin_amdgcn_sched_barrier(0);
}

// per-slot state in LDS by mask format FMT: as k_intersect (isect_update<FMT>)
template <int FMT>
__device__ __forceinline__ void i3_init_slot(u32 p, u64 key, int anchor, bool anchor_in, u32* present, u64* inm, u64* outm,
                                             const Geom& g, int LR) {
    const u64 dm = g.D > 0 ? diag_mask(key, LR, g.D) : 0;
    if (FMT == 0) {
        inm[p] = ((u64)1 << (32 + anchor)) | (anchor_in ? dm : (dm << 16));
    } else if (FMT == 1) {
        present[p] = 1u << anchor;
        inm[p] = anchor_in ? dm : (dm << 32);
    } else {
        present[p] = 1u << anchor;
        inm[p] = anchor_in ? dm : 0;
        outm[p] = anchor_in ? 0 : dm;
    }
}

template <int FMT>
__global__ __launch_bounds__(I3_MAXT, FMT == 0 ? I3_OCC0 : (FMT == 1 ? 6 : 4)) void k_intersect3(Isect3Args a, Geom g) {
    constexpr bool WIDE = FMT == 2;
    __shared__ __attribute__((aligned(16))) u64 heads[I3_SLOTS + 6];
    __shared__ __attribute__((aligned(16))) u64 inm[I3_SLOTS + 8];
    __shared__ __attribute__((aligned(16))) u64 outm[WIDE ? I3_SLOTS + 8 : 1];
    __shared__ u32 present[FMT == 0 ? 1 : I3_SLOTS + 8];
    __shared__ __attribute__((aligned(16))) u32 cnt16[I3_NB / 2];
    __shared__ uint2 rng[2][MAXG];
    __shared__ const u64* keyp[MAXG];
    __shared__ u32 waves[8];
    const u32 tid = threadIdx.x, T = blockDim.x, S = 4 * T, G = gridDim.x;
    const u32 lane = tid & 63;
    const int LR = g.LRrel;
    const u32 full = a.n >= 32 ? 0xFFFFFFFFu : ((1u << a.n) - 1);
    const bool anchor_in = (a.ingroup_bits >> a.anchor) & 1;
    const u32 WPT = (I3_NB / 2 + T - 1) / T;            // counter words per thread in the scan (<= I3_WMAX: T >= 256)
    const int sh = a.sh;
    // lane l < 2 n reads offset (l & 1) of genome l / 2 for the items to come (every wave the same 64 addresses)
    const u32 og = min(lane >> 1, (u32)a.n - 1);
    const u32 __attribute__((address_space(1)))* myoff;      // (stays a GLOBAL pointer: a flat load would also count as an LDS operation)
    {
        // (made opaque HERE, on every path: a load still pending on some path into the loop makes the compiler wait
        // for all loads in flight at the first use of its result inside the loop, on every trip)
        u64 mo = (u64)a.off[og];
        asm volatile("" : "+v"(mo));
        myoff = (const u32 __attribute__((address_space(1)))*)mo;
    }
    auto item_bucket = [&](u32 it, u32 which) {      // first bucket (which = 0) / end bucket (1) of item it, clamped
        const u64 f = ((u64)it + which) << a.mlog;
        return (u32)(f < a.nb ? f : a.nb);
    };
    for (u32 i = tid; i < I3_NB / 2; i += T) cnt16[i] = 0;
    if (tid < 8) waves[tid] = 0;
    if (tid < (u32)a.n) keyp[tid] = a.keys[tid];
    {
        u32 v = myoff[item_bucket(blockIdx.x, lane & 1)];
        asm volatile("" : "+v"(v));
        if (tid < 2 * (u32)a.n) {
            if (lane & 1) rng[0][og].y = v; else rng[0][og].x = v;
        }
    }
    __syncthreads();
    I3State cur;
    cur.it = blockIdx.x;
    cur.g = -1;
    cur.par = 0;
    {
        const uint2 r = rng[0][a.anchor];
        const u32 s = i3_uni(r.x), e = i3_uni(r.y);
        cur.over = (e - s > S) ? 1u : 0u;
        cur.i0 = s;
        cur.e = cur.over ? s : e;
    }
    if (cur.it >= a.nitems) return;
    u32 item_sa = 0, item_cnt = 0;       // the current item's anchor run
    u32 voff = 0;
    I3Regs X, Y;
    i3_issue(X, a, keyp, cur, T);

    // ---- one batch: R holds its keys, st says what they are, nx is the batch after it
    auto process = [&](const I3Regs& R, const I3State& st, const I3State& nx) {
        const u32 tid = opaque_tid();
        // the batch is consumed on EVERY path (an oversized item never looks at it): registers of a load left
        // pending on some path cost a wait for everything in flight where they are next written
        asm volatile("" ::"v"(R.q[0]), "v"(R.q[1]));
        if (st.g < 0) {
            // ===== anchor keys of a new item: slots, sub-bin counts
            item_sa = st.i0;
            item_cnt = st.e - st.i0;
            const u32 cnt = item_cnt;
            if (st.over) {
                if (tid == 0) {
                    const u32 idx = atomicAdd(&a.ovf[0], 1u);
                    if (idx < a.ovf_cap) a.ovf[1 + idx] = st.it;
                    a.itemcnt[st.it] = 0;
                }
            } else {
#pragma unroll
                for (int e = 0; e < (I3_ABL & 4 ? 0 : 4); e++) {
                    const u32 p = I3_POS(e);
                    if (p < cnt) {
                        const u64 key = I3_KEY(R, e);
                        const u64 pre = key & g.pmask;
                        heads[p] = pre;
                        i3_init_slot<FMT>(p, key, a.anchor, anchor_in, present, inm, outm, g, LR);
                        const u32 sb = i3_bin(pre, sh);
                        atomicAdd(&cnt16[sb >> 1], (sb & 1) ? 0x10000u : 1u);
                    }
                }
            }
            __syncthreads();                                                        // (1) heads, counts
            if (!st.over && !(I3_ABL & 8)) {
                // a later member of a run of equal prefixes: its columns go to the run's first slot, it retires
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const u32 p = I3_POS(e);
                    if (p >= 1 && p < cnt) {
                        const u64 key = I3_KEY(R, e);
                        const u64 pre = key & g.pmask;
                        const u64 prev = (e & 1) ? (I3_KEY(R, e - 1) & g.pmask) : heads[p - 1];
                        if (prev == pre) {
                            u32 t = p - 1;
                            while (t > 0 && heads[t - 1] == pre) t--;
                            if (FMT == 0) inm[p] = 0; else present[p] = 0;
                            isect_update<FMT>(t, key, a.anchor, anchor_in, present, inm, outm, g, LR);
                        }
                    }
                }
                // exclusive scan of the counts: binstart, two 16-bit entries per word
                u32 w[I3_WMAX];
                u32 sum = 0;
#pragma unroll
                for (int q = 0; q < I3_WMAX; q++) {
                    const u32 i = tid * WPT + q;
                    w[q] = (q < (int)WPT && i < I3_NB / 2) ? cnt16[i] : 0u;
                    sum += (w[q] & 0xFFFFu) + (w[q] >> 16);
                }
                u32 total;
                u32 ex = block_excl_scan1<8>(sum, waves, total);                     // (2) inside
#pragma unroll
                for (int q = 0; q < I3_WMAX; q++) {
                    const u32 i = tid * WPT + q;
                    const u32 lo16 = ex;
                    ex += w[q] & 0xFFFFu;
                    const u32 hi16 = ex;
                    ex += w[q] >> 16;
                    if (q < (int)WPT && i < I3_NB / 2) cnt16[i] = lo16 | (hi16 << 16);
                }
            }
            // the next item's ranges (loaded at the top of this batch)
            if (tid < 2 * (u32)a.n) {
                if (lane & 1) rng[st.par ^ 1u][og].y = voff; else rng[st.par ^ 1u][og].x = voff;
            }
            __syncthreads();                                                        // (3) bins, next ranges
        } else {
            // ===== keys of genome st.g over the item's buckets: probe.  A bin averages well under one head, so the
            // first FOUR heads of the key's bin are read unconditionally (no data-dependent branch on the common
            // path, the LDS latencies of a thread's four keys overlap); what is left -- a key beyond the fourth head
            // of a crowded bin, one in a thousand -- walks on in ONE loop for the thread's four keys together.
            const u32 cnt = item_cnt;
            const bool ing = (a.ingroup_bits >> st.g) & 1;
            const u32 left = st.e - st.i0;
            u32 h[4];             // slot found, or ~0u
            u32 wt[4];            // walk position (>= cnt: nothing to walk)
            if (!(I3_ABL & 1)) {
                // all four bin reads, then all twelve head reads, then the compares: the fences keep the compiler
                // from sinking a read into the branch that uses it (it then serves one key after the other, each
                // a chain of dependent LDS round trips)
                u32 h0[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const u64 pre = I3_KEY(R, e) & g.pmask;
                    h0[e] = reinterpret_cast<const unsigned short*>(cnt16)[i3_bin(pre, sh)];
                }
                asm volatile("" : "+v"(h0[0]), "+v"(h0[1]), "+v"(h0[2]), "+v"(h0[3]));
                // (two keys at a time: eight head reads in flight, sixteen registers)
#pragma unroll
                for (int e0 = 0; e0 < 4; e0 += 2) {
                    u64 k0[2], k1[2], k2[2], k3[2];
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        k0[j] = heads[h0[e0 + j]];
                        k1[j] = heads[h0[e0 + j] + 1];
                        k2[j] = heads[h0[e0 + j] + 2];
                        k3[j] = heads[h0[e0 + j] + 3];
                    }
                    asm volatile("" : "+v"(k0[0]), "+v"(k0[1]), "+v"(k1[0]), "+v"(k1[1]), "+v"(k2[0]), "+v"(k2[1]), "+v"(k3[0]),
                                 "+v"(k3[1]));
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const int e = e0 + j;
                        const u64 pre = I3_KEY(R, e) & g.pmask;
                        // (a lane past the batch's end holds 0 or -- odd key counts -- the first key of the NEXT bucket,
                        // larger than every head: it must neither match nor walk)
                        const bool valid = I3_POS(e) < left;
                        u32 hh = ~0u;
                        hh = k3[j] == pre ? h0[e] + 3 : hh;
                        hh = k2[j] == pre ? h0[e] + 2 : hh;
                        hh = k1[j] == pre ? h0[e] + 1 : hh;
                        hh = k0[j] == pre ? h0[e] : hh;
                        hh = valid ? hh : ~0u;       // (a stale head past the item's last slot can only 'match' into a slot nobody reads)
                        h[e] = hh;
                        wt[e] = (valid && hh == ~0u && k3[j] < pre && !(I3_ABL & 16)) ? h0[e] + 4 : ~0u;
                    }
                }
            }
            if (!(I3_ABL & 1)) {
                while ((wt[0] < cnt) | (wt[1] < cnt) | (wt[2] < cnt) | (wt[3] < cnt)) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if (wt[e] < cnt) {
                            const u64 pre = I3_KEY(R, e) & g.pmask;
                            const u64 kq = heads[wt[e]];
                            if (kq == pre) { h[e] = wt[e]; wt[e] = ~0u; }
                            else if (kq > pre) wt[e] = ~0u;
                            else wt[e]++;
                        }
                    }
                }
                if (FMT == 0 && g.D == 1) {
                    // (one diagnostic column, the usual case: presence bit | 1 << base, three instructions)
                    const int dsh = 62 - 2 * LR;
                    const u32 hiw = 1u << st.g, ish = ing ? 0u : 16u;
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (h[e] != ~0u) {
                            const u32 bb = (u32)(I3_KEY(R, e) >> dsh) & 3u;
                            atomicOr(&inm[h[e]], ((u64)hiw << 32) | (u64)(1u << (bb + ish)));
                        }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if ((I3_ABL & 64) ? h[e] == 0xFFFFFFF0u : (h[e] != ~0u && !(I3_ABL & 32)))
                            isect_update<FMT>(h[e], I3_KEY(R, e), st.g, ing, present, inm, outm, g, LR);
                }
            }
            if (nx.it != st.it && !st.over && !(I3_ABL & 2)) {
                // ===== last batch of the item: survivors, in order
                __syncthreads();                                                    // (4) probes done
                const u32 cnt = item_cnt;
                bool flag[4];
                u64 im[4], om[4], pr[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const u32 p = I3_POS(e);
                    flag[e] = false;
                    im[e] = om[e] = pr[e] = 0;
                    if (p < cnt) {
                        const u64 s2 = inm[p];
                        pr[e] = heads[p];
                        flag[e] = (FMT == 0 ? (u32)(s2 >> 32) : present[p]) == full;
                        im[e] = FMT == 2 ? s2 : (FMT == 1 ? (s2 & 0xFFFFFFFFull) : (s2 & 0xFFFFull));
                        om[e] = FMT == 2 ? outm[p] : (FMT == 1 ? (s2 >> 32) : ((s2 >> 16) & 0xFFFFull));
                        if (flag[e] && a.apply_filter && g.D > 0) flag[e] = passes_filter(im[e], om[e], g.D, a.apply_filter);
                    }
                }
#pragma unroll
                for (int q = 0; q < I3_WMAX; q++) {
                    const u32 i = tid * WPT + q;
                    if (q < (int)WPT && i < I3_NB / 2) cnt16[i] = 0;                // the next item counts from zero
                }
                const u32 c0 = (flag[0] ? 1u : 0u) + (flag[1] ? 1u : 0u), c1 = (flag[2] ? 1u : 0u) + (flag[3] ? 1u : 0u);
                u32 total;
                const u32 ex = block_excl_scan1<8>(c0 | (c1 << 16), waves, total);   // (5) inside
                const u32 tot0 = total & 0xFFFFu, nsurv = tot0 + (total >> 16);
                if (nsurv) {
                    u32 pos[4];
                    pos[0] = ex & 0xFFFFu;
                    pos[1] = pos[0] + (flag[0] ? 1u : 0u);
                    pos[2] = tot0 + (ex >> 16);
                    pos[3] = pos[2] + (flag[2] ? 1u : 0u);
                    const bufrsrc ws = make_rsrc(a.tmp + item_sa, cnt * (u32)sizeof(kr_cand));
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const u32 o = flag[e] ? pos[e] * (u32)sizeof(kr_cand) : BUF_OOB;
                        u32x4 v;
                        v.x = (u32)pr[e]; v.y = (u32)(pr[e] >> 32); v.z = (u32)im[e]; v.w = (u32)(im[e] >> 32);
                        __builtin_amdgcn_raw_buffer_store_b128(v, ws, o, 0, 0);
                        buf_store_u64(om[e], ws, flag[e] ? o + 16 : BUF_OOB);
                    }
                }
                if (tid == 0) a.itemcnt[st.it] = nsurv;
            }
        }
    };

    for (;;) {
        I3State nxt = cur;
        if (cur.g < 0) {
            const u32 ni = cur.it + G < a.nitems ? cur.it + G : 0u;
            voff = myoff[item_bucket(ni, lane & 1)];
        }
        i3_advance(nxt, a, rng, S, G);
        i3_issue(Y, a, keyp, nxt, T);
        process(X, cur, nxt);
        cur = nxt;
        if (cur.it >= a.nitems) break;
        if (cur.g < 0) {
            const u32 ni = cur.it + G < a.nitems ? cur.it + G : 0u;
            voff = myoff[item_bucket(ni, lane & 1)];
        }
        i3_advance(nxt, a, rng, S, G);
        i3_issue(X, a, keyp, nxt, T);
        process(Y, cur, nxt);
        cur = nxt;
        if (cur.it >= a.nitems) break;
    }
}

// dense, ordered candidate list from the per-item runs of k_intersect3: a workgroup of GI_T threads per GI_ITEMS items.
// Two shapes of list come here.  Without the filter most items hold no survivor: a workgroup whose items hold none reads
// two prefix sums and leaves.  The filtered list of a sorted pair holds something in nearly every item (1.16e6 entries in
// 48 000 items at 2 x 50 Mbp): the workgroup scans its counts in LDS and its threads walk its OUTPUTS, entry by entry, each
// finding its item in the prefix sums (gi_index.inc) -- every lane moves an entry in every trip, where a wave per item
// kept as many lanes busy as the item had entries (about 24 of 64).
#include "gi_index.inc"
#define GI_T 256
__global__ __launch_bounds__(GI_T) void k_gather_items(int sbits, u32 slice, const kr_cand* __restrict__ tmp,
                                                      const u32* __restrict__ offA, int mlog, u32 nb,
                                                      const u32* __restrict__ itemcnt, const u32* __restrict__ itempos,
                                                      kr_cand* __restrict__ out, u32 nunits, u32 cap) {
    if (itempos[nunits] > cap) return;               // (as k_gather_cands)
    const u32 tid = threadIdx.x, first = blockIdx.x * GI_ITEMS;
    const u32 last = first + GI_ITEMS < nunits ? first + GI_ITEMS : nunits;
    const u32 dst = itempos[first], total = itempos[last] - dst;
    if (total == 0) return;                          // (the sparse list: nothing to scan)
    __shared__ u32 pre[GI_ITEMS + 1], srcs[GI_ITEMS];
    if (tid < GI_ITEMS) {                            // (one wave: the scan needs no barrier of its own)
        const u32 it = first + tid;
        const u32 n = it < nunits ? itemcnt[it] : 0u;
        const u64 f = (u64)it << mlog;
        srcs[tid] = n ? offA[f < nb ? f : nb] : 0u;
        u32 s = n;
#pragma unroll
        for (u32 d = 1; d < GI_ITEMS; d <<= 1) {
            const u32 t = __shfl_up(s, d, 64);
            if (tid >= d) s += t;
        }
        pre[tid + 1] = s;
        if (tid == 0) pre[0] = 0;
    }
    __syncthreads();
    const u64 top = sbits ? ((u64)slice << (64 - sbits)) : 0;
    for (u32 o = tid; o < total; o += GI_T) {
        const GiSlot at = gi_slot(pre, o);
        kr_cand c = tmp[(u64)srcs[at.item] + at.offset];
        c.prefix = top | (c.prefix >> sbits);          // relative -> absolute prefix
        out[dst + o] = c;
    }
}
