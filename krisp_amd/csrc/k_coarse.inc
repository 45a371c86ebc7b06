// k_coarse.inc -- part of krisp_hip.hip (one translation unit): a genome that stopped behind pass 1 (256 buckets by the top
// byte of the key: kr_genome_partition) answers a short candidate list without a fine partition.
//
// The list C -- the filtered intersection of the sorted genomes of the call, ascending by prefix -- holds about 1 % of a
// genome's prefixes.  The candidates of ONE top byte (some thousands) fit a hash table in LDS; the genome's keys of that
// byte stream past it once, in whatever order pass 1 left them.  A key under a candidate's prefix ORs the genome's
// presence bit and its diagnostic base into the candidate's state word and joins the genome's hit list -- all that
// kr_collect will ask of this genome.  Exact: a slot's 19-bit tag only gates the look at the candidate's full prefix.

#define CO_T 1024               // threads of k_coarse_probe: two workgroups per CU (8 waves per SIMD, <= 64 VGPRs, 2 x 68 KB LDS)
#define CO_SLOT_LOG 13
#define CO_SLOTS (1u << CO_SLOT_LOG)    // LDS slots: idx << 19 | tag, CO_EMPTY = free
#define CO_BM_LOG 17            // bits of the prefilter in front of the table: 2^17
#define CO_QCAP 1024            // keys of one iteration that passed the prefilter (more: looked up in place)
#define CO_TCAP 6144            // candidates one table takes (three quarters of the slots; idx << 19 | tag never equals CO_EMPTY);
                                // a top byte with more of them is streamed once per CO_TCAP candidates ("rounds")
#define CO_CHUNK 32768u         // keys of one work unit (even: a unit's 16-byte loads keep the parity of the bucket's base)
#define CO_EMPTY 0xFFFFFFFFu
#define CO_UNROLL 4             // 16-byte loads a thread has in flight: 8192 keys per iteration of a workgroup
#define CO_HB 1024              // hits a workgroup gathers in LDS before it takes room in the genome's list (one global atomic per unit)
#define CO_MAXG 24              // genomes of a call on this route: 8 bits of diagnostic sets + 24 presence bits in one state word

// state word of a candidate: bits 0..3 the bases its column shows in coarse ingroup genomes, 4..7 in coarse outgroup
// genomes, bit 8 + j: coarse genome j holds the prefix
__device__ __forceinline__ u32 co_hash(u64 pre) {
    const u32 y = (u32)pre * 0x9E3779B1u;
    return ((u32)(pre >> 32) ^ y) * 0x85EBCA6Bu;
}

// cb[t] = first candidate whose prefix has a top byte >= t (t = 0 .. 256), and the work units of one genome:
// ust[t] = units in front of top byte t; a top byte has rounds x chunks units, the chunk varying fastest
__global__ __launch_bounds__(256) void k_coarse_tables(const kr_cand* __restrict__ cands, u32 n, const u32* __restrict__ base,
                                                       u32 tcap, u32* __restrict__ cb, u32* __restrict__ ust) {
    __shared__ u32 waves[17];
    __shared__ u32 s_cb[257];
    for (u32 t = threadIdx.x; t <= 256; t += 256) {
        u32 l = 0, r = n;
        if (t == 256) l = n;
        else {
            const u64 bound = (u64)t << 56;
            while (l < r) {
                const u32 mid = l + ((r - l) >> 1);
                if (cands[mid].prefix < bound) l = mid + 1; else r = mid;
            }
        }
        s_cb[t] = l;
        cb[t] = l;
    }
    __syncthreads();
    const u32 t = threadIdx.x;
    const u32 nc = s_cb[t + 1] - s_cb[t], len = base[t + 1] - base[t];
    const u32 units = ((nc + tcap - 1) / tcap) * ((len + CO_CHUNK - 1) / CO_CHUNK);
    u32 total;
    const u32 ex = block_excl_scan(units, waves, total);
    ust[t] = ex;
    if (t == 0) ust[256] = total;
}

// One key against the table of the round (linear probing from the hash's top bits; a slot's tag gates the look at the
// candidate's full prefix): a key under a candidate's prefix joins the unit's hits in LDS (the excess of a unit with more
// than CO_HB of them goes straight to the list) and ORs presence + diagnostic base into the candidate's state word
__device__ __forceinline__ void co_lookup(u64 key, u64 pmask, int LR, const u32* slots, u32 c0, const kr_cand* __restrict__ cands,
                                          u32* __restrict__ state, u32 orbits, u32 side_shift, u64* s_hit, u32* s_nhit,
                                          u32* __restrict__ hits, u64* __restrict__ hitkeys, u32 hitcap) {
    const u64 pre = key & pmask;
    const u32 h = co_hash(pre);
    const u32 tag = h & 0x7FFFFu;
    u32 s = h >> (32 - CO_SLOT_LOG);
    for (u32 w = slots[s]; w != CO_EMPTY; w = slots[s]) {
        if ((w & 0x7FFFFu) == tag) {
            const u32 ci = c0 + (w >> 19);
            if (cands[ci].prefix == pre) {
                const u32 at0 = atomicAdd(s_nhit, 1u);
                if (at0 < CO_HB) s_hit[at0] = key;
                else {
                    const u32 pos = atomicAdd(hits, 1u);
                    if (pos < hitcap) hitkeys[pos] = key;
                }
                const u32 bb = (u32)(key >> (62 - 2 * LR)) & 3u;
                atomicOr(&state[ci], orbits | (1u << (side_shift + bb)));
                return;
            }
        }
        s = (s + 1) & (CO_SLOTS - 1);
    }
}

// persistent: workgroup w takes the units [w U / W, (w + 1) U / W) -- neighbours in a top byte, so a table is built once
// per workgroup and top byte (twice at the seams).  hits: u32 count at word 0, keys from byte 16; the count runs on past
// `hitcap` (nothing is written there): the host reads it and sorts the genome fine instead.
//
// Two phases per iteration (2 CO_T CO_UNROLL keys).  About 1 % of the keys hit, so nearly every wave holds a hit: a look-up inside the stream
// would run its dependent chain (slot, tag, the candidate's prefix in global memory) in every wave for one lane's sake.
// Phase 1 only tests a bit of a 2^17-bit prefilter in LDS (set by the candidates' hashes: 3-7 % of the keys pass) and
// queues what passes; phase 2 looks the queued keys up, a thread per key, densely.  A unit's hits gather in LDS and take
// their room in the list with ONE atomic per unit (an atomic per hit wave on the single count word ran at that word's
// ~90 atomics per microsecond: 7.7 ms per genome).
__global__ __launch_bounds__(CO_T, 8) void k_coarse_probe(const u64* __restrict__ keys, const u32* __restrict__ base,
                                                       const u32* __restrict__ cb, const u32* __restrict__ ust,
                                                       const kr_cand* __restrict__ cands, u32* __restrict__ state,
                                                       u32* __restrict__ hits, u32 hitcap, u32 tcap, u32 gbit, u32 side_shift,
                                                       u64 pmask, int LR) {
    __shared__ u32 slots[CO_SLOTS];
    __shared__ u32 bitmap[1u << (CO_BM_LOG - 5)];
    __shared__ u32 s_base[257], s_cb[257], s_ust[257];
    __shared__ u64 s_q[CO_QCAP];
    __shared__ u64 s_hit[CO_HB];
    __shared__ u32 s_nhit, s_hbase, s_qn;
    if (threadIdx.x == 0) { s_nhit = 0; s_qn = 0; }
    for (u32 t = threadIdx.x; t <= 256; t += CO_T) { s_base[t] = base[t]; s_cb[t] = cb[t]; s_ust[t] = ust[t]; }
    __syncthreads();
    const u32 U = s_ust[256];
    const u32 u0 = (u32)(((u64)blockIdx.x * U) / gridDim.x), u1 = (u32)(((u64)(blockIdx.x + 1) * U) / gridDim.x);
    u64* __restrict__ hitkeys = (u64*)(hits + 4);
    const u32 orbits = 1u << (8 + gbit);
    u32 cur_t = ~0u, cur_r = ~0u, c0 = 0;
    for (u32 u = u0; u < u1; u++) {
        u32 lo = 0, hi = 256;                            // largest t with ust[t] <= u and units of its own
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_ust[mid] <= u) lo = mid; else hi = mid;
        }
        const u32 t = lo;
        const u32 b0 = s_base[t], b1 = s_base[t + 1];
        const u32 chunks = (b1 - b0 + CO_CHUNK - 1) / CO_CHUNK;
        const u32 r = (u - s_ust[t]) / chunks, ch = (u - s_ust[t]) - r * chunks;
        if (t != cur_t || r != cur_r) {
            cur_t = t;
            cur_r = r;
            // (the look-ups in the table before are done: every unit ends with a barrier)
            for (u32 i = threadIdx.x; i < CO_SLOTS; i += CO_T) slots[i] = CO_EMPTY;
            for (u32 i = threadIdx.x; i < (1u << (CO_BM_LOG - 5)); i += CO_T) bitmap[i] = 0;
            __syncthreads();
            c0 = s_cb[t] + r * tcap;
            const u32 c1 = min(s_cb[t + 1], c0 + tcap);
            for (u32 i = c0 + threadIdx.x; i < c1; i += CO_T) {
                const u32 h = co_hash(cands[i].prefix);
                const u32 word = ((i - c0) << 19) | (h & 0x7FFFFu);
                u32 s = h >> (32 - CO_SLOT_LOG);
                while (atomicCAS(&slots[s], CO_EMPTY, word) != CO_EMPTY) s = (s + 1) & (CO_SLOTS - 1);
                atomicOr(&bitmap[h >> (37 - CO_BM_LOG)], 1u << ((h >> (32 - CO_BM_LOG)) & 31u));
            }
            __syncthreads();
        }
        const u32 k0 = b0 + ch * CO_CHUNK, k1 = min(b1, k0 + CO_CHUNK);
        const u32 a0 = k0 & ~1u;                         // (16-byte aligned; key a0 may lie in front of the unit, key k1 behind it:
                                                         //  both inside the array, which has two keys of slack, and masked below)
        for (u32 p0 = a0; p0 < k1; p0 += 2 * CO_T * CO_UNROLL) {
            u32x4 v[CO_UNROLL];
            u32 at[CO_UNROLL];
#pragma unroll
            for (int q = 0; q < CO_UNROLL; q++) {
                const u32 p = p0 + 2 * (q * CO_T + threadIdx.x);
                at[q] = p;
                const u32 pc = p < k1 ? p : a0;          // (clamped, never predicated: the loads of a thread stay in flight together)
                v[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(keys + pc));
            }
            // phase 1
#pragma unroll
            for (int q = 0; q < CO_UNROLL; q++) {
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const u64 key = e ? ((u64)v[q].w << 32 | v[q].z) : ((u64)v[q].y << 32 | v[q].x);
                    const u32 idx = at[q] + e;
                    const u32 h = co_hash(key & pmask);
                    const u32 bw = bitmap[h >> (37 - CO_BM_LOG)];
                    if (idx >= k0 && idx < k1 && ((bw >> ((h >> (32 - CO_BM_LOG)) & 31u)) & 1u)) {
                        const u32 qa = atomicAdd(&s_qn, 1u);
                        if (qa < CO_QCAP) s_q[qa] = key;
                        else co_lookup(key, pmask, LR, slots, c0, cands, state, orbits, side_shift, s_hit, &s_nhit, hits, hitkeys, hitcap);
                    }
                }
            }
            // phase 2
            __syncthreads();
            const u32 qn = min(s_qn, (u32)CO_QCAP);
            __syncthreads();                             // (every thread has read the count)
            if (threadIdx.x == 0) s_qn = 0;
            for (u32 i = threadIdx.x; i < qn; i += CO_T)
                co_lookup(s_q[i], pmask, LR, slots, c0, cands, state, orbits, side_shift, s_hit, &s_nhit, hits, hitkeys, hitcap);
            __syncthreads();                             // (the queue is free, its count is zero)
        }
        // the unit's hits from LDS into the list
        const u32 m = min(s_nhit, (u32)CO_HB);
        __syncthreads();                                 // (every thread has read the count: it is the same in all of them)
        if (m) {
            if (threadIdx.x == 0) { s_hbase = atomicAdd(hits, m); s_nhit = 0; }
            __syncthreads();
            const u32 hb = s_hbase;
            for (u32 i = threadIdx.x; i < m; i += CO_T)
                if (hb + i < hitcap) hitkeys[hb + i] = s_hit[i];
            __syncthreads();                             // (the next unit's hits come behind the copy and the reset)
        }
    }
}

// the list C against the state words: a candidate stays when every coarse genome holds it (`need` = their presence bits)
// and the filter passes on the completed masks.  flags / blockcnt as k_cands_flag leaves them
__global__ void k_coarse_flag(kr_cand* __restrict__ cur, u32 n, const u32* __restrict__ state, u32 need, int mode,
                              u32* __restrict__ flags, u32* __restrict__ blockcnt) {
    __shared__ u32 waves[17];
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const u32 st = state[i];
        keep = (st & need) == need;
        if (keep) {
            kr_cand c = cur[i];
            c.in_mask |= st & 15u;
            c.out_mask |= (st >> 4) & 15u;
            keep = passes_filter(c.in_mask, c.out_mask, 1, mode);
            if (keep) cur[i] = c;
        }
        flags[i] = keep ? 1u : 0u;
    }
    u32 tot;
    block_compact(keep, waves, tot);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = tot;
}

// ... and the hit counts of up to CO_MAXG genomes into the host mailbox
struct CoarsePub { const u32* cnt[CO_MAXG]; int n; };
__global__ void k_coarse_publish(CoarsePub p, u32* __restrict__ host) {
    if (blockIdx.x == 0 && (int)threadIdx.x < p.n) host[threadIdx.x] = *p.cnt[threadIdx.x];
}

// kr_collect: the arena rows of the (candidate, coarse genome) pairs from the genome's hit list.  A hit finds its
// candidate in the CURRENT list (ascending; what is left of C -- most hits belong to candidates that fell since) and
// takes a place in the pair's row; k_coarse_rowsort then leaves the row ascending, as k_collect_scan leaves its rows.
// A row with more than COL_CAPM keys raises *overflow (the host sorts the genomes whole: the route of k_collect_scan).
__global__ __launch_bounds__(256) void k_coarse_rows(const u32* __restrict__ hits, u32 hitcap, const kr_cand* __restrict__ cands,
                                                     u32 nc, u32 n, u32 gi, u64 pmask, u64* __restrict__ arena,
                                                     u32* __restrict__ mcnt) {
    const u32 nh = min(hits[0], hitcap);
    const u64* __restrict__ hk = (const u64*)(hits + 4);
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nh; i += gridDim.x * blockDim.x) {
        const u64 key = hk[i], pre = key & pmask;
        u32 l = 0, r = nc;
        while (l < r) {
            const u32 mid = l + ((r - l) >> 1);
            if (cands[mid].prefix < pre) l = mid + 1; else r = mid;
        }
        if (l < nc && cands[l].prefix == pre) {
            const u32 row = l * n + gi;
            const u32 at = atomicAdd(&mcnt[row], 1u);
            if (at < COL_CAPM) arena[(u64)row * COL_CAPM + at] = key;
        }
    }
}

__global__ __launch_bounds__(256) void k_coarse_rowsort(u32 npairs, u32 n, const u32* __restrict__ ibo, u64* __restrict__ arena,
                                                        u32* __restrict__ mcnt, u32* __restrict__ overflow) {
    const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npairs || ibo[idx % n] != 2u) return;
    const u32 m = mcnt[idx];
    if (m > COL_CAPM) {
        atomicAdd(overflow, 1u);
        mcnt[idx] = 0;
        return;
    }
    u64* __restrict__ K = arena + (u64)idx * COL_CAPM;
    for (u32 i = 1; i < m; i++) {                        // (a handful of keys, usually one)
        const u64 key = K[i];
        u32 j = i;
        for (; j > 0 && K[j - 1] > key; j--) K[j] = K[j - 1];
        K[j] = key;
    }
}

// kr_genome_partition: the top-byte buckets' bases out of the lane's scratch into the genome's own offsets array
// (off[0 .. 256]), and the two words finalize() reads of a slice -- off[nb] = the key count, ovf[0] = no oversized bucket
__global__ void k_coarse_keep(const u32* __restrict__ base1, u32* __restrict__ off, u32 nb, u32* __restrict__ ovf) {
    const u32 t = threadIdx.x;
    if (t <= 256) off[t] = base1[t];
    else if (t == 257) off[nb] = base1[256];
    else if (t == 258) ovf[0] = 0;
}
