// k_coarse.inc -- part of krisp_hip.hip (one translation unit): a genome that stopped behind pass 1 (256 buckets by the top
// byte of the key: kr_genome_partition) answers a short candidate list without a fine partition.
//
// The list C -- the filtered intersection of the sorted genomes of the call, ascending by prefix -- holds about 1 % of a
// genome's prefixes.  The candidates of ONE top byte (some thousands) fit a hash table in LDS; the genome's keys of that
// byte stream past it once, in whatever order pass 1 left them.  A key under a candidate's prefix ORs the genome's
// presence bit and its diagnostic base into the candidate's state word and joins the genome's hit list -- all that
// kr_collect will ask of this genome.  Exact: a slot's 19-bit tag only gates the look at the candidate's full prefix.

#include "co_units.inc"        // CO_CHUNK, the numbering of the work units and its decode (shared with a host check)
#include "co_pass.inc"         // co_hash, CO_BM_LOG and the prefilter's bits, the 16-bit slots and the passes of the one-strand form

#define CO_T 1024               // threads of k_coarse_probe: two workgroups per CU (8 waves per SIMD, <= 64 VGPRs, 2 x 75 KB LDS)
#define CO_SLOT_LOG 13
#define CO_SLOTS (1u << CO_SLOT_LOG)    // LDS slots: idx << 19 | tag, CO_EMPTY = free
#define CO_QCAP 2048            // keys of one unit that passed the prefilter (more: the unit is looked up in place)
#define CO_TCAP 6144            // candidates one table takes (three quarters of the slots; idx << 19 | tag never equals CO_EMPTY);
                                // a top byte with more of them is streamed once per CO_TCAP candidates ("rounds")
#define CO_EMPTY 0xFFFFFFFFu
#define CO_UNROLL 4             // 16-byte loads of one register set: 8192 keys per iteration of a workgroup; two sets (A / B)
#define CO_ITER (2u * CO_T * CO_UNROLL)
#define CO_HB 1024              // hits a workgroup gathers in LDS before it takes room in the genome's list (one global atomic per unit)
#define CO_MAXG 24              // genomes of a call on this route: 8 bits of diagnostic sets + 24 presence bits in one state word
#define CO_ROW (2 * CO_MAXG)    // words of a top byte's row: every genome's bucket [b0, b1) (co_units.inc)

// the coarse genomes of one call, one launch for all of them
struct CoarseArgs {
    const u64* keys[CO_MAXG];   // pass 1's output
    const u32* off[CO_MAXG];    // its 257 bucket offsets
    u32* hits[CO_MAXG];         // hit list: u32 count at word 0, keys from byte 16
    u32 hitcap[CO_MAXG];
    u32 bit[CO_MAXG];           // the genome's presence bit in the state word
    u32 side[CO_MAXG];          // 0: ingroup, 4: outgroup -- where its diagnostic bases go in the state word
    u32 n;
};

// state word of a candidate: bits 0..3 the bases its column shows in coarse ingroup genomes, 4..7 in coarse outgroup
// genomes, bit 8 + j: coarse genome j holds the prefix
// (co_hash: co_pass.inc)

// cb[t] = first candidate whose prefix has a top byte >= t (t = 0 .. 256); rows[t] = the buckets of top byte t in every
// genome; ust[t] = units in front of top byte t (co_units.inc).  Also clears the genomes' hit counts.
__global__ __launch_bounds__(256) void k_coarse_tables(const kr_cand* __restrict__ cands, u32 n, CoarseArgs A, u32 tcap,
                                                       u32* __restrict__ cb, u32* __restrict__ ust, u32* rows) {
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
    if (t < 4 * A.n) A.hits[t >> 2][t & 3u] = 0;
    u32* row = rows + t * CO_ROW;
    for (u32 j = 0; j < A.n; j++) {
        row[2 * j] = A.off[j][t];
        row[2 * j + 1] = A.off[j][t + 1];
    }
    const u32 units = co_byte_units(s_cb[t + 1] - s_cb[t], tcap, row, A.n);
    u32 total;
    const u32 ex = block_excl_scan(units, waves, total);
    ust[t] = ex;
    if (t == 0) ust[256] = total;
}

// ---- one-strand form (co_strand.inc): pass 1 wrote the forward record of every window, in 256 buckets by cs_digit.  The
// candidates a key of digit d can meet are two classes -- class 2 d: those whose prefix read forward shows d, class 2 d + 1:
// those whose reverse complement does -- and a round of the probe is one reading of up to tcap candidates of one class:
// its entries (pattern, candidate) against key & mask (pmask / mask_rc).  The three kernels below take k_coarse_tables'
// place: count the classes, scan them (+ rows, units, cleared hit counts), fill the entry array.
#define CS_CLS 512
#define CS_T 1024               // threads of k_strand_count / k_strand_fill: one workgroup per CU at most -- every workgroup ends with
                                // CS_CLS global atomics on the same CS_CLS words, and those run one after the other
struct CoEnt { u64 pat; u32 ci, pad; };

// h[c] += 1 for every active lane, where the lanes of a wave hold equal c in RUNS (the list ascends by prefix, so
// neighbours share their forward class: 64 single adds to one LDS word would run one after the other): the first lane of
// a run adds its length.  -> what the lane's own add would have returned.  Call with all 64 lanes.
__device__ __forceinline__ u32 co_run_add(u32* h, u32 c, bool active) {
    const u32 lane = threadIdx.x & 63u;
    if (!active) c = 0xFFFFFFFFu;
    const u32 prev = (u32)__shfl_up((int)c, 1);
    const bool head = lane == 0 || prev != c;
    const u64 hb = __builtin_amdgcn_ballot_w64(head);
    const u32 leader = 63u - (u32)__clzll((long long)(hb & ((2ull << lane) - 1ull)));      // (bit 0 is set: lane 0 is a head)
    const u64 above = (hb >> lane) >> 1;
    const u32 len = above ? (u32)__builtin_ctzll(above) + 1u : 64u - lane;
    u32 r0 = 0;
    if (head && active) r0 = atomicAdd(&h[c], len);
    return (u32)__shfl((int)r0, (int)leader) + (lane - leader);
}

// cnt[CS_CLS] (zeroed by the host) += the candidates of every class
__global__ __launch_bounds__(CS_T) void k_strand_count(const kr_cand* __restrict__ cands, u32 n, CoStrand S, u32* __restrict__ cnt) {
    __shared__ u32 h[CS_CLS];
    if (threadIdx.x < CS_CLS) h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 i0 = blockIdx.x * CS_T; i0 < n; i0 += gridDim.x * CS_T) {
        const u32 i = i0 + threadIdx.x;
        const bool on = i < n;
        const u64 P = cands[on ? i : n - 1].prefix;
        (void)co_run_add(h, 2 * cs_class_fwd(S, P), on);
        if (on) atomicAdd(&h[2 * cs_class_rev(S, P) + 1], 1u);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < CS_CLS; t += CS_T)
        if (h[t]) atomicAdd(&cnt[t], h[t]);
}

// cls[t] = entries in front of class t (cls[CS_CLS] = 2 n), cursor[] = the same, for k_strand_fill; rows[d] = the buckets of
// digit d in every genome; ust[d] = units in front of digit d: co_byte_units over passes * tcap candidates -- what
// co_units.inc decodes as a unit's round is its PASS (co_pass.inc: forward round p beside reverse round p, or with
// one_pass = 0 one round after the other).  Also clears the genomes' hit counts.
__global__ __launch_bounds__(CS_CLS) void k_strand_tables(const u32* __restrict__ cnt, CoarseArgs A, u32 tcap, u32* __restrict__ cls,
                                                          u32* __restrict__ cursor, u32* __restrict__ ust, u32* rows,
                                                          u32* __restrict__ host_rounds, u32 one_pass) {
    __shared__ u32 waves[17];
    const u32 t = threadIdx.x;
    u32 total;
    const u32 ex = block_excl_scan(cnt[t], waves, total);
    cls[t] = ex;
    cursor[t] = ex;
    if (t == 0) cls[CS_CLS] = total;
    if (t < 4 * A.n) A.hits[t >> 2][t & 3u] = 0;
    u32 units = 0, rf = 0, rr = 0, np = 0;
    if (t < 256) {
        u32* row = rows + t * CO_ROW;
        for (u32 j = 0; j < A.n; j++) {
            row[2 * j] = A.off[j][t];
            row[2 * j + 1] = A.off[j][t + 1];
        }
        rf = co_rounds(cnt[2 * t], tcap);
        rr = co_rounds(cnt[2 * t + 1], tcap);
        np = co_pass_count(cnt[2 * t], cnt[2 * t + 1], tcap, one_pass);
        units = co_byte_units(np * tcap, tcap, row, A.n);
        if (co_row_chunks(row, A.n) == 0) rf = rr = np = 0;  // (a digit without keys: no round is run)
    }
    const u32 ux = block_excl_scan(units, waves, total);
    if (t < 256) ust[t] = ux;
    if (t == 0) ust[256] = total;
    // the forward and the reverse rounds of the call and its passes, for the host's counters (kr_debug_coarse_strand)
    (void)block_excl_scan(rf, waves, total);
    if (t == 0) host_rounds[0] = total;
    (void)block_excl_scan(rr, waves, total);
    if (t == 0) host_rounds[1] = total;
    (void)block_excl_scan(np, waves, total);
    if (t == 0) host_rounds[2] = total;
}

// the entries into their classes: a workgroup counts its candidates' classes in LDS, takes its room in each class with one
// atomic, and places its entries (their order inside a class is free: a round's table is a set)
__global__ __launch_bounds__(CS_T) void k_strand_fill(const kr_cand* __restrict__ cands, u32 n, CoStrand S, u32* __restrict__ cursor,
                                                     CoEnt* __restrict__ ents) {
    __shared__ u32 h[CS_CLS], base[CS_CLS];
    if (threadIdx.x < CS_CLS) h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 i0 = blockIdx.x * CS_T; i0 < n; i0 += gridDim.x * CS_T) {
        const u32 i = i0 + threadIdx.x;
        const bool on = i < n;
        const u64 P = cands[on ? i : n - 1].prefix;
        (void)co_run_add(h, 2 * cs_class_fwd(S, P), on);
        if (on) atomicAdd(&h[2 * cs_class_rev(S, P) + 1], 1u);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < CS_CLS; t += CS_T) {
        base[t] = h[t] ? atomicAdd(&cursor[t], h[t]) : 0u;
        h[t] = 0;
    }
    __syncthreads();
    for (u32 i0 = blockIdx.x * CS_T; i0 < n; i0 += gridDim.x * CS_T) {
        const u32 i = i0 + threadIdx.x;
        const bool on = i < n;
        const u64 P = cands[on ? i : n - 1].prefix;
        const u32 cf = 2 * cs_class_fwd(S, P), cr = 2 * cs_class_rev(S, P) + 1;
        const u32 rank = co_run_add(h, cf, on);
        if (!on) continue;
        CoEnt e;
        e.ci = i;
        e.pad = 0;
        e.pat = P;
        ents[base[cf] + rank] = e;
        e.pat = cs_pattern_rev(S, P);
        ents[base[cr] + atomicAdd(&h[cr], 1u)] = e;
    }
}

// One key against the table at hand (linear probing from the hash's top bits; a slot's tag gates the look at the
// candidate's full prefix).  A hit -- where it goes: the unit's genome -- joins the unit's hits in LDS (the excess of a
// unit with more than CO_HB of them goes straight to the list) and ORs presence + diagnostic base into the candidate's
// state word
struct CoHitSink {
    u32* __restrict__ state;
    u32 orbits, side_shift;
    u64* s_hit;
    u32* s_nhit;
    u32* __restrict__ hits;
    u64* __restrict__ hitkeys;
    u32 hitcap;
    int LR;
};
__device__ __forceinline__ void co_hit(const CoHitSink& K, u64 key, u32 ci) {
    const u32 at0 = atomicAdd(K.s_nhit, 1u);
    if (at0 < CO_HB) K.s_hit[at0] = key;
    else {
        const u32 pos = atomicAdd(K.hits, 1u);
        if (pos < K.hitcap) K.hitkeys[pos] = key;
    }
    const u32 bb = (u32)(key >> (62 - 2 * K.LR)) & 3u;
    atomicOr(&K.state[ci], K.orbits | (1u << (K.side_shift + bb)));
}

// the two-strand form: a key lies under one candidate at most
__device__ __forceinline__ void co_lookup(u64 key, u64 pmask, const u32* slots, u32 c0, const kr_cand* __restrict__ cands,
                                          const CoHitSink& K) {
    const u64 pre = key & pmask;
    const u32 h = co_hash(pre);
    const u32 tag = h & 0x7FFFFu;
    u32 s = h >> (32 - CO_SLOT_LOG);
    for (u32 w = slots[s]; w != CO_EMPTY; w = slots[s]) {
        if ((w & 0x7FFFFu) == tag) {
            const u32 ci = c0 + (w >> 19);
            if (cands[ci].prefix == pre) {
                co_hit(K, key, ci);
                return;
            }
        }
        s = (s + 1) & (CO_SLOTS - 1);
    }
}

// the one-strand form (co_pass.inc): the table holds the pass's forward and reverse entries by the hash of pattern & M, in
// 16-bit slots.  The walk goes on to the first empty slot: entries with equal pattern & M are neighbours, and a key may lie
// under one forward AND one reverse entry.  A forward entry is compared with key & pmask and lists the key; a reverse entry
// is compared with key & mask_rc and the hit is the window's REVERSE record: its key goes to the list, its base to the state
__device__ __forceinline__ void co_lookup16(u64 key, u64 fm, u64 pmask, const uint16_t* slots, const CoPass& P,
                                            const CoEnt* __restrict__ ents, const CoStrand& S, const CoHitSink& K) {
    const u32 h = co_hash(key & fm);
    const u32 tag = co_slot16_tag(h);
    u32 s = co_slot16_home(h);
    for (u32 w = slots[s]; w != CO_SLOT16_EMPTY; w = slots[s]) {
        if (co_slot16_tagof(w) == tag) {
            const u32 i = co_slot16_idx(w);
            const bool fw = i < P.nf;
            const CoEnt en = ents[fw ? P.c0f + i : P.c0r + (i - P.nf)];
            if (en.pat == (key & (fw ? pmask : S.mask_rc))) co_hit(K, fw ? key : cs_rev_key(S, key), en.ci);
        }
        s = (s + 1) & ((1u << CO_SLOT16_LOG) - 1u);
    }
}

// an entry into the 16-bit table: a CAS on the 32-bit word that holds the free slot
__device__ __forceinline__ void co_insert16(u32* slots, u32 h, u32 idx) {
    const u32 val = co_slot16(idx, co_slot16_tag(h));
    u32 s = co_slot16_home(h);
    for (;;) {
        u32* w = slots + (s >> 1);
        const u32 sh = (s & 1u) * 16u;
        const u32 old = *(volatile u32*)w;
        if (((old >> sh) & 0xFFFFu) != CO_SLOT16_EMPTY) {
            s = (s + 1) & ((1u << CO_SLOT16_LOG) - 1u);
            continue;
        }
        // (lost against a neighbour's insert into either half of the word: the same slot is looked at again)
        if (atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (val << sh)) == old) return;
    }
}

// one register set: the iteration at p0 of the unit [.., k1) whose first aligned key is a0.  Clamped into the unit, never
// predicated: the loads of a thread stay in flight together, and none reads behind the unit's (16-byte rounded) end --
// key a0 may lie in front of the unit, key k1 behind it: both inside the array, which has two keys of slack
__device__ __forceinline__ void co_load(u32x4 (&v)[CO_UNROLL], const u64* __restrict__ keys, u32 p0, u32 a0, u32 k1) {
#pragma unroll
    for (int q = 0; q < CO_UNROLL; q++) {
        const u32 p = p0 + 2 * (q * CO_T + threadIdx.x);
        const u32 pc = p < k1 ? p : a0;
        v[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(keys + pc));
    }
}

#define CO_RFL(x) ((u32)__builtin_amdgcn_readfirstlane((int)(x)))

// persistent: workgroup w takes the units [w U / W, (w + 1) U / W) of ALL coarse genomes of the call (co_units.inc: top
// byte -> round -> genome -> chunk) -- neighbours in a (top byte, round), so a table is built once per workgroup and
// round (twice at the seams) and every genome's keys of the byte stream past it.  hits: the count runs on past `hitcap`
// (nothing is written there): the host reads it and sorts the genomes fine instead.
//
// The key stream is software-pipelined over two register sets: the loads of the NEXT iteration -- of this unit, or the
// first of the workgroup's next unit while it lies in the same top byte (its genome's bucket is in the row in LDS) -- are
// issued before phase 1 of this one, so 64 KB per workgroup are in flight while it computes.  A new top byte starts cold:
// its row and its table are fetched first anyway.
//
// Phase 1 (per iteration) only tests the two bits of a key's hash in a 2^17-bit prefilter in LDS (a blocked Bloom filter
// set by the hashes of the table's entries, co_pass.inc: 2-4 % of the keys pass) and queues what passes, all key slots of
// the iteration as one batch: every read, one wait, a ballot per key slot, ONE LDS atomic by one lane for the wave, a
// lane's place from the passing lanes of the earlier slots and the lanes below it.  Phase 2 (per UNIT: its barriers and its dependent global reads would drain the prefetch) looks the
// queued keys up, a thread per key, densely; a unit that overran the queue is read again and looked up in place.  A unit's hits gather
// in LDS and take their room in the genome's list with ONE atomic per unit.
//
// OS: the one-strand form -- cb = the class bounds (k_strand_tables); what the unit numbering calls a round is a PASS
// (co_pass.inc): the forward round p and the reverse round p of the digit in one table of 16-bit slots (one_pass = 0: one
// round after the other, the same kernel).  A key is tested ONCE, under M, the bits both readings share; phase 2 asks a
// queued key both ways (co_lookup16).
template <int OS>
__global__ __launch_bounds__(CO_T, 8) void k_coarse_probe(CoarseArgs A, const u32* __restrict__ cb, const u32* __restrict__ ust,
                                                       const u32* __restrict__ rows, const kr_cand* __restrict__ cands,
                                                       u32* __restrict__ state, u32 tcap, u64 pmask0, int LR,
                                                       const CoEnt* __restrict__ ents, CoStrand S, u32 one_pass) {
    __shared__ u32 slots[CO_SLOTS];
    __shared__ u32 bitmap[1u << (CO_BM_LOG - 5)];
    __shared__ u32 s_ust[257];
    __shared__ u32 s_bnd[CO_ROW];
    __shared__ u64 s_q[CO_QCAP];
    __shared__ u64 s_hit[CO_HB];
    __shared__ u32 s_nhit, s_hbase, s_qn;
    if (threadIdx.x == 0) { s_nhit = 0; s_qn = 0; }
    for (u32 t = threadIdx.x; t <= 256; t += CO_T) s_ust[t] = ust[t];
    __syncthreads();
    const u32 G = A.n;
    const u32 U = s_ust[256];
    const u32 u0 = (u32)(((u64)blockIdx.x * U) / gridDim.x), u1 = (u32)(((u64)(blockIdx.x + 1) * U) / gridDim.x);
    if (u0 >= u1) return;
    const u32 lane = threadIdx.x & 63u;
    // the unit at hand and its genome (all wave-uniform)
    u32 u = u0, t = 0, ust_t = 0, ust_t1 = 0, k0 = 0, k1 = 0, p0 = 0;
    u32 cur_t = ~0u, cur_r = ~0u;
    const u64* __restrict__ kp = nullptr;
    u32 g_cur = 0;                                       // (its hit list, presence bit and side are read at the unit's end)
    bool cold = true;                                    // no load of the iteration at hand has been issued
    // the mask under which a key meets the prefilter and the table: OS: M, the bits both readings share (co_pass.inc)
    const u64 fm = OS ? co_pass_mask(pmask0, S.mask_rc) : pmask0;
    // the slice of the table of (top byte t, pass r): OS: the pass's entries; else cands + c0f.  Asked where the table is
    // built and again at every unit's end: a few scalar loads there, no registers held across the key stream
    auto slice = [&](u32 r) {
        CoPass P = {};
        if (OS) P = co_pass_decode(CO_RFL(cb[2 * t]), CO_RFL(cb[2 * t + 1]), CO_RFL(cb[2 * t + 2]), tcap, r, one_pass);
        else {
            const u32 cb1 = CO_RFL(cb[t + 1]);
            P.c0f = CO_RFL(cb[t]) + r * tcap;
            P.nf = cb1 - P.c0f > tcap ? tcap : cb1 - P.c0f;
        }
        return P;
    };

    // unit `un` of top byte t becomes the unit at hand; its round's table is built unless it stands
    auto adopt = [&](const CoUnit& un) {
        const u32 g = un.genome, r = un.round;
        k0 = un.k0;
        k1 = un.k1;
        p0 = k0 & ~1u;
        kp = A.keys[g];
        g_cur = g;
        if (t != cur_t || r != cur_r) {
            cur_t = t;
            cur_r = r;
            // (the look-ups in the table before are done: every unit ends with a barrier)
            for (u32 i = threadIdx.x; i < CO_SLOTS; i += CO_T) slots[i] = CO_EMPTY;
            for (u32 i = threadIdx.x; i < (1u << (CO_BM_LOG - 5)); i += CO_T) bitmap[i] = 0;
            __syncthreads();
            const CoPass P = slice(r);
            if (OS) {
                for (u32 i = threadIdx.x; i < P.nf + P.nr; i += CO_T) {
                    const u32 h = co_hash(ents[i < P.nf ? P.c0f + i : P.c0r + (i - P.nf)].pat & fm);
                    co_insert16(slots, h, i);
                    atomicOr(&bitmap[co_bloom_word(h)], co_bloom_bits(h));
                }
            } else {
                for (u32 i = threadIdx.x; i < P.nf; i += CO_T) {
                    const u32 h = co_hash(cands[P.c0f + i].prefix);
                    const u32 word = (i << 19) | (h & 0x7FFFFu);
                    u32 s = h >> (32 - CO_SLOT_LOG);
                    while (atomicCAS(&slots[s], CO_EMPTY, word) != CO_EMPTY) s = (s + 1) & (CO_SLOTS - 1);
                    atomicOr(&bitmap[co_bloom_word(h)], co_bloom_bits(h));
                }
            }
            __syncthreads();
        }
    };
    auto uniform = [](CoUnit un) {
        un.round = CO_RFL(un.round); un.genome = CO_RFL(un.genome); un.chunk = CO_RFL(un.chunk);
        un.k0 = CO_RFL(un.k0); un.k1 = CO_RFL(un.k1);
        return un;
    };
    // unit u lies in another top byte than the one before: its row into LDS (every thread is behind a barrier since it
    // last read the row)
    auto new_byte = [&]() {
        t = CO_RFL(co_unit_byte(s_ust, u));
        ust_t = CO_RFL(s_ust[t]);
        ust_t1 = CO_RFL(s_ust[t + 1]);
        if (threadIdx.x < 2 * G) s_bnd[threadIdx.x] = rows[t * CO_ROW + threadIdx.x];
        __syncthreads();
        adopt(uniform(co_unit_decode(u - ust_t, s_bnd, G)));
    };

    // one iteration: V holds its keys (or takes them first: `cold`); NV takes the next one's.  -> the workgroup is done.
    // Every step issues the same loads at the same place and has no other global access before the unit's end, so the
    // compiler's counted waits leave the newer set in flight (k_sort2.inc, the comment at its head).
    auto step = [&](u32x4 (&V)[CO_UNROLL], u32x4 (&NV)[CO_UNROLL]) -> bool {
        const bool last = k1 - p0 <= CO_ITER;
        // what NV takes: this unit's next iteration; behind its last one the first of the next unit, while that lies in
        // the same top byte; else one key pair of this unit for every thread (k1 = 0 clamps all of them to a0)
        bool ahead = false;
        CoUnit un = {};
        const u64* __restrict__ nkp = kp;
        u32 np0 = p0 + CO_ITER, na0 = k0 & ~1u, nk1 = k1;
        if (last) {
            np0 = na0;
            nk1 = 0;
            if (u + 1 < u1 && u + 1 < ust_t1) {
                un = uniform(co_unit_decode(u + 1 - ust_t, s_bnd, G));
                nkp = A.keys[un.genome];
                np0 = na0 = un.k0 & ~1u;
                nk1 = un.k1;
                ahead = true;
            }
        }
        if (cold) co_load(V, kp, p0, p0, k1);
        cold = false;
        co_load(NV, nkp, np0, na0, nk1);
        __builtin_amdgcn_sched_barrier(0);               // (issued here, before anything of this iteration)
        // phase 1
        const int hi = (int)(k1 - p0) - 2 * (int)threadIdx.x;       // this thread's key slots below `hi` lie in front of k1
        const bool front = p0 < k0 && threadIdx.x == 0;            // ... and its first one in front of k0 (an odd k0: key a0)
        // all key slots of the iteration as one batch: every hash, every prefilter read, ONE wait; then the ballots
        // (wave-uniform: they live in scalar registers) and ONE atomic by lane 0 for the wave's room in the queue
        u32 hs[2 * CO_UNROLL], bw[2 * CO_UNROLL];
#pragma unroll
        for (int j = 0; j < 2 * CO_UNROLL; j++) {
            const u32x4& v = V[j >> 1];
            const u64 key = (j & 1) ? ((u64)v.w << 32 | v.z) : ((u64)v.y << 32 | v.x);
            // (no branch around the use of a loaded key: the counted waits must be met on every path)
            hs[j] = co_hash(key & fm);
            bw[j] = bitmap[co_bloom_word(hs[j])];
        }
        u64 bal[2 * CO_UNROLL];
        u32 total = 0;
#pragma unroll
        for (int j = 0; j < 2 * CO_UNROLL; j++) {
            const bool inr = ((j >> 1) * 2 * (int)CO_T + (j & 1) < hi) & !(j == 0 && front);
            const u32 bits = co_bloom_bits(hs[j]);
            bal[j] = __builtin_amdgcn_ballot_w64(((bw[j] & bits) == bits) & inr);
            total += (u32)__popcll(bal[j]);
        }
        if (total) {                                     // (wave-uniform; all 64 lanes are here)
            u32 qb = 0;
            if (lane == 0) qb = atomicAdd(&s_qn, total);
            qb = CO_RFL(qb);                             // + the passing lanes of the earlier slots + those below this lane
#pragma unroll
            for (int j = 0; j < 2 * CO_UNROLL; j++) {
                const u32x4& v = V[j >> 1];
                const u64 key = (j & 1) ? ((u64)v.w << 32 | v.z) : ((u64)v.y << 32 | v.x);
                const u32 qa = qb + __builtin_amdgcn_mbcnt_hi((u32)(bal[j] >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal[j], 0u));
                // (the slot's ballot is its lanes' predicate again: nothing is computed, and no second mask is kept)
                if (__builtin_amdgcn_inverse_ballot_w64(bal[j]) && qa < CO_QCAP) s_q[qa] = key;     // (a key that finds the queue full: see below)
                qb += (u32)__popcll(bal[j]);
            }
        }
        if (!last) { p0 += CO_ITER; return false; }
        // phase 2: the unit's queue
        __syncthreads();
        u32* __restrict__ hits = A.hits[g_cur];
        u64* __restrict__ hitkeys = (u64*)(hits + 4);
        const u32 hitcap = A.hitcap[g_cur];
        const CoHitSink K = {state, 1u << A.bit[g_cur], A.side[g_cur], s_hit, &s_nhit, hits, hitkeys, hitcap, LR};
        const CoPass P = slice(cur_r);
        auto lookup = [&](u64 key) {
            if (OS) co_lookup16(key, fm, pmask0, (const uint16_t*)slots, P, ents, S, K);
            else co_lookup(key, pmask0, slots, P.c0f, cands, K);
        };
        if (s_qn <= CO_QCAP) {
            const u32 qn = s_qn;
            for (u32 i = threadIdx.x; i < qn; i += CO_T) lookup(s_q[i]);
        } else {
            // more keys passed the prefilter than the queue holds, and some were dropped (nothing of the unit has been
            // looked up yet): the queue is discarded and the unit's keys are read again and looked up in place -- exact
            // under any input, and slow only where the prefilter does not filter
            const u32 a0 = k0 & ~1u;
            for (u32 p = a0 + 2 * threadIdx.x; p < k1; p += 2 * CO_T) {
                const u32x4 w = *reinterpret_cast<const u32x4*>(kp + p);
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const u64 key = e ? ((u64)w.w << 32 | w.z) : ((u64)w.y << 32 | w.x);
                    const u32 h = co_hash(key & fm), bits = co_bloom_bits(h);
                    if (p + e >= k0 && p + e < k1 && (bitmap[co_bloom_word(h)] & bits) == bits) lookup(key);
                }
            }
        }
        __syncthreads();                                 // (the look-ups are done: the unit's hits are counted)
        const u32 m = min(s_nhit, (u32)CO_HB);
        __syncthreads();                                 // (every thread has read both counts: they are the same in all of them)
        if (threadIdx.x == 0) {
            s_qn = 0;
            s_nhit = 0;
            if (m) s_hbase = atomicAdd(hits, m);
        }
        if (m) {                                         // the unit's hits from LDS into its genome's list
            __syncthreads();
            const u32 hb = s_hbase;
            for (u32 i = threadIdx.x; i < m; i += CO_T)
                if (hb + i < hitcap) hitkeys[hb + i] = s_hit[i];
        }
        __syncthreads();                                 // (queue and hit buffer are free, their counts zero)
        if (++u >= u1) return true;
        if (ahead) adopt(uniform(co_unit_decode(u - ust_t, s_bnd, G)));   // (decoded again: `un` is not held across the unit)
        else {
            new_byte();
            cold = true;
        }
        return false;
    };

    u32x4 va[CO_UNROLL], vb[CO_UNROLL];
    new_byte();
    for (;;) {
        if (step(va, vb)) break;
        if (step(vb, va)) break;
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
// (per_key: records a key of the array stands for -- 2 where pass 1 wrote one strand for both, co_strand.inc)
__global__ void k_coarse_keep(const u32* __restrict__ base1, u32* __restrict__ off, u32 nb, u32* __restrict__ ovf, u32 per_key) {
    const u32 t = threadIdx.x;
    if (t <= 256) off[t] = base1[t];
    else if (t == 257) off[nb] = per_key * base1[256];
    else if (t == 258) ovf[0] = 0;
}
