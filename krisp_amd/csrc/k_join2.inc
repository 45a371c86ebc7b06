// k_join2.inc -- part of krisp_hip.hip (one translation unit): the intersection of TWO genomes, one of each side, one
// diagnostic column, filter on -- the call the step makes for its pillars -- as a screen and a small exact join.
//
// Why: k_intersect3t<3, true> makes an exact slot array from every anchor key of an item (arrival numbers, a 4096-word
// scan, placement, the walk for equal prefixes, survivor flags over all slots), although about one prefix in a hundred
// survives the filter and more than half of the keys are the same window with the same diagnostic base in both genomes.
// Here every key of the item's buckets, of both genomes, first ORs one bit into a byte screen in LDS (j2_screen.inc:
// slot = a function of the prefix alone); behind a barrier a slot is LIVE iff both genomes reached it and it shows two
// different bases.  Only keys of live slots meet the exact structure: an open-addressing table on the item key
// (64-bit compare-and-swap, an equal prefix ORs into the slot it finds), state word presence << 8 | out << 4 | in as in
// k_intersect3t<3>.  Survivors are listed, ranked by counting among themselves, and written ascending.
//
// Items, batches, the two register sets and the prefetch of the next item's offsets are k_intersect3's (i3_issue, the
// state of i3_advance).  The anchor's batch stays in a third register set until the other genome's batch has set its
// bits, so every key is loaded once.  Where the other genome's run of an item is longer than one batch (rare: the anchor
// is the shorter genome) its batches are walked twice, once to set the screen and once to test it: the second visit
// reads what the same CU read microseconds before.  A live anchor key that finds no room within J2_PROBES slots flags
// its item: it is listed in a.ovf like an oversized one (and counted in a.ovf[I3_OVF_CAP + 2]), the host's redo path
// answers it.  Neither genome's order inside a bucket is looked at.
//
// k_join2<true> (KR_OPT_JOIN2_DENSE, the default): about one key in ten is live, so a key slot's own `if (live) insert` ran
// for about six lanes of a wave, eight times per item, and every key's slot was computed a second time behind the barrier.
// Here the four screen slots of a batch stay in registers from the visit that sets the bits to the test (the anchor's across
// the other genome's visit), and behind barrier (2) / (3) a wave appends its live keys to a queue of its own (j2_queue.inc:
// ballot, lanes below, one 8-byte entry of two shifts; the fill is a scalar) and joins them 64 at a time with every lane
// busy, the rest before the barrier that follows.  The queues are lkey[], which nobody else touches between barriers (1)
// and (4).  The table fills in another order; what it holds behind barrier (4) is the same.  k_join2<false> is the kernel
// without this.
// ----------------------------------------------------------------------------
#include "j2_screen.inc"
#include "j2_queue.inc"

#ifndef J2_OCC
#define J2_OCC 6            // waves per SIMD the kernel is compiled for
#endif
#define J2_FULL_WORD (I3_OVF_CAP + 2)

static_assert(J2Q_CAP * (I3_MAXT / 64) <= J2_TAB, "the waves' queues lie in lkey[]");

// a wave's queue between its own writes and its own reads of other lanes' entries: the compiler keeps the order, the LDS
// counter has run out (the LDS serves one wave's instructions in order; the wait makes that independent of it)
__device__ __forceinline__ void j2q_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool DENSE>
__global__ __launch_bounds__(I3_MAXT, J2_OCC) void k_join2(Isect3Args a, Geom g) {
    __shared__ __attribute__((aligned(16))) u32 scr[J2_SCREEN / 4];
    __shared__ __attribute__((aligned(16))) unsigned long long tkey[J2_TAB];
    __shared__ __attribute__((aligned(16))) u32 tst[J2_TAB];
    __shared__ unsigned long long lkey[J2_TAB];
    __shared__ u32 lst[J2_TAB];
    __shared__ uint2 rng[2][MAXG];
    __shared__ const u64* keyp[MAXG];
    __shared__ u32 ctl[2];                  // [0] survivors listed, [1] a live key found no room
    const u32 tid = threadIdx.x, T = blockDim.x, S = 4 * T, G = gridDim.x;
    const u32 lane = tid & 63;
    const bool anchor_in = (a.ingroup_bits >> a.anchor) & 1;
    const int p0 = a.p0, wbits = a.sh + (int)I3T_NB_LOG - a.p0;
    // a key's state word: presence << 8 | out << 4 | in
    const u32 prA = 1u << (8 + a.anchor), prB = 1u << (8 + (1 - a.anchor));
    const u32 sdA = anchor_in ? 1u : 16u, sdB = anchor_in ? 16u : 1u;
    const u32 og = min(lane >> 1, (u32)a.n - 1);
    const u32 __attribute__((address_space(1)))* myoff;
    {
        u64 mo = (u64)a.off[og];
        asm volatile("" : "+v"(mo));
        myoff = (const u32 __attribute__((address_space(1)))*)mo;
    }
    auto item_bucket = [&](u32 it, u32 which) {
        const u64 f = ((u64)it + which) << a.mlog;
        return (u32)(f < a.nb ? f : a.nb);
    };
    for (u32 i = tid; i < J2_SCREEN / 4; i += T) scr[i] = 0;
    for (u32 i = tid; i < J2_TAB; i += T) { tkey[i] = 0; tst[i] = 0; }
    if (tid < 2) ctl[tid] = 0;
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
    u32 item_sa = 0, item_cnt = 0;
    u32 item_full = 0, item_firstb = 0;       // (wave-uniform, the same in every wave)
    u32 voff = 0;
    I3Regs X, Y, KA;
    KA.q[0] = KA.q[1] = u32x4{0, 0, 0, 0};
    u32 slotA[4] = {0, 0, 0, 0};              // DENSE: the screen slots of KA's keys
    unsigned long long* const myq = lkey + J2Q_CAP * (tid >> 6);       // DENSE: this wave's queue
    const unsigned char* const scrb = reinterpret_cast<const unsigned char*>(scr);      // (byte slot of the screen = j2_byte of its word)
    i3_issue(X, a, keyp, cur, T);

    auto ikey_of = [&](u32 lo, u32 hi) { return j2_item_key(((u64)hi << 32) | lo, p0, wbits); };
    auto base_of = [&](u32 lo) { return __builtin_amdgcn_ubfe(lo, (u32)(p0 - 2), 2u); };
    // an anchor key into the table: its slot is the first of its probe sequence that is free or holds its item key
    auto insert = [&](u64 ik, u32 sw) {
        const unsigned long long want = ik | (1ull << 63);
        u32 h = j2_tab_hash(ik);
        bool placed = false;
        for (u32 t = 0; t < J2_PROBES && !placed; t++) {
            const unsigned long long old = atomicCAS(&tkey[h], 0ull, want);
            if (old == 0ull || old == want) {
                atomicOr(&tst[h], sw);
                placed = true;
            }
            h = (h + 1) & (J2_TAB - 1);
        }
        if (!placed) ctl[1] = 1;
    };
    auto probe = [&](u64 ik, u32 sw) {
        const unsigned long long want = ik | (1ull << 63);
        u32 h = j2_tab_hash(ik);
        for (u32 t = 0; t < J2_PROBES; t++) {
            const unsigned long long old = tkey[h];
            if (old == want) atomicOr(&tst[h], sw);
            if (old == want || old == 0ull) break;
            h = (h + 1) & (J2_TAB - 1);
        }
    };
    // DENSE: one key slot's live keys onto the wave's queue
    // (the ballot of each comparison is the comparison's own mask; the ballot of their conjunction is built from a lane value)
    auto q_push = [&](u32& fill, bool valid, bool lv, u32 lo, u32 hi) {
        const bool live = valid & lv;
        const u64 m = __builtin_amdgcn_ballot_w64(valid) & __builtin_amdgcn_ballot_w64(lv);
        const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));      // = j2q_below(m, lane)
        if (live) myq[j2q_place(fill, below)] = j2q_entry(lo, hi, p0);
        fill = i3_uni(j2q_fill_after(fill, m));
    };
    // DENSE: the n entries on top of the queue, one per lane, into the table (ANCHOR) or past it
    auto q_join = [&](u32& fill, u32 n, bool anchor) {
        j2q_order();
        if (lane < n) {
            const u64 en = myq[j2q_first(fill, n) + lane];
            const u64 ik = j2q_key(en, wbits);
            if (anchor) insert(ik, prA | (sdA << j2q_base(en)));
            else probe(ik, prB | (sdB << j2q_base(en)));
        }
        j2q_order();
        fill = i3_uni(j2q_first(fill, n));
    };
    // DENSE: the live keys of a batch (screen slots sl[]) queued and joined; nothing is left in the queue
    auto q_batch = [&](const I3Regs& K, const u32 (&sl)[4], u32 count, bool anchor) {
        const u32 tid = opaque_tid();
        u32 by[4];
        // (read for every lane: a lane past `count` holds the slot of whatever its load left, inside the screen for any input
        // -- j2_slot keeps J2_SCREEN_LOG bits --, and `valid` keeps it out of the queue)
#pragma unroll
        for (int e = 0; e < 4; e++) by[e] = scrb[sl[e]];
        u32 fill = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            q_push(fill, I3_POS(e) < count, j2_live_byte_min(by[e]), I3_LO(K, e), I3_HI(K, e));
            if (j2q_drains(fill)) q_join(fill, J2Q_DRAIN, anchor);
        }
        if (fill) q_join(fill, fill, anchor);
    };
    auto list_item = [&](u32 it, bool full) {
        const u32 idx = atomicAdd(&a.ovf[0], 1u);
        if (idx < a.ovf_cap) a.ovf[1 + idx] = it;
        if (full) atomicAdd(&a.ovf[J2_FULL_WORD], 1u);
        a.itemcnt[it] = 0;
    };

    // the batch after `st`: as i3_advance for two genomes, but a run of the other genome that takes more than one batch is
    // walked twice -- pass 0 sets the screen, pass 1 tests it (b0 = the run's first key)
    auto advance = [&](I3State& st, u32& pass, u32& b0) {
        if (st.g >= 0 && st.i0 + S < st.e) {
            st.i0 += S;
        } else if (st.g < 0) {
            const uint2 r = rng[st.par][1 - a.anchor];
            st.g = 1 - a.anchor;
            st.i0 = i3_uni(r.x);
            st.e = st.over ? st.i0 : i3_uni(r.y);
            b0 = st.i0;
            pass = 0;
        } else if (pass == 0 && st.e - b0 > S) {
            st.i0 = b0;
            pass = 1;
        } else {
            st.it += G;
            st.par ^= 1u;
            st.g = -1;
            pass = 0;
            const uint2 r = rng[st.par][a.anchor];
            const u32 s = i3_uni(r.x), e = i3_uni(r.y);
            st.over = (e - s > S) ? 1u : 0u;
            st.i0 = s;
            st.e = st.over ? s : e;
        }
        if (st.it >= a.nitems) { st.i0 = 0; st.e = 0; st.over = 0; }
        st.it = i3_uni(st.it); st.g = (int)i3_uni((u32)st.g); st.i0 = i3_uni(st.i0); st.e = i3_uni(st.e);
        st.par = i3_uni(st.par); st.over = i3_uni(st.over);
        pass = i3_uni(pass); b0 = i3_uni(b0);
    };

    auto process = [&](const I3Regs& R, const I3State& st, const u32 pass, const I3State& nx) {
        const u32 tid = opaque_tid();
        asm volatile("" ::"v"(R.q[0]), "v"(R.q[1]));          // (consumed on every path: see k_intersect3)
        if (st.g < 0) {
            // ===== the anchor's keys of a new item: their bits into the screen, the keys kept
            item_sa = st.i0;
            item_cnt = st.e - st.i0;
            item_full = 0;
            item_firstb = 1;
            const u32 cnt = item_cnt;
            if (st.over) {
                if (tid == 0) list_item(st.it, false);
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if (DENSE) {
                        slotA[e] = j2_slot(ikey_of(I3_LO(R, e), I3_HI(R, e)));
                        if (I3_POS(e) < cnt) atomicOr(&scr[slotA[e] >> 2], j2_bit(slotA[e], base_of(I3_LO(R, e)), false));
                    } else if (I3_POS(e) < cnt) {
                        const u32 slot = j2_slot(ikey_of(I3_LO(R, e), I3_HI(R, e)));
                        atomicOr(&scr[slot >> 2], j2_bit(slot, base_of(I3_LO(R, e)), false));
                    }
                }
                KA = R;
            }
            if (tid < 2 * (u32)a.n) {
                if (lane & 1) rng[st.par ^ 1u][og].y = voff; else rng[st.par ^ 1u][og].x = voff;
            }
            __syncthreads();                                                        // (1) anchor's bits, next ranges
        } else if (!st.over) {
            // ===== the other genome's keys over the item's buckets
            const u32 cnt = item_cnt;
            const u32 left = st.e - st.i0;
            const bool last_of_pass = !(st.i0 + S < st.e);
            if (item_firstb) {
                if (tid == 0) ctl[0] = 0;           // (everybody has read the item before's count: barrier (1) lies between)
                item_firstb = 0;
            }
            u32 slotB[4];                           // DENSE: the screen slots of R's keys, for the bits and for the test
            if (DENSE) {
#pragma unroll
                for (int e = 0; e < 4; e++) slotB[e] = j2_slot(ikey_of(I3_LO(R, e), I3_HI(R, e)));
            }
            if (pass == 0) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (I3_POS(e) < left) {
                        const u32 slot = DENSE ? slotB[e] : j2_slot(ikey_of(I3_LO(R, e), I3_HI(R, e)));
                        atomicOr(&scr[slot >> 2], j2_bit(slot, base_of(I3_LO(R, e)), true));
                    }
                if (last_of_pass) {
                    __syncthreads();                                                // (2) the screen is complete
                    if (DENSE) {
                        q_batch(KA, slotA, cnt, true);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (I3_POS(e) < cnt) {
                                const u64 ik = ikey_of(I3_LO(KA, e), I3_HI(KA, e));
                                const u32 slot = j2_slot(ik);
                                if (j2_live_byte(j2_byte(scr[slot >> 2], slot))) insert(ik, prA | (sdA << base_of(I3_LO(KA, e))));
                            }
                    }
                    __syncthreads();                                                // (3) the live anchor keys are in the table
                    item_full = i3_uni(ctl[1]);
                }
            }
            // (one batch: set and tested in one visit; more: tested on the second walk, behind barrier (3))
            if ((nx.it != st.it || pass == 1) && !item_full) {
                if (DENSE) {
                    q_batch(R, slotB, left, false);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (I3_POS(e) < left) {
                            const u64 ik = ikey_of(I3_LO(R, e), I3_HI(R, e));
                            const u32 slot = j2_slot(ik);
                            if (j2_live_byte(j2_byte(scr[slot >> 2], slot))) probe(ik, prB | (sdB << base_of(I3_LO(R, e))));
                        }
                }
            }
            if (nx.it != st.it) {
                // ===== last batch of the item: the survivors, listed, ranked among themselves, written ascending
                __syncthreads();                                                    // (4) probes done
                const bool full = item_full != 0;
                for (u32 i = tid; i < J2_TAB; i += T) {
                    const unsigned long long k = tkey[i];
                    if (k != 0ull) {
                        const u32 s = tst[i];
                        tkey[i] = 0ull;
                        tst[i] = 0;
                        if (!full && (s >> 8) == 3u && (s & (s >> 4) & 15u) == 0) {
                            const u32 idx = atomicAdd(&ctl[0], 1u);
                            lkey[idx] = k;
                            lst[idx] = s;
                        }
                    }
                }
                for (u32 i = 4 * tid; i < J2_SCREEN / 4; i += 4 * T) *reinterpret_cast<uint4*>(&scr[i]) = make_uint4(0, 0, 0, 0);
                if (tid == 0) ctl[1] = 0;
                __syncthreads();                                                    // (5) list, table and screen as the next item needs them
                const u32 nsurv = full ? 0u : i3_uni(ctl[0]);
                if (nsurv) {
                    const u64 base = ((u64)st.it << a.mlog) << g.rb;                // the item's key range starts here
                    const u64 wmask = (1ull << wbits) - 1;
                    kr_cand* out = a.tmp + item_sa;
                    for (u32 i = tid; i < nsurv; i += T) {
                        const unsigned long long k = lkey[i];
                        const u32 s = lst[i];
                        u32 r = 0;
                        for (u32 j = 0; j < nsurv; j++) r += lkey[j] < k ? 1u : 0u;
                        kr_cand c;
                        c.prefix = base | ((k & wmask) << p0);
                        c.in_mask = (u64)(s & 15u);
                        c.out_mask = (u64)((s >> 4) & 15u);
                        out[r] = c;
                    }
                }
                if (tid == 0) {
                    if (full) list_item(st.it, true);
                    else a.itemcnt[st.it] = nsurv;
                }
            }
        }
    };

    u32 cur_pass = 0, b0 = 0;
    for (;;) {
        I3State nxt = cur;
        u32 nxt_pass = cur_pass;
        if (cur.g < 0) {
            const u32 ni = cur.it + G < a.nitems ? cur.it + G : 0u;
            voff = myoff[item_bucket(ni, lane & 1)];
        }
        advance(nxt, nxt_pass, b0);
        i3_issue(Y, a, keyp, nxt, T);
        process(X, cur, cur_pass, nxt);
        cur = nxt;
        cur_pass = nxt_pass;
        if (cur.it >= a.nitems) break;
        if (cur.g < 0) {
            const u32 ni = cur.it + G < a.nitems ? cur.it + G : 0u;
            voff = myoff[item_bucket(ni, lane & 1)];
        }
        advance(nxt, nxt_pass, b0);
        i3_issue(X, a, keyp, nxt, T);
        process(Y, cur, cur_pass, nxt);
        cur = nxt;
        cur_pass = nxt_pass;
        if (cur.it >= a.nitems) break;
    }
}
