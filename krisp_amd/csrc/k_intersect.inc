// k_intersect.inc -- part of krisp_hip.hip (one translation unit): K6-K8: n-way intersection, candidate compaction, record collection, list merge

// ----------------------------------------------------------------------------
// ordered compaction inside a workgroup: position of this thread's flagged item
// ----------------------------------------------------------------------------
__device__ __forceinline__ u32 block_compact(bool flag, u32* lds_waves, u32& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 mask = __ballot(flag);
    u32 pos = __popcll(mask & ((1ull << lane) - 1));
    if (lane == 0) lds_waves[wave] = __popcll(mask);
    __syncthreads();
    u32 basev = 0, tot = 0;
    for (int i = 0; i < nw; i++) {
        u32 t = lds_waves[i];
        if (i < wave) basev += t;
        tot += t;
    }
    total = tot;
    __syncthreads();
    return basev + pos;
}

__device__ __forceinline__ u64 diag_mask(u64 key, int LR, int D) {
    u64 m = 0;
    for (int c = 0; c < D; c++) {
        u32 bb = (u32)(key >> (62 - 2 * (LR + c))) & 3u;
        m |= 1ull << (4 * c + bb);
    }
    return m;
}

// mode 1: the reference's filter (Amplicon.py:495-521: some column whose ingroup and outgroup letter sets are disjoint).
// mode 2 (kr_set_mixed_alphabets: DNA and RNA genomes in one run, whose code 3 is 'T' in some genomes and 'U' in others --
// different letters to the reference, which compares text): a column also passes when the two sets share nothing but
// code 3 -- a superset of the reference's survivors, monotone like mode 1; the host layer, which knows each genome's
// alphabet, decides those columns from the survivors' records (krisp_fasta.py: _mixed_filter)
__device__ __forceinline__ bool passes_filter(u64 im, u64 om, int D, int mode) {
    u64 x = im & om;
    if (mode == 2) x &= 0x7777777777777777ull;
    for (int c = 0; c < D; c++)
        if (((x >> (4 * c)) & 15ull) == 0) return true;
    return false;
}

// ----------------------------------------------------------------------------
// K6  n-way intersection.  One workgroup per chunk of the anchor genome: the
// distinct (left,right) prefixes of the chunk go to LDS; every genome (the
// anchor included) streams its keys of the same bucket range past them
// (order-preserving sub-bins in LDS: ~2 probes per key), OR-ing a presence bit and the diagnostic-column masks.
// Survivors are written in order to tmp[anchor offset ...]; chunkcnt[j] = count.
// ----------------------------------------------------------------------------
#define MAXG 32
// timing aids (tools/isect_ablate.py): parts of the kernel switched off by bits of IsectArgs.dbg.
// They change results, so they exist in a -DKR_ABLATE build only; bit 32 (generic sub-tile path,
// results unchanged) is always available.
#ifdef KR_ABLATE
#define ABL(args, bit) ((args).dbg & (bit))
#else
#define ABL(args, bit) 0
#endif
struct IsectArgs {
    const u64* keys[MAXG];
    const u32* off[MAXG];
    u32 ingroup_bits;
    int n;
    int anchor;
    const uint4* chunkdesc;
    kr_cand* tmp;
    u32* chunkcnt;
    int apply_filter;
    int dbg;   // KR_DBG env: 32 = always take the generic sub-tile path (tests cover both)
    // item-list mode (the oversized items k_intersect3 left behind): workgroup w takes item ovf[1 + w] = the
    // buckets [item << mlog, (item + 1) << mlog) and reports into chunkcnt[item]; ovf[0] = number of items
    const u32* ovf;
    u32 ovf_cap;
    int mlog;
    u32 nb;
};

// per-head state in LDS, by mask format FMT:
//   0 compact (D <= 4)  one u64: present << 32 | out << 16 | in     -> one atomic per matching key
//   1 narrow  (D <= 8)  present u32 + one u64: out << 32 | in
//   2 wide    (D <= 16) present u32 + in u64 + out u64
template <int FMT>
__device__ __forceinline__ void isect_update(u32 h, u64 key, int gi, bool ing, u32* present, u64* inm, u64* outm,
                                             const Geom& g, int LR) {
    const u64 dm = g.D > 0 ? diag_mask(key, LR, g.D) : 0;
    if (FMT == 0) {
        atomicOr((u64*)&inm[h], ((u64)1 << (32 + gi)) | (ing ? dm : (dm << 16)));
    } else {
        atomicOr(&present[h], 1u << gi);
        if (g.D > 0) {
            if (FMT == 2) atomicOr((u64*)(ing ? &inm[h] : &outm[h]), dm);
            else atomicOr((u64*)&inm[h], ing ? dm : (dm << 32));
        }
    }
}

// One stream key against the heads.  The sub-bin table averages one head per bin, so the first
// two heads of the key's bin are read UNCONDITIONALLY (clamped indices): the common path has no
// data-dependent loop, and the probes of a thread's keys overlap their LDS latencies instead of
// running one dependent chain after the other; a fuller bin (8 % of them) walks the rest.
template <int FMT>
__device__ __forceinline__ void isect_probe(u64 key, int gi, bool ing, u64 first, u64 last, int sh,
                                            const u64* heads, const unsigned short* binstart, u32* present,
                                            u64* inm, u64* outm, const Geom& g, int LR, bool valid = true,
                                            bool noatomic = false) {
    const u64 pre = key & g.pmask;
    const bool inside = valid && pre >= first && pre <= last;
    const u32 sb = inside ? (u32)((pre - first) >> sh) : 0u;
    const u32 h0 = binstart[sb];
    const u32 hend = inside ? binstart[sb + 1] : h0;
    const u64 k0 = heads[h0 < IS_SUB ? h0 : 0], k1 = heads[h0 + 1 < IS_SUB ? h0 + 1 : 0];
    u32 h = ~0u;
    if (h0 < hend && k0 == pre) h = h0;
    else if (h0 + 1 < hend && k1 == pre) h = h0 + 1;
    else if (h0 + 2 < hend)
        for (u32 t = h0 + 2; t < hend; t++)
            if (heads[t] == pre) { h = t; break; }
    if (h != ~0u && !noatomic) isect_update<FMT>(h, key, gi, ing, present, inm, outm, g, LR);
}

#define IS_APT (IS_SUB / IS_THREADS)    // anchor keys (and stream keys per batch) per thread
#define IS_NW (IS_THREADS / 64)

// ordered compaction of IS_APT flags per thread (element p = q * IS_THREADS + tid):
// ballots go to LDS, one wave turns the IS_APT * IS_NW group counts into prefixes.
// Returns the total; pos[q] = output slot of element q (valid where flag[q]).
__device__ __forceinline__ u32 compact_flags(const bool (&flag)[IS_APT], u32 (&pos)[IS_APT], u64* masks,
                                             u32* mpref) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 m[IS_APT];
#pragma unroll
    for (int q = 0; q < (int)IS_APT; q++) {
        m[q] = __ballot(flag[q]);
        if (lane == 0) masks[q * IS_NW + wave] = m[q];
    }
    __syncthreads();
    if (wave == 0) {
        const int ng = IS_APT * IS_NW;     // <= 64 groups
        u32 c = lane < ng ? (u32)__popcll(masks[lane]) : 0;
        const u32 x = wave_incl_scan(c);
        if (lane < ng) mpref[lane] = x - c;
        if (lane == 63) mpref[64] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (int)IS_APT; q++)
        pos[q] = mpref[q * IS_NW + wave] + (u32)__popcll(m[q] & ((1ull << lane) - 1));
    return mpref[64];
}

template <int FMT>
__global__ __launch_bounds__(IS_THREADS, FMT == 2 ? 4 : (FMT == 1 ? 6 : IS_OCC0)) void k_intersect(IsectArgs a, Geom g) {
    constexpr bool WIDE = FMT == 2;
    constexpr u32 NBINS = FMT == 0 ? IS_NB0 : IS_NB;
    constexpr int NB_LOG = NBINS == 1024 ? 10 : (NBINS == 2048 ? 11 : (NBINS == 4096 ? 12 : 13));
    __shared__ __attribute__((aligned(16))) u64 heads[IS_SUB];
    __shared__ __attribute__((aligned(16))) u64 inm[IS_SUB];
    __shared__ __attribute__((aligned(16))) u64 outm[WIDE ? IS_SUB : 1];
    __shared__ u32 present[FMT == 0 ? 1 : IS_SUB];
    __shared__ unsigned short binstart[NBINS + 2];
    __shared__ u64 masks[64];
    __shared__ u32 mpref[65];
    __shared__ u32 sstart[MAXG], send[MAXG];
    __shared__ u32 disorder[2];
    const u32 tid = threadIdx.x;
    if (tid == 0) disorder[0] = 0;
    __syncthreads();
    u32 dpar = 0;
    const u64* KA = a.keys[a.anchor];
    const u32* offA = a.off[a.anchor];
    u32 slot = blockIdx.x;
    uint4 cd;
    if (a.ovf) {
        if (blockIdx.x >= min(a.ovf[0], a.ovf_cap)) return;
        slot = a.ovf[1 + blockIdx.x];
        const u64 f0 = (u64)slot << a.mlog, f1 = ((u64)slot + 1) << a.mlog;
        cd.z = (u32)(f0 < a.nb ? f0 : a.nb);
        cd.w = (u32)(f1 < a.nb ? f1 : a.nb);
        cd.x = offA[cd.z];
        cd.y = offA[cd.w];
    } else {
        cd = a.chunkdesc[blockIdx.x];
    }
    const u32 sa = cd.x, ea = cd.y, chi = cd.w;
    if (sa >= ea) {
        if (tid == 0) a.chunkcnt[slot] = 0;
        return;
    }
    const u32 full = a.n >= 32 ? 0xFFFFFFFFu : ((1u << a.n) - 1);
    const int LR = g.LRrel;
    const bool prefix_in_bucket = 2 * LR >= g.b;      // a (left,right) group never spans fine buckets
    const bool anchor_in = (a.ingroup_bits >> a.anchor) & 1;
    u32 nout = 0;
    u32 fcur = cd.z;                                   // first bucket of the current sub-tile
    bool start_ok = true;                              // the sub-tile starts on a bucket boundary
    for (u32 sub = sa; sub < ea;) {
        // ---- sub-tile = whole buckets, at most IS_SUB anchor keys (key-count split only for
        //      a single bucket larger than that)
        u32 fend = chi, subend = ea;
        bool aligned = true;
        if (ea - sub > IS_SUB) {
            u32 l = fcur, r = chi;                     // largest f with offA[f] <= sub + IS_SUB
            while (l < r) {
                u32 mid = (l + r + 1) >> 1;
                if (offA[mid] <= sub + IS_SUB) l = mid; else r = mid - 1;
            }
            if (l > fcur && offA[l] > sub) {
                fend = l;
                subend = offA[l];
            } else {
                aligned = false;
                fend = fcur;
                subend = sub + IS_SUB;
            }
        }
        const u32 cnt = subend - sub;
        const bool fast = start_ok && aligned && prefix_in_bucket && !(a.dbg & 32);
        // ---- every load we can issue now: anchor keys, and (fast) the stream ranges
        u64 ak[IS_APT], pk[IS_APT];
#pragma unroll
        for (int q = 0; q < (int)IS_APT; q++) {
            u32 p = q * IS_THREADS + tid;
            u32 gi = sub + p;
            ak[q] = p < cnt ? KA[gi] : 0;
            pk[q] = (p < cnt && gi > 0) ? KA[gi - 1] : 0;
        }
        if (fast && tid < (u32)a.n) {
            u32 s0 = a.off[tid][fcur], e0 = a.off[tid][fend];
            if ((int)tid == a.anchor) e0 = s0;                     // the anchor's own keys are in registers
            sstart[tid] = s0;
            send[tid] = e0;
        }
        // ---- distinct prefixes, in order
        // kr_intersect may run right behind a sort whose oversized buckets the merge fallback has not ordered yet
        // (h_intersect.inc: that result is thrown away and the intersection redone); everything below takes
        // ascending heads, so a sub-tile with a descent in it is passed over
        bool flag[IS_APT];
        u32 pos[IS_APT];
        bool desc = false;
#pragma unroll
        for (int q = 0; q < (int)IS_APT; q++) {
            u32 p = q * IS_THREADS + tid;
            const u64 pp = pk[q] & g.pmask, pa = ak[q] & g.pmask;     // (callers order by prefix; what follows it may lie anyhow)
            flag[q] = p < cnt && ((sub + p == 0) || pp != pa);
            desc = desc || (p < cnt && pp > pa);
        }
        if (desc) disorder[dpar] = 1;
        u32 nheads = compact_flags(flag, pos, masks, mpref);
        if (tid == 0) disorder[dpar ^ 1u] = 0;         // (the next sub-tile's; this one's is read behind the barrier below)
#pragma unroll
        for (int q = 0; q < (int)IS_APT; q++) {
            if (flag[q]) {
                heads[pos[q]] = ak[q] & g.pmask;
                if (FMT == 0) {
                    inm[pos[q]] = fast ? ((u64)1 << (32 + a.anchor)) : 0ull;
                } else {
                    present[pos[q]] = fast ? (1u << a.anchor) : 0u;
                    inm[pos[q]] = 0;
                    if (WIDE) outm[pos[q]] = 0;
                }
            }
        }
        __syncthreads();
        if (disorder[dpar]) nheads = 0;
        dpar ^= 1u;
        if (nheads > 0) {
            const u64 first = heads[0], last = heads[nheads - 1];
            const u64 span = last - first;
            const int sh = span < NBINS ? 0 : (64 - __clzll((long long)span) - NB_LOG);
            if (!fast && tid < (u32)a.n) {
                const u32 fl = (u32)(first >> g.rb);
                const u32 fh = (u32)((last | ~g.pmask) >> g.rb) + 1;
                u32 s0 = a.off[tid][fl];
                sstart[tid] = s0;
                send[tid] = a.off[tid][fh];
            }
            // order-preserving sub-bins over [first, last]: binstart[sb] = #heads with bin < sb
            for (u32 h = tid; h < (ABL(a, 4096) ? 0u : nheads); h += IS_THREADS) {
                u32 sb = (u32)((heads[h] - first) >> sh);
                u32 prev = h ? (u32)((heads[h - 1] - first) >> sh) + 1 : 0;
                for (u32 q = prev; q <= sb; q++) binstart[q] = (unsigned short)h;
            }
            {
                u32 lastbin = (u32)(span >> sh);
                for (u32 q = lastbin + 1 + tid; q <= NBINS; q += IS_THREADS) binstart[q] = (unsigned short)nheads;
            }
            if (fast && g.D > 0 && !ABL(a, 1024)) {
                // the anchor's own diagnostic columns, straight from registers
#pragma unroll
                for (int q = 0; q < (int)IS_APT; q++) {
                    u32 p = q * IS_THREADS + tid;
                    if (p < cnt) {
                        u32 h = flag[q] ? pos[q] : pos[q] - 1;
                        u64 dm = diag_mask(ak[q], LR, g.D);
                        if (FMT == 2) atomicOr((u64*)(anchor_in ? &inm[h] : &outm[h]), dm);
                        else if (FMT == 1) atomicOr((u64*)&inm[h], anchor_in ? dm : (dm << 32));
                        else atomicOr((u64*)&inm[h], anchor_in ? dm : (dm << 16));
                    }
                }
            }
            __syncthreads();
            // ---- stream the genomes past the heads; first batch of genome g+1 in flight while g is probed
            u64 cur[IS_APT], nxt[IS_APT];
            {
                const u64* K = a.keys[0];
                const u32 s0 = sstart[0], e0 = send[0];
#pragma unroll
                for (int q = 0; q < (int)IS_APT; q++) {
                    u32 i = s0 + q * IS_THREADS + tid;
                    cur[q] = i < e0 ? K[i] : 0;
                }
            }
            for (int gi = 0; gi < (ABL(a, 512) ? 0 : a.n); gi++) {      // (512: kr_debug_intersect, anchor work only)
                const u64* K = a.keys[gi];
                const u32 s = sstart[gi], e = send[gi];
                const bool ing = (a.ingroup_bits >> gi) & 1;
                if (gi + 1 < a.n) {
                    const u64* K2 = a.keys[gi + 1];
                    const u32 s2 = sstart[gi + 1], e2 = send[gi + 1];
#pragma unroll
                    for (int q = 0; q < (int)IS_APT; q++) {
                        u32 i = s2 + q * IS_THREADS + tid;
                        nxt[q] = i < e2 ? K2[i] : 0;
                    }
                }
                for (u32 i0 = s; i0 < e; i0 += IS_SUB) {
                    if (i0 != s) {
#pragma unroll
                        for (int q = 0; q < (int)IS_APT; q++) {
                            u32 i = i0 + q * IS_THREADS + tid;
                            cur[q] = i < e ? K[i] : 0;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < (int)IS_APT; q++) {
                        const u32 i = i0 + q * IS_THREADS + tid;
#ifdef KR_ABLATE
                        if (i < e && (a.dbg & 64)) {            // kr_debug_intersect: stream the keys, no probes
                            if (cur[q] == 0x123456789ull) inm[0] = 1;
                            continue;
                        }
#endif
                        // (unconditional: the LDS reads of the IS_APT probes overlap)
                        isect_probe<FMT>(cur[q], gi, ing, first, last, sh, heads, binstart, present, inm, outm, g, LR,
                                         i < e, ABL(a, 128) != 0);
                    }
                }
#pragma unroll
                for (int q = 0; q < (int)IS_APT; q++) cur[q] = nxt[q];
            }
            __syncthreads();
            // ---- survivors, in order
            if (ABL(a, 2048)) { __syncthreads(); sub = subend; fcur = fend; start_ok = aligned; continue; }   // (timing aid)
            u64 im[IS_APT], om[IS_APT];
#pragma unroll
            for (int q = 0; q < (int)IS_APT; q++) {
                u32 h = q * IS_THREADS + tid;
                flag[q] = false;
                im[q] = om[q] = 0;
                if (h < nheads) {
                    const u64 st = inm[h];
                    flag[q] = (FMT == 0 ? (u32)(st >> 32) : present[h]) == full;
                    im[q] = FMT == 2 ? st : (FMT == 1 ? (st & 0xFFFFFFFFull) : (st & 0xFFFFull));
                    om[q] = FMT == 2 ? outm[h] : (FMT == 1 ? (st >> 32) : ((st >> 16) & 0xFFFFull));
                    if (flag[q] && a.apply_filter && g.D > 0) flag[q] = passes_filter(im[q], om[q], g.D, a.apply_filter);
                }
            }
            const u32 nsurv = compact_flags(flag, pos, masks, mpref);
#pragma unroll
            for (int q = 0; q < (int)IS_APT; q++) {
                if (flag[q]) {
                    kr_cand c;
                    c.prefix = heads[q * IS_THREADS + tid];
                    c.in_mask = im[q];
                    c.out_mask = om[q];
                    a.tmp[(u64)sa + nout + pos[q]] = c;
                }
            }
            nout += nsurv;
            __syncthreads();
        }
        sub = subend;
        fcur = fend;
        start_ok = aligned;
    }
    if (tid == 0) a.chunkcnt[slot] = nout;
}

// ----------------------------------------------------------------------------
// K6b  dense, ordered candidate list from the per-chunk runs
// (launched before the host knows the total: `cap` = room in out[]; when the total exceeds it nothing is
// written and the host, which reads the total after its one synchronisation, grows the list and launches again)
__global__ void k_gather_cands(int sbits, u32 slice, const kr_cand* __restrict__ tmp,
                               const uint4* __restrict__ chunkdesc, const u32* __restrict__ chunkcnt,
                               const u32* __restrict__ chunkpos, kr_cand* __restrict__ out, u32 nunits, u32 cap) {
    if (chunkpos[nunits] > cap) return;
    u32 n = chunkcnt[blockIdx.x];
    if (n == 0) return;
    u64 src = chunkdesc[blockIdx.x].x;
    u32 dst = chunkpos[blockIdx.x];
    const u64 top = sbits ? ((u64)slice << (64 - sbits)) : 0;
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
        kr_cand c = tmp[src + i];
        c.prefix = top | (c.prefix >> sbits);          // relative -> absolute prefix
        out[dst + i] = c;
    }
}

// results the host waits for go straight into its memory (a pinned, device-visible mailbox): one tiny kernel at
// the end of a chain instead of a copy per word -- a 4-byte hipMemcpyAsync is a dispatch of its own with 15-30 us
// around it (profiles/r03: 8 of them per step before every intersection)
__global__ void k_publish(const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ c3,
                          u32* __restrict__ host) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (a) host[0] = *a;
        if (b) host[1] = *b;
        if (c3) host[2] = *c3;
    }
}

// ... the two words finalize() wants of every listed slice (count of oversized buckets, number of keys), one launch for
// all of them: tab lives in pinned host memory beside the mailbox, written by the host right before the launch
struct PubEnt { const u32* ovf; const u32* tot; u32 res; u32 pad; };
__global__ void k_publish_slices(const PubEnt* __restrict__ tab, u32 n, u32* __restrict__ slices) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const PubEnt e = tab[i];
        slices[2 * e.res] = *e.ovf;
        slices[2 * e.res + 1] = *e.tot;
    }
}

// ... the same, `b` (a counter the next round starts from zero) is read and cleared
__global__ void k_publish_reset(const u32* __restrict__ a, u32* __restrict__ b, u32* __restrict__ host) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        host[0] = *a;
        if (b) { host[1] = *b; *b = 0; }
    }
}

// ----------------------------------------------------------------------------
// K7  records of the candidates: for every candidate (a (left,right) prefix, ascending) and
// every listed genome the distinct keys under that prefix with their multiplicities
// (shared.py:210-240: adjacent duplicates fuse, the labels accumulate).  Two passes and a scan,
// no atomics: k_collect_count finds each genome's run of the prefix (binary search inside the
// prefix's fine buckets) and counts its distinct keys; an exclusive scan of the per-candidate
// totals gives every candidate its place; k_collect_emit merges the genomes' runs into
// (key, position of the genome in the call) order -- the order the renderer wants
// (krisp_amd/amplicon.py groups_from_records), so the host does not sort.  A candidate lives in
// exactly one key-space slice.
// ----------------------------------------------------------------------------
#define COL_CAPM 8              // matches of one (candidate, genome) pair the scan of a bucket keeps (more: the genomes are sorted whole)
struct CollectArgs {
    const u64* const* keys;     // [genome * nslices + slice]: sorted (relative) keys
    const u32* const* off;      // [genome * nslices + slice]: fine bucket offsets
    const u32* gid;             // genome ids of the call, in the caller's order
    int n, nslices;
    // KR_OPT_LAZY_ORDER: genomes still in bucket order (ibo[genome] != 0; null = none; 2 = a coarse genome, k_coarse.inc).  k_collect_scan has left the keys of
    // every (candidate, such genome) pair -- found by reading the pair's fine bucket once -- sorted at arena[pair * COL_CAPM ...],
    // mcnt[pair] of them: k_collect_count / k_collect_emit read a pair's run from there instead of the genome
    const u32* ibo;
    const u64* arena;
    const u32* mcnt;
};
// the run of candidate c's prefix in genome gi: keys K[i0 .. e) (for a sorted genome: from the lower bound up to the end of
// the prefix's buckets -- the walk stops at the first other prefix; from the arena: exactly the pair's keys)
__device__ __forceinline__ bool collect_from_arena(const CollectArgs& a, u32 gi) { return a.ibo != nullptr && a.ibo[gi] != 0; }

// first index of genome run: lower bound of the relative prefix `pre` inside its buckets; e = end of those buckets.
// The keys of a fine bucket are spread evenly over its key range (random sequence): the place of `pre` is guessed from
// its bits below the bucket's and met by a gallop + a short binary search -- two or three cache lines instead of the
// six a binary search over ~1500 keys walks (6.5e7 candidates x 2 genomes at configs[4]).
__device__ __forceinline__ u32 collect_lower_bound(const u64* __restrict__ K, const u32* __restrict__ off, u64 pre,
                                                   const Geom& g, u32& e) {
    const u32 f = (u32)(pre >> g.rb);
    const u32 f2 = (u32)((pre | ~g.pmask) >> g.rb) + 1;
    u32 l = off[f], r = off[f2];
    e = r;
    if (f2 == f + 1 && r - l > 32) {
        const u32 frac = (u32)((pre << g.b) >> 32);               // position inside the bucket's key range, 32 bits
        const u32 gs = l + (u32)(((u64)frac * (r - l)) >> 32);      // (< r)
        if (K[gs] < pre) {
            l = gs + 1;
            for (u32 st = 8; ; st *= 2) {
                const u32 p = l + st;
                if (p >= r) break;
                if (K[p] >= pre) { r = p; break; }
                l = p + 1;
            }
        } else {
            r = gs;
            for (u32 st = 8; ; st *= 2) {
                if (r - l <= st) break;
                const u32 p = r - st;
                if (K[p] < pre) { l = p + 1; break; }
                r = p;
            }
        }
    }
    while (l < r) {
        const u32 mid = l + ((r - l) >> 1);
        if (K[mid] < pre) l = mid + 1; else r = mid;
    }
    return l;
}

// A thread per (candidate, genome) -- idx = c * n + gi, so the lanes of a wave walk neighbouring candidates' runs in
// neighbouring genomes' buckets (round 3: a thread per candidate walked its genomes one after the other: 22 ms for
// 6.5e7 candidates of two 3 Gbp genomes).  cnt[idx] = distinct keys of genome gi under candidate c's prefix; the scan
// runs over all ncand * n of them, so a candidate's place is pos[c * n] and nobody adds anything up.
// first[idx] / fmult[idx]: the pair's first key under the prefix and its multiplicity -- all there is to most pairs (one
// distinct key per genome and candidate), and what k_collect_emit works from without reading the genomes again
__global__ __launch_bounds__(256) void k_collect_count(const kr_cand* __restrict__ cands, u32 npairs, CollectArgs a,
                                                       Geom g, u32* __restrict__ lo, u32* __restrict__ cnt,
                                                       u64* __restrict__ first, u32* __restrict__ fmult) {
    const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npairs) return;
    const u32 c = idx / (u32)a.n, gi = idx - c * (u32)a.n;
    u64 pre = cands[c].prefix;                          // absolute
    const u32 s = g.sbits ? (u32)(pre >> (64 - g.sbits)) : 0u;
    pre <<= g.sbits;                                    // relative to its slice
    const u64* __restrict__ K = a.keys[gi * a.nslices + s];
    u32 e, i;
    if (collect_from_arena(a, gi)) {
        K = a.arena + (u64)idx * COL_CAPM;
        i = 0;
        e = a.mcnt[idx];
    } else {
        i = collect_lower_bound(K, a.off[gi * a.nslices + s], pre, g, e);
    }
    lo[idx] = i;
    const u32 i0 = i;
    u32 total = 0, m0 = 0;
    u64 prev = 0, k0 = 0;
    for (; i < e; i++) {
        const u64 key = K[i];
        if ((key & g.pmask) != pre) break;
        total += (i == i0) || key != prev;      // (no sentinel: with k = 32 every 64-bit value is a key)
        if (i == i0) k0 = key;
        m0 += key == k0;
        prev = key;
    }
    cnt[idx] = total;
    first[idx] = k0;
    fmult[idx] = m0;
}

// ... and the records of (c, gi), each to its place in (key, position of the genome in the call) order: the place of
// a key = the candidate's distinct (key', genome') pairs in front of it = over all genomes of the call the distinct
// keys below it, plus the genomes in front of gi that hold the key itself.  The runs are a few keys long and were read
// a moment ago by the neighbouring lanes.
__global__ __launch_bounds__(256) void k_collect_emit(const kr_cand* __restrict__ cands, u32 npairs, CollectArgs a,
                                                      Geom g, const u32* __restrict__ lo, const u32* __restrict__ pos,
                                                      const u64* __restrict__ first, const u32* __restrict__ fmult,
                                                      kr_record* __restrict__ out, u32 cap) {
    const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npairs || pos[npairs] > cap) return;       // (cap: as k_gather_cands)
    if (pos[idx + 1] == pos[idx]) return;                 // (this genome holds nothing under the prefix: a loaded candidate list)
    const u32 n = (u32)a.n;
    const u32 c = idx / n, gi = idx - c * n;
    u64 pre = cands[c].prefix;
    const u32 s = g.sbits ? (u32)(pre >> (64 - g.sbits)) : 0u;
    const u64 top = g.sbits ? ((u64)s << (64 - g.sbits)) : 0;
    pre <<= g.sbits;
    const u32 base = pos[c * n];
    {
        // the usual candidate: at most one distinct key per genome.  Its records are placed from the pairs' first keys
        // (neighbouring lanes' words) -- no genome is read again
        bool simple = true;
        for (u32 gj = 0; gj < n; gj++) simple = simple && pos[c * n + gj + 1] - pos[c * n + gj] <= 1u;
        if (simple) {
            const u64 key = first[idx];
            u32 rank = 0;
            for (u32 gj = 0; gj < n; gj++) {
                if (pos[c * n + gj + 1] == pos[c * n + gj]) continue;
                const u64 k2 = first[c * n + gj];
                rank += (k2 < key) || (k2 == key && gj < gi);
            }
            kr_record rec;
            rec.key = top | (key >> g.sbits);
            rec.genome = a.gid[gi];
            rec.count = fmult[idx];
            out[base + rank] = rec;
            return;
        }
    }
    const u32 f2 = (u32)((pre | ~g.pmask) >> g.rb) + 1;
    const bool mine_arena = collect_from_arena(a, gi);
    const u64* __restrict__ K = mine_arena ? a.arena + (u64)idx * COL_CAPM : a.keys[gi * a.nslices + s];
    const u32 e = mine_arena ? a.mcnt[idx] : a.off[gi * a.nslices + s][f2];
    u32 i = lo[idx];
    while (i < e) {
        const u64 key = K[i];
        if ((key & g.pmask) != pre) break;
        u32 m = 1;
        for (i++; i < e && K[i] == key; i++) m++;
        u32 rank = 0;
        for (u32 gj = 0; gj < n; gj++) {
            const bool their_arena = collect_from_arena(a, gj);
            const u64* __restrict__ K2 = their_arena ? a.arena + (u64)(c * n + gj) * COL_CAPM : a.keys[gj * a.nslices + s];
            const u32 e2 = their_arena ? a.mcnt[c * n + gj] : a.off[gj * a.nslices + s][f2];
            bool first = true;
            u64 prev = 0;
            for (u32 j = lo[c * n + gj]; j < e2; j++) {
                const u64 k2 = K2[j];
                if (k2 > key || (k2 & g.pmask) != pre) break;
                if (first || k2 != prev) rank += (k2 < key) || gj < gi;
                first = false;
                prev = k2;
            }
        }
        kr_record rec;
        rec.key = top | (key >> g.sbits);
        rec.genome = a.gid[gi];
        rec.count = m;
        out[base + rank] = rec;
    }
}

// K7s  KR_OPT_LAZY_ORDER: the genomes of a kr_collect call may still lie in bucket order.  A candidate's run in a genome lies
// inside ONE fine bucket (2 LRrel >= b, the host checks): a wave per (candidate, genome in bucket order) reads that
// bucket once -- ~1500 keys, 12 KB -- keeps the keys under the candidate's prefix (a handful: usually one) and leaves them
// sorted in the pair's arena row.  A pair with more than COL_CAPM keys, or a bucket beyond the LDS sort's capacity, raises
// *overflow: the host then sorts the genomes whole and collects from them.  (Round 6 first sorted the touched buckets in
// place -- k_touch_desc + k_localsort2 per genome: 0.2 ms for 10^4 candidates x 4 genomes; reading them is 0.07.)
__global__ __launch_bounds__(256) void k_collect_scan(const kr_cand* __restrict__ cands, u32 npairs, CollectArgs a, Geom g,
                                                      u64* __restrict__ arena, u32* __restrict__ mcnt, u32* __restrict__ overflow) {
    __shared__ u64 sm[4][COL_CAPM];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 idx = blockIdx.x * 4 + wave;
    if (idx >= npairs) return;
    const u32 c = idx / (u32)a.n, gi = idx - c * (u32)a.n;
    if (a.ibo[gi] != 1u) return;                        // (0: a sorted genome; 2: a coarse one, its rows come from its hit list: k_coarse_rows)
    u64 pre = cands[c].prefix;                          // absolute
    const u32 s = g.sbits ? (u32)(pre >> (64 - g.sbits)) : 0u;
    pre <<= g.sbits;
    const u32 f = (u32)(pre >> g.rb);
    const u64* __restrict__ K = a.keys[gi * a.nslices + s];
    const u32* __restrict__ off = a.off[gi * a.nslices + s];
    const u32 lo = off[f], hi = off[f + 1];
    u32 m = 0;                                          // matches so far (wave-uniform)
    for (u32 i0 = lo; i0 < hi; i0 += 64) {
        const u32 i = i0 + lane;
        const u64 key = i < hi ? K[i] : 0;
        const bool hit = i < hi && (key & g.pmask) == pre;
        const u64 bal = __ballot(hit);
        if (bal) {
            const u32 at = m + (u32)__popcll(bal & ((1ull << lane) - 1));
            if (hit && at < COL_CAPM) sm[wave][at] = key;
            m += (u32)__popcll(bal);
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (m > COL_CAPM) {
        if (lane == 0) { atomicAdd(overflow, 1u); mcnt[idx] = 0; }
        return;
    }
    // rank by counting among the <= COL_CAPM matches (equal keys keep their arrival order)
    if (lane < m) {
        const u64 key = sm[wave][lane];
        u32 r = 0;
        for (u32 j = 0; j < m; j++) {
            const u64 o = sm[wave][j];
            r += (o < key) || (o == key && j < lane);
        }
        arena[(u64)idx * COL_CAPM + r] = key;
    }
    if (lane == 0) mcnt[idx] = m;
}

// ----------------------------------------------------------------------------
// K8  candidate list (x) candidate list, and/or the diagnostic filter
// ----------------------------------------------------------------------------
// (m_dev != nullptr: the length of `other` is read on the device -- word 0 of the header that travels behind a list in
// the multi-GPU exchange, h_comm.inc: the host launches the merge without having seen the count)
__global__ void k_cands_flag(kr_cand* __restrict__ cur, u32 n, const kr_cand* __restrict__ other, u32 m,
                             int have_other, int apply_filter, int D, u32* __restrict__ flags,
                             u32* __restrict__ blockcnt, const u64* __restrict__ m_dev) {
    __shared__ u32 waves[17];
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (m_dev) m = (u32)m_dev[0];
    if (i < n) {
        kr_cand c = cur[i];
        keep = true;
        if (have_other) {
            u32 l = 0, r = m;
            while (l < r) {
                u32 mid = l + ((r - l) >> 1);
                if (other[mid].prefix < c.prefix) l = mid + 1; else r = mid;
            }
            if (l < m && other[l].prefix == c.prefix) {
                c.in_mask |= other[l].in_mask;
                c.out_mask |= other[l].out_mask;
                cur[i] = c;
            } else {
                keep = false;
            }
        }
        if (keep && apply_filter && D > 0) keep = passes_filter(c.in_mask, c.out_mask, D, apply_filter);
        flags[i] = keep ? 1u : 0u;
    }
    u32 tot;
    block_compact(keep, waves, tot);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = tot;
}

// Genomes join a candidate list instead of an intersection (kr_cands_probe, round 5: the streaming flow of genome sets
// beyond one GPU's memory -- a later batch's genomes look the running candidates up instead of being intersected whole).
// Every candidate looks its prefix up in each genome, given as tables [genome][slice] (ingroup_bits by position): absent
// anywhere -> dropped; else the genome's diagnostic bases join the masks and the filter is applied -- safe on partial
// masks, the predicate is monotone (masks only grow).  flags / blockcnt as k_cands_flag leaves them; slice-aware as
// k_collect_count is (the candidate's slice = the top bits of its absolute prefix).
__global__ void k_cands_probe_tab(kr_cand* __restrict__ cur, u32 n, CollectArgs a, u32 ingroup_bits, int apply_filter, Geom g,
                                  u32* __restrict__ flags, u32* __restrict__ blockcnt) {
    __shared__ u32 waves[17];
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    if (i < n) {
        kr_cand c = cur[i];
        keep = true;
        u64 pre = c.prefix;                                 // absolute
        const u32 s = g.sbits ? (u32)(pre >> (64 - g.sbits)) : 0u;
        pre <<= g.sbits;                                    // relative to its slice
        for (int gi = 0; gi < a.n && keep; gi++) {
            const u64* __restrict__ K = a.keys[gi * a.nslices + s];
            u32 e;
            u32 p = collect_lower_bound(K, a.off[gi * a.nslices + s], pre, g, e);
            u64 dm = 0;
            bool found = false;
            for (; p < e; p++) {
                const u64 key = K[p];
                if ((key & g.pmask) != pre) break;
                found = true;
                dm |= diag_mask(key, g.LRrel, g.D);
            }
            keep = found;
            if ((ingroup_bits >> gi) & 1u) c.in_mask |= dm; else c.out_mask |= dm;
        }
        if (keep && apply_filter && g.D > 0) keep = passes_filter(c.in_mask, c.out_mask, g.D, apply_filter);
        if (keep) cur[i] = c;
        flags[i] = keep ? 1u : 0u;
    }
    u32 tot;
    block_compact(keep, waves, tot);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = tot;
}

__global__ void k_cands_compact(const kr_cand* __restrict__ cur, u32 n, const u32* __restrict__ flags,
                                const u32* __restrict__ blockpos, kr_cand* __restrict__ out) {
    __shared__ u32 waves[17];
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = i < n && flags[i] != 0;
    u32 tot;
    u32 pos = block_compact(keep, waves, tot);
    if (keep) out[blockpos[blockIdx.x] + pos] = cur[i];
}
