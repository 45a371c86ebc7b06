// k_design.inc -- part of krisp_hip.hip (one translation unit): the primer design pass (--design-primers, DESIGN §15): a
// primer pair per region, every figure an integer.  The host driver is h_design.inc; the model's integers and the options
// arrive in a kr_design_params on the device (the library holds no table of its own).
//
// k_design: a workgroup of ONE wavefront per region, so every step below is in lockstep and the running best pair lives
// in registers.  In LDS: the model's 40 table entries, and per side (0: the left flank as written, 1: the reverse
// complement of the right flank, so that a primer of either side is a substring read 5'->3') the base codes, the prefix
// sums of the steps' dH and dS, a packed prefix count (G or C | other letters | ends of 5 equal bases: 10 bits each), and a
// DENSE table of penalties, one u32 per (length, start): DES_DEAD where the candidate does not exist or fails a filter.
//   1a  a lane per candidate: letters, GC, poly-X, clamp, end GC and Tm are O(1) from the prefixes -> its penalty.
//   1b  the wave per surviving candidate: its self duplex figure (des_duplex: a lane per alignment, a walk along it).
//   2   the rows of the left table in order; a row that cannot beat the best so far with the least right penalty is
//       skipped; 64 right candidates a step: product size and (penalty, tie key) < best are a lane's test, the pair duplex
//       is run by the wave on the lanes that pass, lowest key of the step first.  best only ever takes a pair that passed
//       everything, and a pair is only passed over when its key is not below best: the result is the definition's argmin.
//   3   the winner's figures again, one 64-byte record by plain vector stores.  No atomics, no scratch buffer in memory.
// k_design<true> (kr_design_hairpins, DESIGN §17) also holds every candidate to max_sec for its hairpin figure: the loop
// table (54 ints, loop lengths 3 .. 56) lies in LDS behind the model's, 1b runs des_hairpin on a survivor of 1a before its
// self duplex, and 3 stores the winner's two figures into a second array of 8 bytes a region.  k_design<false> is the
// kernel without any of it.
// k_design_top (kr_design_run_top, DESIGN §25; behind k_design below) keeps the `top` least passing pairs of a region in
// the place of the least: 2's bound is the top-th least key so far, 3 runs once per slot.
#define DES_T 64
#define DES_DEAD 0xffffffffu
#define DES_TAB 48                  // ints of the table in LDS: nn_dh 16, nn_ds 16, term_dh 4, term_ds 4 (40, padded)
#define DES_MAX_FLANK 1023          // (10-bit prefix counts)
#define DES_MAX_TEMPLATE 2047       // (11-bit starts in the key)
#define DES_MIN_LOOP 3              // bases a hairpin's innermost pair encloses at least ...
#define DES_MAX_LOOP 56             // ... and at most: 60 bases, two pairs
#define DES_LOOP_TAB 56             // ints of the loop table in LDS: entry l - DES_MIN_LOOP, 54 used

struct DesignGeom {
    u32 L, D, R, W;
    u32 len[2], nlen[2];            // per side: letters, primer lengths that fit (size_lo .. min(size_hi, len))
    u32 o_code[2], o_ph[2], o_ps[2], o_pc[2], o_pen[2];     // byte offsets in the dynamic LDS
    u32 lds_bytes;
};

struct DesSide {
    const uint8_t* code;
    const int* ph;
    const int* ps;
    const u32* pc;
    u32* pen;
    u32 len, nlen;
};

__host__ __device__ inline void design_geom(int L, int D, int R, int size_lo, int size_hi, bool hairpins, DesignGeom* g) {
    g->L = (u32)L; g->D = (u32)D; g->R = (u32)R; g->W = (u32)(L + D + R);
    g->len[0] = (u32)L; g->len[1] = (u32)R;
    u32 o = (DES_TAB + (hairpins ? DES_LOOP_TAB : 0)) * 4;
    for (int q = 0; q < 2; q++) {
        const int n = (int)g->len[q];
        const int top = size_hi < n ? size_hi : n;
        g->nlen[q] = top >= size_lo ? (u32)(top - size_lo + 1) : 0u;
        g->o_code[q] = o; o += ((u32)n + 3u) & ~3u;
        g->o_ph[q] = o; o += ((u32)n + 1) * 4;
        g->o_ps[q] = o; o += ((u32)n + 1) * 4;
        g->o_pc[q] = o; o += ((u32)n + 1) * 4;
        g->o_pen[q] = o; o += g->nlen[q] * (u32)n * 4;
    }
    g->lds_bytes = (o + 15u) & ~15u;
}

__device__ __forceinline__ int des_wave_max(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ u32 des_wave_min(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, (u32)__shfl_xor((int)v, o, 64));
    return v;
}

__device__ __forceinline__ int des_wave_scan(int v, u32 lane) {       // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if ((int)lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ u32 des_code(uint8_t ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }

// Tm in mK of the duplex of the bases [a, b] of a side with its complement: (dH 10^6) // dS, both negative (kr_design_table
// has checked that the model keeps them so), extra = what the caller adds to dS beside the salt (concentration, symmetry)
__device__ __forceinline__ int des_tm(const int* tab, const DesSide& X, u32 a, u32 b, int salt, int extra) {
    const u32 ca = X.code[a], cb = X.code[b];
    const long long dh = (long long)(X.ph[b] - X.ph[a]) + tab[32 + ca] + tab[32 + cb];
    const long long ds = (long long)(X.ps[b] - X.ps[a]) + tab[36 + ca] + tab[36 + cb] + (long long)salt * (int)(b - a) + extra;
    return (int)((u64)(-dh * 1000000ll) / (u64)(-ds));
}

// the oligo [u, u + n) of a side alone: is it its own reverse complement, and its Tm
__device__ __forceinline__ int des_oligo_tm(const int* tab, const DesSide& X, u32 u, u32 n, const kr_design_params* __restrict__ P) {
    bool self = !(n & 1u);
    for (u32 k = 0; self && k < n / 2; k++) self = X.code[u + k] + X.code[u + n - 1 - k] == 3u;
    return des_tm(tab, X, u, u + n - 1, P->salt_ds, self ? P->conc_self_ds + P->sym_ds : P->conc_ds);
}

// the duplex figure of the oligos X[xu, xu + nx) and Y[yu, yu + ny), by the whole wave: a lane per antiparallel alignment
// c = i + j, a walk along i; every maximal run of >= 2 Watson-Crick pairs gives the Tm of its bases on X; `end` takes the
// runs that hold the 3' base of X (i = nx - 1) or of Y (j = ny - 1).  Both results are the same in every lane.
__device__ __forceinline__ void des_duplex(const int* tab, const DesSide& X, u32 xu, u32 nx, const DesSide& Y, u32 yu, u32 ny, int salt,
                                           int conc, u32 lane, int* any_out, int* end_out) {
    int any = 0, end = 0;
    const int nd = (int)(nx + ny) - 1;
    for (int c = (int)lane; c < nd; c += DES_T) {
        const int ilo = max(0, c - ((int)ny - 1)), ihi = min((int)nx - 1, c);
        int run0 = -1;
        for (int i = ilo; i <= ihi + 1; i++) {
            const bool pair = i <= ihi && X.code[xu + i] + Y.code[yu + c - i] == 3u;
            if (pair) {
                if (run0 < 0) run0 = i;
            } else if (run0 >= 0) {
                const int i1 = i - 1;
                if (i1 > run0) {
                    const int tm = des_tm(tab, X, xu + run0, xu + i1, salt, conc);
                    any = max(any, tm);
                    if (i1 == (int)nx - 1 || c - run0 == (int)ny - 1) end = max(end, tm);
                }
                run0 = -1;
            }
        }
    }
    *any_out = des_wave_max(any);
    *end_out = des_wave_max(end);
}

// the hairpin figure of the oligo X[u, u + n) (DESIGN §17), by the whole wave: a lane per fold c = i + j, 4 <= c <= 2 n - 6
// (2 n - 9 folds: a second round of lanes from n = 37 on), a walk along i from the outermost pair inwards as far as j - i
// >= 4 holds; every maximal run of >= 2 Watson-Crick pairs gives the Tm of its bases on the 5' arm with the loop's dS
// (loop[l - DES_MIN_LOOP], l = the bases the innermost pair encloses) in the place of the concentration term.  The same in
// every lane.
__device__ __forceinline__ int des_hairpin(const int* tab, const int* loop, const DesSide& X, u32 u, u32 n, int salt, u32 lane) {
    int hp = 0;
    const int last = 2 * (int)n - 6;
    for (int c = 4 + (int)lane; c <= last; c += DES_T) {
        const int ilo = max(0, c - ((int)n - 1)), ihi = (c - 4) >> 1;
        int run0 = -1;
        for (int i = ilo; i <= ihi + 1; i++) {
            const bool pair = i <= ihi && X.code[u + i] + X.code[u + c - i] == 3u;
            if (pair) {
                if (run0 < 0) run0 = i;
            } else if (run0 >= 0) {
                const int i1 = i - 1;
                if (i1 > run0) hp = max(hp, des_tm(tab, X, u + run0, u + i1, salt, loop[c - 2 * i1 - 1 - DES_MIN_LOOP]));
                run0 = -1;
            }
        }
    }
    return des_wave_max(hp);
}

__device__ __forceinline__ u64 des_key(u32 pen, u32 ls, u32 ln, u32 rs, u32 rn) {
    return ((u64)pen << 34) | ((u64)ls << 23) | ((u64)ln << 17) | ((u64)rs << 6) | rn;
}

// P: the kr_design_params and, for HP, behind them the 64 ints of a kr_hairpin_params; hp_out: HP only
template <bool HP>
__global__ __launch_bounds__(DES_T) void k_design(const uint8_t* __restrict__ templates, u32 nregions, DesignGeom g,
                                                  const kr_design_params* __restrict__ P, kr_design_record* __restrict__ out,
                                                  int2* __restrict__ hp_out) {
    extern __shared__ __align__(16) u32 des_lds[];
    const u32 region = blockIdx.x, lane = threadIdx.x;
    if (region >= nregions) return;
    unsigned char* const lds = (unsigned char*)des_lds;
    int* const tab = (int*)des_lds;
    const int* const loop = tab + DES_TAB;
    uint8_t* codew[2];
    int* phw[2];
    int* psw[2];
    u32* pcw[2];
    DesSide S[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        codew[q] = lds + g.o_code[q];
        phw[q] = (int*)(lds + g.o_ph[q]);
        psw[q] = (int*)(lds + g.o_ps[q]);
        pcw[q] = (u32*)(lds + g.o_pc[q]);
        S[q].code = codew[q]; S[q].ph = phw[q]; S[q].ps = psw[q]; S[q].pc = pcw[q];
        S[q].pen = (u32*)(lds + g.o_pen[q]);
        S[q].len = g.len[q]; S[q].nlen = g.nlen[q];
    }
    const int lo = P->size_lo, hi = P->size_hi, salt = P->salt_ds, conc = P->conc_ds, max_sec = P->max_sec;

    // ---- the table, the codes of both sides
    if (lane < 40) tab[lane] = ((const int*)P)[lane];
    if (HP && lane < DES_MAX_LOOP - DES_MIN_LOOP + 1) tab[DES_TAB + lane] = ((const int*)(P + 1))[DES_MIN_LOOP + lane];
    const uint8_t* T = templates + (u64)region * g.W;
    for (u32 i = lane; i < g.L; i += DES_T) codew[0][i] = (uint8_t)des_code(T[i]);
    for (u32 i = lane; i < g.R; i += DES_T) {
        const u32 cd = des_code(T[g.W - 1 - i]);
        codew[1][i] = (uint8_t)(cd < 4u ? 3u - cd : 4u);
    }
    __syncthreads();

    // ---- prefix sums along each side, 64 positions a step: entry i + 1 holds the steps (i, i + 1) .. and the letters .. i
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const u32 n = g.len[q];
        int ch = 0, cs = 0, cc = 0;
        if (lane == 0) { phw[q][0] = 0; psw[q][0] = 0; pcw[q][0] = 0; }
        for (u32 base = 0; base < n; base += DES_T) {
            const u32 i = base + lane;
            int h = 0, s = 0, cnt = 0;
            if (i < n) {
                const u32 a = codew[q][i];
                if (i + 1 < n) {
                    const u32 b = codew[q][i + 1];
                    if (a < 4u && b < 4u) { h = tab[4 * a + b]; s = tab[16 + 4 * a + b]; }
                }
                bool five = i >= 4;
                for (u32 k = 1; five && k < 5; k++) five = codew[q][i - k] == a;
                cnt = (int)((a == 1u || a == 2u) ? 1u : 0u) | (int)((a >= 4u ? 1u : 0u) << 10) | (int)((five ? 1u : 0u) << 20);
            }
            h = des_wave_scan(h, lane) + ch;
            s = des_wave_scan(s, lane) + cs;
            cnt = des_wave_scan(cnt, lane) + cc;          // (three 10-bit counts, none above 1023: no carry between them)
            if (i < n) { phw[q][i + 1] = h; psw[q][i + 1] = s; pcw[q][i + 1] = (u32)cnt; }
            ch = __shfl(h, 63, 64); cs = __shfl(s, 63, 64); cc = __shfl(cnt, 63, 64);
        }
    }
    __syncthreads();

    // ---- 1a: a lane per candidate
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const DesSide& X = S[q];
        const u32 total = X.nlen * X.len;
        for (u32 e = lane; e < total; e += DES_T) {
            const u32 n = (u32)lo + e / X.len, u = e % X.len;
            u32 pen = DES_DEAD;
            if (u + n <= X.len) {
                const u32 pe = X.pc[u + n], pu = X.pc[u];
                const int gc = (int)(pe & 1023u) - (int)(pu & 1023u);
                const bool letters = ((pe >> 10) & 1023u) == ((pu >> 10) & 1023u);
                const bool poly = (pe >> 20) != (X.pc[u + 4] >> 20);
                const int clamp = (int)(pe & 1023u) - (int)(X.pc[u + n - (u32)P->gc_clamp] & 1023u);
                const int endgc = (int)(pe & 1023u) - (int)(X.pc[u + n - 5] & 1023u);
                if (letters && !poly && 100 * gc >= P->gc_lo * (int)n && 100 * gc <= P->gc_hi * (int)n && clamp == P->gc_clamp &&
                    endgc <= P->max_end_gc) {
                    const int tm = des_oligo_tm(tab, X, u, n, P);
                    if (tm >= P->tm_lo && tm <= P->tm_hi) pen = (u32)(abs(tm - P->tm_opt) + 500 * abs(2 * (int)n - (lo + hi)));
                }
            }
            X.pen[e] = pen;
        }
    }
    __syncthreads();

    // ---- 1b: the wave per survivor: (its hairpin figure,) self_any and self_end
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const DesSide& X = S[q];
        const u32 total = X.nlen * X.len;
        for (u32 base = 0; base < total; base += DES_T) {
            const u32 e = base + lane;
            u64 mask = __ballot(e < total && X.pen[e] != DES_DEAD);
            while (mask) {
                const u32 e2 = base + (u32)__ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u32 n = (u32)lo + e2 / X.len, u = e2 % X.len;
                if (HP && des_hairpin(tab, loop, X, u, n, salt, lane) > max_sec) {
                    if (lane == 0) X.pen[e2] = DES_DEAD;
                    continue;
                }
                int any, end;
                des_duplex(tab, X, u, n, X, u, n, salt, conc, lane, &any, &end);
                if ((any > max_sec || end > max_sec) && lane == 0) X.pen[e2] = DES_DEAD;
            }
        }
    }
    __syncthreads();

    // ---- 2: the best pair
    const DesSide& A = S[0];
    const DesSide& B = S[1];
    const u32 totl = A.nlen * A.len, totr = B.nlen * B.len;
    u32 minr = DES_DEAD;
    for (u32 e = lane; e < totr; e += DES_T) minr = min(minr, B.pen[e]);
    minr = des_wave_min(minr);
    u64 best = ~0ull;
    if (minr != DES_DEAD) {
#pragma unroll 1
        for (u32 el = 0; el < totl; el++) {
            const u32 pl = A.pen[el];
            if (pl == DES_DEAD || (u64)pl + minr > (best >> 34)) continue;
            const u32 nl = (u32)lo + el / A.len, ul = el % A.len;
            for (u32 base = 0; base < totr; base += DES_T) {
                const u32 er = base + lane;
                u64 key = ~0ull;
                if (er < totr) {
                    const u32 pr = B.pen[er];
                    if (pr != DES_DEAD) {
                        const u32 nr = (u32)lo + er / B.len, ur = er % B.len;
                        const int size = (int)(g.W - ur - ul);            // first base of the left primer .. last of the right site
                        if (size >= P->amp_lo && size <= P->amp_hi) key = des_key(pl + pr, ul, nl, g.W - ur - nr, nr);
                    }
                }
                u64 mask = __ballot(key < best);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const u64 k = ((u64)(u32)__shfl((int)(key >> 32), l, 64) << 32) | (u32)__shfl((int)(u32)key, l, 64);
                    if (k >= best) continue;
                    const u32 e2 = base + (u32)l;
                    int any, end;
                    des_duplex(tab, A, ul, nl, B, e2 % B.len, (u32)lo + e2 / B.len, salt, conc, lane, &any, &end);
                    if (any <= max_sec && end <= max_sec) best = k;
                }
            }
        }
    }

    // ---- 3: the record
    const bool found = best != ~0ull;
    const u32 ls = found ? (u32)(best >> 23) & 2047u : 0u, ln = found ? (u32)(best >> 17) & 63u : (u32)lo;
    const u32 rs = found ? (u32)(best >> 6) & 2047u : g.W - (u32)lo, rn = found ? (u32)best & 63u : (u32)lo;
    const u32 ur = g.W - rs - rn;
    int lsa = 0, lse = 0, rsa = 0, rse = 0, pa = 0, pe = 0;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
    if (found) {
        des_duplex(tab, A, ls, ln, A, ls, ln, salt, conc, lane, &lsa, &lse);
        des_duplex(tab, B, ur, rn, B, ur, rn, salt, conc, lane, &rsa, &rse);
        des_duplex(tab, A, ls, ln, B, ur, rn, salt, conc, lane, &pa, &pe);
        // (kr_design_record, little endian: found, product_size, pair_penalty, the four u16 of the pair; the two Tm, the
        // two u16 GC counts, the two penalties)
        w0 = make_uint4(1u, rs + rn - ls, (u32)(best >> 34), ls | (ln << 16));
        w1 = make_uint4(rs | (rn << 16), (u32)des_oligo_tm(tab, A, ls, ln, P), (u32)des_oligo_tm(tab, B, ur, rn, P),
                        ((A.pc[ls + ln] & 1023u) - (A.pc[ls] & 1023u)) | (((B.pc[ur + rn] & 1023u) - (B.pc[ur] & 1023u)) << 16));
    }
    if (lane == 0) {
        uint4* o = (uint4*)(out + region);
        o[0] = w0;
        o[1] = w1;
        o[2] = found ? make_uint4(A.pen[(ln - (u32)lo) * A.len + ls], B.pen[(rn - (u32)lo) * B.len + ur], (u32)lsa, (u32)lse) : w0;
        o[3] = make_uint4((u32)rsa, (u32)rse, (u32)pa, (u32)pe);
    }
    if (HP) {
        int2 hp = make_int2(0, 0);
        if (found) hp = make_int2(des_hairpin(tab, loop, A, ls, ln, salt, lane), des_hairpin(tab, loop, B, ur, rn, salt, lane));
        if (lane == 0) hp_out[region] = hp;
    }
}

__device__ __forceinline__ u64 des_shfl64(u64 v, int l) {
    return ((u64)(u32)__shfl((int)(v >> 32), l, 64) << 32) | (u32)__shfl((int)(u32)v, l, 64);
}

// ---- the shortlist kernel of --primer-candidates (DESIGN §25).  k_design_top's steps are the inline pieces below: des_tables
// (the tables, 1a and 1b, statement for statement k_design's) and des_record (3 for one key, which k_design_top runs per
// slot).  k_design above does not call them: built from these pieces it computes the same records but compiles to other
// registers (60 VGPRs and 95 / 90 SGPRs against 62 and 93 / 88), and the pass that every run of --design-primers takes keeps
// the code it was measured with.  A change to a step of k_design belongs in both places; tests/test_gpu_design_shortlist.py
// holds slot 0 of k_design_top to k_design's bytes.
//
// des_tables: the model's table, both sides' codes, prefixes and penalty tables of `region` in the LDS at `lds`, the
// survivors of 1a and 1b marked -> S[0], S[1]; ends with a barrier
template <bool HP>
__device__ __forceinline__ void des_tables(unsigned char* const lds, const uint8_t* __restrict__ templates, u32 region, u32 lane,
                                           const DesignGeom& g, const kr_design_params* __restrict__ P, DesSide (&S)[2]) {
    int* const tab = (int*)lds;
    const int* const loop = tab + DES_TAB;
    uint8_t* codew[2];
    int* phw[2];
    int* psw[2];
    u32* pcw[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        codew[q] = lds + g.o_code[q];
        phw[q] = (int*)(lds + g.o_ph[q]);
        psw[q] = (int*)(lds + g.o_ps[q]);
        pcw[q] = (u32*)(lds + g.o_pc[q]);
        S[q].code = codew[q]; S[q].ph = phw[q]; S[q].ps = psw[q]; S[q].pc = pcw[q];
        S[q].pen = (u32*)(lds + g.o_pen[q]);
        S[q].len = g.len[q]; S[q].nlen = g.nlen[q];
    }
    const int lo = P->size_lo, hi = P->size_hi, salt = P->salt_ds, conc = P->conc_ds, max_sec = P->max_sec;

    // ---- the table, the codes of both sides
    if (lane < 40) tab[lane] = ((const int*)P)[lane];
    if (HP && lane < DES_MAX_LOOP - DES_MIN_LOOP + 1) tab[DES_TAB + lane] = ((const int*)(P + 1))[DES_MIN_LOOP + lane];
    const uint8_t* T = templates + (u64)region * g.W;
    for (u32 i = lane; i < g.L; i += DES_T) codew[0][i] = (uint8_t)des_code(T[i]);
    for (u32 i = lane; i < g.R; i += DES_T) {
        const u32 cd = des_code(T[g.W - 1 - i]);
        codew[1][i] = (uint8_t)(cd < 4u ? 3u - cd : 4u);
    }
    __syncthreads();

    // ---- prefix sums along each side, 64 positions a step: entry i + 1 holds the steps (i, i + 1) .. and the letters .. i
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const u32 n = g.len[q];
        int ch = 0, cs = 0, cc = 0;
        if (lane == 0) { phw[q][0] = 0; psw[q][0] = 0; pcw[q][0] = 0; }
        for (u32 base = 0; base < n; base += DES_T) {
            const u32 i = base + lane;
            int h = 0, s = 0, cnt = 0;
            if (i < n) {
                const u32 a = codew[q][i];
                if (i + 1 < n) {
                    const u32 b = codew[q][i + 1];
                    if (a < 4u && b < 4u) { h = tab[4 * a + b]; s = tab[16 + 4 * a + b]; }
                }
                bool five = i >= 4;
                for (u32 k = 1; five && k < 5; k++) five = codew[q][i - k] == a;
                cnt = (int)((a == 1u || a == 2u) ? 1u : 0u) | (int)((a >= 4u ? 1u : 0u) << 10) | (int)((five ? 1u : 0u) << 20);
            }
            h = des_wave_scan(h, lane) + ch;
            s = des_wave_scan(s, lane) + cs;
            cnt = des_wave_scan(cnt, lane) + cc;          // (three 10-bit counts, none above 1023: no carry between them)
            if (i < n) { phw[q][i + 1] = h; psw[q][i + 1] = s; pcw[q][i + 1] = (u32)cnt; }
            ch = __shfl(h, 63, 64); cs = __shfl(s, 63, 64); cc = __shfl(cnt, 63, 64);
        }
    }
    __syncthreads();

    // ---- 1a: a lane per candidate
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const DesSide& X = S[q];
        const u32 total = X.nlen * X.len;
        for (u32 e = lane; e < total; e += DES_T) {
            const u32 n = (u32)lo + e / X.len, u = e % X.len;
            u32 pen = DES_DEAD;
            if (u + n <= X.len) {
                const u32 pe = X.pc[u + n], pu = X.pc[u];
                const int gc = (int)(pe & 1023u) - (int)(pu & 1023u);
                const bool letters = ((pe >> 10) & 1023u) == ((pu >> 10) & 1023u);
                const bool poly = (pe >> 20) != (X.pc[u + 4] >> 20);
                const int clamp = (int)(pe & 1023u) - (int)(X.pc[u + n - (u32)P->gc_clamp] & 1023u);
                const int endgc = (int)(pe & 1023u) - (int)(X.pc[u + n - 5] & 1023u);
                if (letters && !poly && 100 * gc >= P->gc_lo * (int)n && 100 * gc <= P->gc_hi * (int)n && clamp == P->gc_clamp &&
                    endgc <= P->max_end_gc) {
                    const int tm = des_oligo_tm(tab, X, u, n, P);
                    if (tm >= P->tm_lo && tm <= P->tm_hi) pen = (u32)(abs(tm - P->tm_opt) + 500 * abs(2 * (int)n - (lo + hi)));
                }
            }
            X.pen[e] = pen;
        }
    }
    __syncthreads();

    // ---- 1b: the wave per survivor: (its hairpin figure,) self_any and self_end
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const DesSide& X = S[q];
        const u32 total = X.nlen * X.len;
        for (u32 base = 0; base < total; base += DES_T) {
            const u32 e = base + lane;
            u64 mask = __ballot(e < total && X.pen[e] != DES_DEAD);
            while (mask) {
                const u32 e2 = base + (u32)__ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u32 n = (u32)lo + e2 / X.len, u = e2 % X.len;
                if (HP && des_hairpin(tab, loop, X, u, n, salt, lane) > max_sec) {
                    if (lane == 0) X.pen[e2] = DES_DEAD;
                    continue;
                }
                int any, end;
                des_duplex(tab, X, u, n, X, u, n, salt, conc, lane, &any, &end);
                if ((any > max_sec || end > max_sec) && lane == 0) X.pen[e2] = DES_DEAD;
            }
        }
    }
    __syncthreads();
}

// 3: the record of the pair `key` names (des_key; ~0: no pair, all zero) at out, by plain vector stores of lane 0, and for HP
// its two hairpin figures at hp_out.  Every figure is computed again by the whole wave
template <bool HP>
__device__ __forceinline__ void des_record(const int* tab, const DesSide& A, const DesSide& B, const DesignGeom& g,
                                           const kr_design_params* __restrict__ P, u32 lane, u64 key,
                                           kr_design_record* __restrict__ out, int2* __restrict__ hp_out) {
    const int* const loop = tab + DES_TAB;
    const int lo = P->size_lo, salt = P->salt_ds, conc = P->conc_ds;
    const bool found = key != ~0ull;
    const u32 ls = found ? (u32)(key >> 23) & 2047u : 0u, ln = found ? (u32)(key >> 17) & 63u : (u32)lo;
    const u32 rs = found ? (u32)(key >> 6) & 2047u : g.W - (u32)lo, rn = found ? (u32)key & 63u : (u32)lo;
    const u32 ur = g.W - rs - rn;
    int lsa = 0, lse = 0, rsa = 0, rse = 0, pa = 0, pe = 0;
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
    if (found) {
        des_duplex(tab, A, ls, ln, A, ls, ln, salt, conc, lane, &lsa, &lse);
        des_duplex(tab, B, ur, rn, B, ur, rn, salt, conc, lane, &rsa, &rse);
        des_duplex(tab, A, ls, ln, B, ur, rn, salt, conc, lane, &pa, &pe);
        // (kr_design_record, little endian: found, product_size, pair_penalty, the four u16 of the pair; the two Tm, the
        // two u16 GC counts, the two penalties)
        w0 = make_uint4(1u, rs + rn - ls, (u32)(key >> 34), ls | (ln << 16));
        w1 = make_uint4(rs | (rn << 16), (u32)des_oligo_tm(tab, A, ls, ln, P), (u32)des_oligo_tm(tab, B, ur, rn, P),
                        ((A.pc[ls + ln] & 1023u) - (A.pc[ls] & 1023u)) | (((B.pc[ur + rn] & 1023u) - (B.pc[ur] & 1023u)) << 16));
    }
    if (lane == 0) {
        uint4* o = (uint4*)out;
        o[0] = w0;
        o[1] = w1;
        o[2] = found ? make_uint4(A.pen[(ln - (u32)lo) * A.len + ls], B.pen[(rn - (u32)lo) * B.len + ur], (u32)lsa, (u32)lse) : w0;
        o[3] = make_uint4((u32)rsa, (u32)rse, (u32)pa, (u32)pe);
    }
    if (HP) {
        int2 hp = make_int2(0, 0);
        if (found) hp = make_int2(des_hairpin(tab, loop, A, ls, ln, salt, lane), des_hairpin(tab, loop, B, ur, rn, salt, lane));
        if (lane == 0) *hp_out = hp;
    }
}

// k_design_top (--primer-candidates, DESIGN §25): the `top` least keys of a region's passing pairs, 1 <= top <= DES_MAX_TOP,
// as records out[region * top + j], j = rank - 1, and for HP their hairpin figures hp_out[region * top + j]; a slot beyond
// the region's pairs is zero.  The tables, 1a and 1b are k_design's.  2 is its branch-and-bound with the bound at the
// top-th least accepted key so far (~0 while fewer are held): the row skip, the ballot and the re-test read that bound, a
// pair enters the list only after its pair duplex passes, and every (el, er) is visited once, so no key enters twice.  The
// list is one register a lane: lane j holds the (j + 1)-th least accepted key, ~0 behind the last, ascending over the wave.
// An insert is a ballot of the lanes whose key is greater, a __shfl_up of those lanes and the new key into the first of
// them (what falls off lane top - 1 moves on to the lanes behind it, which nothing reads); the bound is a __shfl of lane
// top - 1.  Every value of 2 is wave-uniform but that register: no indexed array, no scratch.  3 runs once per slot.
#define DES_MAX_TOP 8

template <bool HP>
__global__ __launch_bounds__(DES_T) void k_design_top(const uint8_t* __restrict__ templates, u32 nregions, DesignGeom g,
                                                      const kr_design_params* __restrict__ P, u32 top,
                                                      kr_design_record* __restrict__ out, int2* __restrict__ hp_out) {
    extern __shared__ __align__(16) u32 des_lds[];
    const u32 region = blockIdx.x, lane = threadIdx.x;
    if (region >= nregions) return;
    const int* const tab = (const int*)des_lds;
    DesSide S[2];
    des_tables<HP>((unsigned char*)des_lds, templates, region, lane, g, P, S);
    const int lo = P->size_lo, salt = P->salt_ds, conc = P->conc_ds, max_sec = P->max_sec;

    // ---- 2: the top least pairs
    const DesSide& A = S[0];
    const DesSide& B = S[1];
    const u32 totl = A.nlen * A.len, totr = B.nlen * B.len;
    u32 minr = DES_DEAD;
    for (u32 e = lane; e < totr; e += DES_T) minr = min(minr, B.pen[e]);
    minr = des_wave_min(minr);
    u64 mine = ~0ull, bound = ~0ull;                // this lane's key of the list; the key of lane top - 1
    if (minr != DES_DEAD) {
#pragma unroll 1
        for (u32 el = 0; el < totl; el++) {
            const u32 pl = A.pen[el];
            if (pl == DES_DEAD || (u64)pl + minr > (bound >> 34)) continue;
            const u32 nl = (u32)lo + el / A.len, ul = el % A.len;
            for (u32 base = 0; base < totr; base += DES_T) {
                const u32 er = base + lane;
                u64 key = ~0ull;
                if (er < totr) {
                    const u32 pr = B.pen[er];
                    if (pr != DES_DEAD) {
                        const u32 nr = (u32)lo + er / B.len, ur = er % B.len;
                        const int size = (int)(g.W - ur - ul);
                        if (size >= P->amp_lo && size <= P->amp_hi) key = des_key(pl + pr, ul, nl, g.W - ur - nr, nr);
                    }
                }
                u64 mask = __ballot(key < bound);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const u64 k = des_shfl64(key, l);
                    if (k >= bound) continue;
                    const u32 e2 = base + (u32)l;
                    int any, end;
                    des_duplex(tab, A, ul, nl, B, e2 % B.len, (u32)lo + e2 / B.len, salt, conc, lane, &any, &end);
                    if (any > max_sec || end > max_sec) continue;
                    // (k < bound <= the key of every lane from top - 1 on: a greater lane there is, the first of them takes k)
                    const u64 up = ((u64)(u32)__shfl_up((int)(mine >> 32), 1, 64) << 32) | (u32)__shfl_up((int)(u32)mine, 1, 64);
                    const u32 first = (u32)__ffsll((long long)__ballot(mine > k)) - 1u;
                    mine = lane < first ? mine : lane == first ? k : up;
                    bound = des_shfl64(mine, (int)top - 1);
                }
            }
        }
    }

    // ---- 3: the records, a slot a turn
#pragma unroll 1
    for (u32 j = 0; j < top; j++) {
        const u64 slot = (u64)region * top + j;
        des_record<HP>(tab, A, B, g, P, lane, des_shfl64(mine, (int)j), out + slot, HP ? hp_out + slot : nullptr);
    }
}
