// k_guides.inc -- part of krisp_hip.hip (one translation unit): the guide pass (--out_guides, DESIGN §18): for every region
// the protospacer window next to the enzyme's PAM that differs most from the region's outgroup rows, every figure an
// integer.  The host driver is h_guides.inc; the options arrive by value in a GuideArgs.
//
// k_guides: a workgroup of ONE wavefront per region, as k_design.  Only the columns [lo, hi) of a region are ever read.
// In LDS, indexed by the template's column:
//   code   the template's base codes (4: no base)
//   pa     prefix counts of G or C (low half) and of letters that are no base (high half); pr: of the ends of runs of five
//          equal letters.  Entry i + 1 counts the columns lo .. i; entry lo is 0.
//   dmin   per window start p the least mm(o) over the outgroup rows so far, ssum their sum
//   mm     the current outgroup row's prefix count of mismatch flags (u16), entry i - lo + 1 counts the columns lo .. i
//   1  the codes and the two prefix counts, 64 columns a step (a wave scan with a carry).
//   2  the outgroup rows one after the other, however many there are: the row's mismatch flags, their prefix count, then a
//      lane per window: mm(o) = mm[p + g] - mm[p] in O(1) into dmin and ssum (each lane owns its windows: no atomics).
//   3  a lane per (window, strand): bounds, letters, PAM, GC and poly-X are O(1) from the prefixes (the PAM a loop over
//      its letters), d and s come from 2 -> the candidate's key, the greatest of which the lane keeps in registers; a wave
//      maximum and a wave sum of the counts.
//   4  the record, 32 bytes by two plain vector stores of lane 0.  No atomics, no scratch.
// The steps are inline pieces (gui_tables: 1 and 2, gui_key: 3's test of one candidate, gui_record: 4) that k_guides_top, the
// shortlist kernel of --guide-candidates at the end of this file, shares.
// The key orders candidates as the definition does (greatest first): d | s | 8191 - |2 p + g - (2 L + D)| | + before - |
// 2047 - p, in 6 + 32 + 13 + 1 + 11 bits.  No candidate has the key 0.
#define GUI_T 64
#define GUI_MAX_TEMPLATE 2047       // (11-bit starts in the key: the designer's limit)
#define GUI_MIN_SIZE 12
#define GUI_MAX_SIZE 40
#define GUI_MAX_PAM 8
#define GUI_MAX_ROWS ((u64)1 << 26) // rows of one region: their mismatches' sum stays below 2^32

struct GuideArgs {
    u32 g, a, b;                    // guide_size, len(pam5), len(pam3)
    u32 pam5, pam3;                 // the motifs' masks, 4 bits a letter, letter j at bits 4 j
    int gc_lo, gc_hi, min_mm;
};

struct GuideGeom {
    u32 K, center;                  // center = 2 L + D
    u32 o_pa, o_pr, o_dmin, o_ssum, o_mm;   // byte offsets in the dynamic LDS (code lies at 0)
    u32 lds_bytes;
};

__host__ __device__ inline void guide_geom(int K, int L, int D, GuideGeom* g) {
    g->K = (u32)K; g->center = (u32)(2 * L + D);
    u32 o = ((u32)K + 3u) & ~3u;
    g->o_pa = o; o += ((u32)K + 1) * 4;
    g->o_pr = o; o += ((u32)K + 1) * 4;
    g->o_dmin = o; o += (u32)K * 4;
    g->o_ssum = o; o += (u32)K * 4;
    g->o_mm = o; o += (((u32)K + 1) * 2 + 3u) & ~3u;
    g->lds_bytes = (o + 15u) & ~15u;
}

__device__ __forceinline__ u64 gui_wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u64 t = ((u64)(u32)__shfl_xor((int)(v >> 32), o, 64) << 32) | (u32)__shfl_xor((int)(u32)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

__device__ __forceinline__ u32 gui_wave_sum(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (u32)__shfl_xor((int)v, o, 64);
    return v;
}

// the LDS tables of one region, and the columns it reads
struct GuiRegion {
    uint8_t* code;
    u32 *pa, *pr, *dmin, *ssum;
    unsigned short* mm;
    u32 lo, hi, npos;               // window starts lo .. lo + npos - 1
};

// steps 1 and 2 of a region's wavefront: the tables (rows, row_off and bounds are the batch's)
__device__ __forceinline__ GuiRegion gui_tables(unsigned char* lds, const uint8_t* __restrict__ rows, const u64* __restrict__ row_off,
                                                const u32* __restrict__ bounds, u32 region, u32 lane, const GuideGeom& G,
                                                const GuideArgs& P) {
    GuiRegion R;
    uint8_t* const code = R.code = lds;
    u32* const pa = R.pa = (u32*)(lds + G.o_pa);
    u32* const pr = R.pr = (u32*)(lds + G.o_pr);
    u32* const dmin = R.dmin = (u32*)(lds + G.o_dmin);
    u32* const ssum = R.ssum = (u32*)(lds + G.o_ssum);
    unsigned short* const mm = R.mm = (unsigned short*)(lds + G.o_mm);
    const u32 K = G.K, g = P.g;
    // (the host has checked lo <= hi <= K; the kernel holds itself to K all the same)
    const u32 hi = R.hi = min(bounds[2 * region + 1], K), lo = R.lo = min(bounds[2 * region], hi);
    const u64 first = row_off[region], end = row_off[region + 1];
    const uint8_t* const T = rows + first * K;
    const u32 npos = R.npos = hi - lo >= g ? hi - lo - g + 1 : 0u;

    // ---- 1: the template's codes, then its prefix counts over [lo, hi)
    for (u32 i = lo + lane; i < hi; i += GUI_T) code[i] = (uint8_t)des_code(T[i]);
    for (u32 e = lane; e < npos; e += GUI_T) { dmin[lo + e] = g; ssum[lo + e] = 0u; }
    if (lane == 0) { pa[lo] = 0u; pr[lo] = 0u; }
    __syncthreads();
    {
        int ca = 0, cr = 0;
        for (u32 base = lo; base < hi; base += GUI_T) {
            const u32 i = base + lane;
            int va = 0, vr = 0;
            if (i < hi) {
                const u32 c = code[i];
                bool five = i >= lo + 4;
                for (u32 k = 1; five && k < 5; k++) five = code[i - k] == c;
                va = (int)((c == 1u || c == 2u) ? 1u : 0u) | (int)((c >= 4u ? 1u : 0u) << 16);
                vr = five ? 1 : 0;
            }
            va = des_wave_scan(va, lane) + ca;          // (two counts of at most 2047 each: no carry between the halves)
            vr = des_wave_scan(vr, lane) + cr;
            if (i < hi) { pa[i + 1] = (u32)va; pr[i + 1] = (u32)vr; }
            ca = __shfl(va, 63, 64); cr = __shfl(vr, 63, 64);
        }
    }
    __syncthreads();

    // ---- 2: the outgroup rows
    if (npos) {
#pragma unroll 1
        for (u64 r = first + 1; r < end; r++) {
            const uint8_t* const O = rows + r * K;
            int carry = 0;
            if (lane == 0) mm[0] = 0;
            for (u32 base = lo; base < hi; base += GUI_T) {
                const u32 i = base + lane;
                int f = 0;
                if (i < hi) {
                    const u32 c = des_code(O[i]);
                    f = (c < 4u && c != code[i]) ? 1 : 0;
                }
                f = des_wave_scan(f, lane) + carry;
                if (i < hi) mm[i - lo + 1] = (unsigned short)f;
                carry = __shfl(f, 63, 64);
            }
            __syncthreads();
            for (u32 e = lane; e < npos; e += GUI_T) {
                const u32 m = (u32)mm[e + g] - (u32)mm[e];
                dmin[lo + e] = min(dmin[lo + e], m);
                ssum[lo + e] += m;
            }
            __syncthreads();
        }
    }
    return R;
}

// step 3 for (window, strand) e of the region: the candidate's key, or 0 where it is none
__device__ __forceinline__ u64 gui_key(const GuiRegion& R, u32 e, const GuideGeom& G, const GuideArgs& P) {
    const uint8_t* const code = R.code;
    const u32* const pa = R.pa;
    const u32 lo = R.lo, hi = R.hi, g = P.g;
    const u32 p = lo + (e >> 1), strand = e & 1u;
    const u32 before = strand ? P.b : P.a, after = strand ? P.a : P.b;      // columns of the footprint beside the window
    if (p < lo + before || p + g + after > hi) return 0;
    const u32 fl = p - before, fr = p + g + after;
    if ((pa[fr] >> 16) != (pa[fl] >> 16)) return 0;                          // a letter that is no base
    bool ok = true;
    // the motifs as read on the guide's strand: on '-' letter j is the complement of the column counted from the far end
    for (u32 j = 0; ok && j < P.a; j++) {
        const u32 c = strand ? 3u - code[p + g + P.a - 1 - j] : code[p - P.a + j];
        ok = ((P.pam5 >> (4 * j)) & (1u << c)) != 0;
    }
    for (u32 j = 0; ok && j < P.b; j++) {
        const u32 c = strand ? 3u - code[p - 1 - j] : code[p + g + j];
        ok = ((P.pam3 >> (4 * j)) & (1u << c)) != 0;
    }
    if (!ok) return 0;
    const int gc = (int)(pa[p + g] & 0xffffu) - (int)(pa[p] & 0xffffu);
    if (100 * gc < P.gc_lo * (int)g || 100 * gc > P.gc_hi * (int)g) return 0;
    if (R.pr[p + g] != R.pr[p + 4]) return 0;                                // a run of five ends inside the window
    const u32 d = R.dmin[p];
    if ((int)d < P.min_mm) return 0;
    const int off = (int)(2 * p + g) - (int)G.center;
    return ((u64)d << 57) | ((u64)R.ssum[p] << 25) | ((u64)(8191u - (u32)abs(off)) << 12) | ((u64)(1u - strand) << 11) | (2047u - p);
}

// step 4: the record of the candidate `key` (0: none) of a region with `count` candidates, by two plain vector stores
__device__ __forceinline__ void gui_record(const GuiRegion& R, u32 g, u64 key, u32 count, kr_guide_record* out) {
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = make_uint4(0, 0, count, 0);
    if (key) {
        const u32 p = 2047u - ((u32)key & 2047u);
        w0 = make_uint4(1u, 1u - ((u32)(key >> 11) & 1u), p, (u32)(key >> 57));
        w1 = make_uint4((u32)(key >> 25), (R.pa[p + g] & 0xffffu) - (R.pa[p] & 0xffffu), count, 0u);
    }
    uint4* o = (uint4*)out;
    o[0] = w0;
    o[1] = w1;
}

__global__ __launch_bounds__(GUI_T) void k_guides(const uint8_t* __restrict__ rows, const u64* __restrict__ row_off,
                                                  const u32* __restrict__ bounds, u32 nregions, GuideGeom G, GuideArgs P,
                                                  kr_guide_record* __restrict__ out) {
    extern __shared__ __align__(16) u32 gui_lds[];
    const u32 region = blockIdx.x, lane = threadIdx.x;
    if (region >= nregions) return;
    const GuiRegion R = gui_tables((unsigned char*)gui_lds, rows, row_off, bounds, region, lane, G, P);

    // ---- 3: a lane per (window, strand)
    u64 best = 0;
    u32 count = 0;
    for (u32 e = lane; e < 2 * R.npos; e += GUI_T) {
        const u64 key = gui_key(R, e, G, P);
        if (!key) continue;
        best = key > best ? key : best;
        count++;
    }
    best = gui_wave_max(best);
    count = gui_wave_sum(count);

    // ---- 4: the record
    if (lane == 0) gui_record(R, P.g, best, count, out + region);
}

// k_guides_top (--guide-candidates, DESIGN §22): the `top` greatest keys of a region, 1 <= top <= GUI_MAX_TOP, as records
// out[region * top + j], j = rank - 1; a slot beyond the region's candidates is zero but `candidates`.  Steps 1 and 2 are
// k_guides'.  3: the candidates e and e + 64 are one lane's, so a lane may hold several of the top: every lane keeps its own
// GUI_MAX_TOP greatest keys, descending, in registers (an insert of compare-and-swaps, fully unrolled: no indexed array).
// Then `top` rounds: the wave maximum of the lanes' heads is the next rank -- keys are unique per (window, strand), so one
// lane holds it and pops it -- and lane j keeps round j's winner.  4: lane j < top writes slot j.  No atomics, no scratch.
#define GUI_MAX_TOP 8

__global__ __launch_bounds__(GUI_T) void k_guides_top(const uint8_t* __restrict__ rows, const u64* __restrict__ row_off,
                                                      const u32* __restrict__ bounds, u32 nregions, GuideGeom G, GuideArgs P, u32 top,
                                                      kr_guide_record* __restrict__ out) {
    extern __shared__ __align__(16) u32 gui_lds[];
    const u32 region = blockIdx.x, lane = threadIdx.x;
    if (region >= nregions) return;
    const GuiRegion R = gui_tables((unsigned char*)gui_lds, rows, row_off, bounds, region, lane, G, P);

    // ---- 3: a lane per (window, strand), the lane's greatest keys in k0 >= k1 >= ... >= k7
    u64 k0 = 0, k1 = 0, k2 = 0, k3 = 0, k4 = 0, k5 = 0, k6 = 0, k7 = 0;
    u32 count = 0;
#define GUI_SIFT(slot) { const u64 lo_ = key < slot ? key : slot; slot = key < slot ? slot : key; key = lo_; }
    for (u32 e = lane; e < 2 * R.npos; e += GUI_T) {
        u64 key = gui_key(R, e, G, P);
        if (!key) continue;
        count++;
        GUI_SIFT(k0) GUI_SIFT(k1) GUI_SIFT(k2) GUI_SIFT(k3) GUI_SIFT(k4) GUI_SIFT(k5) GUI_SIFT(k6) GUI_SIFT(k7)
    }
#undef GUI_SIFT
    count = gui_wave_sum(count);
    u64 mine = 0;                                       // lane j: the key of rank j + 1
    for (u32 j = 0; j < top; j++) {
        const u64 win = gui_wave_max(k0);
        if (win == 0) break;                            // (wave-uniform: the candidates are used up)
        if (lane == j) mine = win;
        if (k0 == win) { k0 = k1; k1 = k2; k2 = k3; k3 = k4; k4 = k5; k5 = k6; k6 = k7; k7 = 0; }
    }

    // ---- 4: the records
    if (lane < top) gui_record(R, P.g, mine, count, out + (u64)region * top + lane);
}
