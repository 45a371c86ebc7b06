// k_panel.inc -- part of krisp_hip.hip (one translation unit): the panel pass (--panel, DESIGN §23): of the regions with a
// designed pair, in the order the host gives them, the first N that are different loci and whose primers do not prime on
// each other's.  The host driver is h_panel.inc; the pieces that index memory are panel_step.inc; the duplex model is
// k_design.inc's (des_duplex, des_tm), read from the kr_design_params kr_design_table left on the device.
//
// k_panel_round: ONE launch per round r, N launches on one stream, no host decision between them.  On the device: two
// bytes (fate, by) and two ints (cross_any, cross_end) per candidate, and pick[0 .. N]: pick[r] = the position of member
// r + 1, 0xffffffff while there is none (pick[0] = 0).  A round whose pick[r] is the sentinel returns at once.
//   the workgroup (persistent: the grid is sized to the device): the member's windows of 16 bases on both strands into the
//   table in LDS, the member's two primers -- codes, prefix sums of the steps' dH and dS -- behind it; once per round.
//   a wavefront per alive candidate above pick[r]: a lane per forward window, a ballot says same locus (fate 2); else its
//   two primers into the wave's slice of LDS, the four duplexes candidate x member, the running maxima, and either fate 3
//   or atomicMin(&pick[r + 1], position).  A candidate is touched by one wave in a round, and the next round is the next
//   launch: plain loads and stores; the minimum of integers is the same on every run.
// Integers only, no scratch buffer in memory.
#define PAN_T 256                   // threads of a workgroup: four waves
#define PAN_WAVES (PAN_T / DES_T)
#define PAN_PRIMER 64               // codes of a primer's slot (a primer has at most 60)
#define PAN_NONE 0xffffffffu        // pick[]: no member

// a primer in LDS: what des_tm and des_duplex read of a DesSide
struct PanPrimer {
    uint8_t code[PAN_PRIMER];
    int ph[PAN_PRIMER + 1];
    int ps[PAN_PRIMER + 1];
};

// the lanes of one wave have written LDS that other lanes of the wave read next (no workgroup barrier: the waves of a
// workgroup run different numbers of candidates)
__device__ __forceinline__ void pan_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// one wave: the primer template[start, start + n) (rc: its reverse complement) into p, n <= 60
__device__ __forceinline__ void pan_load_primer(PanPrimer* p, const int* tab, const uint8_t* t, u32 W, u32 start, u32 n, bool rc,
                                                u32 lane) {
    const u32 a = panel_primer_code(t, W, start, n, lane, rc), b = panel_primer_code(t, W, start, n, lane + 1, rc);
    int h = 0, s = 0;
    if (a < 4u && b < 4u) { h = tab[4 * a + b]; s = tab[16 + 4 * a + b]; }
    h = des_wave_scan(h, lane);
    s = des_wave_scan(s, lane);
    if (lane < PAN_PRIMER) {
        p->code[lane] = (uint8_t)a;
        p->ph[lane + 1] = h;
        p->ps[lane + 1] = s;
    }
    if (lane == 0) { p->ph[0] = 0; p->ps[0] = 0; }
}

__device__ __forceinline__ DesSide pan_side(const PanPrimer* p, u32 n) {
    DesSide S;
    S.code = p->code; S.ph = p->ph; S.ps = p->ps; S.pc = nullptr; S.pen = nullptr; S.len = n; S.nlen = 0;
    return S;
}

// pairs: ls, ln, rs, rn per candidate; state: fate, by per candidate; cross: any, end per candidate
__global__ __launch_bounds__(PAN_T) void k_panel_round(const uint8_t* __restrict__ templates, const ushort4* __restrict__ pairs,
                                                       u32 ncand, u32 W, u32 r, const kr_design_params* __restrict__ P,
                                                       u32* pick, uint8_t* state, int2* cross) {
    __shared__ __align__(16) u32 table[PANEL_SLOTS];
    __shared__ __align__(16) int tab[DES_TAB];
    __shared__ __align__(16) PanPrimer member[2];
    __shared__ __align__(16) PanPrimer mine[PAN_WAVES][2];
    __shared__ __align__(16) u32 poly_t[4];
    const u32 tid = threadIdx.x, lane = tid & (DES_T - 1), wave = tid / DES_T;
    const u32 m = pick[r];
    if (m >= ncand) return;         // (the sentinel: the panel ended short of this round)

    for (u32 i = tid; i < PANEL_SLOTS; i += PAN_T) table[i] = PANEL_EMPTY;
    if (tid < 40) tab[tid] = ((const int*)P)[tid];
    if (tid == 0) poly_t[0] = 0u;
    __syncthreads();
    const uint8_t* const Tm = templates + (u64)m * W;
    for (u32 i = tid; i + PANEL_K <= W; i += PAN_T) {
        u32 kf, kr;
        if (panel_window_keys(Tm, W, i, &kf, &kr)) {
            panel_insert(table, poly_t, kf);
            panel_insert(table, poly_t, kr);
        }
    }
    const ushort4 mp = pairs[m];
    if (wave < 2) pan_load_primer(&member[wave], tab, Tm, W, wave ? mp.z : mp.x, wave ? mp.w : mp.y, wave != 0, lane);
    if (blockIdx.x == 0 && tid == 0) { state[2 * (u64)m] = 1; state[2 * (u64)m + 1] = (uint8_t)(r + 1); }
    __syncthreads();

    const int salt = P->salt_ds, conc = P->conc_ds, max_sec = P->max_sec;
    const u32 has_t = poly_t[0];
    const DesSide Y[2] = {pan_side(&member[0], mp.y), pan_side(&member[1], mp.w)};
    const u32 ny[2] = {mp.y, mp.w};
    bool asked = false;             // this wave has named its first survivor: the later ones lie above it
    const u64 stride = (u64)gridDim.x * PAN_WAVES;
    for (u64 c = (u64)m + 1 + (u64)blockIdx.x * PAN_WAVES + wave; c < ncand; c += stride) {
        if (state[2 * c] != 0) continue;
        const uint8_t* const T = templates + c * W;
        // ---- same locus: a lane per forward window
        bool same = false;
        for (u32 base = 0; base + PANEL_K <= W && !same; base += DES_T) {
            u32 kf, kr;
            const bool hit = panel_window_keys(T, W, base + lane, &kf, &kr) && panel_probe(table, has_t, kf);
            same = __ballot(hit) != 0ull;
        }
        if (same) {
            if (lane == 0) { state[2 * c] = 2; state[2 * c + 1] = (uint8_t)(r + 1); }
            continue;
        }
        // ---- the four duplexes, the candidate's primer in the left role
        const ushort4 cp = pairs[c];
        pan_wave_sync();            // (the wave's earlier reads of its slice are over)
        pan_load_primer(&mine[wave][0], tab, T, W, cp.x, cp.y, false, lane);
        pan_load_primer(&mine[wave][1], tab, T, W, cp.z, cp.w, true, lane);
        pan_wave_sync();
        const u32 nx[2] = {cp.y, cp.w};
        int any = 0, end = 0;
#pragma unroll
        for (int x = 0; x < 2; x++) {
            const DesSide X = pan_side(&mine[wave][x], nx[x]);
#pragma unroll
            for (int y = 0; y < 2; y++) {
                int a, e;
                des_duplex(tab, X, 0, nx[x], Y[y], 0, ny[y], salt, conc, lane, &a, &e);
                any = max(any, a);
                end = max(end, e);
            }
        }
        const bool clash = any > max_sec || end > max_sec;
        if (lane == 0) {
            const int2 was = cross[c];
            cross[c] = make_int2(max(was.x, any), max(was.y, end));
            if (clash) {
                state[2 * c] = 3;
                state[2 * c + 1] = (uint8_t)(r + 1);
            } else if (!asked) {
                atomicMin(&pick[r + 1], (u32)c);
            }
        }
        asked = asked || !clash;
    }
}
