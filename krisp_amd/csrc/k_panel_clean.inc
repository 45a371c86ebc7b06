// k_panel_clean.inc -- part of krisp_hip.hip (one translation unit): the clean panel selection (--panel-clean, DESIGN §26):
// the panel pass (k_panel.inc) with two more causes to drop a candidate, both read from the primer sites of every input
// genome: a primer that forms a product with itself (fate 5, before the first round) and a primer that forms a product
// with a primer of a member (fate 4, after the round of that member).  The host driver is h_panel_clean.inc; the pieces
// that index memory are pclean_step.inc.  The sites are k_prim_scan's, kept for all genomes in one store with a record
// number of their own (k_pclean_append).
//
// A round r is three launches on one stream, no host decision between them:
//   k_panel_round(r)   as it is: the member's fate, same locus (2), clash (3), the running figures; its atomicMin leaves in
//                      pick[r + 1] a position at or below the next member's
//   k_pclean_cross(r)  a thread per stored site; only the sites of the member's two texts walk: an opening site forward over
//                      the closing sites in reach, a closing site backward over the opening ones; every alive owner above
//                      the member of a partner's text gets (4, r + 1).  Equal words from several threads: one 16-bit store
//   k_pclean_next      one workgroup: from the position pick[r + 1] holds, the first candidate with fate 0 -> pick[r + 1]
// Before round 0 k_pclean_self (a thread per stored site: an opening site walks to the first closing site of its own text)
// and k_pclean_next for pick[0].  Integers only, no atomics in memory (k_pclean_next: one atomicMin in LDS), no scratch.
#define PCL_T 256

// store[n0 + i] = the genome's site i, unit[n0 + i] = base + its record in the genome
__global__ __launch_bounds__(PCL_T) void k_pclean_append(const kr_product_site* __restrict__ sites, const u32* __restrict__ rec, u64 ns,
                                                         u32 base, kr_product_site* __restrict__ store, u32* __restrict__ unit, u64 n0) {
    for (u64 i = (u64)blockIdx.x * PCL_T + threadIdx.x; i < ns; i += (u64)gridDim.x * PCL_T) {
        store[n0 + i] = sites[i];
        unit[n0 + i] = base + rec[i];
    }
}

__global__ __launch_bounds__(PCL_T) void k_pclean_self(PcleanStore S, PcleanOwners O, uint16_t* state, u32 ncand) {
    for (u64 i = (u64)blockIdx.x * PCL_T + threadIdx.x; i < S.ns; i += (u64)gridDim.x * PCL_T) pclean_self_site(S, O, i, state, ncand);
}

// rows: the table rows of every candidate's left and right primer
__global__ __launch_bounds__(PCL_T) void k_pclean_cross(PcleanStore S, PcleanOwners O, const u32* __restrict__ rows, const u32* __restrict__ pick,
                                                        u32 r, uint16_t* state, u32 ncand) {
    const u32 m = pick[r];
    if (m >= ncand) return;         // (the sentinel: the panel ended short of this round)
    const u32 tx = rows[2 * (u64)m], ty = rows[2 * (u64)m + 1];
    for (u64 i = (u64)blockIdx.x * PCL_T + threadIdx.x; i < S.ns; i += (u64)gridDim.x * PCL_T)
        pclean_cross_site(S, O, i, tx, ty, m, r + 1u, state, ncand);
}

// pick[slot] holds a position at or below the first alive candidate's, or the sentinel -> the first alive candidate's
// position, or the sentinel.  One workgroup; 4 PCL_T candidates a turn
__global__ __launch_bounds__(PCL_T) void k_pclean_next(u32* pick, u32 slot, const uint16_t* __restrict__ state, u32 ncand) {
    __shared__ u32 found;
    const u32 from = pick[slot];
    if (from >= ncand) return;
    if (threadIdx.x == 0) found = PCLEAN_NONE;
    __syncthreads();
    for (u64 base = from; base < ncand; base += 4 * PCL_T) {
        u32 mine = PCLEAN_NONE;
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            const u64 c = base + k * PCL_T + threadIdx.x;
            if (c < ncand && pclean_fate(state, ncand, (u32)c) == 0u) mine = min(mine, (u32)c);
        }
        if (mine != PCLEAN_NONE) atomicMin(&found, mine);
        __syncthreads();
        const u32 f = found;
        __syncthreads();            // (every thread has read it before a later turn's atomicMin)
        if (f != PCLEAN_NONE) break;
    }
    if (threadIdx.x == 0) pick[slot] = found;
}
