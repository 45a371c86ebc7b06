// panel_step.inc -- part of krisp_hip.hip, and of tests/panel_step_check.cpp: the pieces of the panel pass (k_panel.inc,
// DESIGN §23) that index memory, in plain C++ for host and device: no LDS, no thread index.  A translation unit without HIP
// defines __host__ and __device__ empty before it includes this file.
//
// Same locus: two templates share a window of PANEL_K bases, the second read on either strand.  A window is a u32 key, two
// bits a base, the first base in the top bits; the member's windows of both strands stand in an open-addressing table of
// PANEL_SLOTS u32, and a candidate's forward windows are probed in it.  Every u32 is a key, so the one key that looks like an
// empty slot (PANEL_EMPTY: sixteen T) is kept beside the table in a flag word.  An insert that meets its own key is done:
// 2032 equal windows fill one slot.  Every index is tested against its bound before the load; a slot's index is masked.
#include <stdint.h>

#define PANEL_K 16u                 // bases of a window
#define PANEL_MAX_TEMPLATE 2047u    // (k_design.inc's DES_MAX_TEMPLATE): at most 2 x 2032 keys
#define PANEL_SLOTS 8192u           // a power of two, above twice the keys
#define PANEL_EMPTY 0xffffffffu

// A C G T = 0 1 2 3 (des_code of k_design.inc), every other byte 4
__host__ __device__ inline uint32_t panel_code(uint32_t ch) {
    return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
}

// the window [i, i + PANEL_K) of a template of W bytes -> its key as written and the key of its reverse complement; false
// where the window does not lie inside the template or holds a byte other than A, C, G, T: no window
__host__ __device__ inline bool panel_window_keys(const uint8_t* t, uint32_t W, uint32_t i, uint32_t* fwd, uint32_t* rev) {
    if (W < PANEL_K || i > W - PANEL_K) return false;
    uint32_t f = 0u, r = 0u;
    for (uint32_t j = 0; j < PANEL_K; j++) {
        const uint32_t c = panel_code(t[i + j]);
        if (c > 3u) return false;
        f = (f << 2) | c;
        r |= (3u - c) << (2u * j);
    }
    *fwd = f;
    *rev = r;
    return true;
}

__host__ __device__ inline uint32_t panel_slot(uint32_t key) { return ((key * 0x9e3779b1u) >> 19) & (PANEL_SLOTS - 1u); }

// compare-and-swap of a table word: atomic among the lanes of a workgroup on the device, plain on the host
__host__ __device__ inline uint32_t panel_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}

// table: PANEL_SLOTS words, all PANEL_EMPTY before the first insert; poly_t: one word, 0 before it.  false: the table is
// full (it cannot be: at most 4064 keys)
__host__ __device__ inline bool panel_insert(uint32_t* table, uint32_t* poly_t, uint32_t key) {
    if (key == PANEL_EMPTY) {
        *poly_t = 1u;               // (every lane that writes it writes 1)
        return true;
    }
    uint32_t s = panel_slot(key);
    for (uint32_t step = 0; step < PANEL_SLOTS; step++) {
        const uint32_t old = panel_cas(table + s, PANEL_EMPTY, key);
        if (old == PANEL_EMPTY || old == key) return true;
        s = (s + 1u) & (PANEL_SLOTS - 1u);
    }
    return false;
}

__host__ __device__ inline bool panel_probe(const uint32_t* table, uint32_t poly_t, uint32_t key) {
    if (key == PANEL_EMPTY) return poly_t != 0u;
    uint32_t s = panel_slot(key);
    for (uint32_t step = 0; step < PANEL_SLOTS; step++) {
        const uint32_t got = table[s];
        if (got == key) return true;
        if (got == PANEL_EMPTY) return false;
        s = (s + 1u) & (PANEL_SLOTS - 1u);
    }
    return false;
}

// base i of a primer, read 5'->3', as its code: the left primer is template[start, start + n) as written, the right one
// (rc) the reverse complement of template[start, start + n).  4 for an index outside the primer or the template
__host__ __device__ inline uint32_t panel_primer_code(const uint8_t* t, uint32_t W, uint32_t start, uint32_t n, uint32_t i, bool rc) {
    if (i >= n || start > W || n > W - start) return 4u;
    const uint32_t c = panel_code(t[rc ? start + n - 1u - i : start + i]);
    return rc && c < 4u ? 3u - c : c;
}
