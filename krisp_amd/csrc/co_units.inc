// co_units.inc -- part of krisp_hip.hip, and of tests/coarse_units_check.cpp: the work units of the coarse route
// (k_coarse.inc) in plain C++ for host and device: no HIP call, no LDS, no thread index.  A translation unit without HIP
// defines __host__ and __device__ empty before it includes this file.
//
// One call streams G coarse genomes past the candidate list.  A unit is at most CO_CHUNK keys of ONE genome's bucket of one
// top byte, looked up in the table of one round (tcap candidates of that byte).  Units are numbered
//     top byte -> round -> genome -> chunk,          the chunk varying fastest,
// so a contiguous slice of the numbers changes (top byte, round) monotonically: a workgroup builds a table once and
// streams every genome's keys of that byte past it.  A top byte without candidates, and a genome without keys in a byte,
// have no unit.
//
// The buckets of a top byte t travel as a "row": bnd[2 j], bnd[2 j + 1] = genome j's keys [b0, b1) of that byte.
#include <stdint.h>

#define CO_CHUNK 32768u         // keys of one work unit (even: a unit's 16-byte loads keep the parity of the bucket's base)

struct CoUnit {
    uint32_t round, genome, chunk;
    uint32_t k0, k1;            // the unit's keys [k0, k1) of the genome's key array: inside the bucket, never empty
};

__host__ __device__ inline uint32_t co_chunks(uint32_t len) { return len / CO_CHUNK + (len % CO_CHUNK ? 1u : 0u); }

// chunks of all genomes in one round of a top byte
__host__ __device__ inline uint32_t co_row_chunks(const uint32_t* bnd, uint32_t G) {
    uint32_t s = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 1
#endif
    for (uint32_t j = 0; j < G; j++) s += co_chunks(bnd[2 * j + 1] - bnd[2 * j]);
    return s;
}

// units of a top byte with nc candidates
__host__ __device__ inline uint32_t co_byte_units(uint32_t nc, uint32_t tcap, const uint32_t* bnd, uint32_t G) {
    return (nc / tcap + (nc % tcap ? 1u : 0u)) * co_row_chunks(bnd, G);
}

// the top byte of unit u < ust[256]: the largest t with ust[t] <= u (ust[t] = units in front of top byte t, ust[0] = 0;
// such a t has units of its own)
__host__ __device__ inline uint32_t co_unit_byte(const uint32_t* ust, uint32_t u) {
    uint32_t lo = 0, hi = 256;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ust[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// unit v (counted from the top byte's first: v = u - ust[t] < co_byte_units) of the byte with the row bnd
__host__ __device__ inline CoUnit co_unit_decode(uint32_t v, const uint32_t* bnd, uint32_t G) {
    CoUnit r;
    const uint32_t per = co_row_chunks(bnd, G);
    r.round = v / per;
    uint32_t w = v - r.round * per, j = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 1
#endif
    for (; j + 1 < G; j++) {
        const uint32_t c = co_chunks(bnd[2 * j + 1] - bnd[2 * j]);
        if (w < c) break;
        w -= c;
    }
    r.genome = j;
    r.chunk = w;
    const uint32_t b1 = bnd[2 * j + 1];
    r.k0 = bnd[2 * j] + w * CO_CHUNK;
    r.k1 = b1 - r.k0 > CO_CHUNK ? r.k0 + CO_CHUNK : b1;
    return r;
}
