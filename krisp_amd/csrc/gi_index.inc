// gi_index.inc -- part of krisp_hip.hip, and of tests/gather_index_check.cpp: the index arithmetic of k_gather_items
// (k_intersect3.inc) in plain C++ for host and device: no HIP call, no LDS, no thread index.  A translation unit without
// HIP defines __host__ and __device__ empty before it includes this file.
//
// A workgroup gathers the survivors of GI_ITEMS consecutive items into one contiguous run of the dense list.  pre[0 ..
// GI_ITEMS] are the exclusive prefix sums of the items' counts (pre[0] = 0, pre[GI_ITEMS] = the workgroup's total).
// Output o < pre[GI_ITEMS] of the workgroup is entry o - pre[j] of item j, the largest j with pre[j] <= o: such an item
// is never empty (pre[j + 1] > o), whatever empty items lie in front of or behind it.
#include <stdint.h>

#define GI_ITEMS_LOG 6
#define GI_ITEMS (1u << GI_ITEMS_LOG)   // items of one workgroup (the search below takes GI_ITEMS_LOG steps)

struct GiSlot {
    uint32_t item, offset;      // item j < GI_ITEMS of the workgroup, entry offset < count[j] inside it
};

__host__ __device__ inline GiSlot gi_slot(const uint32_t* pre, uint32_t o) {
    uint32_t j = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t s = GI_ITEMS >> 1; s; s >>= 1)
        if (pre[j + s] <= o) j += s;            // (j + s <= GI_ITEMS - 1)
    GiSlot r;
    r.item = j;
    r.offset = o - pre[j];
    return r;
}
