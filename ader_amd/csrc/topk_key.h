// The 64-bit candidate key of the top-K kernels (topk.hip: k_topk_tile / k_topk_merge; logits_x3.hip: k_lx3t / k_topk3_finish):
// order-preserving float bits above, the complemented 1-based item id below, so ONE unsigned compare is the total order (score
// descending, item id ascending) and no two candidates of a row compare equal.  Key 0 = "no candidate".
#pragma once
#include "common.h"

typedef unsigned long long u64;

__device__ __forceinline__ u64 topk_key(float s, int item1) {
    uint32_t u = __float_as_uint(s + 0.0f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (uint32_t)~(uint32_t)item1;
}
__device__ __forceinline__ float topk_score(u64 key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ int topk_item(u64 key) { return (int)~(uint32_t)key; }
