// The statistics of a row's softmax over its logits s_1..s_N, carried beside a logit-tile walk (topk_stats.hip):
//   lse     = log sum_i exp(s_i)
//   entropy = -sum_i p_i log p_i,  p_i = exp(s_i - lse), in nats.
// State of any subset of the items: (m, l, u) with m = max s, l = sum exp(s - m), u = sum exp(s - m) (s - m).  Then lse = m + log l and
// entropy = log l - u / l: every term of l and of -u is >= 0, so nothing cancels when one item dominates (lse - sum p s subtracts two
// numbers of the size of the dominant logit).  A non-empty state has l >= 1 (its maximum contributes exp(0)).
// The empty state is (-inf, 0, 0).  Moving a state to a maximum mn >= m, d = m - mn <= 0:  l <- l e^d,  u <- e^d (u + d l);  a state
// with l == 0 is skipped, so d = -inf never meets l = 0 and no NaN is formed.  Merging states = all of them moved to their common
// maximum (a maximum of floats is exact in any order), then l and u added.
// PRECISION.  A lane's running state is float32 (stat_add4: the hot loop).  Whatever joins states -- lanes, waves, ranges -- moves
// them in double (stat_move_d: exact d, one double exp) and adds in double, and the readout is in double with one rounding to float32:
// measured with float32 merges and readout, the readout alone (logf, then m + log l in the binade of lse) cost up to 1.5 ulp of lse and
// the ordered float32 sum over the ranges another 1 - 2 (profiles/topk_stats.txt).  A partial between the kernels is float32.
// Every float operation is stated: no contraction is left to the compiler (fmaf / fma where a fused operation is meant), so the two
// walks that include this header compute the same bits from the same logits.
#pragma once
#include "common.h"

struct RowStat { float m, l, u; };

__device__ __forceinline__ RowStat stat_empty() {
    RowStat s;
    s.m = -INFINITY; s.l = 0.0f; s.u = 0.0f;
    return s;
}
// s, a state at maximum s.m <= mn, restated at maximum mn (float32: a lane's own running state)
__device__ __forceinline__ void stat_move(RowStat& s, float mn) {
#pragma clang fp contract(off)
    if (s.l > 0.0f) {
        const float d = s.m - mn, e = expf(d);      // d == 0: e == 1, and l, u keep their bits
        s.u = e * fmaf(d, s.l, s.u);
        s.l = s.l * e;
    }
    s.m = mn;
}
// the 4 logits v[0..3] of a lane's tile row enter s; bit r of `valid` clear: v[r] is not an item of the row
__device__ __forceinline__ void stat_add4(RowStat& s, const f32x4 v, unsigned valid) {
#pragma clang fp contract(off)
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if ((valid >> r) & 1u) mt = fmaxf(mt, v[r]);
    if (mt > s.m) stat_move(s, mt);                  // (nothing valid: mt = -inf, never above s.m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if ((valid >> r) & 1u) {
            const float t = v[r] - s.m, e = expf(t);
            s.l = s.l + e;
            s.u = fmaf(e, t, s.u);
        }
}
// (L, U) <- the float32 state (m, l, u) moved to the maximum mn >= m, in double; an empty state gives (0, 0)
__device__ __forceinline__ void stat_move_d(float m, float l, float u, float mn, double& L, double& U) {
#pragma clang fp contract(off)
    L = 0.0; U = 0.0;
    if (l > 0.0f) {
        const double d = (double)m - (double)mn, e = exp(d);      // d == 0: e == 1
        L = e * (double)l;
        U = e * fma(d, (double)l, (double)u);
    }
}
// (L >= 1 for a row with at least one item)
__device__ __forceinline__ void stat_readout(float m, double L, double U, float& lse, float& entropy) {
#pragma clang fp contract(off)
    const double ll = log(L);
    lse = (float)((double)m + ll);
    entropy = (float)(ll - U / L);
}
