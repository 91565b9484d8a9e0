// The model's distribution beside its order: for every row the log-sum-exp and the entropy of softmax(logits) over ALL items 1..N -- the
// distribution the loss trains -- out of the walk that k_topk_tile (topk.hip) makes anyway, so that logprob = score - lse is one
// subtraction and no [B, N] matrix is written.
//   k_topk_tile_stats + k_topk_merge + k_stats_merge    items / scores of ader_topk_items, byte for byte, plus lse / entropy [B]
//                                                       (Engine.recommend_stats, ader_topk_items_stats)
//   k_row_stats + k_stats_merge                         lse / entropy [B] alone                (Engine.row_stats, ader_row_stats)
// Both tile kernels are ONE statement of the walk (stats_walk<KEYS>): logit_tile.h's (range, chunk) walk, tile stream and mma_tile<2>
// call, so a logit is k_logits_tile<MODE_STORE>'s float32 and a lane holds 2 rows x 4 items per tile; row_stats.h's (m, l, u) state per
// (lane, row), into which every item with it < ncol[row] enters, SEEN OR NOT: exclusion removes an item from the answer, not from the
// distribution, so the probabilities of an answer need not sum to 1.  KEYS adds k_topk_tile's seen mask, keys and row buffer, which
// read the accumulators and nothing of the state.
// ORDER OF THE SUMS, fixed: a lane adds its items in tile order, in float32.  After the range's last tile the row's maximum over its 16
// lanes is taken (__shfl_xor 16, 32 over the four lanes q = lane >> 4 of a wave, then the four waves mw through LDS -- E_l, free by
// then; a maximum is exact in any order), every lane moves its state there in double, and the sums are added in double: q by
// __shfl_xor 16, then 32, then the waves in mw order.  One float32 partial (m, l, u, 0) per (range, row) goes to spart [ranges][Bp][4],
// an empty range's being the empty state.  k_stats_merge moves the partials of a row to their common maximum and adds them in
// ascending range order, in double, and rounds lse and entropy once.  No float atomics: lse and entropy are a pure function of (rep row,
// table, N, Bp) -- Bp because ader_topk_ranges(N, Bp) sets the partition -- and the two tile kernels give the same bits, both stating
// the same float operations on the same logits (row_stats.h leaves no contraction open).
// This is a translation unit of its own for topk.hip's reason: one more caller of stage_tile or mma_tile<2> there changes the code
// emitted for the kernels already there (tools/isa_digest.py).  k_topk_merge is reached through topk.hip's host launcher.
#include "logit_tile.h"
#include "row_stats.h"
#include "../../include/ader_hip.h"

#define STATS_KMAX 64      // ader_topk_kmax()
#define STATS_RMAX 256     // ranges k_stats_merge holds per row in LDS: ader_topk_ranges never exceeds it

struct StatsArgs {
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1) : [N,H]
    int B, Bp, H, N;
    const int* ncol;       // [Bp] N for real rows, 0 for padding rows
    const int* seen;       // [B, seen_ld] 1-based ids never to be returned (0 = none), or NULL                   (KEYS)
    int seen_ld, k, ranges;
    u64* part;             // [ranges][Bp][k]                                                                     (KEYS)
    float* spart;          // [ranges][Bp][4]: m, l, u, 0
    float* lse;            // [B]
    float* entropy;        // [B]
};

template <bool KEYS>
__device__ __forceinline__ void stats_walk(const StatsArgs& a, float* smem) {
    float* E_l = smem;                                       // [TI][LDE]; after the last tile: the waves' states [4][TB][4]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    u64* buf = (u64*)(R_l + TB * LDE);                       // [TB][k + 64]                                      (KEYS, as are the next three)
    const int k = a.k, ldb = k + TI;
    u64* thr = buf + TB * ldb;                               // [TB]
    u64* msk = thr + TB;                                     // [TB] bit i: item tile0 + i is in the row's seen list
    int* cnt = (int*)(msk + TB);                             // [TB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    int range, bc, s_begin, s_end;
    if (!tile_walk(a.Bp / TB, a.ranges, (a.N + TI - 1) / TI, range, bc, s_begin, s_end)) return;
    stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
    if (KEYS) {
        rowbuf_init(thr, cnt, tid);
        if (tid < TB) msk[tid] = 0;
    }
    int nc[2];
    RowStat st[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        nc[j] = a.ncol[bc * TB + nw * 32 + j * 16 + r16];
        st[j] = stat_empty();
    }
    float pre[TILE_STAGE_REGS];
    if (s_begin < s_end) tile_load(pre, a.emb1, s_begin * TI, a.N, H, tid);
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();                                     // the previous tile's MFMA reads, filter and compaction are done
        tile_store(E_l, pre, tid);
        if (KEYS && a.seen) seen_mask_tile(msk, a.seen, a.seen_ld, a.B, bc * TB, tile0, tid);
        __syncthreads();
        if (s + 1 < s_end) tile_load(pre, a.emb1, tile0 + TI, a.N, H, tid);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il0 = mw * 16 + q * 4, item0 = tile0 + il0;      // this lane's 4 consecutive items
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned in = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) in |= (unsigned)(item0 + r < nc[j]) << r;
            stat_add4(st[j], acc[j], in);                          // seen or not: nothing crosses lanes here
        }
        if (KEYS) {
            int over = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int bl = nw * 32 + j * 16 + r16;              // batch row within the chunk
                const u64 t = thr[bl];
                const unsigned sm = (unsigned)(msk[bl] >> il0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int it = item0 + r;
                    rowbuf_propose(buf, ldb, cnt, k, bl, it < nc[j] && !((sm >> r) & 1u), topk_key(acc[j][r], it + 1), t, over);
                }
            }
            if (__syncthreads_or(over)) rowbuf_compact(buf, ldb, thr, cnt, k, wave, lane);
        }
    }
    __syncthreads();                                         // the last tile's MFMA reads of E_l are done: E_l is free
    if (KEYS) rowbuf_flush(a.part + ((size_t)range * a.Bp + bc * TB) * k, buf, ldb, cnt, k, tid);
    float* wm = E_l;                                         // [4][TB] the waves' row maxima
    double* red = (double*)(E_l + 4 * TB);                   // [4][TB][2] the waves' (L, U) at the row's maximum
    float mrow[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        mrow[j] = fmaxf(st[j].m, __shfl_xor(st[j].m, 16, 64));
        mrow[j] = fmaxf(mrow[j], __shfl_xor(mrow[j], 32, 64));
        if (q == 0) wm[mw * TB + nw * 32 + j * 16 + r16] = mrow[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int bl = nw * 32 + j * 16 + r16;
        const float mx = fmaxf(fmaxf(wm[bl], wm[TB + bl]), fmaxf(wm[2 * TB + bl], wm[3 * TB + bl]));      // the range's maximum of the row
        double L, U;
        stat_move_d(st[j].m, st[j].l, st[j].u, mx, L, U);
        L = L + __shfl_xor(L, 16, 64); U = U + __shfl_xor(U, 16, 64);      // (an add commutes: the four lanes end with the same sums)
        L = L + __shfl_xor(L, 32, 64); U = U + __shfl_xor(U, 32, 64);
        if (q == 0) { red[(mw * TB + bl) * 2] = L; red[(mw * TB + bl) * 2 + 1] = U; }
    }
    __syncthreads();
    if (tid < TB) {
        const float mx = fmaxf(fmaxf(wm[tid], wm[TB + tid]), fmaxf(wm[2 * TB + tid], wm[3 * TB + tid]));
        double L = red[tid * 2], U = red[tid * 2 + 1];
#pragma unroll
        for (int w = 1; w < 4; ++w) { L = L + red[(w * TB + tid) * 2]; U = U + red[(w * TB + tid) * 2 + 1]; }
        float* out = a.spart + ((size_t)range * a.Bp + bc * TB + tid) * 4;      // 16-byte aligned: one store
        *(float4*)out = make_float4(mx, (float)L, (float)U, 0.0f);
    }
}

__global__ __launch_bounds__(512) void k_topk_tile_stats(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    stats_walk<true>(a, smem);
}
__global__ __launch_bounds__(512) void k_row_stats(StatsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    stats_walk<false>(a, smem);
}

// One wave per real row, four rows per workgroup.  The maximum of the row's `ranges` partial maxima is exact in any order; lane i moves
// partials i, i + 64, ... to it (row_stats.h: (m1, l1, u1) merged into max m, in double) and parks (L, U) in LDS; lane 0 adds them in
// ascending range order and reads lse and entropy out, in double, rounded once.  An empty range's partial moves to (0, 0).
__global__ __launch_bounds__(256) void k_stats_merge(StatsArgs a) {
    __shared__ double sl[4][STATS_RMAX], su[4][STATS_RMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x * 4 + wave;
    float mx = -INFINITY;
    if (b < a.B) {                                           // (wave-uniform)
        for (int r = lane; r < a.ranges; r += 64) mx = fmaxf(mx, a.spart[((size_t)r * a.Bp + b) * 4]);
        mx = wave_max(mx);
        for (int r = lane; r < a.ranges; r += 64) {
            const float4 p = *(const float4*)(a.spart + ((size_t)r * a.Bp + b) * 4);
            stat_move_d(p.x, p.y, p.z, mx, sl[wave][r], su[wave][r]);
        }
    }
    __syncthreads();
    if (b < a.B && lane == 0) {
        double L = 0.0, U = 0.0;
        for (int r = 0; r < a.ranges; ++r) { L += sl[wave][r]; U += su[wave][r]; }
        stat_readout(mx, L, U, a.lse[b], a.entropy[b]);
    }
}

// ============================================================================================= C ABI
// ader_topk_items' -2 conditions (topk.hip: topk_bad)
static bool stats_bad(int B, int Bp, int H, int N, const int* seen, int seen_ld, int k) {
    return k < 1 || k > STATS_KMAX || Bp % TB != 0 || Bp > MAXB || B > Bp || H > HP || H < 1 || N < 1 || (seen && seen_ld < 1);
}
static void stats_fill(StatsArgs& a, const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, float* spart,
                       float* lse, float* entropy) {
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ncol = ncol; a.seen = nullptr; a.seen_ld = 0; a.k = 1;
    a.ranges = ader_topk_ranges(N, Bp); a.part = nullptr; a.spart = spart; a.lse = lse; a.entropy = entropy;
}
static size_t stats_lds(size_t tail) { return (size_t)(2 * 64 * LDE) * sizeof(float) + tail; }      // the two operand tiles + the tail
static size_t stats_rowbuf_lds(int k) { return (size_t)TB * (k + TI) * sizeof(u64) + TB * (2 * sizeof(u64) + sizeof(int)); }      // buf, thr, msk, cnt

// in topk.hip: k_topk_merge over part [ranges][Bp][k] -> items / scores [B,k], the second launch of ader_topk_items
int topk_merge_launch(int B, int Bp, int k, int ranges, unsigned long long* part, int* items, float* scores, void* stream);

extern "C" {

// floats of spart for (N, Bp): 4 per (range, padded row), ranges = ader_topk_ranges(N, Bp)
int ader_row_stats_floats(int N, int Bp) { return ader_topk_ranges(N, Bp) * (Bp > 0 ? Bp : 0) * 4; }

// lse / entropy [B] of softmax over the logits of items 1..N (log-sum-exp; -sum p log p in nats) for every real row; nothing is written
// for padding rows.  ncol: [Bp] = N for real rows, 0 for padding; spart: ader_row_stats_floats(N,Bp) floats of scratch.  Enqueue only.
int ader_row_stats(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, float* spart, float* lse,
                   float* entropy, void* stream) {
    if (stats_bad(B, Bp, H, N, nullptr, 0, 1)) return -2;
    if (B <= 0) return 0;
    StatsArgs a;
    stats_fill(a, rep, emb, B, Bp, H, N, ncol, spart, lse, entropy);
    if (a.ranges > STATS_RMAX) return -2;
    const size_t lds = stats_lds(0);
    const int rc = ader_dyn_lds<k_row_stats>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_row_stats, dim3(a.ranges * (Bp / TB)), dim3(512), lds, st, a);
    hipLaunchKernelGGL(k_stats_merge, dim3((B + 3) / 4), dim3(256), 0, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}
// ader_topk_items (same arguments, same -2 conditions, the same bytes of items / scores) and ader_row_stats out of one catalog walk.
// lse / entropy run over ALL of 1..N whatever seen removes from the answer, and are ader_row_stats' bits for the same (rows, N, Bp).
int ader_topk_items_stats(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* seen, int seen_ld,
                          int k, unsigned long long* part, float* spart, int* items, float* scores, float* lse, float* entropy,
                          void* stream) {
    if (stats_bad(B, Bp, H, N, seen, seen_ld, k)) return -2;
    if (B <= 0) return 0;
    StatsArgs a;
    stats_fill(a, rep, emb, B, Bp, H, N, ncol, spart, lse, entropy);
    if (a.ranges > STATS_RMAX) return -2;
    a.seen = seen; a.seen_ld = seen_ld; a.k = k; a.part = part;
    const size_t lds = stats_lds(stats_rowbuf_lds(k));
    int rc = ader_dyn_lds<k_topk_tile_stats>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_topk_tile_stats, dim3(a.ranges * (Bp / TB)), dim3(512), lds, st, a);
    rc = topk_merge_launch(B, Bp, k, a.ranges, part, items, scores, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_stats_merge, dim3((B + 3) / 4), dim3(256), 0, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
