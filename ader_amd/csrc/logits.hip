// Full-catalog logits, softmax cross-entropy / distillation loss and their gradients, float32 path.
// Reference: ADER.py:88-93 (logits = rep . item_emb^T over items 1..N, one-hot CE), ADER.py:108-137
// (ADER loss: CE on the train rows + lambda * soft-label CE of the exemplar rows against softmax(teacher)
// over the first Np columns), ADER.py:99-103 (rank of every item = argsort(argsort(-logits))).
//
// The [B,N] logits / one-hot / softmax tensors of the TF graph are never materialised: every pass
// recomputes 64x64 logit tiles on v_mfma_f32_16x16x4_f32 from LDS-staged table rows (each table row is
// read once per pass, coalesced) and reduces them on the fly:
//   k_logits_tile<LSE>   per-row online (max, sum-exp, target.logit) partials      -> k_lse_loss
//   k_logits_tile<RANK>  per-row count of items ranked before the target           (Evaluator, util.py:323-325)
//   k_logits_tile<STORE> dense logits (teacher logits of selected exemplars, util.py:433; model.logits fetch)
//   k_target_logit / k_pair_logit_rank   the RANK bits of single (row, item) pairs: a row's target, the x3 rank filter's recheck
//   k_teacher_rows      the STORE bits of a step's exemplar rows from stored teacher representations  (TeacherRep, util.py:433)
//   k_logits_bwd_drep    dRep[b,:] = sum_n dlogit[b,n] E[n,:]   (b-chunk x item-range workgroups, slabs)
//   k_logits_bwd_de      dE[n,:]   = sum_b dlogit[b,n] rep[b,:] (item-tile workgroups; rows written once, no atomics)
// with dlogit[b,n] = w_b * (softmax_b[n] - target_b[n]) for n < ncol_b, else 0.
// Row descriptors (RowInfo): label, ncol (N for one-hot rows, Np for distilled rows), weight
// (1/B_train or lambda/B_ex, global counts under data parallelism), teacher row + teacher log-sum-exp.
// The operand layout, stage_tile and the tile stream are logit_tile.h's; the exact top-K family that selects from the STORE bits
// (Engine.recommend, recommend_among, recommend_wide) is topk.hip: a translation unit of its own, because one more caller of stage_tile
// or mma_tile<2> in this file changes the code the compiler emits for k_logits_bwd_de / k_logits_bwd_drep (tools/isa_digest.py).
#include "logit_tile.h"
#include "../../include/ader_hip.h"

#define LDD 68          // 64x64 dlogit tile

enum { MODE_LSE = 0, MODE_RANK = 1, MODE_STORE = 2 };

struct RowInfo {
    const int* lab;        // [Bp] 1-based target item, 0 = soft target only
    const int* ncol;       // [Bp] valid columns (0 for padding rows)
    const float* wrow;     // [Bp] loss weight
    const int* trow;       // [Bp] teacher row or -1
    const float* tlse;     // [Bp] teacher log-sum-exp
    const float* teacher;  // [*, ldt]
    long ldt;
};

struct LogitArgs {
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1) : [N,H]
    int B, Bp, H, N;
    RowInfo ri;
    // MODE_LSE
    float* part;           // [grid][Bp][3]
    int sub;               // 64-item sub-tiles per workgroup
    // MODE_RANK
    const float* tlogit;   // [Bp] logit of the target item (computed by the same MFMA path)
    int* rank;             // [Bp] zero-initialised
    // MODE_STORE
    float* out; long ldo;  // [B, ldo]
    // backward
    const float* lse;      // [Bp]
    float* demb1;          // gradient row of item 1 : [N,H]
    float* slab;           // drep slabs [ranges][Bp][HP]
    int ranges;
};

__device__ __forceinline__ void merge_ml(float& m, float& l, float m2, float l2) {
    const float mn = fmaxf(m, m2);
    const float a = (m == -INFINITY) ? 0.0f : l * expf(m - mn);
    const float b = (m2 == -INFINITY) ? 0.0f : l2 * expf(m2 - mn);
    m = mn; l = a + b;
}

// C^T tile: rows = items (MFMA M), cols = batch rows (MFMA N) so that per-batch-row reductions over items
// are lane-local.  8 waves: wave (mw = w&3 -> 16 items, nw = w>>2 -> 32 batch rows).
template <int MODE>
__global__ __launch_bounds__(512) void k_logits_tile(LogitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;             // [TB][LDE]
    float* wp = R_l + TB * LDE;              // [4][TB][3] wave partials
    float* run = wp + 4 * TB * 3;            // [MAXB][3] running (m, l, dot) per batch row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    if (MODE == MODE_LSE)
        for (int i = tid; i < a.Bp; i += 512) { run[i * 3 + 0] = -INFINITY; run[i * 3 + 1] = 0.0f; run[i * 3 + 2] = 0.0f; }
    const int nsub = (MODE == MODE_LSE) ? a.sub : 1;
    for (int st = 0; st < nsub; ++st) {
        const int tile0 = (blockIdx.x * nsub + st) * TI;
        if (tile0 >= a.N) break;
        __syncthreads();
        stage_tile(E_l, a.emb1, tile0, a.N, H, tid, 512);
        for (int bc = 0; bc < a.Bp / TB; ++bc) {
            __syncthreads();
            stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
            __syncthreads();
            f32x4 acc[2];
            acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
            mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
            const int item0 = tile0 + mw * 16 + q * 4;        // this lane's 4 consecutive items
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int bl = nw * 32 + j * 16 + r16;        // batch row within the chunk
                const int b = bc * TB + bl;
                const int nc = a.ri.ncol[b];
                if (MODE == MODE_STORE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (b < a.B && item0 + r < a.N) a.out[(size_t)b * a.ldo + item0 + r] = acc[j][r];
                } else if (MODE == MODE_RANK) {
                    const int tgt = a.ri.lab[b] - 1;
                    const float tl = a.tlogit[b];
                    int cnt = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int it = item0 + r;
                        // the target never counts itself, even if k_target_logit's rounding ever differed from the tile's
                        if (it < nc && it != tgt) cnt += (acc[j][r] > tl) || (acc[j][r] == tl && it < tgt);
                    }
                    cnt += __shfl_xor(cnt, 16, 64);
                    cnt += __shfl_xor(cnt, 32, 64);
                    if (q == 0 && cnt) atomicAdd(a.rank + b, cnt);
                } else {
                    float m = -INFINITY, l = 0.0f, dot = 0.0f;
                    const int tgt = a.ri.lab[b] - 1;
                    const int tr = a.ri.trow[b];
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (item0 + r < nc) m = fmaxf(m, acc[j][r]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int it = item0 + r;
                        if (it < nc) {
                            const float s = acc[j][r];
                            l += expf(s - m);
                            if (it == tgt) dot += s;
                            if (tr >= 0) dot += expf(a.ri.teacher[(size_t)tr * a.ri.ldt + it] - a.ri.tlse[b]) * s;
                        }
                    }
#pragma unroll
                    for (int o = 16; o <= 32; o <<= 1) {
                        const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
                        merge_ml(m, l, m2, l2);
                        dot += __shfl_xor(dot, o, 64);
                    }
                    if (q == 0) { float* w = wp + (mw * TB + bl) * 3; w[0] = m; w[1] = l; w[2] = dot; }
                }
            }
            if (MODE == MODE_LSE) {
                __syncthreads();
                if (tid < TB) {
                    float* rn = run + (bc * TB + tid) * 3;
                    float m = rn[0], l = rn[1], dot = rn[2];
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const float* p = wp + (w * TB + tid) * 3;
                        merge_ml(m, l, p[0], p[1]);
                        dot += p[2];
                    }
                    rn[0] = m; rn[1] = l; rn[2] = dot;
                }
            }
        }
    }
    if (MODE == MODE_LSE) {
        __syncthreads();
        float* o = a.part + (size_t)blockIdx.x * a.Bp * 3;
        for (int i = tid; i < a.Bp * 3; i += 512) o[i] = run[i];
    }
}


// Row descriptors for one step: train rows first (one-hot targets, ADER.py:118-121), exemplar rows after
// (ADER.py:113-137): distilled rows (ex_trow != NULL) use ncol = Np and a teacher row; one-hot exemplar rows
// (disable_distillation, ADER.py:126-131) use their label over all N columns; padding rows get ncol = 0.
__global__ __launch_bounds__(256) void k_build_rowinfo(const int* __restrict__ pos, int n_train, const int* __restrict__ ex_pos,
                                                       const int* __restrict__ ex_trow, int n_ex, int N, int Np, float w_train, float w_ex,
                                                       int Bp, int* __restrict__ lab, int* __restrict__ ncol, float* __restrict__ wrow,
                                                       int* __restrict__ trow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Bp) return;
    int l = 0, nc = 0, tr = -1; float w = 0.0f;
    // A label / teacher row of 0 / -1 marks a PADDING row (data-parallel shards are padded to equal row counts): weight 0,
    // so it adds nothing to the loss or to any gradient.  Real labels are item ids >= 1 (util.py:161-171).
    if (i < n_train) { l = pos[i]; nc = N; w = (l > 0) ? w_train : 0.0f; }
    else if (i < n_train + n_ex) {
        const int e = i - n_train;
        if (ex_trow) { nc = Np; tr = ex_trow[e]; w = (tr >= 0) ? w_ex : 0.0f; if (tr < 0) tr = 0; }
        else { nc = N; l = ex_pos[e]; w = (l > 0) ? w_ex : 0.0f; }
    }
    lab[i] = l; ncol[i] = nc; wrow[i] = w; trow[i] = tr;
}

// lse[b] = logsumexp over the row's valid columns; rowloss[b] = w_b * (lse_b - sum_n target_n * logit_n).
// One wave per batch row merges the per-workgroup partials in a fixed order.
__global__ __launch_bounds__(256) void k_lse_loss(const float* __restrict__ part, int nparts, int Bp, int B,
                                                  const float* __restrict__ wrow, float* __restrict__ lse, float* __restrict__ rowloss) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + wave;
    if (b >= Bp) return;
    float m = -INFINITY, l = 0.0f, dot = 0.0f;
    for (int p = lane; p < nparts; p += 64) {
        const float* x = part + ((size_t)p * Bp + b) * 3;
        merge_ml(m, l, x[0], x[1]);
        dot += x[2];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
        merge_ml(m, l, m2, l2);
        dot += __shfl_xor(dot, o, 64);
    }
    if (lane == 0) {
        const float z = (b < B && l > 0.0f) ? m + logf(l) : 0.0f;
        lse[b] = z;
        rowloss[b] = (b < B) ? wrow[b] * (z - dot) : 0.0f;
    }
}

// out[0] = sum_i x[i] (single workgroup, fixed tree: deterministic)
__global__ __launch_bounds__(256) void k_sum(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// Row-wise log-sum-exp of the teacher logits (softmax(exemplar_logits), ADER.py:135): one workgroup per row.
__global__ __launch_bounds__(256) void k_row_lse(const float* __restrict__ x, long ld, int ncols, const int* __restrict__ rows,
                                                 float* __restrict__ out) {
    __shared__ float red[256];
    const int r = rows ? rows[blockIdx.x] : blockIdx.x;
    if (r < 0) { if (threadIdx.x == 0) out[blockIdx.x] = 0.0f; return; }
    const float* p = x + (size_t)r * ld;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < ncols; i += 256) m = fmaxf(m, p[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]); __syncthreads(); }
    m = red[0];
    __syncthreads();
    float l = 0.0f;
    for (int i = threadIdx.x; i < ncols; i += 256) l += expf(p[i] - m);
    red[threadIdx.x] = l;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = m + logf(red[0]);
}

__device__ __forceinline__ float dlogit(const LogitArgs& a, int b, int it, float s, int nc, float w, float z, int tgt, int tr, float tz) {
    if (it >= nc) return 0.0f;
    float p = expf(s - z);
    if (it == tgt) p -= 1.0f;
    if (tr >= 0) p -= expf(a.ri.teacher[(size_t)tr * a.ri.ldt + it] - tz);
    return w * p;
}

// dE tile: one workgroup per 64 items, loops over all batch chunks; wave (mw, nw) owns dE rows 16mw.. x columns 80nw..
__global__ __launch_bounds__(512) void k_logits_bwd_de(LogitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;
    float* R_l = E_l + TI * LDE;
    float* D_l = R_l + TB * LDE;             // [items][batch] dlogit^T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile0 = blockIdx.x * TI;
    stage_tile(E_l, a.emb1, tile0, a.N, H, tid, 512);
    f32x4 dacc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) dacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int bc = 0; bc < a.Bp / TB; ++bc) {
        __syncthreads();
        stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
        __syncthreads();
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il = mw * 16 + q * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16;
            const int b = bc * TB + bl;
            const int nc = a.ri.ncol[b], tgt = a.ri.lab[b] - 1, tr = a.ri.trow[b];
            const float w = a.ri.wrow[b], z = a.lse[b], tz = a.ri.tlse[b];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                D_l[(il + r) * LDD + bl] = dlogit(a, b, tile0 + il + r, acc[j][r], nc, w, z, tgt, tr, tz);
        }
        __syncthreads();
        mma_tile<5>(D_l + mw * 16 * LDD, LDD, 1, R_l + nw * 80, LDE, 1, TB / 4, dacc, lane);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int h = nw * 80 + j * 16 + r16;
        if (h >= H) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int it = tile0 + mw * 16 + q * 4 + r;
            if (it < a.N) a.demb1[(size_t)it * H + h] = dacc[j][r];
        }
    }
}

// dRep: workgroup = (batch chunk, item range); dRep chunk accumulated in registers over the range, written as a slab.
// Block -> (range, chunk) mapping keeps the chunks that stream the same item range on one XCD (blocks b and b+8
// share an XCD) so the table rows are re-read from that XCD's L2 rather than HBM.  Speed only, not correctness.
__global__ __launch_bounds__(512) void k_logits_bwd_drep(LogitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;
    float* R_l = E_l + TI * LDE;
    float* D_l = R_l + TB * LDE;             // [batch][items] dlogit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    const int nchunk = a.Bp / TB;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int range = xcd + 8 * (slot / nchunk), bc = slot % nchunk;
    if (range >= a.ranges) return;
    const int nsub_total = (a.N + TI - 1) / TI;
    const int per = (nsub_total + a.ranges - 1) / a.ranges;
    const int s_begin = range * per, s_end = min(nsub_total, s_begin + per);
    stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
    f32x4 racc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) racc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // row constants of this lane's 4 batch rows (D rows = (lane>>4)*4 + r)
    int nc[4], tgt[4], tr[4]; float w[4], z[4], tz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bc * TB + mw * 16 + q * 4 + r;
        nc[r] = a.ri.ncol[b]; tgt[r] = a.ri.lab[b] - 1; tr[r] = a.ri.trow[b];
        w[r] = a.ri.wrow[b]; z[r] = a.lse[b]; tz[r] = a.ri.tlse[b];
    }
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();
        stage_tile(E_l, a.emb1, tile0, a.N, H, tid, 512);
        __syncthreads();
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(R_l + mw * 16 * LDE, LDE, 1, E_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int il = nw * 32 + j * 16 + r16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = bc * TB + mw * 16 + q * 4 + r;
                D_l[(mw * 16 + q * 4 + r) * LDD + il] = dlogit(a, b, tile0 + il, acc[j][r], nc[r], w[r], z[r], tgt[r], tr[r], tz[r]);
            }
        }
        __syncthreads();
        mma_tile<5>(D_l + mw * 16 * LDD, LDD, 1, E_l + nw * 80, LDE, 1, TI / 4, racc, lane);
    }
    float* o = a.slab + ((size_t)range * a.Bp + bc * TB) * HP;
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            o[(size_t)(mw * 16 + q * 4 + r) * HP + nw * 80 + j * 16 + r16] = racc[j][r];
}

// Logit of each row's target item through the same MFMA k-order as the tile kernels (so the == comparison of the
// rank kernel is exact): 64 batch rows x their 64 gathered target rows, diagonal extracted.
__global__ __launch_bounds__(256) void k_target_logit(LogitArgs a, float* __restrict__ tl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;
    float* R_l = E_l + TI * LDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int bc = blockIdx.x;
    for (int i = tid; i < 64 * LDE; i += 256) {
        const int r = i / LDE, c = i - r * LDE;
        const int b = bc * TB + r;
        const int t = (b < a.B) ? a.ri.lab[b] - 1 : -1;
        E_l[i] = (t >= 0 && t < a.N && c < H) ? a.emb1[(size_t)t * H + c] : 0.0f;
        R_l[i] = (b < a.B && c < H) ? a.rep[(size_t)b * H + c] : 0.0f;
    }
    __syncthreads();
    // wave w: items (targets) 16w..16w+15 x batch rows 16w..16w+15 (only the diagonal block is needed)
    f32x4 acc[1];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mma_tile<1>(E_l + wave * 16 * LDE, LDE, 1, R_l + wave * 16 * LDE, 1, LDE, ksteps, acc, lane);
    const int col = lane & 15, q = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (q * 4 + r == col) { const int b = bc * TB + wave * 16 + col; tl[b] = acc[0][r]; }
}

// The recheck of the x3 rank filter (k_lx3k, logits_x3.hip): k_target_logit generalised from "row b with its own target" to a list of
// (row, item, x3 logit) pairs.  A wave takes 16 pairs, their 16 table rows and 16 rep rows in the [64][LDE] layout, runs the same
// mma_tile<1> k-order and reads the diagonal: the very bits k_logits_tile<MODE_RANK> computes for that pair, so its comparison gives
// the same answer.  diag[0] = entries the filter asked for (min(diag[0], cap) are in the list); diag[1] <- max |s_x3 - s| / delta as
// float bits (non-negative: an integer max orders them) -- the observed error of the filter as a share of its band.
__global__ __launch_bounds__(256) void k_pair_logit_rank(LogitArgs a, const float* __restrict__ delta, const int* __restrict__ cand,
                                                         int cap, int* __restrict__ diag) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;
    float* R_l = E_l + TI * LDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int count = min(diag[0], cap);
    const int p0 = blockIdx.x * 64;
    if (p0 >= count) return;                                  // (the grid is sized for cap)
    for (int i = tid; i < 64 * LDE; i += 256) {
        const int r = i / LDE, c = i - r * LDE;
        int b = -1, it = -1;
        if (p0 + r < count) { b = cand[3 * (size_t)(p0 + r)]; it = cand[3 * (size_t)(p0 + r) + 1]; }
        const bool ok = b >= 0 && b < a.B && it >= 0 && it < a.N && c < H;
        E_l[i] = ok ? a.emb1[(size_t)it * H + c] : 0.0f;
        R_l[i] = ok ? a.rep[(size_t)b * H + c] : 0.0f;
    }
    __syncthreads();
    f32x4 acc[1];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mma_tile<1>(E_l + wave * 16 * LDE, LDE, 1, R_l + wave * 16 * LDE, 1, LDE, ksteps, acc, lane);
    const int col = lane & 15, q = lane >> 4;
    const int p = p0 + wave * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (q * 4 + r == col && p < count) {
            const int b = cand[3 * (size_t)p], it = cand[3 * (size_t)p + 1];
            if (b < 0 || b >= a.B || it < 0 || it >= a.N) continue;
            const float s = acc[0][r], s3 = __int_as_float(cand[3 * (size_t)p + 2]);
            const float tl = a.tlogit[b], d = delta[b];
            const int tgt = a.ri.lab[b] - 1;
            if ((s > tl) || (s == tl && it < tgt)) atomicAdd(a.rank + b, 1);
            const float err = d > 0.0f ? fabsf(s3 - s) / d : 0.0f;
            if (err > 0.0f) atomicMax(diag + 1, __float_as_int(err));
        }
}

// ============================================================================================= teacher rows from stored representations
// ader_teacher_rows: the teacher logits of one step's exemplar rows (util.py:433, consumed by ADER.py:134-135), regenerated from the
// teacher's representations trep [E,H] and the item table as it stood when the teacher was taken, instead of being kept as an [E, Np]
// tensor.  rows[e, n] is the float32 k_logits_tile<MODE_STORE> writes for representation trep[ex_trow[e]] against item n + 1: the same
// [64][LDE] operand layout, the same mma_tile<2> call, the same ksteps -- and a (row, item) result of that chain does not depend on
// which other rows or items share the tile, so the bits are the stored teacher's.  logit_tile.h's walk and tile stream: workgroup =
// (64-row chunk, contiguous range of 64-item tiles); the chunk's representations are gathered by ex_trow into LDS once, the range's
// table tiles stream through E_l with the next tile's loads in flight (registers) under the current tile's MFMAs.  Every (row, item) is written by
// exactly one lane: no atomics on floats, no reduction across workgroups.  Padding rows (ex_trow < 0, e >= n_ex) are written as 0.0f
// whatever the table holds; a teacher row >= E is never read: the row is written as padding and the status word flagged.
struct TeachArgs {
    const float* trep;     // [E,H]
    const float* emb1;     // snapshot table row 1 (item 1) : [N,H]
    const int* ex_trow;    // [n_ex] teacher row or -1
    int n_ex, Bk, E, H, N, ranges;
    float* rows;           // [Bk, ldr]
    long ldr;
    int* trow_local;       // [Bk]
    int* status;           // engine status word, or NULL
};

__global__ __launch_bounds__(512) void k_teacher_rows(TeachArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    int* tr_l = (int*)(R_l + TB * LDE);                      // [TB] teacher row of the chunk's rows, -1 = padding
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    int range, bc, s_begin, s_end;
    if (!tile_walk(a.Bk / TB, a.ranges, (a.N + TI - 1) / TI, range, bc, s_begin, s_end)) return;
    if (tid < TB) {
        const int e = bc * TB + tid;
        int t = (e < a.n_ex) ? a.ex_trow[e] : -1;
        if (t >= a.E) { if (a.status) atomicOr(a.status, ADER_ST_BAD_TROW); t = -1; }
        if (t < 0) t = -1;
        tr_l[tid] = t;
        if (range == 0) a.trow_local[e] = (t >= 0) ? e : -1;          // (range 0 exists for every chunk, with or without tiles)
    }
    __syncthreads();
    for (int i = tid; i < 64 * LDE; i += 512) {                        // stage_tile's layout, the rows gathered
        const int r = i / LDE, c = i - r * LDE;
        const int t = tr_l[r];
        R_l[i] = (t >= 0 && c < H) ? a.trep[(size_t)t * H + c] : 0.0f;
    }
    bool real[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) real[j] = tr_l[nw * 32 + j * 16 + r16] >= 0;
    const bool vec_ok = (((uintptr_t)a.rows) & 15) == 0;               // (ldr % 4 == 0 and item0 % 4 == 0: a lane's 4 items are one 16-byte piece)
    float pre[TILE_STAGE_REGS];
    if (s_begin < s_end) tile_load(pre, a.emb1, s_begin * TI, a.N, H, tid);
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();                                               // the previous tile's MFMA reads are done (first pass: R_l is staged)
        tile_store(E_l, pre, tid);
        __syncthreads();
        if (s + 1 < s_end) tile_load(pre, a.emb1, tile0 + TI, a.N, H, tid);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int item0 = tile0 + mw * 16 + q * 4;                     // this lane's 4 consecutive items
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = bc * TB + nw * 32 + j * 16 + r16;            // e < Bk: every row of the chunk is written
            const f32x4 v = real[j] ? acc[j] : (f32x4){0.f, 0.f, 0.f, 0.f};
            float* o = a.rows + (size_t)e * a.ldr + item0;
            if (vec_ok && item0 + 3 < a.N) {
                *(f32x4*)o = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (item0 + r < a.N) o[r] = v[r];
            }
        }
    }
}

// ============================================================================================= C ABI
static const size_t kTileLds = (size_t)(2 * 64 * LDE + 4 * TB * 3 + MAXB * 3) * sizeof(float);
static const size_t kBwdLds = (size_t)(2 * 64 * LDE + 64 * LDD) * sizeof(float);
static const size_t kTgtLds = (size_t)(2 * 64 * LDE) * sizeof(float);

static int fill_args(LogitArgs& a, const float* rep, const float* emb, int B, int Bp, int H, int N, const int* lab, const int* ncol,
                     const float* wrow, const int* trow, const float* tlse, const float* teacher, long ldt) {
    if (Bp % TB != 0 || Bp > MAXB || B > Bp || H > HP || H < 1) return -2;
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N;
    a.ri.lab = lab; a.ri.ncol = ncol; a.ri.wrow = wrow; a.ri.trow = trow; a.ri.tlse = tlse; a.ri.teacher = teacher; a.ri.ldt = ldt;
    a.part = nullptr; a.sub = 1; a.tlogit = nullptr; a.rank = nullptr; a.out = nullptr; a.ldo = 0; a.lse = nullptr;
    a.demb1 = nullptr; a.slab = nullptr; a.ranges = 0;
    return 0;
}

// the two exact-f32 pieces of ader_rank_targets_x3 (logits_x3.hip): target logits, and the recheck of the filter's list
int rank_target_logit_launch(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                             float* tlogit, void* stream) {
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, target, ncol, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    rc = ader_dyn_lds<k_target_logit>(kTgtLds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_target_logit, dim3(Bp / TB), dim3(256), kTgtLds, (hipStream_t)stream, a, tlogit);
    HIP_LAUNCH_CHECK();
    return 0;
}
int rank_pairs_launch(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                      const float* tlogit, const float* delta, const int* cand, int cap, int* diag, int* rank, void* stream) {
    if (cap <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, target, ncol, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    rc = ader_dyn_lds<k_pair_logit_rank>(kTgtLds);
    if (rc) return rc;
    a.tlogit = tlogit; a.rank = rank;
    hipLaunchKernelGGL(k_pair_logit_rank, dim3((cap + 63) / 64), dim3(256), kTgtLds, (hipStream_t)stream, a, delta, cand, cap, diag);
    HIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

// Sub-tiles per workgroup / number of partial slabs for a catalog of N items.
int ader_logits_sub(int N) {
    const int nsub = (N + TI - 1) / TI;
    int sub = nsub / 2048;
    if (sub < 1) sub = 1;
    if (sub > 8) sub = 8;
    return sub;
}
int ader_logits_parts(int N) {
    const int nsub = (N + TI - 1) / TI;
    const int sub = ader_logits_sub(N);
    return (nsub + sub - 1) / sub;
}
int ader_logits_ranges(int N, int Bp) {
    const int nsub = (N + TI - 1) / TI;
    int target = 1024 / (Bp / TB);          // ~1024 workgroups
    int r = 8;
    while (r * 2 <= target && r * 2 <= nsub) r *= 2;
    return r;                                // multiple of 8
}

int ader_build_rowinfo(const int* pos, int n_train, const int* ex_pos, const int* ex_trow, int n_ex, int N, int Np, float w_train,
                       float w_ex, int Bp, int* lab, int* ncol, float* wrow, int* trow, void* stream) {
    if (Bp <= 0) return 0;
    hipLaunchKernelGGL(k_build_rowinfo, dim3((Bp + 255) / 256), dim3(256), 0, (hipStream_t)stream, pos, n_train, ex_pos, ex_trow, n_ex, N,
                       Np, w_train, w_ex, Bp, lab, ncol, wrow, trow);
    HIP_LAUNCH_CHECK();
    return 0;
}

int ader_row_lse(const float* x, long ld, int ncols, const int* rows, int nrows, float* out, void* stream) {
    if (nrows <= 0) return 0;
    hipLaunchKernelGGL(k_row_lse, dim3(nrows), dim3(256), 0, (hipStream_t)stream, x, ld, ncols, rows, out);
    HIP_LAUNCH_CHECK();
    return 0;
}

// Forward: lse[Bp], rowloss[Bp], loss[1].  part: ader_logits_parts(N) * Bp * 3 floats of scratch.
int ader_logits_loss_fwd(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* lab, const int* ncol,
                         const float* wrow, const int* trow, const float* tlse, const float* teacher, long ldt, float* part,
                         float* lse, float* rowloss, float* loss, void* stream) {
    if (B <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, lab, ncol, wrow, trow, tlse, teacher, ldt);
    if (rc) return rc;
    rc = ader_dyn_lds<k_logits_tile<MODE_LSE>>(kTileLds);
    if (rc) return rc;
    a.part = part; a.sub = ader_logits_sub(N);
    const int parts = ader_logits_parts(N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_logits_tile<MODE_LSE>, dim3(parts), dim3(512), kTileLds, st, a);
    hipLaunchKernelGGL(k_lse_loss, dim3((Bp + 3) / 4), dim3(256), 0, st, part, parts, Bp, B, wrow, lse, rowloss);
    hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, st, rowloss, B, loss);
    HIP_LAUNCH_CHECK();
    return 0;
}

// Backward, part 1: dRep [B,H] (slab: ader_logits_ranges(N,Bp) * Bp * 160 floats of scratch).
int ader_logits_bwd_drep(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* lab, const int* ncol,
                         const float* wrow, const int* trow, const float* tlse, const float* teacher, long ldt, const float* lse,
                         float* slab, float* drep, void* stream) {
    if (B <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, lab, ncol, wrow, trow, tlse, teacher, ldt);
    if (rc) return rc;
    rc = ader_dyn_lds<k_logits_bwd_drep>(kBwdLds);
    if (rc) return rc;
    a.lse = lse; a.slab = slab; a.ranges = ader_logits_ranges(N, Bp);
    const int nchunk = Bp / TB;
    hipLaunchKernelGGL(k_logits_bwd_drep, dim3(a.ranges * nchunk), dim3(512), kBwdLds, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return ader_reduce_slabs(slab, (long)Bp * HP, a.ranges, HP, B, H, drep, nullptr, stream);
}

// Backward, part 2: table gradient rows 1..N (overwritten; every row written exactly once, no atomics).
int ader_logits_bwd_demb(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* lab, const int* ncol,
                         const float* wrow, const int* trow, const float* tlse, const float* teacher, long ldt, const float* lse,
                         float* demb, void* stream) {
    if (B <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, lab, ncol, wrow, trow, tlse, teacher, ldt);
    if (rc) return rc;
    rc = ader_dyn_lds<k_logits_bwd_de>(kBwdLds);
    if (rc) return rc;
    a.lse = lse; a.demb1 = demb + H;
    hipLaunchKernelGGL(k_logits_bwd_de, dim3((N + TI - 1) / TI), dim3(512), kBwdLds, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

// Dense logits out[b, 0:N] = rep[b] . E[1..N]^T   (ADER.py:92; exemplar teacher logits, util.py:433)
int ader_logits_store(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol_all, float* out, long ldo,
                      void* stream) {
    if (B <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, nullptr, ncol_all, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    rc = ader_dyn_lds<k_logits_tile<MODE_STORE>>(kTileLds);
    if (rc) return rc;
    a.out = out; a.ldo = ldo;
    hipLaunchKernelGGL(k_logits_tile<MODE_STORE>, dim3((N + TI - 1) / TI), dim3(512), kTileLds, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

// rank[b] = #{n < N : logit[b,n] > logit[b,t]  or (== and n < t)},  t = target[b]-1   (0-based rank, ties -> lower index first)
// tlogit: Bp floats scratch; ncol: [Bp] = N for real rows, 0 for padding; rank: [Bp] (zeroed here).
int ader_rank_targets(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                      float* tlogit, int* rank, void* stream) {
    if (B <= 0) return 0;
    LogitArgs a;
    int rc = fill_args(a, rep, emb, B, Bp, H, N, target, ncol, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    rc = ader_dyn_lds<k_logits_tile<MODE_RANK>>(kTileLds);
    if (rc) return rc;
    rc = ader_dyn_lds<k_target_logit>(kTgtLds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(rank, 0, sizeof(int) * (size_t)Bp, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_target_logit, dim3(Bp / TB), dim3(256), kTgtLds, st, a, tlogit);
    a.tlogit = tlogit; a.rank = rank;
    hipLaunchKernelGGL(k_logits_tile<MODE_RANK>, dim3((N + TI - 1) / TI), dim3(512), kTileLds, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

// Teacher logits of a step's exemplar rows from stored representations (kernel above).  ader_teacher_ranges: item ranges per 64-row
// chunk -- about one workgroup per CU over the Bk/64 chunks, at most one range per four 64-item tiles (the tile stream is what hides the
// table loads), a multiple of 8 (the block -> (range, chunk) mapping), so a small catalog leaves some ranges empty.
int ader_teacher_ranges(int Np, int Bk) {
    const int nsub = (Np + TI - 1) / TI;
    const int nchunk = Bk / TB > 0 ? Bk / TB : 1;
    int target = 256 / nchunk / 8 * 8;
    if (target < 8) target = 8;
    int r = ((nsub + 3) / 4 + 7) / 8 * 8;
    if (r > target) r = target;
    if (r < 8) r = 8;
    return r;
}
// rows[e, 0:Np] = the bits ader_logits_store writes for trep[ex_trow[e]] against items 1..Np of temb (row 0 = the padding item), e < n_ex
// and ex_trow[e] >= 0: trow_local[e] = e; padding rows (ex_trow[e] < 0, or n_ex <= e < Bk): rows[e, 0:Np] = 0.0f, trow_local[e] = -1.
// Columns [Np, ldr) are not written.  lse (NULL: none) [Bk] <- ader_row_lse(rows, ldr, Np, trow_local, Bk): the same kernel, hence the
// same bits; 0.0 for padding rows.  ex_trow[e] >= E is the caller's error: the row becomes a padding row and status (NULL: none) gets
// ADER_ST_BAD_TROW.  Enqueue only.  -2 when H > 160, Bk % 64 != 0, n_ex > Bk, Np < 1, ldr < Np or ldr % 4 != 0.
int ader_teacher_rows(const float* trep, const float* temb, const int* ex_trow, int n_ex, int Bk, int E, int H, int Np, float* rows,
                      long ldr, int* trow_local, float* lse, int* status, void* stream) {
    if (H > HP || H < 1 || Bk <= 0 || Bk % TB != 0 || n_ex < 0 || n_ex > Bk || E < 0 || Np < 1 || ldr < Np || ldr % 4 != 0) return -2;
    TeachArgs a;
    a.trep = trep; a.emb1 = temb + H; a.ex_trow = ex_trow; a.n_ex = n_ex; a.Bk = Bk; a.E = E; a.H = H; a.N = Np;
    a.ranges = ader_teacher_ranges(Np, Bk); a.rows = rows; a.ldr = ldr; a.trow_local = trow_local; a.status = status;
    const size_t lds = (size_t)(2 * 64 * LDE) * sizeof(float) + TB * sizeof(int);
    const int rc = ader_dyn_lds<k_teacher_rows>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_teacher_rows, dim3(a.ranges * (Bk / TB)), dim3(512), lds, st, a);
    if (lse) hipLaunchKernelGGL(k_row_lse, dim3(Bk), dim3(256), 0, st, rows, ldr, Np, trow_local, lse);
    HIP_LAUNCH_CHECK();
    return 0;
}
// The column window of ader_teacher_rows' rows that a rank of the catalog-sharded scheme reads (util.py:433, ADER.py:134-135 with the
// table sharded): rows_win[e, c] = the float32 ader_teacher_rows writes at column item_begin + c of row e, c < n_loc = the shard's items
// [item_begin + 1, item_begin + item_count] below Np (shard_items).  k_teacher_rows as it stands: its table operand starts at the
// shard's first item, its catalog is the n_loc items, and its range partition runs over them -- a (row, item) result does not depend on
// its tile neighbours, so the window holds the dense teacher's bits.  Nothing outside [0, n_loc) of a row is written; n_loc == 0 writes
// trow_local (and the status word) only: every range of the launch is empty and the table operand is never dereferenced.
int ader_teacher_rows_shard(const float* trep, const float* temb, const int* ex_trow, int n_ex, int Bk, int E, int H, int Np,
                            int item_begin, int item_count, float* rows_win, long ldr, int* trow_local, int* status, void* stream) {
    if (H > HP || H < 1 || Bk <= 0 || Bk % TB != 0 || n_ex < 0 || n_ex > Bk || E < 0 || Np < 1 || item_begin < 0 || item_count < 0 ||
        item_begin % 4 != 0 || ldr % 4 != 0) return -2;
    const int n_loc = shard_items(Np, item_begin, item_count);
    if (ldr < n_loc) return -2;
    TeachArgs a;
    a.trep = trep; a.emb1 = temb + (size_t)H * (1 + (n_loc > 0 ? item_begin : 0)); a.ex_trow = ex_trow; a.n_ex = n_ex; a.Bk = Bk; a.E = E; a.H = H;
    a.N = n_loc; a.ranges = ader_teacher_ranges(n_loc, Bk); a.rows = rows_win; a.ldr = ldr; a.trow_local = trow_local; a.status = status;
    const size_t lds = (size_t)(2 * 64 * LDE) * sizeof(float) + TB * sizeof(int);
    const int rc = ader_dyn_lds<k_teacher_rows>(lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_teacher_rows, dim3(a.ranges * (Bk / TB)), dim3(512), lds, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
