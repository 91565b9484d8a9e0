// Exact top-K items for wide answers, k up to 1024 (Engine.recommend_wide, torch.ops.ader.topk_items_wide): slab and select.
// The contract is ader_topk_items' (logits.hip): items == the head of the stable argsort of -logits over items 1..N, the scores the very
// float32 of k_logits_tile<MODE_STORE> -- the same [64][LDE] operand layout, the same mma_tile<2> call, the same ksteps -- order (score
// descending, item id ascending), item 0 / -inf when fewer than k candidates exist.  What differs is where the selection happens:
// k_topk_tile keeps k + 64 keys per row in LDS, which ends at k = 64; here no buffer in LDS grows with k.
//
// Per row, in global memory: a list of cap 64-bit keys (topk_key.h), a count, a threshold key (0 = none yet) and a status word.  The
// catalog is walked in slabs of 64-item tiles (ader_topk_wide_slabs, a pure host function of (N, k, cap)):
//   k_topk_wide_tile    appends to a row's list every key of the slab that beats the row's threshold; it selects nothing;
//   k_topk_wide_select  after every slab cuts the list to its best k, sorted, and sets the threshold to the k-th key (0 if fewer);
//                       after the last slab it unpacks items / scores instead.
// Slab 0 covers items [0, min(N, cap)): every candidate is appended and the list cannot overflow.  With `seen` items done the next slab
// has max(64, 64 floor(seen min(1, (cap - k) / (G k)) / 64)) items, G = WIDE_GROWTH = 32: an item beats the k-th best of `seen`
// exchangeable items with probability about k / seen, so a slab is expected to append about 1 / G of the free room cap - k.  The rest of
// the room is for catalogs whose scores trend with the item id (a briefly trained table, whose untrained upper half of the
// id range scores about one standard deviation above the trained half, overflowed at G = 4 and k = 1024).
//
// CORRECTNESS.  After slab j an unflagged row's list is the exact top-k of the items of slabs <= j, as a set: the filter drops only
// keys that k kept keys already beat (the threshold is the k-th best of an earlier prefix, and the best k only improve), every key
// that passes is stored, and the select keeps the best k of what is stored.  The best k of a set under a total order do not depend on
// the order the set was written in: atomics only hand out slots, and every output is derived from sorted keys -- k_topk_tile's
// argument without its in-kernel compaction.  A key whose slot would be >= cap is dropped and the row's status word is set: a flagged
// row's output is unspecified, and the caller recomputes it.  Nothing outside [0, cap) of a row's list is ever written.
#include "common.h"
#include "topk_key.h"
#include "../../include/ader_hip.h"

#define HP 160
#define LDE 162         // (row, k) operand reads conflict-free: logits.hip's operand layout
#define TI 64           // items per tile
#define TB 64           // batch rows per chunk
#define MAXB 1024       // max (padded) batch rows per launch
#define WIDE_KMAX 1024
#define WIDE_CAP 4096   // default and largest list capacity: 32 KB of keys, what k_topk_wide_select sorts in LDS
#define WIDE_GROWTH 32  // a slab is sized to append about (cap - k) / WIDE_GROWTH keys per row of exchangeable items

struct WideArgs {
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1) : [N,H]
    int B, Bp, H, N;
    const int* ncol;       // [Bp] N for real rows, 0 for padding rows
    const int* seen;       // [B, seen_ld] 1-based ids never to be returned (0 = none), or NULL
    int seen_ld, k, cap;
    int s_begin, s_end;    // the slab's 64-item tiles [s_begin, s_end)
    int runs;              // tile runs per 64-row chunk
    int slab, last;        // slab index; last: this select unpacks
    u64* list;             // [Bp][cap]
    int* cnt;              // [Bp] keys appended to the row's list (may pass cap: the excess was dropped)
    u64* thr;              // [Bp] the row's k-th best key at its last select, 0 = none
    int* row_status;       // [Bp] != 0: a key of the row was dropped
    int* diag;             // [0] largest list length a select after slab 0 met, [1] flagged rows
    int* items;            // [B,k]
    float* scores;         // [B,k]
};

// Workgroup = (64-row chunk, contiguous run of the slab's tiles), block -> (run, chunk) as in k_topk_tile: the chunks of one run share an
// XCD, hence the L2 that holds the run's table tiles.  The chunk's rep rows are staged once; the run's table tiles stream through E_l,
// the next tile's loads in flight (registers) under the current tile's MFMAs.
//   filter    a lane proposes (row, item) when the item is a column of the row, is not in the row's seen mask and its key beats the row's
//             threshold, read once per workgroup: it does not change during a launch;
//   reserve   slots per (workgroup, tile, row): an LDS atomic per proposal counts the tile's proposals of the row and gives the key its
//             local position, then one thread per row does ONE returning global atomicAdd on the row's count (a global atomic per key
//             would serialise on one word, and slab 0 appends everything);
//   store     key -> list[row][base + local position] if that is < cap, else the row is flagged with a plain store.
#define WIDE_STAGE_REGS ((64 * LDE + 511) / 512)
__global__ __launch_bounds__(512) void k_topk_wide_tile(WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    u64* thr = (u64*)(R_l + TB * LDE);                       // [TB]
    u64* msk = thr + TB;                                     // [TB] bit i: item tile0 + i is in the row's seen list
    int* tcnt = (int*)(msk + TB);                            // [TB] this tile's proposals of the row
    int* base = tcnt + TB;                                   // [TB] the first slot of this tile's keys in the row's list
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    const int nchunk = a.Bp / TB;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int run = xcd + 8 * (slot / nchunk), bc = slot % nchunk;
    if (run >= a.runs) return;
    const int ntile = a.s_end - a.s_begin;
    const int s_begin = a.s_begin + (int)((long)run * ntile / a.runs), s_end = a.s_begin + (int)((long)(run + 1) * ntile / a.runs);
    if (s_begin >= s_end) return;
    for (int i = tid; i < 64 * LDE; i += 512) {              // stage_tile's layout (logits.hip)
        const int r = i / LDE, c = i - r * LDE;
        R_l[i] = (bc * TB + r < a.B && c < H) ? a.rep[(size_t)(bc * TB + r) * H + c] : 0.0f;
    }
    if (tid < TB) { thr[tid] = a.thr[bc * TB + tid]; msk[tid] = 0; }
    int nc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int b = bc * TB + nw * 32 + j * 16 + r16;
        nc[j] = b < a.B ? a.ncol[b] : 0;
    }
    float pre[WIDE_STAGE_REGS];                              // the next tile, in stage_tile's element order
    auto load_tile = [&](int tile0) {
#pragma unroll
        for (int n = 0; n < WIDE_STAGE_REGS; ++n) {
            const int i = tid + n * 512, r = i / LDE, c = i - r * LDE;
            pre[n] = (i < 64 * LDE && tile0 + r < a.N && c < H) ? a.emb1[(size_t)(tile0 + r) * H + c] : 0.0f;
        }
    };
    load_tile(s_begin * TI);
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();                                     // the previous tile's MFMA reads and its reads of base[] are done
#pragma unroll
        for (int n = 0; n < WIDE_STAGE_REGS; ++n)
            if (tid + n * 512 < 64 * LDE) E_l[tid + n * 512] = pre[n];
        if (tid < TB) tcnt[tid] = 0;
        if (a.seen) {                                        // thread (row = tid / 8, part = tid % 8): the 8 lanes of a row are neighbours
            const int row = tid >> 3, b = bc * TB + row;
            u64 m = 0;
            if (b < a.B)
                for (int t = tid & 7; t < a.seen_ld; t += 8) {
                    const unsigned d = (unsigned)(a.seen[(size_t)b * a.seen_ld + t] - 1 - tile0);      // id 0 -> d wraps: never < 64
                    if (d < 64u) m |= 1ull << d;
                }
            m |= __shfl_xor(m, 1, 64); m |= __shfl_xor(m, 2, 64); m |= __shfl_xor(m, 4, 64);
            if ((tid & 7) == 0) msk[row] = m;
        }
        __syncthreads();
        if (s + 1 < s_end) load_tile(tile0 + TI);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il0 = mw * 16 + q * 4, item0 = tile0 + il0;      // this lane's 4 consecutive items
        int pos[2][4];                                             // local position of a proposed key, -1: not proposed
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16;                  // batch row within the chunk
            const u64 t = thr[bl];
            const unsigned sm = (unsigned)(msk[bl] >> il0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int it = item0 + r;
                const bool pass = it < nc[j] && !((sm >> r) & 1u) && topk_key(acc[j][r], it + 1) > t;
                pos[j][r] = pass ? atomicAdd(tcnt + bl, 1) : -1;
            }
        }
        __syncthreads();
        if (tid < TB) {
            const int n = tcnt[tid];
            base[tid] = n ? atomicAdd(a.cnt + bc * TB + tid, n) : 0;      // (n > 0 only for rows below B: nc is 0 elsewhere)
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16, b = bc * TB + bl;
            const int b0 = base[bl];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (pos[j][r] < 0) continue;
                const int p = b0 + pos[j][r];
                if (p >= 0 && p < a.cap) a.list[(size_t)b * a.cap + p] = topk_key(acc[j][r], item0 + r + 1);
                else a.row_status[b] = 1;
            }
        }
    }
}

// One workgroup per real row, after every slab: the row's min(count, cap) keys into LDS, padded with key 0 to the next power of two,
// a bitonic network sorts them descending (keys of a row are distinct; key 0 sinks to the end).  Then either the best k go back to the
// head of the list, count <- min(count, k), threshold <- the k-th key if there are k, else 0; or, after the last slab, items / scores
// are unpacked, padded with item 0 / -inf.
__global__ __launch_bounds__(512) void k_topk_wide_select(WideArgs a) {
    __shared__ u64 s[WIDE_CAP];
    const int tid = threadIdx.x, b = blockIdx.x, k = a.k;
    const int raw = a.cnt[b];
    const int n = raw < a.cap ? (raw < 0 ? 0 : raw) : a.cap;
    int P = 64;
    while (P < n) P <<= 1;                                   // P <= WIDE_CAP: cap <= WIDE_CAP, a power of two
    const u64* lp = a.list + (size_t)b * a.cap;
    for (int i = tid; i < P; i += 512) s[i] = i < n ? lp[i] : 0;
    __syncthreads();
    for (int sz = 2; sz <= P; sz <<= 1)
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int t = tid; t < (P >> 1); t += 512) {
                const int i = ((t / st) * 2 * st) + (t % st), j = i + st;
                const u64 x = s[i], y = s[j];
                const bool desc = (i & sz) == 0;
                if ((x < y) == desc && x != y) { s[i] = y; s[j] = x; }
            }
            __syncthreads();
        }
    const int m = n < k ? n : k;
    if (tid == 0) {
        if (a.slab > 0) atomicMax(a.diag, raw);
        if (a.last && a.row_status[b]) atomicAdd(a.diag + 1, 1);
    }
    if (!a.last) {
        u64* wp = a.list + (size_t)b * a.cap;
        for (int i = tid; i < m; i += 512) wp[i] = s[i];     // m <= k < cap
        if (tid == 0) { a.cnt[b] = m; a.thr[b] = n >= k ? s[k - 1] : 0; }
    } else {
        for (int j = tid; j < k; j += 512) {
            const bool real = j < m;
            a.items[(size_t)b * k + j] = real ? topk_item(s[j]) : 0;
            a.scores[(size_t)b * k + j] = real ? topk_score(s[j]) : -INFINITY;
        }
    }
}

// Items of the slab that follows `seen` items: max(64, 64 floor(seen min(1, (cap - k) / (WIDE_GROWTH k)) / 64)), in integers.
static inline long wide_next_slab(long seen, int k, int cap) {
    const long room = cap - k, full = (long)WIDE_GROWTH * k;
    const long f = room >= full ? seen / 64 : seen * room / (full * 64);
    return f < 1 ? 64 : 64 * f;
}
static inline bool wide_bad(int N, int k, int cap) {
    return N < 1 || k < 1 || k > WIDE_KMAX || cap % 64 != 0 || cap < k + 64 || cap > WIDE_CAP;
}
// tile runs per 64-row chunk for a slab of ntile tiles: about one workgroup per CU over the chunks (ader_topk_ranges' rule)
static inline int wide_runs(int ntile, int nchunk) {
    int target = 256 / (nchunk > 0 ? nchunk : 1);
    if (target < 8) target = 8;
    return ntile < target ? ntile : target;
}

extern "C" {

int ader_topk_wide_kmax(void) { return WIDE_KMAX; }
int ader_topk_wide_cap(void) { return WIDE_CAP; }

// The slab schedule of ader_topk_items_wide, host only: the number of slabs; begin (NULL: none) gets the boundaries begin[0] = 0 < ... <
// begin[slabs] = N, as many of them as fit into max ints.  -2 when N < 1, k outside 1..1024, or cap not a multiple of 64 in
// [k + 64, 4096].
int ader_topk_wide_slabs(int N, int k, int cap, int* begin, int max) {
    if (wide_bad(N, k, cap)) return -2;
    int n = 0;
    long seen = 0;
    if (begin && max > 0) begin[0] = 0;
    while (seen < N) {
        long len = seen == 0 ? cap : wide_next_slab(seen, k, cap);
        if (len > N - seen) len = N - seen;
        seen += len;
        ++n;
        if (begin && n < max) begin[n] = (int)seen;
    }
    return n;
}

// ader_topk_items' contract for 1 <= k <= 1024 by slab and select (kernels above).  list: Bp * cap 64-bit keys; cnt, row_status: [Bp]
// ints; thr: [Bp] 64-bit keys; diag: [2] ints -- all zeroed here.  Afterwards row_status[b] != 0 marks a row whose list overflowed: its
// items / scores are unspecified.  diag[0] = the largest list length a select after slab 0 met (above cap: that row overflowed), diag[1]
// = rows with row_status != 0.  Enqueue only: 2 * ader_topk_wide_slabs(N, k, cap) launches.
int ader_topk_items_wide(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* seen, int seen_ld,
                         int k, int cap, unsigned long long* list, int* cnt, unsigned long long* thr, int* row_status, int* diag,
                         int* items, float* scores, void* stream) {
    if (Bp % TB != 0 || Bp > MAXB || Bp < 0 || B > Bp || H > HP || H < 1 || (seen && seen_ld < 1) || wide_bad(N, k, cap)) return -2;
    if (B <= 0) return 0;
    WideArgs a;
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ncol = ncol; a.seen = seen; a.seen_ld = seen_ld;
    a.k = k; a.cap = cap; a.list = list; a.cnt = cnt; a.thr = thr; a.row_status = row_status; a.diag = diag; a.items = items; a.scores = scores;
    const size_t lds = (size_t)(2 * 64 * LDE) * sizeof(float) + TB * (2 * sizeof(u64) + 2 * sizeof(int));
    const int rc = ader_dyn_lds<k_topk_wide_tile>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)Bp, st);
    if (e == hipSuccess) e = hipMemsetAsync(thr, 0, sizeof(u64) * (size_t)Bp, st);
    if (e == hipSuccess) e = hipMemsetAsync(row_status, 0, sizeof(int) * (size_t)Bp, st);
    if (e == hipSuccess) e = hipMemsetAsync(diag, 0, sizeof(int) * 2, st);
    if (e != hipSuccess) return (int)e;
    const int nchunk = Bp / TB;
    long seen_items = 0;
    for (int slab = 0; seen_items < N; ++slab) {
        long len = slab == 0 ? cap : wide_next_slab(seen_items, k, cap);
        if (len > N - seen_items) len = N - seen_items;
        a.s_begin = (int)(seen_items / TI); a.s_end = (int)((seen_items + len + TI - 1) / TI);      // (slab starts are multiples of 64)
        a.runs = wide_runs(a.s_end - a.s_begin, nchunk);
        seen_items += len;
        a.slab = slab; a.last = seen_items >= N;
        hipLaunchKernelGGL(k_topk_wide_tile, dim3((a.runs + 7) / 8 * 8 * nchunk), dim3(512), lds, st, a);
        hipLaunchKernelGGL(k_topk_wide_select, dim3(B), dim3(512), 0, st, a);
    }
    HIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
