// Exact top-K items, float32 path: the k best items of every row by (score descending, item id ascending) -- the order of
// ader_rank_targets and of tf.argsort (ADER.py:103) -- where the score of (b, n) is the float32 of k_logits_tile<MODE_STORE> (logits.hip):
// the operand layout, the mma_tile<2> call and the ksteps of logit_tile.h.  items == the head of the stable argsort of -logits over items
// 1..N, item 0 / -inf when fewer than k candidates exist.
//   k_topk_tile + k_topk_merge               all items 1..N, k <= 64                      (Engine.recommend, ader_topk_items)
//   k_topk_cand + k_topk_merge               the items of one ascending id list, k <= 64  (Engine.recommend_among, ader_topk_items_cand)
//   k_topk_wide_tile + k_topk_wide_select    all items 1..N, k <= 1024, slab and select   (Engine.recommend_wide, ader_topk_items_wide)
// and the evaluation-side twin of the second form, the rank of a row's target under the same order:
//   k_rank_cand                              the items of one ascending id list           (Engine.rank_targets_among, ader_rank_targets_cand)
// and the forms whose list differs from row to row, ids [B, ld]: one kernel, a tile = 64 positions of ONE row's list
//   k_rowlist<STORE>                         the scores of the listed items, any ids      (Engine.score_items, ader_score_items)
//   k_rowlist<KEYS> + k_topk_merge           the k <= 64 best of each row's own list      (Engine.recommend_per_row, ader_topk_items_rows)
//   k_rowlist<RANK>                          the target's rank among each row's own list  (Engine.rank_targets_per_row, ader_rank_targets_rows)
// (The first form with every row's log-sum-exp and entropy out of the same walk is topk_stats.hip, a translation unit of its own for the
// reason given below; it reaches k_topk_merge through topk_merge_launch.)
// A candidate is one 64-bit key (topk_key.h): order-preserving float bits above, the complemented 1-based item id below, so ONE unsigned
// compare is the total order and no two candidates of a row compare equal.  Key 0 = "no candidate".  (The MFMA chain starts from +0 and
// rounds to nearest, so it never yields -0; topk_key still folds -0 onto +0, as == does.)
// The best k of a set under a total order do not depend on the order the set was visited in: that is the whole determinism argument --
// atomics only hand out slots, the kept SET is the same however they land, and every output is derived from sorted keys.
// This family is a translation unit of its own so that its kernels can call stage_tile and mma_tile<2>: in logits.hip one more caller
// of either changes the code the compiler emits for the f32 training kernels (tools/isa_digest.py).
#include "logit_tile.h"
#include "../../include/ader_hip.h"

#define TOPK_KMAX 64
#define WIDE_KMAX 1024
#define WIDE_CAP 4096   // default and largest list capacity: 32 KB of keys, what k_topk_wide_select sorts in LDS
#define WIDE_GROWTH 32  // a slab is sized to append about (cap - k) / WIDE_GROWTH keys per row of exchangeable items

struct TopkCommon {        // what every launcher of the family fills the same way (topk_fill)
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1) : [N,H]
    int B, Bp, H, N;
    const int* ncol;       // [Bp] N for real rows, 0 for padding rows
    const int* seen;       // [B, seen_ld] 1-based ids never to be returned (0 = none), or NULL
    int seen_ld, k;
};
struct TopkArgs : TopkCommon {
    int ranges;
    u64* part;             // [ranges][Bp][k]
    int* items;            // [B,k]
    float* scores;         // [B,k]
};

// Workgroup = (64-row chunk, contiguous range of 64-item tiles): logit_tile.h's walk, tile stream and row buffer.  A lane proposes
// (row, item) only if the item is a column of the row, is not marked seen, and its key beats the row's threshold.
__global__ __launch_bounds__(512) void k_topk_tile(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    u64* buf = (u64*)(R_l + TB * LDE);                       // [TB][k + 64]
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
    rowbuf_init(thr, cnt, tid);
    if (tid < TB) msk[tid] = 0;
    int nc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) nc[j] = a.ncol[bc * TB + nw * 32 + j * 16 + r16];
    float pre[TILE_STAGE_REGS];
    if (s_begin < s_end) tile_load(pre, a.emb1, s_begin * TI, a.N, H, tid);
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();                                     // the previous tile's MFMA reads, filter and compaction are done
        tile_store(E_l, pre, tid);
        if (a.seen) seen_mask_tile(msk, a.seen, a.seen_ld, a.B, bc * TB, tile0, tid);
        __syncthreads();
        if (s + 1 < s_end) tile_load(pre, a.emb1, tile0 + TI, a.N, H, tid);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il0 = mw * 16 + q * 4, item0 = tile0 + il0;      // this lane's 4 consecutive items
        int over = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16;                  // batch row within the chunk
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
    __syncthreads();
    rowbuf_flush(a.part + ((size_t)range * a.Bp + bc * TB) * k, buf, ldb, cnt, k, tid);
}

// One workgroup per real row: the best k of the row's ranges * k partial keys by the same filter / append / compact over batches of 256
// keys (buffer k + 256), a final compaction that sorts, then unpack.  Key 0 (an empty slot of a range) never beats the threshold.
__global__ __launch_bounds__(256) void k_topk_merge(TopkArgs a) {
    __shared__ u64 mb[TOPK_KMAX + 256];
    __shared__ u64 mthr;
    __shared__ int mcnt;
    const int tid = threadIdx.x, b = blockIdx.x, k = a.k, total = a.ranges * k;
    if (tid == 0) { mthr = 0; mcnt = 0; }
    __syncthreads();
    for (int base = 0; base <= total; base += 256) {                // the pass at base >= total appends nothing: the final, sorting compaction
        const int i = base + tid;
        const bool last = base + 256 > total;
        u64 key = 0;
        if (i < total) { const int rg = i / k; key = a.part[((size_t)rg * a.Bp + b) * k + (i - rg * k)]; }
        int over = 0;
        if (key > mthr) { const int p = atomicAdd(&mcnt, 1); mb[p] = key; over = (p >= k); }
        if (__syncthreads_or(over | last)) {
            const int n = mcnt;                                     // n <= k + 256 <= 320: at most two keys per thread
            const u64 e0 = tid < n ? mb[tid] : 0, e1 = tid + 256 < n ? mb[tid + 256] : 0;
            int r0 = 0, r1 = 0;
            for (int j = 0; j < n; ++j) { const u64 x = mb[j]; r0 += x > e0; r1 += x > e1; }
            __syncthreads();
            if (tid < n && r0 < k) { mb[r0] = e0; if (r0 == k - 1) mthr = e0; }
            if (tid + 256 < n && r1 < k) { mb[r1] = e1; if (r1 == k - 1) mthr = e1; }
            if (tid == 0) mcnt = min(n, k);
            __syncthreads();
        }
        if (last) break;
    }
    const int n = mcnt;
    for (int j = tid; j < k; j += 256) {
        const bool real = j < n;
        a.items[(size_t)b * k + j] = real ? topk_item(mb[j]) : 0;
        a.scores[(size_t)b * k + j] = real ? topk_score(mb[j]) : -INFINITY;
    }
}

// ============================================================================================= the items of a candidate list
// ader_topk_items_cand: ader_topk_items' contract over the items of one strictly ascending id list cand[M] shared by every row, with
// work proportional to M.  k_topk_tile with four differences: tile s is positions [64s, 64s + 64) of the list and its 64 table rows
// are GATHERED into E_l (tile_load_ids); a position can be dead; the seen ids are looked up in the tile's ids; the key carries the
// true item id.  A (row, item) result of the chain does not depend on which items share its tile, so a score is
// k_logits_tile<MODE_STORE>'s float32 and the order, ties included, is ader_topk_items'.  Pipeline per tile s: its rows are written to
// E_l from registers, the rows of tile s + 1 are loaded into registers under the MFMAs, and the ids of tile s + 2 are fetched by wave 0
// (the row addresses depend on the ids, so the ids run one tile ahead of the rows).  The ids of a tile and the mask of its live
// positions sit in LDS, two slots: the loads of tile s + 1 read one slot while the keys and the seen mask of tile s are built from
// the other.
// Position p is live iff p < M, cand[p] >= 1, cand[p] > cand[p-1] and cand[p] <= N; for a row it also needs cand[p] <= ncol[row] and a
// clear seen bit.  A dead position gets a zero operand row and is never proposed: no id outside [1, N] forms an address.  cand[p] < 1
// or cand[p] <= cand[p-1] flags ADER_ST_BAD_CAND: every list that is not strictly ascending is reported, and its result is unspecified
// (two equal keys in a row would break the rank-by-count compaction) but every access stays in bounds -- the row buffer's invariant
// holds for any list.
// Seen ids: the tile's ids are ascending (positions past M hold INT_MAX), so the 8 threads of a row look each seen id up by binary
// search and set the bit of the position it sits at.
struct TopkCandArgs {
    TopkArgs t;            // N: the last item of the table that may be read; ranges, part: over the M positions
    const int* cand;       // [M] strictly ascending 1-based item ids
    int M;
    int* status;           // status word or NULL
};

__global__ __launch_bounds__(512) void k_topk_cand(TopkCandArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const TopkArgs& a = ca.t;
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    u64* buf = (u64*)(R_l + TB * LDE);                       // [TB][k + 64]
    const int k = a.k, ldb = k + TI;
    u64* thr = buf + TB * ldb;                               // [TB]
    u64* msk = thr + TB;                                     // [TB] bit i: the id at position i of the tile is in the row's seen list
    u64* lm = msk + TB;                                      // [2] bit i: position i of the slot's tile is live
    int* cnt = (int*)(lm + 2);                               // [TB]
    int* idl = cnt + TB;                                     // [2][TI] the slot's ids
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    int range, bc, s_begin, s_end;
    if (!tile_walk(a.Bp / TB, a.ranges, (ca.M + TI - 1) / TI, range, bc, s_begin, s_end)) return;
    int nid = 0;                                             // wave 0: the id at position `lane` of the tile fetched last, and that tile's
    u64 nlm = 0;                                             // live mask
    auto fetch_ids = [&](int s) {                            // wave 0 only
        const int p = s * TI + lane;
        int id = 0x7fffffff;
        bool bad = false;
        if (p < ca.M) {
            id = ca.cand[p];
            const int prev = p > 0 ? ca.cand[p - 1] : 0;
            bad = id < 1 || id <= prev;
        }
        const u64 anybad = __ballot(bad);
        if (anybad && lane == 0 && ca.status) atomicOr(ca.status, ADER_ST_BAD_CAND);
        nid = id;
        nlm = __ballot(p < ca.M && !bad && id <= a.N);
    };
    if (wave == 0 && s_begin < s_end) {
        fetch_ids(s_begin);
        idl[(s_begin & 1) * TI + lane] = nid;
        if (lane == 0) lm[s_begin & 1] = nlm;
    }
    stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
    rowbuf_init(thr, cnt, tid);
    if (tid < TB) msk[tid] = 0;
    int nc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) nc[j] = a.ncol[bc * TB + nw * 32 + j * 16 + r16];
    float pre[TILE_STAGE_REGS];
    __syncthreads();                                         // the first tile's ids are in LDS
    if (s_begin < s_end) tile_load_ids(pre, a.emb1, idl + (s_begin & 1) * TI, lm[s_begin & 1], H, tid);
    if (wave == 0 && s_begin + 1 < s_end) fetch_ids(s_begin + 1);
    for (int s = s_begin; s < s_end; ++s) {
        const int cur = s & 1;
        const int* ids = idl + cur * TI;
        __syncthreads();                                     // the previous tile's MFMA reads, filter and compaction are done
        tile_store(E_l, pre, tid);
        if (wave == 0 && s + 1 < s_end) {                    // the other slot's last readers (tile s - 1) are behind the barrier above
            idl[(cur ^ 1) * TI + lane] = nid;
            if (lane == 0) lm[cur ^ 1] = nlm;
        }
        if (a.seen) {                                        // thread (row = tid / 8, part = tid % 8): the 8 lanes of a row are neighbours
            const int row = tid >> 3, b = bc * TB + row;
            const int lo = ids[0], hi = ids[TI - 1];
            u64 m = 0;
            if (b < a.B)
                for (int t = tid & 7; t < a.seen_ld; t += 8) {
                    const int sid = a.seen[(size_t)b * a.seen_ld + t];
                    if (sid < lo || sid > hi) continue;
                    int x = 0;                               // the first position whose id is >= sid: x + h - 1 <= 62, x <= 63
#pragma unroll
                    for (int h = TI / 2; h; h >>= 1)
                        if (ids[x + h - 1] < sid) x += h;
                    if (ids[x] == sid) m |= 1ull << x;
                }
            m |= __shfl_xor(m, 1, 64); m |= __shfl_xor(m, 2, 64); m |= __shfl_xor(m, 4, 64);
            if ((tid & 7) == 0) msk[row] = m;
        }
        __syncthreads();
        if (s + 1 < s_end) tile_load_ids(pre, a.emb1, idl + (cur ^ 1) * TI, lm[cur ^ 1], H, tid);
        if (wave == 0 && s + 2 < s_end) fetch_ids(s + 2);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il0 = mw * 16 + q * 4;                     // this lane's 4 consecutive positions of the tile
        const u64 dead = ~lm[cur];
        int id4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) id4[r] = ids[il0 + r];
        int over = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16;           // batch row within the chunk
            const u64 t = thr[bl];
            const unsigned sm = (unsigned)((msk[bl] | dead) >> il0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                rowbuf_propose(buf, ldb, cnt, k, bl, !((sm >> r) & 1u) && id4[r] <= nc[j], topk_key(acc[j][r], id4[r]), t, over);
        }
        if (__syncthreads_or(over)) rowbuf_compact(buf, ldb, thr, cnt, k, wave, lane);
    }
    __syncthreads();
    rowbuf_flush(a.part + ((size_t)range * a.Bp + bc * TB) * k, buf, ldb, cnt, k, tid);
}

// ============================================================================================= the rank of a target among a candidate list
// ader_rank_targets_cand: k_logits_tile<MODE_RANK>'s count (logits.hip) over k_topk_cand's gathered tile stream.  rank[b] = the number
// of live positions of the list whose id c is a column of row b, is not seen by it, is not its target t, and whose score beats the
// target's: s(b,c) > tl[b], or == with c < t -- the order of the keys above, so rank_targets_cand(b, items[b, j]) == j for what
// ader_topk_items_cand returns over the same list.  tl[b] is k_target_logit's float32 (the same chain on the target's own table row),
// so the target may be absent from the list; listed, it is skipped by id.
// The walk, the id slots two tiles ahead, the gather, the live rule, ADER_ST_BAD_CAND and the seen lookup are k_topk_cand's, restated
// here: lifted into helpers that both call, they change the code emitted for k_topk_cand (tools/isa_digest.py).  What differs is what
// happens to an accumulator: no key, no row buffer, no third barrier, no second launch.  A lane owns two batch rows (j = 0, 1) and 4 positions of every tile, and
// keeps one integer count per row over all tiles of its range; after the last tile the counts of the four lanes that share a row are
// added (__shfl_xor 16, 32) and the wave issues one integer atomicAdd per row with a non-zero count.  Integer adds commute: rank is a
// pure function of the inputs, for any list (a list that is not strictly ascending is flagged, its dead positions count for nothing).
struct RankCandArgs {
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1); N: the last item of the table that may be read
    int B, Bp, H, N;
    const int* target;     // [Bp] 1-based target item
    const int* ncol;       // [Bp] N for real rows, 0 for padding rows
    const int* seen;       // [B, seen_ld] 1-based ids never to be counted (0 = none), or NULL
    int seen_ld, ranges;   // ranges: over the M positions
    const int* cand;       // [M] strictly ascending 1-based item ids
    int M;
    const float* tlogit;   // [Bp] the target's logit (k_target_logit)
    int* rank;             // [Bp] zeroed by the launcher
    int* status;           // status word or NULL
};

__global__ __launch_bounds__(512) void k_rank_cand(RankCandArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [TB][LDE]
    u64* msk = (u64*)(R_l + TB * LDE);                       // [TB] bit i: the id at position i of the tile is in the row's seen list
    u64* lm = msk + TB;                                      // [2] bit i: position i of the slot's tile is live
    int* idl = (int*)(lm + 2);                               // [2][TI] the slot's ids
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mw = wave & 3, nw = wave >> 2;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int r16 = lane & 15, q = lane >> 4;
    int range, bc, s_begin, s_end;
    if (!tile_walk(a.Bp / TB, a.ranges, (a.M + TI - 1) / TI, range, bc, s_begin, s_end)) return;
    if (s_begin >= s_end) return;                            // an empty range counts nothing
    int nid = 0;                                             // wave 0: the id at position `lane` of the tile fetched last, and that tile's
    u64 nlm = 0;                                             // live mask
    auto fetch_ids = [&](int s) {                            // wave 0 only
        const int p = s * TI + lane;
        int id = 0x7fffffff;
        bool bad = false;
        if (p < a.M) {
            id = a.cand[p];
            const int prev = p > 0 ? a.cand[p - 1] : 0;
            bad = id < 1 || id <= prev;
        }
        const u64 anybad = __ballot(bad);
        if (anybad && lane == 0 && a.status) atomicOr(a.status, ADER_ST_BAD_CAND);
        nid = id;
        nlm = __ballot(p < a.M && !bad && id <= a.N);
    };
    if (wave == 0) {
        fetch_ids(s_begin);
        idl[(s_begin & 1) * TI + lane] = nid;
        if (lane == 0) lm[s_begin & 1] = nlm;
    }
    stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
    if (tid < TB) msk[tid] = 0;
    int nc[2], tg[2], cnt[2];
    float tl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int b = bc * TB + nw * 32 + j * 16 + r16;      // b < Bp: ncol, target and tlogit hold Bp entries
        nc[j] = a.ncol[b]; tg[j] = a.target[b]; tl[j] = a.tlogit[b]; cnt[j] = 0;
    }
    float pre[TILE_STAGE_REGS];
    __syncthreads();                                         // the first tile's ids are in LDS
    tile_load_ids(pre, a.emb1, idl + (s_begin & 1) * TI, lm[s_begin & 1], H, tid);
    if (wave == 0 && s_begin + 1 < s_end) fetch_ids(s_begin + 1);
    for (int s = s_begin; s < s_end; ++s) {
        const int cur = s & 1;
        const int* ids = idl + cur * TI;
        __syncthreads();                                     // the previous tile's MFMA reads and its reads of msk, lm and the ids are done
        tile_store(E_l, pre, tid);
        if (wave == 0 && s + 1 < s_end) {                    // the other slot's last readers (tile s - 1) are behind the barrier above
            idl[(cur ^ 1) * TI + lane] = nid;
            if (lane == 0) lm[cur ^ 1] = nlm;
        }
        if (a.seen) {                                        // thread (row = tid / 8, part = tid % 8): the 8 lanes of a row are neighbours
            const int row = tid >> 3, b = bc * TB + row;
            const int lo = ids[0], hi = ids[TI - 1];
            u64 m = 0;
            if (b < a.B)
                for (int t = tid & 7; t < a.seen_ld; t += 8) {
                    const int sid = a.seen[(size_t)b * a.seen_ld + t];
                    if (sid < lo || sid > hi) continue;
                    int x = 0;                               // the first position whose id is >= sid: x + h - 1 <= 62, x <= 63
#pragma unroll
                    for (int h = TI / 2; h; h >>= 1)
                        if (ids[x + h - 1] < sid) x += h;
                    if (ids[x] == sid) m |= 1ull << x;
                }
            m |= __shfl_xor(m, 1, 64); m |= __shfl_xor(m, 2, 64); m |= __shfl_xor(m, 4, 64);
            if ((tid & 7) == 0) msk[row] = m;
        }
        __syncthreads();
        if (s + 1 < s_end) tile_load_ids(pre, a.emb1, idl + (cur ^ 1) * TI, lm[cur ^ 1], H, tid);
        if (wave == 0 && s + 2 < s_end) fetch_ids(s + 2);
        f32x4 acc[2];
        acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane);
        const int il0 = mw * 16 + q * 4;                     // this lane's 4 consecutive positions of the tile
        const u64 dead = ~lm[cur];
        int id4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) id4[r] = ids[il0 + r];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int bl = nw * 32 + j * 16 + r16;           // batch row within the chunk
            const unsigned sm = (unsigned)((msk[bl] | dead) >> il0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // the target never counts itself, listed or not, seen or not (MODE_RANK's rule)
                const bool in = !((sm >> r) & 1u) && id4[r] <= nc[j] && id4[r] != tg[j];
                cnt[j] += in && ((acc[j][r] > tl[j]) || (acc[j][r] == tl[j] && id4[r] < tg[j]));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int c = cnt[j];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if (q == 0 && c) atomicAdd(a.rank + bc * TB + nw * 32 + j * 16 + r16, c);
    }
}

// ============================================================================================= every row's own item list
// ader_score_items / ader_topk_items_rows / ader_rank_targets_rows: the list differs from row to row -- ids [B, ld], C positions per row
// (the input of a re-ranking stage, the sampled negatives of an evaluation, a per-user eligibility set) -- so nothing of a tile is
// shared between rows and the work is n * C gathered table rows.  Workgroup = (row b, 64 positions of its list), 256 threads:
//   wave 0      the tile's 64 ids -> idl, the mask of its live positions -> lm[0] (a dead position's id forms no address);
//   all         the row's rep -> R_l [LDE] and its seen ids -> sl, then the 64 table rows gathered into E_l [64][LDE] as tile_load_ids
//               does, a dead position's row zero; meanwhile wave 1 scans sl for the id of position `lane` -> lm[1];
//   wave w      mma_tile<1> over positions 16w .. 16w + 15 with a column stride of 0: the one rep row is broadcast to all 16 MFMA columns,
//               and the lanes with (lane & 15) == 0 hold acc[0][r] = the score of position 16w + 4 (lane >> 4) + r.
// The matrix unit is 1/16 used: the kernel is a gather of 4H bytes per pair.  The operands of a pair, their k order and ksteps are the
// tile kernels', and a pair's chain does not depend on what else its tile holds: a score is k_logits_tile<MODE_STORE>'s float32.
//   ROWLIST_STORE   scores[b, p] = the score, -inf at a dead position: id <= 0, id > N or id > ncol[b].  Any order, duplicates allowed: a
//                   position's result depends on that position alone.
//   ROWLIST_KEYS    topk_key(score, id) of every live, unseen position p -> part[p / k][b][p % k], key 0 elsewhere up to ranges * k:
//                   k_topk_merge's input, ranges = ceil(C / k), and its output is ader_topk_items_cand's over the row's own list.
//   ROWLIST_RANK    k_rank_cand's count over the row's list against tl[b] = k_target_logit's float32, one integer atomicAdd per wave.
// KEYS and RANK take every row's list as strictly ascending ids >= 1 followed by 0 padding (ragged lists share one ld): a position with
// id < 0, or p > 0 and id > 0 and (ids[b, p-1] == 0 or id <= ids[b, p-1]), flags ADER_ST_BAD_CAND and is dead; the result is then
// unspecified (two equal keys would break k_topk_merge's rank-by-count) but every access stays in bounds, whatever the list.
enum { ROWLIST_STORE = 0, ROWLIST_KEYS = 1, ROWLIST_RANK = 2 };
#define ROWLIST_STAGE_REGS ((TI * LDE + 255) / 256)
struct RowlistArgs {
    const float* rep;      // [B,H]
    const float* emb1;     // table row 1 (item 1); N: the last item of the table that may be read
    int B, Bp, H, N;
    const int* ncol;       // [B] columns of the row, or NULL: N
    const int* ids;        // [B, ld] 1-based item ids, C positions per row
    int ld, C, ntile;      // ntile: 64-position tiles per row
    const int* seen;       // [B, seen_ld] 1-based ids never to be returned or counted (0 = none), or NULL     (KEYS, RANK)
    int seen_ld;
    float* scores;         // [B, ld_scores]                                   (STORE)
    int ld_scores;
    u64* part;             // [ranges][Bp][k]                                  (KEYS)
    int k, ranges;
    const int* target;     // [Bp] 1-based target item                         (RANK)
    const float* tlogit;   // [Bp] the target's logit (k_target_logit)
    int* rank;             // [Bp] zeroed by the launcher
    int* status;           // status word or NULL
};

template <int MODE>
__global__ __launch_bounds__(256) void k_rowlist(RowlistArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                       // [TI][LDE]
    float* R_l = E_l + TI * LDE;                             // [LDE]
    u64* lm = (u64*)(R_l + LDE);                             // [0] bit i: position i of the tile is live, [1] its id is seen by the row
    int* idl = (int*)(lm + 2);                               // [TI] the tile's ids
    int* sl = idl + TI;                                      // [seen_ld] the row's seen ids
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, ksteps = (H + 3) >> 2;
    const int b = blockIdx.x / a.ntile, p0 = (blockIdx.x - b * a.ntile) * TI;      // b < B: the grid is B * ntile
    const int* row = a.ids + (size_t)b * a.ld;
    if (wave == 0) {
        const int p = p0 + lane;
        int id = 0, nc = a.N;
        bool bad = false;
        if (p < a.C) {
            id = row[p];
            if (a.ncol) nc = min(nc, a.ncol[b]);
            if (MODE != ROWLIST_STORE) {
                const int prev = p > 0 ? row[p - 1] : 0;
                bad = id < 0 || (p > 0 && id > 0 && (prev == 0 || id <= prev));
            }
        }
        if (MODE != ROWLIST_STORE) {
            const u64 anybad = __ballot(bad);
            if (anybad && lane == 0 && a.status) atomicOr(a.status, ADER_ST_BAD_CAND);
        }
        const u64 live = __ballot(id >= 1 && id <= nc && !bad);
        idl[lane] = id;
        if (lane == 0) { lm[0] = live; lm[1] = 0; }
    }
    for (int i = tid; i < LDE; i += 256) R_l[i] = i < H ? a.rep[(size_t)b * H + i] : 0.0f;
    if (MODE != ROWLIST_STORE && a.seen)
        for (int i = tid; i < a.seen_ld; i += 256) sl[i] = a.seen[(size_t)b * a.seen_ld + i];
    __syncthreads();                                         // ids, live mask, rep row and seen ids are in LDS
    const u64 live = lm[0];
    float pre[ROWLIST_STAGE_REGS];                           // tile_load_ids for 256 threads: every load of the gather is in flight at once
#pragma unroll
    for (int n = 0; n < ROWLIST_STAGE_REGS; ++n) {
        const int i = tid + n * 256, r = (i / LDE) & (TI - 1), c = i - (i / LDE) * LDE;
        const bool ok = i < TI * LDE && c < H && ((live >> r) & 1ull);
        pre[n] = ok ? a.emb1[(size_t)(idl[r] - 1) * H + c] : 0.0f;
    }
    if (MODE != ROWLIST_STORE && a.seen && wave == 1) {
        const int id = idl[lane];
        bool s = false;
        for (int t = 0; t < a.seen_ld; ++t) s |= sl[t] == id;      // (id 0 matches a padding 0 of seq: the position is dead anyway)
        const u64 sm = __ballot(s);
        if (lane == 0) lm[1] = sm;
    }
#pragma unroll
    for (int n = 0; n < ROWLIST_STAGE_REGS; ++n)
        if (tid + n * 256 < TI * LDE) E_l[tid + n * 256] = pre[n];
    __syncthreads();                                         // E_l and the seen mask are complete
    f32x4 acc[1];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mma_tile<1>(E_l + wave * 16 * LDE, LDE, 1, R_l, 1, 0, ksteps, acc, lane);
    const int q = lane >> 4, il0 = wave * 16 + q * 4;        // the 4 positions of the tile a lane with (lane & 15) == 0 holds
    const bool owner = (lane & 15) == 0;
    if (MODE == ROWLIST_STORE) {
        if (owner)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (p0 + il0 + r < a.C) a.scores[(size_t)b * a.ld_scores + p0 + il0 + r] = ((live >> (il0 + r)) & 1ull) ? acc[0][r] : -INFINITY;
    } else if (MODE == ROWLIST_KEYS) {
        const u64 in = live & ~lm[1];
        if (owner)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = p0 + il0 + r;
                if (p >= a.ranges * a.k) continue;
                const int rg = p / a.k;
                a.part[((size_t)rg * a.Bp + b) * a.k + (p - rg * a.k)] = ((in >> (il0 + r)) & 1ull) ? topk_key(acc[0][r], idl[il0 + r]) : 0;
            }
    } else {
        const u64 in = live & ~lm[1];
        const int tg = a.target[b];
        const float tl = a.tlogit[b];
        int c = 0;
        if (owner)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = idl[il0 + r];
                // the target never counts itself, listed or not, seen or not (MODE_RANK's rule)
                const bool ok = ((in >> (il0 + r)) & 1ull) && id != tg;
                c += ok && ((acc[0][r] > tl) || (acc[0][r] == tl && id < tg));
            }
        c += __shfl_xor(c, 16, 64);                          // (the other lanes hold 0)
        c += __shfl_xor(c, 32, 64);
        if (lane == 0 && c) atomicAdd(a.rank + b, c);
    }
}

// ============================================================================================= wide answers, k up to 1024: slab and select
// k_topk_tile keeps k + 64 keys per row in LDS, which ends at k = 64; here no buffer in LDS grows with k.
// Per row, in global memory: a list of cap 64-bit keys, a count, a threshold key (0 = none yet) and a status word.  The catalog is
// walked in slabs of 64-item tiles (ader_topk_wide_slabs, a pure host function of (N, k, cap)):
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
// that passes is stored, and the select keeps the best k of what is stored -- k_topk_tile's argument without its in-kernel
// compaction.  A key whose slot would be >= cap is dropped and the row's status word is set: a flagged row's output is unspecified,
// and the caller recomputes it.  Nothing outside [0, cap) of a row's list is ever written.
struct WideArgs : TopkCommon {
    int cap;
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

// Workgroup = (64-row chunk, contiguous run of the slab's tiles): logit_tile.h's walk over the slab's tiles and its tile stream.
//   filter    a lane proposes (row, item) when the item is a column of the row, is not in the row's seen mask and its key beats the row's
//             threshold, read once per workgroup: it does not change during a launch;
//   reserve   slots per (workgroup, tile, row): an LDS atomic per proposal counts the tile's proposals of the row and gives the key its
//             local position, then one thread per row does ONE returning global atomicAdd on the row's count (a global atomic per key
//             would serialise on one word, and slab 0 appends everything);
//   store     key -> list[row][base + local position] if that is < cap, else the row is flagged with a plain store.
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
    int run, bc, s_begin, s_end;
    if (!tile_walk(a.Bp / TB, a.runs, a.s_end - a.s_begin, run, bc, s_begin, s_end)) return;
    s_begin += a.s_begin; s_end += a.s_begin;
    if (s_begin >= s_end) return;
    stage_tile(R_l, a.rep, bc * TB, a.B, H, tid, 512);
    if (tid < TB) { thr[tid] = a.thr[bc * TB + tid]; msk[tid] = 0; }
    int nc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int b = bc * TB + nw * 32 + j * 16 + r16;
        nc[j] = b < a.B ? a.ncol[b] : 0;
    }
    float pre[TILE_STAGE_REGS];
    tile_load(pre, a.emb1, s_begin * TI, a.N, H, tid);
    for (int s = s_begin; s < s_end; ++s) {
        const int tile0 = s * TI;
        __syncthreads();                                     // the previous tile's MFMA reads and its reads of base[] are done
        tile_store(E_l, pre, tid);
        if (tid < TB) tcnt[tid] = 0;
        if (a.seen) {                                        // seen_mask_tile (logit_tile.h), written out: through the call this kernel
            const int row = tid >> 3, b = bc * TB + row;     // measured 1 - 2 % slower (profiles/topk_refactor.txt)
            u64 m = 0;
            if (b < a.B)
                for (int t = tid & 7; t < a.seen_ld; t += 8) {
                    const unsigned d = (unsigned)(a.seen[(size_t)b * a.seen_ld + t] - 1 - tile0);
                    if (d < 64u) m |= 1ull << d;
                }
            m |= __shfl_xor(m, 1, 64); m |= __shfl_xor(m, 2, 64); m |= __shfl_xor(m, 4, 64);
            if ((tid & 7) == 0) msk[row] = m;
        }
        __syncthreads();
        if (s + 1 < s_end) tile_load(pre, a.emb1, tile0 + TI, a.N, H, tid);
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

// ============================================================================================= C ABI
// the arguments every launcher shares: -2's conditions, the common fields, and the LDS of two operand tiles plus the kernel's own tail
static bool topk_bad(int B, int Bp, int H, int N, const int* seen, int seen_ld, int k, int kmax) {
    return k < 1 || k > kmax || Bp % TB != 0 || Bp > MAXB || B > Bp || H > HP || H < 1 || N < 1 || (seen && seen_ld < 1);
}
static void topk_fill(TopkCommon& a, const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* seen,
                      int seen_ld, int k) {
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ncol = ncol; a.seen = seen; a.seen_ld = seen_ld; a.k = k;
}
static size_t tile_lds(size_t tail) { return (size_t)(2 * 64 * LDE) * sizeof(float) + tail; }
#define ROWLIST_SEEN_MAX 4096     // seen ids per row that k_rowlist stages in LDS (a session's length)
#define ROWLIST_CMAX 65536        // list positions per row
static size_t rowlist_lds(int seen_ld) {      // E_l, R_l, lm, idl, sl
    return (size_t)(TI * LDE + LDE) * sizeof(float) + 2 * sizeof(u64) + (size_t)(TI + seen_ld) * sizeof(int);
}
static bool rowlist_bad(const int* ids, int ld, int C, const int* seen, int seen_ld) {
    return C < 0 || C > ROWLIST_CMAX || ld < C || (C > 0 && !ids) || (seen && seen_ld > ROWLIST_SEEN_MAX);
}
static size_t rowbuf_lds(int k) { return (size_t)TB * (k + TI) * sizeof(u64) + TB * (2 * sizeof(u64) + sizeof(int)); }      // buf, thr, msk, cnt

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

// in logits.hip: the exact-f32 logit of every row's target (k_target_logit), what ader_rank_targets compares against
int rank_target_logit_launch(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                             float* tlogit, void* stream);

// for topk_stats.hip, whose tile kernel fills `part` as k_topk_tile does: k_topk_merge over part [ranges][Bp][k] -> items / scores
// [B,k], the second launch of ader_topk_items (host code only: the kernels of this file are as they were, tools/isa_digest.py)
int topk_merge_launch(int B, int Bp, int k, int ranges, unsigned long long* part, int* items, float* scores, void* stream) {
    if (k < 1 || k > TOPK_KMAX || ranges < 1 || B > Bp) return -2;
    if (B <= 0) return 0;
    TopkArgs a = {};
    a.B = B; a.Bp = Bp; a.k = k; a.ranges = ranges; a.part = part; a.items = items; a.scores = scores;
    hipLaunchKernelGGL(k_topk_merge, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

// ader_topk_ranges: item ranges per 64-row chunk -- about one workgroup per CU over the Bp/64 chunks, a multiple of 8 (the block ->
// (range, chunk) mapping), so it may exceed the number of 64-item tiles: such ranges are empty.
int ader_topk_kmax(void) { return TOPK_KMAX; }
int ader_topk_ranges(int N, int Bp) {
    const int nsub = (N + TI - 1) / TI;
    const int nchunk = Bp / TB > 0 ? Bp / TB : 1;
    int target = 256 / nchunk / 8 * 8;
    if (target < 8) target = 8;
    int r = (nsub + 7) / 8 * 8;
    if (r > target) r = target;
    if (r < 8) r = 8;
    return r;
}
// items / scores [B,k]: the first k of items 1..N (minus the non-zero ids of seen[b, 0:seen_ld], if seen) by (score descending, id
// ascending); fewer than k candidates: the tail is item 0, score -inf.  ncol: [Bp] = N for real rows, 0 for padding; seen: [B, seen_ld]
// or NULL; part: ader_topk_ranges(N,Bp) * Bp * k keys of scratch.  Enqueue only.
int ader_topk_items(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* seen, int seen_ld,
                    int k, unsigned long long* part, int* items, float* scores, void* stream) {
    if (topk_bad(B, Bp, H, N, seen, seen_ld, k, TOPK_KMAX)) return -2;
    if (B <= 0) return 0;
    TopkArgs a;
    topk_fill(a, rep, emb, B, Bp, H, N, ncol, seen, seen_ld, k);
    a.ranges = ader_topk_ranges(N, Bp); a.part = part; a.items = items; a.scores = scores;
    const size_t lds = tile_lds(rowbuf_lds(k));
    const int rc = ader_dyn_lds<k_topk_tile>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_topk_tile, dim3(a.ranges * (Bp / TB)), dim3(512), lds, st, a);
    hipLaunchKernelGGL(k_topk_merge, dim3(B), dim3(256), 0, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}
// ader_topk_items over the items of cand[0:M] only: a strictly ascending list of 1-based ids, shared by every row; ids above N are
// ignored, as seen ids above N are.  N: no table row beyond item N is read.  M = 0: every row is padding (cand may be NULL).
// part: ader_topk_ranges(M,Bp) * Bp * k keys of scratch.  status (NULL: none): ADER_ST_BAD_CAND is OR-ed in when the list is not
// strictly ascending or holds an id < 1; the result is then unspecified, and nothing outside the table is read.  Enqueue only.
int ader_topk_items_cand(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* cand, int M,
                         const int* seen, int seen_ld, int k, unsigned long long* part, int* items, float* scores, int* status,
                         void* stream) {
    if (topk_bad(B, Bp, H, N, seen, seen_ld, k, TOPK_KMAX) || M < 0 || (M > 0 && !cand)) return -2;
    if (B <= 0) return 0;
    TopkCandArgs ca;
    TopkArgs& a = ca.t;
    topk_fill(a, rep, emb, B, Bp, H, N, ncol, seen, seen_ld, k);
    a.ranges = ader_topk_ranges(M, Bp); a.part = part; a.items = items; a.scores = scores;
    ca.cand = cand; ca.M = M; ca.status = status;
    const size_t lds = tile_lds(rowbuf_lds(k) + 2 * sizeof(u64) + 2 * TI * sizeof(int));      // + lm, idl
    const int rc = ader_dyn_lds<k_topk_cand>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_topk_cand, dim3(a.ranges * (Bp / TB)), dim3(512), lds, st, ca);
    hipLaunchKernelGGL(k_topk_merge, dim3(B), dim3(256), 0, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}
// rank[b] = #{c in cand[0:M] : 1 <= c <= min(N, ncol[b]), c != t, c not in seen[b], s(b,c) > s(b,t) or (== and c < t)}, t = target[b]:
// ader_rank_targets' count over ader_topk_items_cand's list (same cand, M, N, seen, status and -2 conditions).  tlogit: Bp floats of
// scratch; rank: [Bp] (zeroed here).  M = 0: the clear of rank and nothing else.  Enqueue only.
int ader_rank_targets_cand(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                           const int* cand, int M, const int* seen, int seen_ld, float* tlogit, int* rank, int* status, void* stream) {
    if (topk_bad(B, Bp, H, N, seen, seen_ld, 1, 1) || M < 0 || (M > 0 && !cand)) return -2;
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(rank, 0, sizeof(int) * (size_t)Bp, st);
    if (e != hipSuccess) return (int)e;
    if (M == 0) return 0;
    const size_t lds = tile_lds(TB * sizeof(u64) + 2 * sizeof(u64) + 2 * TI * sizeof(int));      // msk, lm, idl
    int rc = ader_dyn_lds<k_rank_cand>(lds);
    if (rc) return rc;
    rc = rank_target_logit_launch(rep, emb, B, Bp, H, N, target, ncol, tlogit, stream);
    if (rc) return rc;
    RankCandArgs a;
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.target = target; a.ncol = ncol; a.seen = seen;
    a.seen_ld = seen_ld; a.ranges = ader_topk_ranges(M, Bp); a.cand = cand; a.M = M; a.tlogit = tlogit; a.rank = rank; a.status = status;
    hipLaunchKernelGGL(k_rank_cand, dim3(a.ranges * (Bp / TB)), dim3(512), lds, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

// scores[b, p] (row stride ld_scores >= C) = the logit of item ids[b, p] (row stride ld >= C) for row b, the float32 of
// ader_logits_store; -inf where the id is outside [1, min(N, ncol[b])].  ncol: [B], or NULL: N for every row.  Any ids, in any order.
// C = 0 or B <= 0: nothing is launched.  Enqueue only.
int ader_score_items(const float* rep, const float* emb, int B, int H, int N, const int* ncol, const int* ids, int ld, int C,
                     float* scores, int ld_scores, void* stream) {
    if (H > HP || H < 1 || N < 1 || C < 0 || ld < C || ld_scores < C || (C > 0 && !ids)) return -2;
    if (B <= 0 || C == 0) return 0;
    RowlistArgs a = {};
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = B; a.H = H; a.N = N; a.ncol = ncol; a.ids = ids; a.ld = ld; a.C = C;
    a.ntile = (C + TI - 1) / TI; a.scores = scores; a.ld_scores = ld_scores;
    if ((long)B * a.ntile > 0x7fffffffL) return -2;
    const size_t lds = rowlist_lds(0);
    const int rc = ader_dyn_lds<k_rowlist<ROWLIST_STORE>>(lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rowlist<ROWLIST_STORE>, dim3(B * a.ntile), dim3(256), lds, (hipStream_t)stream, a);
    HIP_LAUNCH_CHECK();
    return 0;
}
// ader_topk_items_cand with a list per row: ids [B, ld], C positions per row, every row strictly ascending ids >= 1 followed by 0
// padding; ids above N (or ncol[b]) are ignored.  part: ader_topk_rows_ranges(C,k) * Bp * k keys of scratch.  C = 0: every row is
// padding (ids may be NULL).  status (NULL: none): ADER_ST_BAD_CAND is OR-ed in for a row that is not in that form; the result is then
// unspecified, and nothing outside the table or the buffers is touched.  seen_ld <= ROWLIST_SEEN_MAX.  Enqueue only.
int ader_topk_rows_ranges(int C, int k) { return (C > 0 && k > 0) ? (C + k - 1) / k : 1; }
int ader_topk_items_rows(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* ids, int ld, int C,
                         const int* seen, int seen_ld, int k, unsigned long long* part, int* items, float* scores, int* status,
                         void* stream) {
    if (topk_bad(B, Bp, H, N, seen, seen_ld, k, TOPK_KMAX) || rowlist_bad(ids, ld, C, seen, seen_ld)) return -2;
    if (B <= 0) return 0;
    TopkArgs t;
    topk_fill(t, rep, emb, B, Bp, H, N, ncol, seen, seen_ld, k);
    t.ranges = ader_topk_rows_ranges(C, k); t.part = part; t.items = items; t.scores = scores;
    RowlistArgs a = {};
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ncol = ncol; a.ids = ids; a.ld = ld; a.C = C;
    a.ntile = (t.ranges * k + TI - 1) / TI;                  // every slot of part is written: ranges * k >= C
    a.seen = seen; a.seen_ld = seen_ld; a.part = part; a.k = k; a.ranges = t.ranges; a.status = status;
    const size_t lds = rowlist_lds(seen ? seen_ld : 0);
    const int rc = ader_dyn_lds<k_rowlist<ROWLIST_KEYS>>(lds);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rowlist<ROWLIST_KEYS>, dim3(B * a.ntile), dim3(256), lds, st, a);
    hipLaunchKernelGGL(k_topk_merge, dim3(B), dim3(256), 0, st, t);
    HIP_LAUNCH_CHECK();
    return 0;
}
// ader_rank_targets_cand with a list per row (ids, ld, C, seen, status and -2 as ader_topk_items_rows): rank[b] = the number of
// positions of row b's list whose id c is live, not seen, != t = target[b], and s(b,c) > s(b,t) or (== and c < t) -- so the rank of
// ader_topk_items_rows' items[b, j] > 0 over the same arguments is j.  tlogit: Bp floats of scratch; rank: [Bp] (zeroed here).
// C = 0: the clear of rank and nothing else.  Enqueue only.
int ader_rank_targets_rows(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                           const int* ids, int ld, int C, const int* seen, int seen_ld, float* tlogit, int* rank, int* status,
                           void* stream) {
    if (topk_bad(B, Bp, H, N, seen, seen_ld, 1, 1) || rowlist_bad(ids, ld, C, seen, seen_ld)) return -2;
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(rank, 0, sizeof(int) * (size_t)Bp, st);
    if (e != hipSuccess) return (int)e;
    if (C == 0) return 0;
    const size_t lds = rowlist_lds(seen ? seen_ld : 0);
    int rc = ader_dyn_lds<k_rowlist<ROWLIST_RANK>>(lds);
    if (rc) return rc;
    rc = rank_target_logit_launch(rep, emb, B, Bp, H, N, target, ncol, tlogit, stream);
    if (rc) return rc;
    RowlistArgs a = {};
    a.rep = rep; a.emb1 = emb + H; a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ncol = ncol; a.ids = ids; a.ld = ld; a.C = C;
    a.ntile = (C + TI - 1) / TI; a.seen = seen; a.seen_ld = seen_ld; a.target = target; a.tlogit = tlogit; a.rank = rank; a.status = status;
    hipLaunchKernelGGL(k_rowlist<ROWLIST_RANK>, dim3(B * a.ntile), dim3(256), lds, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

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

// ader_topk_items' contract for 1 <= k <= 1024 by slab and select.  list: Bp * cap 64-bit keys; cnt, row_status: [Bp] ints; thr: [Bp]
// 64-bit keys; diag: [2] ints -- all zeroed here.  Afterwards row_status[b] != 0 marks a row whose list overflowed: its items / scores
// are unspecified.  diag[0] = the largest list length a select after slab 0 met (above cap: that row overflowed), diag[1] = rows with
// row_status != 0.  Enqueue only: 2 * ader_topk_wide_slabs(N, k, cap) launches.
int ader_topk_items_wide(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* ncol, const int* seen, int seen_ld,
                         int k, int cap, unsigned long long* list, int* cnt, unsigned long long* thr, int* row_status, int* diag,
                         int* items, float* scores, void* stream) {
    if (Bp < 0 || topk_bad(B, Bp, H, N, seen, seen_ld, k, WIDE_KMAX) || wide_bad(N, k, cap)) return -2;
    if (B <= 0) return 0;
    WideArgs a;
    topk_fill(a, rep, emb, B, Bp, H, N, ncol, seen, seen_ld, k);
    a.cap = cap; a.list = list; a.cnt = cnt; a.thr = thr; a.row_status = row_status; a.diag = diag; a.items = items; a.scores = scores;
    const size_t lds = tile_lds(TB * (2 * sizeof(u64) + 2 * sizeof(int)));      // thr, msk, tcnt, base
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
