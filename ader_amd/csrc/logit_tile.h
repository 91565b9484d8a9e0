// What the exact-f32 logit-tile kernels share (logits.hip, topk.hip): a 64-item x 64-row logit tile on v_mfma_f32_16x16x4_f32 from two
// [64][LDE] operand tiles in LDS, by mma_tile<2>(E_l + mw * 16 * LDE, LDE, 1, R_l + nw * 32 * LDE, 1, LDE, ksteps, acc, lane).  The
// score of a (row, item) pair is that chain's float32 and depends on nothing else in the tile, so every kernel that fills the operands
// through the pieces below computes k_logits_tile<MODE_STORE>'s bits.
#pragma once
#include "common.h"
#include "topk_key.h"

#ifndef HP
#define HP 160          // (lbf_common.h states the same value)
#endif
#define LDE 162         // (row, k) operand reads conflict-free
#define TI 64           // items per tile
#define TB 64           // batch rows per chunk
#define MAXB 1024       // max (padded) batch rows per launch

__device__ __forceinline__ void stage_tile(float* dst, const float* src, int row0, int nrows, int H, int tid, int nthreads) {
    // dst[r][c] = src[(row0+r)*H + c] for row0+r < nrows, c < H; zeros elsewhere.  [64][LDE]
    for (int i = tid; i < 64 * LDE; i += nthreads) {
        const int r = i / LDE, c = i - r * LDE;
        dst[i] = (row0 + r < nrows && c < H) ? src[(size_t)(row0 + r) * H + c] : 0.0f;
    }
}

// ---------------------------------------------------------------- the (range, chunk) walk
// Workgroup = (64-row chunk bc, contiguous range of 64-item tiles [s_begin, s_end)): the floor partition of ntile tiles into `ranges`
// ranges, so a range may be empty.  Block -> (range, chunk) keeps the chunks that stream the same range on one XCD (blocks b and b + 8
// share an XCD), hence on the L2 that holds the range's table tiles: speed only, not correctness.  false: the block has no range.
__device__ __forceinline__ bool tile_walk(int nchunk, int ranges, int ntile, int& range, int& bc, int& s_begin, int& s_end) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    range = xcd + 8 * (slot / nchunk); bc = slot % nchunk;
    s_begin = (int)((long)range * ntile / ranges); s_end = (int)((long)(range + 1) * ntile / ranges);
    return range < ranges;
}

// ---------------------------------------------------------------- the tile stream (512 threads)
// The chunk's rep rows are staged once (stage_tile); the range's table tiles stream through E_l, tile s + 1 held in registers, in
// stage_tile's element order, while tile s is multiplied.  Per tile, in this order:
//   barrier 1    the previous tile's MFMA reads of E_l, and whatever else the kernel read from per-tile LDS state, are done;
//   tile_store   pre[] -> E_l (and the kernel's per-tile LDS state: seen mask, counters, the other id slot);
//   barrier 2    E_l is complete;
//   tile_load*   tile s + 1 -> pre[]: issued behind barrier 2 so that the loads are in flight under the MFMAs, and pre[] is free
//                because tile_store has read it;
//   mma_tile<2>.
#define TILE_STAGE_REGS ((64 * LDE + 511) / 512)

// pre <- the 64 consecutive table rows from item row tile0 (rows >= N and columns >= H: zeros)
__device__ __forceinline__ void tile_load(float (&pre)[TILE_STAGE_REGS], const float* emb1, int tile0, int N, int H, int tid) {
#pragma unroll
    for (int n = 0; n < TILE_STAGE_REGS; ++n) {
        const int i = tid + n * 512, r = i / LDE, c = i - r * LDE;
        pre[n] = (i < 64 * LDE && tile0 + r < N && c < H) ? emb1[(size_t)(tile0 + r) * H + c] : 0.0f;
    }
}
// pre <- the table rows of the 64 1-based ids in ids[], gathered; a position whose bit of `live` is clear gets a zero row and its id
// forms no address (consecutive threads still cover consecutive floats of one table row)
__device__ __forceinline__ void tile_load_ids(float (&pre)[TILE_STAGE_REGS], const float* emb1, const int* ids, u64 live, int H, int tid) {
#pragma unroll
    for (int n = 0; n < TILE_STAGE_REGS; ++n) {
        const int i = tid + n * 512, r = (i / LDE) & (TI - 1), c = i - (i / LDE) * LDE;
        const bool ok = i < 64 * LDE && c < H && ((live >> r) & 1ull);
        pre[n] = ok ? emb1[(size_t)(ids[r] - 1) * H + c] : 0.0f;
    }
}
__device__ __forceinline__ void tile_store(float* E_l, const float (&pre)[TILE_STAGE_REGS], int tid) {
#pragma unroll
    for (int n = 0; n < TILE_STAGE_REGS; ++n)
        if (tid + n * 512 < 64 * LDE) E_l[tid + n * 512] = pre[n];
}

// ---------------------------------------------------------------- seen ids of a tile of consecutive items
// msk[row] bit i <- item tile0 + i + 1 is among seen[b, 0:seen_ld], b = row0 + row: per tile, 8 threads per row fold the row's ids that
// fall into the tile into a 64-bit mask (no over-selection, no second pass).  Written between the tile's two barriers.
__device__ __forceinline__ void seen_mask_tile(u64* msk, const int* seen, int seen_ld, int B, int row0, int tile0, int tid) {
    const int row = tid >> 3, b = row0 + row;                // thread (row = tid / 8, part = tid % 8): the 8 lanes of a row are neighbours
    u64 m = 0;
    if (b < B)
        for (int t = tid & 7; t < seen_ld; t += 8) {
            const unsigned d = (unsigned)(seen[(size_t)b * seen_ld + t] - 1 - tile0);      // id 0 -> d wraps: never < 64
            if (d < 64u) m |= 1ull << d;
        }
    m |= __shfl_xor(m, 1, 64); m |= __shfl_xor(m, 2, 64); m |= __shfl_xor(m, 4, 64);
    if ((tid & 7) == 0) msk[row] = m;
}

// ---------------------------------------------------------------- the row buffer of the LDS top-K
// Per batch row of the chunk a candidate buffer buf[row][0 : ldb], ldb = k + 64 keys (topk_key.h), its fill cnt[row] and thr[row], the
// row's k-th best key at its last compaction (0 before the first):
//   propose  a key that the caller's filter lets through and that beats thr[row] goes to buf[row][cnt[row]++] (LDS atomic: hands out
//            the slot, nothing else);
//   compact  a row holding more than k keys is cut to its best k, sorted, and thr[row] <- its k-th.  Workgroup-uniform, decided by one
//            __syncthreads_or per tile over propose's `over` flags;
//   flush    behind a barrier after the last tile: the row's keys, zero padded to k, to the (range, chunk) block of `part`.
// INVARIANT: every row enters a tile with cnt <= k, a 64-position tile proposes at most 64 keys per row, and every row with cnt > k is
// compacted before the next tile: cnt <= k + 64 = the buffer's size, always, whatever the keys are.
// The best k of a set under a total order do not depend on the order the set was visited in: the atomics only hand out slots, the kept
// SET is the same however they land, and every output is derived from sorted keys.
__device__ __forceinline__ void rowbuf_init(u64* thr, int* cnt, int tid) {
    if (tid < TB) { thr[tid] = 0; cnt[tid] = 0; }
}
// over |= the row now holds more than k keys
__device__ __forceinline__ void rowbuf_propose(u64* buf, int ldb, int* cnt, int k, int row, bool pass, u64 key, u64 thr_row, int& over) {
    if (pass && key > thr_row) {
        const int p = atomicAdd(cnt + row, 1);               // p < k + 64 (the invariant above)
        buf[row * ldb + p] = key;
        over |= (p >= k);
    }
}
// wave w compacts rows 8w .. 8w+7 (8 waves)
__device__ __forceinline__ void rowbuf_compact(u64* buf, int ldb, u64* thr, int* cnt, int k, int wave, int lane) {
    for (int rr = 0; rr < TB / 8; ++rr) {
        const int row = wave * (TB / 8) + rr, n = cnt[row];
        if (n <= k) continue;                                // (wave-uniform)
        u64* bp = buf + row * ldb;
        const u64 e0 = lane < n ? bp[lane] : 0, e1 = lane + 64 < n ? bp[lane + 64] : 0;      // n <= k + 64 <= 128
        int r0 = 0, r1 = 0;                                  // keys of a row are distinct: rank = number of larger keys
        for (int i = 0; i < n; ++i) { const u64 x = bp[i]; r0 += x > e0; r1 += x > e1; }
        // in place: a rank depends on every read of the loop, and one wave's LDS operations are performed in order
        if (lane < n && r0 < k) { bp[r0] = e0; if (r0 == k - 1) thr[row] = e0; }
        if (lane + 64 < n && r1 < k) { bp[r1] = e1; if (r1 == k - 1) thr[row] = e1; }
        if (lane == 0) cnt[row] = k;
    }
}
__device__ __forceinline__ void rowbuf_flush(u64* out, const u64* buf, int ldb, const int* cnt, int k, int tid) {
    for (int i = tid; i < TB * k; i += 512) {
        const int row = i / k, j = i - row * k;
        out[i] = j < cnt[row] ? buf[row * ldb + j] : 0;      // (an empty range writes zeros: no candidate)
    }
}
