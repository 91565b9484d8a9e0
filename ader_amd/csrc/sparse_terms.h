// The LIGHT path of the sparse terms of the fused table updates (k_tab_upd, k_tab16, k_tab32x3): the input-embedding gradient rows
// are added to, and the weighted target rows subtracted from, the dE staging tile of one 64-row tile, in the (id, position) order
// of the tile's bucketed lists -- no atomics, bit-reproducible.  (The heavy path of a hot item's bucket is each kernel's own.)
#pragma once

#define SPV 3                      // input-embedding gradient rows prefetched under the GEMM phase

// A MACRO, expanded where it is used, and not a function: k_tab32x3 runs this block under "#pragma clang fp contract(off)" (the x3
// update kernels share this arithmetic and must agree bit for bit), the bf16-grade kernels do not and may fuse the multiply-add.
// The pragma is lexical -- a shared inline function would quietly give one side the other's rounding.
//   SPB_      entries per batch (the loads of a batch are independent)
//   SPV_      float [SPV]: the prefetched, already scaled gradient rows of the tile (column tid)
//   TG_VAL_   TG_VAL_(b): column tid of operand row b times its weight f.wrow[b].  (The whole product, not the row's value alone: the
//             kernels write its two factors in different orders, and the order decides the instruction stream.)
// In scope at the expansion: f (FuseArgs), ms / mg (the tile's two list records [k0, k1, 8 x (id, row)], in LDS), F_l (the staging
// tile [64][H]), H, tid (< H: thread c owns column c of every row), id_lo / id_hi (the tile's ids are [id_lo, id_hi)).
#define SPARSE_TERMS_LIGHT(SPB_, SPV_, TG_VAL_)                                                            \
    {                                                                                                      \
        const int k0s = ms[0], k1s = ms[1];                                                                \
        _Pragma("unroll") for (int i = 0; i < SPV; ++i) {    /* rows already in registers (same (id, row) order) */ \
            if (k0s + i < k1s) {                                                                           \
                const int id = ms[2 + 2 * i];                                                              \
                if (id < id_hi) F_l[(id - id_lo) * H + tid] += (SPV_)[i];                                  \
            }                                                                                              \
        }                                                                                                  \
        /* entries SPV..7 of the bucket are in the LDS record, the rest in the global lists.  Batches of SPB_ entries: ids and */ \
        /* rows first, then every gradient row, then the adds in entry order (the order fixes the rounding) -- a hot item's */ \
        /* bucket holds hundreds of entries, and one dependent memory round trip per ENTRY made its workgroup the straggler of */ \
        /* the launch (Zipf ids: 1.02 ms against 0.84 ms for uniform ids).  The loads are UNCONDITIONAL (row 0 for entries that do */ \
        /* not count): under a per-entry branch hipcc waits for each load at the end of its branch -- one round trip per entry */ \
        for (int k = k0s + SPV, i = SPV; k < k1s; k += (SPB_), i += (SPB_)) {                              \
            int idv[SPB_], rw[SPB_];                                                                       \
            float val[SPB_];                                                                               \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u) {                                           \
                const int ic = (i + u) < 8 ? (i + u) : 7;                                                  \
                const int id_c = ms[2 + 2 * ic], row_c = ms[3 + 2 * ic];     /* the first 8 entries: from the LDS record */ \
                const bool in = k + u < k1s;                                                               \
                int id_g = 0, row_g = 0;                                                                   \
                if (i + (SPB_) > 8) {                        /* (batch-uniform) later entries: from the global lists, */ \
                    const int ke = in ? k + u : k0s;         /*  UNCONDITIONAL loads of an always-valid entry */ \
                    id_g = f.sp_ids[ke]; row_g = f.sp_rows[ke];                                            \
                }                                                                                          \
                idv[u] = !in ? 0x7fffffff : ((i + u < 8) ? id_c : id_g);                                   \
                rw[u] = !in ? 0 : ((i + u < 8) ? row_c : row_g);                                           \
            }                                                                                              \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u)      /* (ids beyond max_item have no table row) */ \
                val[u] = f.sp_src[(size_t)rw[u] * H + tid] * ((idv[u] < id_hi) ? f.sp_scale : 0.0f);       \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u)                                             \
                if (idv[u] < id_hi) F_l[(idv[u] - id_lo) * H + tid] += val[u];                             \
        }                                                                                                  \
        for (int k = mg[0], k1 = mg[1], i = 0; k < k1; k += (SPB_), i += (SPB_)) {                         \
            int idv[SPB_], bw[SPB_];                                                                       \
            float val[SPB_];                                                                               \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u) {                                           \
                const int ic = (i + u) < 8 ? (i + u) : 7;                                                  \
                const int id_c = mg[2 + 2 * ic], b_c = mg[3 + 2 * ic];                                     \
                const bool in = k + u < k1;                                                                \
                int id_g = 0, b_g = 0;                                                                     \
                if (i + (SPB_) > 8) {                                                                      \
                    const int ke = in ? k + u : mg[0];                                                     \
                    id_g = f.tg_ids[ke]; b_g = f.tg_rows[ke];                                              \
                }                                                                                          \
                idv[u] = !in ? 0x7fffffff : ((i + u < 8) ? id_c : id_g);                                   \
                bw[u] = !in ? 0 : ((i + u < 8) ? b_c : b_g);                                               \
            }                                                                                              \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u)                                             \
                val[u] = TG_VAL_(bw[u]) * ((idv[u] < id_hi) ? 1.0f : 0.0f);                                \
            _Pragma("unroll") for (int u = 0; u < (SPB_); ++u)                                             \
                if (idv[u] < id_hi) F_l[(idv[u] - id_lo) * H + tid] -= val[u];                             \
        }                                                                                                  \
    }
