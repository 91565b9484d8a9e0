// Shared pieces of the bf16-MFMA logit kernels (logits_bf16.hip, logits_x3.hip, table_update.hip).  gfx950 only.
#pragma once
#include "common.h"

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));

#define HP 160
#define LDR 168                 // bf16 elements per LDS / rep_bf row
#define LOG2E 1.4426950408889634f
#define RESCALE_THR 6.0f        // lazy online-softmax rescale threshold (log2 units): p <= 2^6

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// accumulator row of register `reg` for lane half hh (C/D layout of the 32x32 MFMA)
__device__ __forceinline__ int acc_row(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

// 4(k) x 16(n) transposed LDS read: lane (q = (lane&15)>>2, p = lane&3) supplies the address of row k0+q, cols n0+4p..;
// lane i of the 16-lane group receives column n0+i of rows k0..k0+3.
__device__ __forceinline__ bf16x4 tr_read(const bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)p);
}

typedef __attribute__((address_space(3))) bf16 lds_bf16;
__device__ __forceinline__ bf16x4 tr_read3(const lds_bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)p);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& v, int s) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)v[8 * s + j];
    return o;
}


// workgroup barrier that orders LDS traffic only (__syncthreads also drains every outstanding global access of the wave)
__device__ __forceinline__ void lds_only_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ int lower_bound_i32(const int* __restrict__ a, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// Sparse terms and optimiser constants of the fused table update (table_update.hip): when the whole gradient of a table row is
// available inside the workgroup that owns it -- the dense logits term from the MFMAs, plus the sparse input-embedding rows and
// one-hot target rows looked up in id-sorted lists -- the TF-Adam update of that row (ADER.py:96) is applied in place.
struct FuseArgs {
    const int* sp_ids; const int* sp_rows; int n_sp; const float* sp_src; float sp_scale;   // input-embedding rows (sorted by id)
    const int* tg_ids; const int* tg_rows; int n_tg; const float* wrow;                      // one-hot targets (sorted by id)
    const int* tile_meta;       // per 64-row tile: [2 lists][18] = {k0, k1, first 8 (id, row) entries} (ader_tab_tile_meta)
    float* emb1; float* m1; float* v1; bf16* sh1w;   // row of item 1 of theta/m/v and of the bf16 shadow (NULL: no shadow)
    float lr_t, omb1, omb2, eps;
    const float* extra1;        // EXTRA: dense gradient rows to add (row of item 1; [.,H] fp32), e.g. distilled rows' term
};
// host side: the fields FuseArgs shares with table_update_sh.hip's FuseArgs128, from the arguments of the C ABI (lists, tables
// [item_num+1, H] and their shadow or NULL, Adam constants, extra_grad or NULL); the caller adds how its kernel finds a tile's
// list entries (tile_meta / bucket offsets).  Everything else is zero.
template <class F>
static inline F fuse_args(const int* sp_ids, const int* sp_rows, int n_sp, const float* sp_src, float sp_scale, const int* tg_ids,
                          const int* tg_rows, int n_tg, const float* wrow, float* emb, float* adam_m, float* adam_v, void* shadow, int H,
                          float lr_t, float beta1, float beta2, float eps, const float* extra_grad) {
    F f = {};
    f.sp_ids = sp_ids; f.sp_rows = sp_rows; f.n_sp = n_sp; f.sp_src = sp_src; f.sp_scale = sp_scale;
    f.tg_ids = tg_ids; f.tg_rows = tg_rows; f.n_tg = n_tg; f.wrow = wrow;
    f.emb1 = emb + H; f.m1 = adam_m + H; f.v1 = adam_v + H; f.sh1w = shadow ? (bf16*)shadow + LDR : nullptr;
    f.lr_t = lr_t; f.omb1 = 1.0f - beta1; f.omb2 = 1.0f - beta2; f.eps = eps;
    f.extra1 = extra_grad ? extra_grad + H : nullptr;
    return f;
}
// The tile range of a fused update: the C ABI counts 128-item tiles [tile_begin, tile_begin + tile_count) (tile_count < 0: all; a
// rank's rows of a row-sharded table), the kernels 64-row tiles.  *t0 / *tiles: the first 64-row tile and how many, clipped to the
// ceil(N / 64) that exist; false: none.
static inline bool tab_tile_range(int N, int tile_begin, int tile_count, int* t0, int* tiles) {
    const int all = (N + 63) / 64;
    const int tb = (tile_begin < 0 ? 0 : tile_begin) * 2;
    int te = tile_count < 0 ? all : tb + tile_count * 2;
    if (te > all) te = all;
    *t0 = tb; *tiles = te - tb;
    return te > tb;
}

// arguments of the fp32-table update kernels (table_update.hip: k_tab_upd, table_update_x3.hip: k_tab32x3); tiles are 64 rows
struct TabArgs {
    const float* emb1;      // fp32 table, row of item 1: GEMM operand source (and the parameters, FuseArgs.emb1 == this)
    int vrows;              // table rows that exist from emb1 on (item_num)
    const bf16* rep_hi;     // [Bp][LDR] bf16(rep), zero padded
    const bf16* rep_lo;     // [Bp][LDR] bf16(rep - hi)   (X3)
    const void* rep_img;    // k_tab32x3: LDS images of the rep chunks (ader_x3_rep_image); NULL elsewhere
    const float* off;       // [Bp] log2(w_b) - lse2_b; -inf for rows without a loss term
    int Bp, H, N, tile_off;
    int tile_end;           // k_tab32x3: first 64-row tile beyond the launch (its workgroups own PAIRS of tiles)
    float* demb1;           // !ADAM: gradient row of item 1
    // KD rows (ADER.py:132-137): batch rows [kd_row0, Bp) are distilled exemplar rows: dlogit = w (softmax(s[:Np]) - softmax(t)),
    // zero for items >= Np.  kd_row0 % 128 == 0; = Bp: none.  trow / tlse2: [Bp] as written by ader_lx3_fwd_kd_lnf.
    int kd_row0, Np;
    const float* teacher; long ldt; const int* trow; const float* tlse2;
};
// host side: the table slice, the operand planes (rep_lo NULL: bf16 grade), the batch and the catalog, no distilled rows; the launcher
// sets tile_off / rep_img / demb1 where it has them, and tab_args_kd adds the distilled rows
static inline TabArgs tab_args(const float* emb1, int vrows, const void* rep_hi, const void* rep_lo, const float* off, int Bp, int H,
                               int N) {
    TabArgs a = {};
    a.emb1 = emb1; a.vrows = vrows; a.rep_hi = (const bf16*)rep_hi; a.rep_lo = (const bf16*)rep_lo; a.off = off;
    a.Bp = Bp; a.H = H; a.N = N; a.kd_row0 = Bp;
    return a;
}
static inline void tab_args_kd(TabArgs& a, int kd_row0, int Np, const float* teacher, long ldt, const int* trow, const float* tlse2) {
    a.kd_row0 = kd_row0; a.Np = Np; a.teacher = teacher; a.ldt = ldt; a.trow = trow; a.tlse2 = tlse2;
}

// arguments of the x3 flash forward kernels (logits_bf16.hip: k_lx3_fwd, logits_x3.hip: k_lx3g / k_lx3p / k_lx3r)
struct Lx3Args {
    const float* emb1;          // fp32 table, row of item 1
    int vrows;                  // table rows available from emb1 (item_num)
    const bf16* rep_hi; const bf16* rep_lo;     // [Bp][LDR]
    int Bp, H, N, ranges;
    float* pm; float* pl; float* pO;
    // distilled rows (as LbfArgs): rows [kd_row0, Bp) take the softmax over the first Np items and have a teacher readout chunk
    int kd_row0, Np;
    const float* teacher; long ldt; const int* trow; const float* tlse2; float* pO2;
    int ranges2;                // item ranges of the readout launch (it is a launch of its own in x3 mode: its own partition)
};
// host side: the table slice, the operand planes, the batch, the catalog and the softmax partials, no distilled rows; lx3_args_kd adds them
static inline Lx3Args lx3_args(const float* emb1, int vrows, const void* rep_hi, const void* rep_lo, int Bp, int H, int N, int ranges,
                               float* pm, float* pl, float* pO) {
    Lx3Args x = {};
    x.emb1 = emb1; x.vrows = vrows; x.rep_hi = (const bf16*)rep_hi; x.rep_lo = (const bf16*)rep_lo;
    x.Bp = Bp; x.H = H; x.N = N; x.ranges = ranges; x.pm = pm; x.pl = pl; x.pO = pO; x.kd_row0 = Bp;
    return x;
}
static inline void lx3_args_kd(Lx3Args& x, int kd_row0, int Np, const float* teacher, long ldt, const int* trow, const float* tlse2,
                               float* pO2, int ranges2) {
    x.kd_row0 = kd_row0; x.Np = Np; x.teacher = teacher; x.ldt = ldt; x.trow = trow; x.tlse2 = tlse2; x.pO2 = pO2; x.ranges2 = ranges2;
}
// the launchers of logits_x3.hip that the C ABI (logits_bf16.hip) calls: the x3 forward on conflict-free block images where
// lx3f_supports(H) (k_lx3p; it launches k_lx3g itself for H != 150), and the teacher readout of distilled steps k_lx3r where
// lx3r_supports(x) (H = 150, 16-byte aligned teacher rows, at least one whole block)
bool lx3f_supports(int H);
int lx3p_launch(const Lx3Args& x, void* stream);
bool lx3r_supports(const Lx3Args& x);
int lx3r_launch(const Lx3Args& x, void* stream);
