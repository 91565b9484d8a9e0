// Full-catalog logits + softmax cross-entropy at float32 grade: the flash forward kernels on the conflict-free block images.
// Reference: ADER.py:88-93 (logits = rep . item_emb^T, one-hot softmax CE) in float32: every product as three bf16 MFMAs on hi/lo
// operand splits (hi.hi + lo.hi + hi.lo, ~2^-16 relative, fp32 accumulate, fp32 softmax).
//
// The flash forward of flash_walk.h, whose block span, online softmax, P split and epilogues k_lx3_fwd (logits_bf16.hip) expands
// too: per 32-item block S^T = E.rep^T, online max / sum-exp, and the probabilities go
// back into the matrix core as the A operand of O[b,:] += P^T.E (the softmax-weighted readout = dRep up to the target term), so
// nothing [rows, N]-sized is ever written.  The table block is split into hi/lo on its way into LDS as the bank-conflict-free image
// of x3_image.h (16-byte k-chunks [kc][item][8 channels]), and both operand reads -- ds_read_b128 rows for S^T, ds_read_b64_tr_b16
// k-major for the readout -- are pipelined by hand ahead of their MFMAs.
//
// Five kernels stream the table through that image.  They share ONE walk, stated once below: a workgroup = (item range, 128-row chunk)
// on one XCD, 32 batch rows per wave on v_mfma_f32_32x32x16_bf16, the range's 32-item blocks through three LDS buffers, and per block
// the S^T phase (G3_SPHASE) and / or the readout (G3_READOUT).  What each adds:
//   k_lx3g  the flash forward: F3 staging (by k-chunks, any supported H), S^T, online softmax, readout.  Launched for H != 150
//   k_lx3p  the same arithmetic with the softmax / staging vector work issued inside the MFMA phases, P3 staging (memory order,
//           H = 150 only): the default forward
//   k_lx3r  the teacher readout of distilled steps (ADER.py:132-137): P3 staging two blocks ahead, P from the teacher logits instead
//           of an S^T phase, readout
//   k_lx3k  the FILTER of the evaluation ranking (ADER.py:99-103, util.py:323-325): F3 staging, S^T, then counts the items whose x3
//           logit is provably above the row's target logit and lists the undecidable (row, item) pairs for the exact recheck
//   k_lx3t  the FILTER of the top-K recommendation: F3 staging, S^T, then keeps per row a small superset of the exact top-k
//           (filter / append / compact on x3 keys) for k_topk3_finish
// (k_lx3f, 16 rows per wave on 16x16x32 tiles, and k_lx3h, k_lx3g's blocking on 16x16x32 tiles, were measured 25 % and 4 % slower in
// round 3 -- NOTEBOOK.md -- and removed in round 4.)
// Output partials (pm, pl, pO per item range) and the merge (k_lbf_combine<true>) are those of k_lx3_fwd.  gfx950 only.
#include "flash_walk.h"
#include "x3_image.h"
#include "logit_tile.h"
#include "../../include/ader_hip.h"

#define F3_RND 3                  // staging rounds of k_lx3g: 12 units of (8 items x 8 k-chunks), 4 waves
#define G3_ROWS 128                // batch rows per workgroup

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// ===========================================================================================================================
// The shared walk: the layout-independent pieces (FW_*: workgroup map and block span, online softmax, P split, epilogues) are
// flash_walk.h's; here stand the pieces of the block images.  Every piece is a macro over the kernel's locals, expanded in the kernel,
// and not a function: as functions the operand reads compile to other streams.  Names a piece expects in scope are the ones the
// pieces before it define.

// ---- workgroup prologue.  G3_WG_MAP: tid / lane / wave / r32 / hh, then FW_XCD_MAP's (range, bc)
#define G3_WG_MAP(ranges_, nchunk_)                                                                       \
    const int tid = threadIdx.x, lane = tid & 63;                                                         \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                            \
    const int r32 = lane & 31, hh = lane >> 5;                                                            \
    FW_XCD_MAP(ranges_, nchunk_)
// G3_WG_BLOCKS: FW_WG_SPAN's block span; b0 = the wave's first row; and the LDS zero fill: pads of every image (k-chunks >=
// ceil(H/8), bytes between the quads) stay zero, the block stores never touch them.  (b0 stands behind nb_blocks and not in
// G3_WG_MAP: in front of the span's divisions hipcc schedules the scalar prologue of all five kernels differently --
// profiles/logits_x3_refactor_isa.txt)
#define G3_WG_BLOCKS(ranges_, ncat_, ncol_)                                                               \
    FW_WG_SPAN(ranges_, ncat_, ncol_)                                                                     \
    const int b0 = bc * G3_ROWS + wave * 32;                                                              \
    for (int i = tid; i < 3 * X3B_IMG_B / 16; i += 256) ((uint4*)smem_raw)[i] = make_uint4(0u, 0u, 0u, 0u);
// rep fragments: lane (batch row r32, k-half hh) holds rep[b0 + r32][16 ks + 8 hh + 0..7]
#define G3_REP_FRAGS()                                                                                    \
    bf16x8 rh[10], rl[10];                                                                                \
    _Pragma("unroll") for (int ks = 0; ks < 10; ++ks) {                                                   \
        rh[ks] = *(const bf16x8*)(a.rep_hi + (size_t)(b0 + r32) * LDR + 16 * ks + 8 * hh);                \
        rl[ks] = *(const bf16x8*)(a.rep_lo + (size_t)(b0 + r32) * LDR + 16 * ks + 8 * hh);                \
    }

// ---- the operand reads of a block image (x3_image.h, 32x32x16 maps) and the rotation of its three LDS buffers.
// Per-lane byte offsets into a block image, with lane, r32 = lane & 31 and hh = lane >> 5 in scope: t_off = transposed read of (item
// 4 hh + q4, channels 16 g1 + 4 p4.. of a 32-channel block = k-chunks 2 g1 + (p4 >> 1) of its four); a_off = row read of (item r32,
// k-half hh)
#define G3_T_OFF()                                                                                        \
    const int q4 = (lane & 15) >> 2, p4 = lane & 3, g1 = (lane >> 4) & 1;                                 \
    const int t_off = X3B_KC * (2 * g1 + (p4 >> 1)) + 16 * (4 * hh + q4) + 8 * (p4 & 1);
#define G3_A_OFF() const int a_off = X3B_KC * hh + 16 * r32;
// S^T = 32 items x 32 batch rows: A = table rows (lane: item r32, k = 8 hh..8 hh + 7 of the k-step), B = rep fragments.
// set_ = {hi, lo} of k-step ks_ of the image at img_
#define G3_LOADA(set_, img_, ks_)                                                                         \
    { const char* ap_ = (img_) + a_off + 2 * X3B_KC * (ks_);                                              \
      set_[0] = *(const bf16x8*)ap_; set_[1] = *(const bf16x8*)(ap_ + X3B_PLANE_B); }
// transposed reads of the 32-channel block nb_ of plane pl_ (0 hi, 1 lo) of the image at Bh: {items 4hh.., 8 + 4hh.., 16 + 4hh..,
// 24 + 4hh..}
#define G3_LOADT(set_, nb_, pl_)                                                                          \
    { const bf16* tp_ = (const bf16*)(Bh + t_off + 4 * X3B_KC * (nb_) + (pl_) * X3B_PLANE_B);              \
      set_[0] = tr_read(tp_); set_[1] = tr_read(tp_ + 64); set_[2] = tr_read(tp_ + 128); set_[3] = tr_read(tp_ + 192); }
// three LDS buffers: block i is read from buffer i % 3 while block i + 1 (stored during iteration i - 1) waits in the next one and
// block i + 2 -- requested at the head of iteration i, converted and stored between its two MFMA phases -- goes into the third:
// the staging registers are live only under the S^T phase, where the operand sets are small
__device__ __forceinline__ int g3_buf_next(int b) { return b == 2 ? 0 : b + 1; }       // (i + 1) % 3 from i % 3
__device__ __forceinline__ int g3_buf_new(int b) { return b == 0 ? 2 : b - 1; }        // (i + 2) % 3

// ---- the plain S^T phase: S_ = logits of the block image at img_ against the rep fragments rh / rl.  Ten k-steps of three MFMAs
// (lo.hi + hi.lo + hi.hi), the operand sets two k-steps ahead of their use
#define G3_SPHASE(S_, img_)                                                                               \
    {                                                                                                     \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) S_[j] = 0.0f;                                      \
        bf16x8 fa[2][2];                                                                                  \
        G3_LOADA(fa[0], img_, 0);                                                                         \
        G3_LOADA(fa[1], img_, 1);                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        _Pragma("unroll") for (int ks = 0; ks < 10; ++ks) {                                               \
            bf16x8* A_ = fa[ks & 1];                             /* {hi, lo} */                           \
            S_ = mfma_bf16(A_[1], rh[ks], S_);                                                            \
            S_ = mfma_bf16(A_[0], rl[ks], S_);                                                            \
            S_ = mfma_bf16(A_[0], rh[ks], S_);                                                            \
            if (ks + 2 < 10) G3_LOADA(fa[ks & 1], img_, ks + 2);                                          \
            __builtin_amdgcn_sched_barrier(0);                                                            \
        }                                                                                                 \
    }

// ---- the plain readout O += P^T . E of the block image at Bh, with FW_PSPLIT's A operands pa0 / pa1 (hi) and pl0 / pl1 (lo).
// G3_READOUT_LOADS: the first transposed reads (ft: half sets {items 4hh.., 8 + 4hh.., 16 + 4hh.., 24 + 4hh..} of ONE plane; hi, lo,
// hi, lo ...), which do not depend on P.  G3_READOUT: ten half steps, 30 MFMAs, the reads three half steps ahead
#define G3_READOUT_LOADS()                                                                              \
        bf16x4 ft[3][4];                                                                                  \
        G3_LOADT(ft[0], 0, 0);                                                                            \
        G3_LOADT(ft[1], 0, 1);                                                                            \
        G3_LOADT(ft[2], 1, 0);
#define G3_READOUT()                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        _Pragma("unroll") for (int hs = 0; hs < 10; ++hs) {      /* half step: (channel block nb = hs >> 1, plane hs & 1) */ \
            bf16x4* T_ = ft[hs % 3];                                                                      \
            bf16x8 v0, v1;                                                                                \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) { v0[j] = T_[0][j]; v0[4 + j] = T_[1][j]; v1[j] = T_[2][j]; v1[4 + j] = T_[3][j]; } \
            if ((hs & 1) == 0) {                                 /* hi plane of the table: P lo and P hi */ \
                O[hs >> 1] = mfma_bf16(pl0, v0, O[hs >> 1]);                                              \
                O[hs >> 1] = mfma_bf16(pl1, v1, O[hs >> 1]);                                              \
                O[hs >> 1] = mfma_bf16(pa0, v0, O[hs >> 1]);                                              \
                O[hs >> 1] = mfma_bf16(pa1, v1, O[hs >> 1]);                                              \
            } else {                                             /* lo plane: P hi */                     \
                O[hs >> 1] = mfma_bf16(pa0, v0, O[hs >> 1]);                                              \
                O[hs >> 1] = mfma_bf16(pa1, v1, O[hs >> 1]);                                              \
            }                                                                                             \
            if (hs + 3 < 10) G3_LOADT(ft[hs % 3], (hs + 3) >> 1, (hs + 3) & 1);                           \
            __builtin_amdgcn_sched_barrier(0);                                                            \
        }

// ---- F3 staging (k_lx3g / k_lx3k / k_lx3t): a table block = 32 rows of H floats on its way into an LDS block image, by k-chunks.
// Round r (0..2) of wave w covers items 8 w.. and k-chunks 8 r..: lane l -> item + (l & 7), k-chunk + (l >> 3): the 8 lanes of an
// LDS write group store 8 consecutive 16-byte slots (conflict-free), and a wave's two 16-byte loads per slot touch 2 cache lines
// per table row.
#define F3_LOCALS()                                                                                       \
    const int nfull = H >> 3, rem = H & 7;                 /* full k-chunks; channels of the partial one (0, 4 or 6: see launcher) */ \
    /* round r of this lane: item it_ (a wave stages the same 8 items in every round), k-chunk 8 r + kc0 */ \
    const int it_ = 8 * wave + (lane & 7), kc0 = lane >> 3;                                               \
    const int voff = 4 * (it_ * H + 8 * kc0);              /* byte offset inside the block (round r: + 256 r) */ \
    const int voffp = voff + 4 * (rem - 4);                /* second vector of the partial k-chunk: ends with the row */ \
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc((void*)a.emb1, 0, a.vrows * H * 4, 0x00020000); \
    const int dst0 = X3B_KC * kc0 + 16 * it_;              /* byte offset inside a plane (round r: + 8 k-chunks) */ \
    f32x4_t sa[F3_RND], sb[F3_RND];
#define F3_KC(r_) (8 * (r_) + kc0)
#define F3_PART(r_) (rem && F3_KC(r_) == nfull)
#define F3_VALID(r_) (F3_KC(r_) < nfull || F3_PART(r_))
// Block loads through a buffer descriptor of the table (base in scalar registers, ONE 32-bit per-lane offset, the block's
// offset as the scalar offset, the round's as the instruction's immediate): no 64-bit per-lane pointers, and rows beyond the
// table's last one (only in its last block; their items are >= N: outside the softmax) come back as zeros from the hardware
// range check.  Lanes without a k-chunk read whatever follows their row (never stored).  NOTHING is selected on the loaded data
// here -- a select would make hipcc wait for each load right behind its issue.
#define F3_LOAD(blk_)                                                                                     \
    {                                                                                                     \
        const int so_ = (blk_) * (FB * 4) * H;              /* byte offset of the block (< 2^31: checked by the launcher) */ \
        _Pragma("unroll") for (int r = 0; r < F3_RND; ++r) {                                              \
            const u32x4_t va_ = __builtin_amdgcn_raw_buffer_load_b128(trs, voff + 256 * r, so_, 0);         \
            const u32x4_t vb_ = __builtin_amdgcn_raw_buffer_load_b128(trs, (F3_PART(r) ? voffp : voff + 16) + 256 * r, so_, 0); \
            sa[r] = __builtin_bit_cast(f32x4_t, va_); sb[r] = __builtin_bit_cast(f32x4_t, vb_);           \
        }                                                                                                 \
    }
// hi = bf16(x), lo = bf16(x - hi), 8 channels -> one 16-byte slot per plane
#define F3_STORE(buf_)                                                                                    \
    {                                                                                                     \
        unsigned char* dst_ = smem_raw + (buf_) * X3B_IMG_B;                                               \
        _Pragma("unroll") for (int r = 0; r < F3_RND; ++r) {                                              \
            float x_[8];                                                                                  \
            x_[0] = sa[r][0]; x_[1] = sa[r][1]; x_[2] = sa[r][2]; x_[3] = sa[r][3];                       \
            if (F3_PART(r)) {       /* rem = 6: channels 4,5 are elements 2,3 of the shifted vector; rem = 4: none */ \
                x_[4] = (rem == 6) ? sb[r][2] : 0.f; x_[5] = (rem == 6) ? sb[r][3] : 0.f; x_[6] = 0.f; x_[7] = 0.f; \
            } else { x_[4] = sb[r][0]; x_[5] = sb[r][1]; x_[6] = sb[r][2]; x_[7] = sb[r][3]; }            \
            bf16x8 h_, l_;                                                                                \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) { h_[j] = (bf16)x_[j]; l_[j] = (bf16)(x_[j] - (float)h_[j]); } \
            if (F3_VALID(r)) {                                                                            \
                *(bf16x8*)(dst_ + dst0 + 8 * X3B_KC * r) = h_;                                            \
                *(bf16x8*)(dst_ + X3B_PLANE_B + dst0 + 8 * X3B_KC * r) = l_;                              \
            }                                                                                             \
        }                                                                                                 \
    }
// The walk over the range's blocks with F3 staging.  Between F3_WALK_BEGIN() and F3_WALK_END() stands the kernel's per-block body,
// with i (block of the range), i0 (its first item), Bh (its image) and S (its logits: the S^T phase is done) in scope.  Block i + 2
// is requested at the head of iteration i and stored behind the S^T phase
#define F3_WALK_BEGIN()                                                                                   \
    if (nb_blocks > 0) F3_LOAD(blk_begin);                                                                \
    __syncthreads();                                       /* zero fill done */                           \
    if (nb_blocks > 0) F3_STORE(0);                                                                       \
    if (nb_blocks > 1) { F3_LOAD(blk_begin + 1); F3_STORE(1); }                                           \
    int bcur = 0;                                          /* i % 3 */                                    \
    for (int i = 0; i < nb_blocks; ++i) {                                                                 \
        __syncthreads();                                   /* blocks i and i + 1 are in LDS; every wave is done with block i - 1 */ \
        const bool more = i + 2 < nb_blocks;                                                              \
        if (more) F3_LOAD(blk_begin + i + 2);                                                             \
        const char* Bh = (const char*)(smem_raw + bcur * X3B_IMG_B);                                      \
        const int i0 = (blk_begin + i) * FB;                                                           \
        f32x16 S;                                                                                         \
        G3_SPHASE(S, Bh)                                                                                  \
        if (more) F3_STORE(g3_buf_new(bcur));
#define F3_WALK_END()                                                                                     \
        bcur = g3_buf_next(bcur);                                                                         \
    }

// ---- P3 staging (k_lx3p / k_lx3r, H = 150): a block = 32 table rows of 150 floats, as 16-byte pieces read in memory order.  Lane l ->
// item 8 wave + (l >> 3), piece (l & 7) + 8 r of the row's 37.5 (round r = 0..4): a wave-instruction reads 8 x 128 contiguous bytes --
// ~12 cache lines, every byte used -- where the F3 k-chunk mapping reads 8 x 8 half-used 32-byte pieces (~20 lines, each touched by
// two instructions); 5 loads instead of 6.  A piece = 4 channels = half a k-chunk slot: one ds_write_b64 per plane (two-way bank
// conflicts, hidden under the VGPR-to-LDS transfer of the store).  The loads go through a buffer descriptor of the table as in
// F3_LOAD; rows beyond the table's last one come back as zeros from the hardware range check.  sc_ = the staging set, f32x4_t [5].
// The kernel's locals: qb, itb (the lane's piece and item), trs, voffb, dstb.  (They are written out in both kernels: each keeps its
// instruction stream only with its own order of qb and itb, so one shared statement of them serves one kernel and not the other.)
#define P3_LOAD(sc_, blk_)                                                                              \
    {                                                                                                     \
        const int so_ = (blk_) * (FB * 4) * H;              /* byte offset of the block (< 2^31: checked by the launcher) */ \
        _Pragma("unroll") for (int r = 0; r < 5; ++r)                                                     \
            sc_[r] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(trs, voffb + 128 * r, so_, 0)); \
    }
#define P3_STORE(sc_, buf_)                                                                               \
    {                                                                                                     \
        unsigned char* dst_ = smem_raw + (buf_) * X3B_IMG_B;                                              \
        _Pragma("unroll") for (int r = 0; r < 5; ++r) {                                                   \
            const int p_ = qb + 8 * r;                          /* piece 37 = channels 148, 149 and two floats of the next row */ \
            float x_[4];                                        /* pieces 38, 39 = channels 152..159: zeros (no branch) */ \
            x_[0] = (r == 4 && p_ >= 38) ? 0.f : sc_[r][0]; x_[1] = (r == 4 && p_ >= 38) ? 0.f : sc_[r][1]; \
            x_[2] = (r == 4 && p_ >= 37) ? 0.f : sc_[r][2]; x_[3] = (r == 4 && p_ >= 37) ? 0.f : sc_[r][3]; \
            bf16x4 h_, l_;                                                                                \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) { h_[j] = (bf16)x_[j]; l_[j] = (bf16)(x_[j] - (float)h_[j]); } \
            *(bf16x4*)(dst_ + dstb + 4 * X3B_KC * r) = h_;                                                \
            *(bf16x4*)(dst_ + X3B_PLANE_B + dstb + 4 * X3B_KC * r) = l_;                                  \
        }                                                                                                 \
    }

// ---------------------------------------------------------------------------------------------------------------------------
// k_lx3g: 32 batch rows per wave on v_mfma_f32_32x32x16_bf16 (128 per workgroup, two workgroups per CU): every LDS operand fragment
// feeds twice the flops of a 16x16x32 form with 16-row waves, which keeps the LDS pipe as busy as the matrix pipe.
// Register plan (<= 256): rep fragments 80, O 80, S / P 16, one block in flight 24, operand sets 16 / 32.
__global__ __launch_bounds__(256, 2) void k_lx3g(Lx3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // [3 buffers][block image]
    G3_WG_MAP(a.ranges, a.Bp / G3_ROWS)
    const int H = a.H;
    const int N = (bc * G3_ROWS >= a.kd_row0) ? a.Np : a.N;            // columns of this chunk's softmax (distilled rows: first Np)
    G3_WG_BLOCKS(a.ranges, a.N, N)
    G3_REP_FRAGS()
    FW_O_ZERO()
    float m_run = -INFINITY, l_run = 0.0f;
    F3_LOCALS()
    G3_T_OFF()
    G3_A_OFF()
    F3_WALK_BEGIN()
        __builtin_amdgcn_sched_barrier(0);
        G3_READOUT_LOADS()                                 // they do not depend on S: in flight under the softmax section
        __builtin_amdgcn_sched_barrier(0);
        FW_SOFTMAX_HEAD()
        FW_EXP_SUM()
        FW_PSPLIT()
        G3_READOUT()
    F3_WALK_END()
    FW_STORE_ML()
    FW_STORE_O(a.pO + ((size_t)range * a.Bp + b0) * HP)
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_lx3p: k_lx3g with the softmax of block i issued INSIDE the S phase of block i + 1.  Stamps of k_lx3g (NOTEBOOK.md): a wave
// spends 2,400 of a block's 5,300 clocks in vector-only phases (staging, softmax) and the two waves of a SIMD mostly take turns --
// the kernel is bound by the waves' serial chains, not by the matrix pipe (68 % busy).  Here the logits of the NEXT block are
// accumulated (a second S, 16 registers) while the exp / sum / hi-lo split of the current block's logits are placed between its
// MFMAs; the rescale test (a branch) stays in front.  Same arithmetic in the same order as k_lx3g: bit-equal results.
// (H = 150 only.  It stays a template although HT has one value: the benchmark picks this kernel's counters by the name prefix
//  "k_lx3p<".)
template <int HT>
__global__ __launch_bounds__(256, 2) void k_lx3p(Lx3Args a) {
    static_assert(HT == 150, "k_lx3p: piece staging (H = 150) only");
    constexpr int H = HT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // [3 buffers][block image]
    G3_WG_MAP(a.ranges, a.Bp / G3_ROWS)
    const int N = (bc * G3_ROWS >= a.kd_row0) ? a.Np : a.N;            // columns of this chunk's softmax (distilled rows: first Np)
    G3_WG_BLOCKS(a.ranges, a.N, N)
    G3_REP_FRAGS()
    FW_O_ZERO()
    float m_run = -INFINITY, l_run = 0.0f;
    const int qb = lane & 7, ib = lane >> 3;               // P3 staging locals
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc((void*)a.emb1, 0, a.vrows * H * 4, 0x00020000);
    const int itb = 8 * wave + ib;
    const int voffb = itb * (4 * H) + 16 * qb;               // round r: + 128 r
    const int dstb = X3B_KC * (qb >> 1) + 16 * itb + 8 * (qb & 1);      // round r: + 4 k-chunks
    f32x4_t sc[5];
    G3_T_OFF()
    G3_A_OFF()
    if (nb_blocks > 0) P3_LOAD(sc, blk_begin);
    __syncthreads();                                       // zero fill done
    if (nb_blocks > 0) P3_STORE(sc, 0);
    if (nb_blocks > 1) { P3_LOAD(sc, blk_begin + 1); P3_STORE(sc, 1); }
    int bcur = 0;                                          // i % 3
    // softmax of ONE pair of logits of the current block (elements 2 q_, 2 q_ + 1 of S): p = exp2(s log2e - m), running sum in
    // element order (the order of k_lx3g: bit-equal results), hi / lo split into packed pairs
#define P3_PAIR(q_)                                                                                       \
    { const float p0_ = __builtin_amdgcn_exp2f(fmaf(S[2 * (q_)], LOG2E, nm));                             \
      const float p1_ = __builtin_amdgcn_exp2f(fmaf(S[2 * (q_) + 1], LOG2E, nm));                         \
      ls += p0_; ls += p1_;                                                                               \
      bf16x2 h_; h_[0] = (bf16)p0_; h_[1] = (bf16)p1_;                                                    \
      bf16x2 l_; l_[0] = (bf16)(p0_ - (float)h_[0]); l_[1] = (bf16)(p1_ - (float)h_[1]);                  \
      ph2[q_] = __builtin_bit_cast(uint32_t, h_); pl2[q_] = __builtin_bit_cast(uint32_t, l_); }
    // the readout's A operands from the packed pairs ph2 / pl2
#define P3_PACK()                                                                                         \
        bf16x8 pa0, pa1, pl0, pl1;                                                                        \
        {   typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));                                  \
            pa0 = __builtin_bit_cast(bf16x8, (u32x4_){ph2[0], ph2[1], ph2[2], ph2[3]});                   \
            pa1 = __builtin_bit_cast(bf16x8, (u32x4_){ph2[4], ph2[5], ph2[6], ph2[7]});                   \
            pl0 = __builtin_bit_cast(bf16x8, (u32x4_){pl2[0], pl2[1], pl2[2], pl2[3]});                   \
            pl1 = __builtin_bit_cast(bf16x8, (u32x4_){pl2[4], pl2[5], pl2[6], pl2[7]});                   \
        }
    f32x16 S;
    // ---- block 0's logits: a plain S phase (no softmax to hide yet)
    __syncthreads();                                       // blocks 0 and 1 are in LDS
    if (nb_blocks > 0) G3_SPHASE(S, (const char*)smem_raw)
    int i = 0;
    for (; i + 2 < nb_blocks; ++i) {                       // (every iteration stages a block: NO branch between the S phase and the readout --
        __syncthreads();                                   //  across one the compiler sinks the whole softmax to its first use)
        P3_LOAD(sc, blk_begin + i + 2);
        const int bnext = g3_buf_next(bcur), bnew = g3_buf_new(bcur);
        const char* Bh = (const char*)(smem_raw + bcur * X3B_IMG_B);
        const char* Bs = (const char*)(smem_raw + bnext * X3B_IMG_B);
        const int i0 = (blk_begin + i) * FB;
        FW_SOFTMAX_HEAD()
        uint32_t ph2[8], pl2[8];                           // P hi / lo as packed bf16 pairs
        // ---- the NEXT block's S phase, with this block's softmax in the shadows of its MFMAs: a matrix instruction holds the SIMD's
        // vector issue for 8 of its 32 clocks, so a few vector instructions placed BETWEEN the three MFMAs of a k-step cost nothing
        // while the matrix pipe is busy.  Per k-step: the exp of one pair of logits, and the sum / hi-lo split of the PREVIOUS pair
        // (its exp results are a k-step old: no wait).  hipcc does not interleave the two chains by itself: the order is pinned as
        // written (a sched_barrier after every piece).
        f32x16 Sn;
#pragma unroll
        for (int j = 0; j < 16; ++j) Sn[j] = 0.0f;
        bf16x8 fa[2][2];
        G3_LOADA(fa[0], Bs, 0);
        G3_LOADA(fa[1], Bs, 1);
        __builtin_amdgcn_sched_barrier(0);
        // (order pinned piece by piece: the machine scheduler's own interleaving -- sched_group_barrier -- is reverted at 254
        //  registers, and vector instructions left to instruction selection all land behind the MFMAs)
#pragma unroll
        for (int ks = 0; ks < 10; ++ks) {
            bf16x8* A_ = fa[ks & 1];
            Sn = mfma_bf16(A_[1], rh[ks], Sn);
            __builtin_amdgcn_sched_barrier(0);
            if (ks < 8) {                                   // exp of pair ks
                S[2 * ks] = __builtin_amdgcn_exp2f(fmaf(S[2 * ks], LOG2E, nm));
                S[2 * ks + 1] = __builtin_amdgcn_exp2f(fmaf(S[2 * ks + 1], LOG2E, nm));
            }
            __builtin_amdgcn_sched_barrier(0);
            Sn = mfma_bf16(A_[0], rl[ks], Sn);
            __builtin_amdgcn_sched_barrier(0);
            if (ks >= 1 && ks < 9) {                        // pair ks - 1 (its exp results are a k-step old): sum, hi
                const int q = ks - 1;
                ls += S[2 * q]; ls += S[2 * q + 1];
                bf16x2 h_; h_[0] = (bf16)S[2 * q]; h_[1] = (bf16)S[2 * q + 1];
                ph2[q] = __builtin_bit_cast(uint32_t, h_);
                S[2 * q] -= (float)h_[0]; S[2 * q + 1] -= (float)h_[1];
            }
            __builtin_amdgcn_sched_barrier(0);
            Sn = mfma_bf16(A_[0], rh[ks], Sn);
            __builtin_amdgcn_sched_barrier(0);
            if (ks >= 1 && ks < 9) {                        // ... lo
                const int q = ks - 1;
                bf16x2 l_; l_[0] = (bf16)S[2 * q]; l_[1] = (bf16)S[2 * q + 1];
                pl2[q] = __builtin_bit_cast(uint32_t, l_);
            }
            if (ks + 2 < 10) G3_LOADA(fa[ks & 1], Bs, ks + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        l_run += ls;
        // ---- the readout O += P^T . E of block i, with the conversion of block i + 2 (fp32 -> hi / lo image: ~17 vector instructions
        // and two 8-byte LDS stores per 16-byte piece) in the shadows of its MFMAs: round r of the staging goes with half steps 2 r, 2 r + 1
        G3_READOUT_LOADS()
        P3_PACK()
        unsigned char* dstn = smem_raw + bnew * X3B_IMG_B + dstb;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            float x_[4];
            bf16x4 h_, l_;
            // ---- half step 2 r: hi plane of the table (channel block r): P lo and P hi
            {
                bf16x4* T_ = ft[(2 * r) % 3];
                bf16x8 v0, v1;
#pragma unroll
                for (int j = 0; j < 4; ++j) { v0[j] = T_[0][j]; v0[4 + j] = T_[1][j]; v1[j] = T_[2][j]; v1[4 + j] = T_[3][j]; }
                O[r] = mfma_bf16(pl0, v0, O[r]);
                __builtin_amdgcn_sched_barrier(0);
                {   const int p_ = qb + 8 * r;                  // pieces 38, 39 = channels 152..159: zeros (no branch)
                    x_[0] = (r == 4 && p_ >= 38) ? 0.f : sc[r][0]; x_[1] = (r == 4 && p_ >= 38) ? 0.f : sc[r][1];
                    x_[2] = (r == 4 && p_ >= 37) ? 0.f : sc[r][2]; x_[3] = (r == 4 && p_ >= 37) ? 0.f : sc[r][3];
                }
                __builtin_amdgcn_sched_barrier(0);
                O[r] = mfma_bf16(pl1, v1, O[r]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) h_[j] = (bf16)x_[j];
                __builtin_amdgcn_sched_barrier(0);
                O[r] = mfma_bf16(pa0, v0, O[r]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) x_[j] -= (float)h_[j];
                __builtin_amdgcn_sched_barrier(0);
                O[r] = mfma_bf16(pa1, v1, O[r]);
                if (2 * r + 3 < 10) G3_LOADT(ft[(2 * r) % 3], (2 * r + 3) >> 1, (2 * r + 3) & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- half step 2 r + 1: lo plane: P hi
            {
                bf16x4* T_ = ft[(2 * r + 1) % 3];
                bf16x8 v0, v1;
#pragma unroll
                for (int j = 0; j < 4; ++j) { v0[j] = T_[0][j]; v0[4 + j] = T_[1][j]; v1[j] = T_[2][j]; v1[4 + j] = T_[3][j]; }
                O[r] = mfma_bf16(pa0, v0, O[r]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) l_[j] = (bf16)x_[j];
                *(bf16x4*)(dstn + 4 * X3B_KC * r) = h_;
                __builtin_amdgcn_sched_barrier(0);
                O[r] = mfma_bf16(pa1, v1, O[r]);
                __builtin_amdgcn_sched_barrier(0);
                *(bf16x4*)(dstn + X3B_PLANE_B + 4 * X3B_KC * r) = l_;
                if (2 * r + 4 < 10) G3_LOADT(ft[(2 * r + 1) % 3], (2 * r + 4) >> 1, (2 * r + 4) & 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        S = Sn;
        bcur = bnext;
    }
    for (; i < nb_blocks; ++i) {                           // ---- the last two blocks: plain order (nothing left to stage)
        __syncthreads();
        const int bnext = g3_buf_next(bcur);
        const char* Bh = (const char*)(smem_raw + bcur * X3B_IMG_B);
        const char* Bs = (const char*)(smem_raw + bnext * X3B_IMG_B);
        const int i0 = (blk_begin + i) * FB;
        FW_SOFTMAX_HEAD()
        uint32_t ph2[8], pl2[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) P3_PAIR(q);
        f32x16 Sn;
#pragma unroll
        for (int j = 0; j < 16; ++j) Sn[j] = 0.0f;         // (copied into S below also when there is no next block)
        if (i + 1 < nb_blocks) G3_SPHASE(Sn, Bs)
        l_run += ls;
        __builtin_amdgcn_sched_barrier(0);
        G3_READOUT_LOADS()
        P3_PACK()
        G3_READOUT()
        S = Sn;
        bcur = bnext;
    }
#undef P3_PACK
#undef P3_PAIR
    FW_STORE_ML()
    FW_STORE_O(a.pO + ((size_t)range * a.Bp + b0) * HP)
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_lx3r: the TEACHER READOUT of a distilled step (ADER.py:132-137) as its own launch: O2[b,:] = sum_{j < Np} softmax(teacher_b)_j E_j
// for the 128-row chunks of exemplar rows -- k_lx3g's readout half (same block images, same hand-pipelined transposed reads, same
// 30 MFMAs per block and wave) fed by the teacher logits instead of an S phase: lane (row r32, half hh) loads the 16 teacher
// logits of its accumulator positions (four 16-byte loads), p = exp2(t log2e - tlse2) is exact (the teacher's log-sum-exp is known),
// split hi / lo.  HBM-bound (teacher tile + table block per 32 items): both streams run TWO blocks ahead of their use in registers
// (table: two staging sets, converted into the third LDS buffer at the head of an iteration; teacher: two sets), and the block
// barrier orders LDS traffic only -- __syncthreads would drain those loads.  Replaces k_lx3_fwd<true> (logits_bf16.hip: one
// block of lookahead, per-lane branches around the teacher loads; 0.30 ms against 0.2 at cfg-S + 128 exemplar rows) for H = 150,
// 16-byte aligned teacher rows.  Output partials pO2 [range][Bk][160] as before.
__global__ __launch_bounds__(256, 2) void k_lx3r(Lx3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // [3 buffers][block image]
    constexpr int H = 150;
    const int Bk = a.Bp - a.kd_row0, Np = a.Np;
    G3_WG_MAP(a.ranges2, Bk / G3_ROWS)                     // b0 = first exemplar row of the wave (row of the padded batch: + kd_row0)
    G3_WG_BLOCKS(a.ranges2, Np, Np)
    FW_O_ZERO()
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc((void*)a.emb1, 0, a.vrows * H * 4, 0x00020000);     // P3 staging locals
    const int itb = 8 * wave + (lane >> 3), qb = lane & 7;
    const int voffb = itb * (4 * H) + 16 * qb;
    const int dstb = X3B_KC * (qb >> 1) + 16 * itb + 8 * (qb & 1);
    f32x4_t sc[2][5];                                      // two staging sets
    // teacher logits of this lane's accumulator positions: row r32, items 8 q + 4 hh + 0..3 of the block (register 4 q + k)
    const int tr = a.trow[a.kd_row0 + b0 + r32];
    const float tl2 = a.tlse2[a.kd_row0 + b0 + r32];
    const float* trp = a.teacher + (size_t)(tr < 0 ? 0 : tr) * a.ldt + 4 * hh;
    float tt[2][16];
    // Everything inside the block loop is unconditional -- a load under a branch becomes a phi of two register sets (hipcc then spilled
    // a whole staging set: loads straight into scratch).  Table blocks past the range are real rows (or zeros from the descriptor's
    // range check) that are stored into a buffer nobody reads; teacher blocks are clamped to the last FULL block of [0, Np).  The one
    // partial block of a launch (Np % 32 != 0; last range only) is peeled: element-wise clamped loads, validity applied to p.
    const int nfull_all = Np / FB;                      // >= 1 (launcher)
#define R3_TLOAD(set_, blk_)                                                                              \
    {                                                                                                     \
        const int i0_ = min((blk_), nfull_all - 1) * FB;                                               \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                   \
            const f32x4_t v_ = *(const f32x4_t*)(trp + i0_ + 8 * q);                                      \
            tt[set_][4 * q] = v_[0]; tt[set_][4 * q + 1] = v_[1]; tt[set_][4 * q + 2] = v_[2]; tt[set_][4 * q + 3] = v_[3]; \
        }                                                                                                 \
    }
#define R3_TSLOW(set_, blk_)                                                                              \
    {                                                                                                     \
        const int i0_ = (blk_) * FB;                                                                   \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                     \
            _Pragma("unroll") for (int k = 0; k < 4; ++k)                                                 \
                tt[set_][4 * q + k] = trp[min(i0_ + 8 * q + k, Np - 1 - 4 * hh)];                         \
    }
    G3_T_OFF()
    const int nb_full = max(0, min(blk_end, nfull_all) - blk_begin);       // full blocks of this range (the rest: the partial one)
    // prologue: blocks 0, 1 -> LDS buffers 0, 1; blocks 2, 3 -> staging sets 0, 1; teacher blocks 0, 1 -> sets 0, 1
    P3_LOAD(sc[0], blk_begin);
    P3_LOAD(sc[1], blk_begin + 1);
    R3_TLOAD(0, blk_begin);
    R3_TLOAD(1, blk_begin + 1);
    __syncthreads();                                       // zero fill done
    P3_STORE(sc[0], 0);
    P3_STORE(sc[1], 1);
    P3_LOAD(sc[0], blk_begin + 2);
    P3_LOAD(sc[1], blk_begin + 3);
    int bcur = 0;                                          // i % 3
    // one iteration (block i, register sets e_ = i & 1): block i + 2 (requested two iterations ago) goes into the buffer block i - 1
    // was read from, block i + 4 is requested; P from the teacher set, which is then refilled with block i + 2
#define R3_ITER(e_)                                                                                       \
    {                                                                                                     \
        lds_only_barrier();                                /* blocks i, i + 1 in LDS; every wave is done with block i - 1 */ \
        P3_STORE(sc[e_], g3_buf_new(bcur));                                                               \
        P3_LOAD(sc[e_], blk_begin + i + 4);                                                               \
        const char* Bh = (const char*)(smem_raw + bcur * X3B_IMG_B);                                      \
        G3_READOUT_LOADS()                                                                                \
        f32x16 S;                                                                                         \
        const int lim_ = (tr >= 0) ? Np - (blk_begin + i) * FB - 4 * hh : 0;     /* items of this lane's positions inside [0, Np) */ \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                                  \
            const float x_ = __builtin_amdgcn_exp2f(fmaf(tt[e_][j], LOG2E, -tl2));                        \
            S[j] = ((j & 3) + 8 * (j >> 2) < lim_) ? x_ : 0.0f;                                           \
        }                                                                                                 \
        R3_TLOAD(e_, blk_begin + i + 2);                                                                  \
        FW_PSPLIT()                                                                                       \
        G3_READOUT()                                                                                      \
        bcur = g3_buf_next(bcur);                                                                         \
        ++i;                                                                                              \
    }
    int i = 0;
    while (i < nb_full) {
        R3_ITER(0)
        if (i >= nb_full) break;                           // workgroup-uniform
        R3_ITER(1)
    }
    if (nb_blocks > nb_full) {                             // the partial block (its table rows are already on their way)
        if (i & 1) { R3_TSLOW(1, blk_begin + i); R3_ITER(1) } else { R3_TSLOW(0, blk_begin + i); R3_ITER(0) }
    }
#undef R3_TSLOW
#undef R3_ITER
#undef R3_TLOAD
    FW_STORE_O(a.pO2 + ((size_t)range * Bk + b0) * HP)
}

// ---- launchers.  The grid of the shared walk: one workgroup per (item range, 128-row chunk)
static dim3 x3_grid(int ranges, int rows) { return dim3(ranges * (rows / G3_ROWS)); }
// the block offsets of the buffer loads are 32-bit
static bool x3_table_fits(int vrows, int H) { return (long)vrows * H * 4 < (1l << 31); }

// teacher readout launch: x.ranges2 item ranges x (Bp - kd_row0) / 128 chunks.  false: the shape is not k_lx3r's (caller falls back)
bool lx3r_supports(const Lx3Args& x) {
    return x.H == 150 && x.Np >= FB && (x.ldt & 3) == 0 && (((uintptr_t)x.teacher) & 15) == 0 && (long)(x.vrows + 5 * FB) * x.H * 4 < (1l << 31);      // (block offsets are 32-bit; the stream runs 4 blocks ahead)
}
int lx3r_launch(const Lx3Args& x, void* stream) {
    if (int e = ader_dyn_lds<k_lx3r>(3 * X3B_IMG_B)) return e;
    hipLaunchKernelGGL(k_lx3r, x3_grid(x.ranges2, x.Bp - x.kd_row0), dim3(256), 3 * X3B_IMG_B, (hipStream_t)stream, x);
    return 0;
}

bool lx3f_supports(int H) { return (H & 1) == 0 && H >= 8 && H <= HP && ((H & 7) == 0 || (H & 7) == 4 || (H & 7) == 6); }
// what the filters k_lx3k / k_lx3t ask of a call's shapes: whole 128-row chunks, an H with an F3 staging, N items of an 8-byte
// aligned table that the 32-bit block offsets reach
static bool x3_filter_shapes_ok(const float* emb, int item_num, int B, int Bp, int H, int N) {
    return Bp % G3_ROWS == 0 && B <= Bp && lx3f_supports(H) && N >= 1 && N <= item_num && !((uintptr_t)emb & 7) && x3_table_fits(item_num, H);
}

// x.ranges must be ader_lbf_ranges(x.N, x.Bp); Bp % 128 == 0
int lx3g_launch(const Lx3Args& x, void* stream) {
    if (int e = ader_dyn_lds<k_lx3g>(3 * X3B_IMG_B)) return e;
    if (!x3_table_fits(x.vrows, x.H)) return -2;
    hipLaunchKernelGGL(k_lx3g, x3_grid(x.ranges, x.Bp), dim3(256), 3 * X3B_IMG_B, (hipStream_t)stream, x);
    return 0;
}

int lx3p_launch(const Lx3Args& x, void* stream) {
    if (int e = ader_dyn_lds<k_lx3p<150>>(3 * X3B_IMG_B)) return e;
    if (!x3_table_fits(x.vrows, x.H)) return -2;
    if (x.H != 150) return lx3g_launch(x, stream);                 // (the pipelined form exists for the reference's hidden size only)
    hipLaunchKernelGGL(k_lx3p<150>, x3_grid(x.ranges, x.Bp), dim3(256), 3 * X3B_IMG_B, (hipStream_t)stream, x);
    return 0;
}


// ---------------------------------------------------------------------------------------------------------------------------
// Evaluation ranking on the bf16 matrix cores, rank-identical to the exact-f32 kernel (k_logits_tile<MODE_RANK>, logits.hip).
// rank[b] = #{n : s[b,n] > tl[b] or (s[b,n] == tl[b] and n < t_b)} with s, tl from the f32 MFMA chain.  k_lx3k computes every s at x3
// grade (s3) and decides a pair only where the decision cannot differ:  s3 > tl + delta_b  =>  s > tl (counts),  s3 < tl - delta_b  =>
// s < tl (does not); the pairs inside the band go to a list, which k_pair_logit_rank (logits.hip) re-evaluates through the exact chain.
//
// delta_b = KAPPA |rep_b|_2 Emax, Emax = max_n |E_n|_2 (both norms rounded up), KAPPA = 2^-13.  Derivation, with P = sum_k |r_k||e_k|
// <= |r||e| (Cauchy-Schwarz) and x = hi + lo + eps, |lo| <= 2^-9 |x|, |eps| <= 2^-18 |x| for the bf16 (8-bit significand) splits:
//   products   r e - (hi hi + lo hi + hi lo) = lo lo + eps terms:  <= 2^-18 + 2 2^-18 + O(2^-27) < 2^-16 per product (the project's
//              stated x3 bound; profiles/probe_f16x3_r6.txt measured 2^-18.5)                                   -> 2^-16     P
//   x3 sum     3 x 160 terms accumulated in fp32, one rounding of <= 2^-24 of the running sum each                -> 480 2^-24 P
//   exact sum  160 fused multiply-adds in fp32 (v_mfma_f32_16x16x4_f32: an fma chain in k order)                  -> 160 2^-24 P
// |s3 - s| <= (2^-16 + 640 2^-24) P = 2^-14.19 P < 2^-14.1 |r||e|.  KAPPA doubles that: the MFMA's internal accumulate rounding is not
// documented as round-to-nearest (a truncating accumulate doubles the two sum terms), and the band edges tl +- delta are themselves
// rounded (<= 2^-24 (|tl| + delta) <= 2^-10.9 delta).  ader_amd/engine/infer.py RANK_X3_KAPPA restates the value; the host test emulates
// the bound, the GPU tests read the observed |s3 - s| / delta (diag[1]) and require it <= 0.5.
#define RANK_X3_KAPPA 0x1p-13f
#define RANK_NORM_UP 1.0005f        // sqrt of an fp32 sum of <= 160 squares is within 2^-16 of the norm: x (1 + 2^-11) rounds it UP

struct RankX3Args {
    const float* emb1; int vrows;                   // fp32 table, row of item 1; rows available from it (item_num)
    const bf16* rep_hi; const bf16* rep_lo;         // [Bp][LDR] (k_lx3_prep)
    int Bp, H, N, ranges;
    const int* target; const int* ncol;             // [Bp] 1-based target; N for real rows, 0 for padding rows
    const float* tlogit; const float* delta;        // [Bp] exact-f32 target logit (k_target_logit); band half-width
    int* cand; int cap;                             // [cap][3] = (row, item, bits of s3)
    int* diag;                                      // [0] entries requested (keeps counting past cap = overflow), [1] recheck's max err / delta
    int* rank;                                      // [Bp], zeroed by the launcher
};

// Emax: one wave per table row, grid-stride; integer atomic max on the float's bit pattern (norms are non-negative)
__global__ __launch_bounds__(256) void k_rank_emax(const float* __restrict__ emb1, int H, int N, float* __restrict__ emax) {
    const int lane = threadIdx.x & 63;
    float m = 0.0f;
    for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += gridDim.x * 4) {
        const float* p = emb1 + (size_t)n * H;
        float ss = 0.0f;
        for (int c = lane; c < H; c += 64) ss = fmaf(p[c], p[c], ss);
        m = fmaxf(m, wave_sum(ss));
    }
    if (lane == 0) atomicMax((int*)emax, __float_as_int(sqrtf(m) * RANK_NORM_UP));
}
// delta[b] = KAPPA |rep_b| Emax (0 for padding rows): one wave per batch row
__global__ __launch_bounds__(256) void k_rank_delta(const float* __restrict__ rep, int B, int Bp, int H, const float* __restrict__ emax,
                                                    float* __restrict__ delta) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= Bp) return;
    float ss = 0.0f;
    if (b < B)
        for (int c = lane; c < H; c += 64) { const float x = rep[(size_t)b * H + c]; ss = fmaf(x, x, ss); }
    ss = wave_sum(ss);
    if (lane == 0) delta[b] = RANK_X3_KAPPA * (sqrtf(ss) * RANK_NORM_UP) * emax[0];
}

// k_lx3k: k_lx3g's blocking, staging and S^T phase (128 batch rows per workgroup, 32 per wave, rep fragments in registers, the fp32
// table streamed in 32-item blocks through the three-buffer hi/lo block image, three v_mfma_f32_32x32x16_bf16 per k-step) without the
// softmax and the readout.  Lane (r32, hh) holds batch row b0 + r32 and the 16 items acc_row(j, hh) of the block: the band test is
// lane-local, the count stays in a register over the whole item range and leaves as ONE integer atomicAdd per row and workgroup
// (integer adds: the result does not depend on the order).  List slots are reserved with an atomic add on diag[0] and written with
// ordinary stores while slot < cap; a lane that has seen the list full stops asking (the counter is beyond cap by then: overflow).
// Register plan: rep fragments 80, S 16, one block in flight 24, operand sets 16, row state and addressing ~20; 200 compiled, no
// scratch.  That would admit two waves per SIMD with room to spare, but the three block images (3 x 22.5 KiB of the CU's 160 KiB of
// LDS) admit two workgroups per CU whatever the registers: the bound is k_lx3g's (256, 2), and a tighter one would only buy spills.
__global__ __launch_bounds__(256, 2) void k_lx3k(RankX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // [3 buffers][block image]
    G3_WG_MAP(a.ranges, a.Bp / G3_ROWS)
    const int H = a.H, N = a.N;
    G3_WG_BLOCKS(a.ranges, N, N)
    G3_REP_FRAGS()
    // this lane's batch row: live items [0, nc) without the target; the band around its exact target logit
    const int b = b0 + r32;
    const int nc = min(a.ncol[b], N), tgt = a.target[b] - 1;
    const float tl = a.tlogit[b], dl = a.delta[b];
    const float s_hi = tl + dl, s_lo = tl - dl;
    int cnt = 0;
    bool full = false;
    F3_LOCALS()
    G3_A_OFF()
    F3_WALK_BEGIN()
        unsigned band = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int it = i0 + acc_row(j, hh);
            const bool live = it < nc && it != tgt;
            const bool above = S[j] > s_hi, below = S[j] < s_lo;
            cnt += (live && above) ? 1 : 0;
            band |= (live && !above && !below) ? (1u << j) : 0u;       // (a NaN logit is undecided too: the recheck treats it as the exact kernel does)
        }
        if (band && !full) {                               // rare: ~2 KAPPA sqrt(H / 2 pi) of the pairs for Gaussian-like operands
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((band >> j) & 1u) {
                    const int sl = atomicAdd(a.diag, 1);
                    if (sl < a.cap) {
                        int* c = a.cand + 3 * (size_t)sl;
                        c[0] = b; c[1] = i0 + acc_row(j, hh); c[2] = __float_as_int(S[j]);
                    } else full = true;
                }
        }
    F3_WALK_END()
    cnt += __shfl_xor(cnt, 32, 64);                        // the two half-waves hold different items of the same batch row
    if (hh == 0 && cnt) atomicAdd(a.rank + b, cnt);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Top-K recommendation on the bf16 matrix cores, byte-identical to ader_topk_items (k_topk_tile + k_topk_merge, topk.hip): the same
// items in the same order (score descending, id ascending) and the same float32 score bits, by construction and not by tolerance.
// k_lx3t computes every catalog logit at x3 grade (s3) and keeps, per row, a small SUPERSET of the exact top-k; k_topk3_finish merges
// the ranges' sets, recomputes the kept (row, item) pairs on the exact chain and selects the best k by the exact key.
//
// Why it is exact.  s = exact-chain score, s3 = x3 score, d = delta_b = KAPPA |rep_b| Emax (norms rounded up: k_rank_delta's value, the
// derivation above), so |s3 - s| < d / 2.  Let t3 be the k-th largest s3 over ANY subset U of the row's live items that holds >= k.
//   1. The k items of U with s3 >= t3 each have s > t3 - d/2: the row's exact k-th best score is >= t3 - d/2.
//   2. Any item of the exact top-k therefore has s3 > t3 - d.
//   3. So C = {n : !(s3_n < t3 - d)} contains the exact top-k -- for the running t3 of any prefix of the catalog and for the final one
//      (t3 only grows as U grows, and every C is cut with a t3 of a subset of the live items).
//   4. Every member of C outside the exact top-k has a smaller exact key than every member inside it: the best k of C by the exact
//      64-bit key (topk_key of the exact score and id, a total order) ARE the answer.
// The test is written !(s3 < lo): a NaN edge keeps everything.  The edge lo = t3 - d is computed in float32; its rounding
// (<= 2^-24 (|t3| + d) <= 2^-10.9 d, as for the rank filter's edges) is inside KAPPA's factor of two over the derived 2^-14.1.
// Where the guarantee cannot be given the row is marked in status[b] and the caller takes ader_topk_items' answer for it: a kept set
// larger than k + band keys (ties or near-ties across rank k: a constant row, a zero rep row), or a NaN s3 (non-finite operands: the
// error bound says nothing about them).
//
// k_lx3t: k_lx3k's blocking, staging and S^T phase; after each block a lane holds 16 x3 scores of its row and runs k_topk_tile's
// filter / append / compact on keys of (order-preserving s3 bits, complemented id), with one change: a compaction keeps EVERY key with
// !(s3 < t3 - d), t3 = the score of the k-th best key, not "the best k".  Per row: a buffer of k + band + 32 keys, its count (LDS), its
// lower edge lo and its overflow flag (registers of the lane pair that owns the row).  A wave owns its 32 rows' buffers outright -- both
// lanes that append to a row and the 64 lanes that compact it belong to it -- so compaction is decided by a wave ballot, with no
// workgroup barrier, and one wave's LDS operations are performed in order.
// INVARIANT: every row enters a block with cnt <= keep = k + band; a 32-item block proposes at most 32 keys per row; every row with
// cnt > keep is compacted to <= keep before the next block (more than keep inside the band: overflow, cut to the best keep): cnt <=
// keep + 32 = the buffer's size, always -- also when every item beats the threshold (scores increasing with the id).
// LDS: the three block images (67.5 KiB) + 128 rows x (keep + 32) keys x 8 B.  At k = 20, band = 16 that is 135.5 KiB: one workgroup
// per CU whatever k (two would need the buffers in 12.5 KiB = 12 keys per row).  Taken as it is: a retry loop with a smaller slack costs
// a workgroup barrier per block, and 64-row workgroups halve the flops per staged table byte; what it costs -- one wave per SIMD, no
// second workgroup to hide the barriers and the compactions -- is measured (0.60 of k_topk_tile at N = 10^6, 1.5 - 2.4 x
// it at the shipped catalogs, where a workgroup walks ~25 - 42 blocks and its rows' edges are loose for most of them).  160 KiB bounds
// keep + 32 <= 88: TK3_KMAX = 40 with band <= 16; a larger k takes the f32 kernels.  Registers: k_lx3k's plan + ~12 of row state
// (212 compiled, no scratch).
#define TK3_KMAX 40
#define TK3_BANDMAX 16

struct TopkX3Args {
    const float* rep; const float* emb1; int vrows; // fp32 rep [B,H]; fp32 table, row of item 1; rows available from it (item_num)
    const bf16* rep_hi; const bf16* rep_lo;         // [Bp][LDR] (k_lx3_prep)
    int B, Bp, H, N, ranges, k, keep;               // keep = k + band
    const int* ncol;                                // [Bp] N for real rows, 0 for padding rows
    const int* seen; int seen_ld;                   // [B, seen_ld] 1-based ids never to be returned (0 = none), or NULL
    const float* delta;                             // [Bp] band width d (k_rank_delta)
    u64* part3;                                     // [ranges][Bp][keep] kept x3 keys, zeros behind a row's count
    int* status;                                    // [Bp] != 0: the row's result is not guaranteed (zeroed by the launcher)
    int* diag;                                      // [0] kept pairs, [1] overflowed rows, [2] float bits of max |s3 - s| / d
    int* items; float* scores;                      // [B,k]
};

__global__ __launch_bounds__(256, 1) void k_lx3t(TopkX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];      // [3 buffers][block image] | buf [128][keep + 32] | cnt [128]
    G3_WG_MAP(a.ranges, a.Bp / G3_ROWS)
    const int H = a.H, N = a.N;
    G3_WG_BLOCKS(a.ranges, N, N)
    const int k = a.k, keep = a.keep, ldb = keep + FB;
    u64* buf = (u64*)(smem_raw + 3 * X3B_IMG_B);
    int* cnt = (int*)(buf + G3_ROWS * ldb);
    if (tid < G3_ROWS) cnt[tid] = 0;
    G3_REP_FRAGS()
    // this lane's batch row (shared with lane ^ 32, which holds the block's other 16 items): live items [0, nc) without the seen ids
    const int b = b0 + r32, wrow = wave * 32 + r32;
    const int nc = min(a.ncol[b], N);
    const float dl = a.delta[b];
    u64* mybuf = buf + wrow * ldb;
    int* mycnt = cnt + wrow;
    float lo = -INFINITY;                                  // the row's lower edge t3 - d at its last compaction
    int ovf = 0;
    // seen ids: the lane pair folds the row's ids that fall into the block into a 32-bit mask; rows without an id in this item range
    // (most, when the range is a small part of the catalog) never look again
    const int* srow = (a.seen && b < a.B) ? a.seen + (size_t)b * a.seen_ld : nullptr;
    int any_seen = 0;
    if (srow)
        for (int t = hh; t < a.seen_ld; t += 2)
            any_seen |= (unsigned)(srow[t] - 1 - blk_begin * FB) < (unsigned)(nb_blocks * FB);        // id 0 wraps: never inside
    any_seen |= __shfl_xor(any_seen, 32, 64);
    F3_LOCALS()
    G3_A_OFF()
    F3_WALK_BEGIN()
        unsigned sm = 0u;                                  // bit i: item i0 + i is in the row's seen list
        if (any_seen)
            for (int t = hh; t < a.seen_ld; t += 2) {
                const unsigned d = (unsigned)(srow[t] - 1 - i0);
                if (d < (unsigned)FB) sm |= 1u << d;
            }
        sm |= __shfl_xor(sm, 32, 64);
        // filter + append: a key goes in unless its x3 score is provably outside the band below the row's running k-th best
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int il = acc_row(j, hh);
            const float s = S[j];
            if (i0 + il < nc && !((sm >> il) & 1u) && !(s < lo)) {
                if (s != s) ovf = 1;                       // a NaN x3 score: the bound does not cover it
                else {
                    const int p = atomicAdd(mycnt, 1);     // p < keep + 32 (the invariant above)
                    mybuf[p] = topk_key(s, i0 + il + 1);
                }
            }
        }
        // compact: the wave's rows that hold more than keep keys, one after the other, all 64 lanes on a row
        const u64 need = __ballot(*mycnt > keep);
        unsigned rows = (unsigned)need | (unsigned)(need >> 32);
        while (rows) {
            const int rr = __ffs(rows) - 1;
            rows &= rows - 1;
            u64* bp = buf + (wave * 32 + rr) * ldb;
            const int n = cnt[wave * 32 + rr];             // keep < n <= keep + 32 <= 88: at most two keys per lane
            const u64 e0 = lane < n ? bp[lane] : 0, e1 = lane + 64 < n ? bp[lane + 64] : 0;
            // keys of a row are distinct: rank = number of larger keys.  The keys are broadcast from the lanes that hold them (the index
            // is wave-uniform: v_readlane), not read back from LDS one by one: with one wave per SIMD nothing hides that latency
            const unsigned e0l = (unsigned)e0, e0h = (unsigned)(e0 >> 32), e1l = (unsigned)e1, e1h = (unsigned)(e1 >> 32);
            int r0 = 0, r1 = 0;
            for (int q = 0; q < min(n, 64); ++q) {
                const u64 x = ((u64)(unsigned)__builtin_amdgcn_readlane((int)e0h, q) << 32) | (unsigned)__builtin_amdgcn_readlane((int)e0l, q);
                r0 += x > e0; r1 += x > e1;
            }
            for (int q = 64; q < n; ++q) {
                const u64 x = ((u64)(unsigned)__builtin_amdgcn_readlane((int)e1h, q - 64) << 32) | (unsigned)__builtin_amdgcn_readlane((int)e1l, q - 64);
                r0 += x > e0; r1 += x > e1;
            }
            // t3 = the score of the key of rank k - 1 (n > keep >= k: there is one), from the lane that holds it
            const u64 h0 = __ballot(lane < n && r0 == k - 1), h1 = __ballot(lane + 64 < n && r1 == k - 1);
            const u64 tk = h0 ? __shfl(e0, __ffsll(h0) - 1, 64) : __shfl(e1, __ffsll(h1) - 1, 64);
            const float nlo = topk_score(tk) - __shfl(dl, rr, 64);
            // no key is a NaN, so the kept keys are the head of the sorted order: a kept key's rank is its new place
            const bool k0 = lane < n && !(topk_score(e0) < nlo), k1 = lane + 64 < n && !(topk_score(e1) < nlo);
            const int m = __popcll(__ballot(k0)) + __popcll(__ballot(k1));
            // in place: every key was read into a register before the first store, and one wave's LDS operations are performed in order
            if (k0 && r0 < keep) bp[r0] = e0;
            if (k1 && r1 < keep) bp[r1] = e1;
            if (lane == 0) cnt[wave * 32 + rr] = min(m, keep);
            if (r32 == rr) { lo = nlo; ovf |= m > keep; }  // more than keep keys inside the band: the row's result is discarded
        }
    F3_WALK_END()
    ovf |= __shfl_xor(ovf, 32, 64);
    if (hh == 0 && ovf) atomicOr(a.status + b, 1);
    u64* o = a.part3 + ((size_t)range * a.Bp + b0) * keep;  // the wave's 32 rows (an empty range writes zeros: no candidate)
    for (int i = lane; i < 32 * keep; i += 64) {
        const int row = i / keep, j = i - row * keep;
        o[i] = j < cnt[wave * 32 + row] ? buf[(wave * 32 + row) * ldb + j] : 0;
    }
}

// One workgroup per real row: (1) the keys of the ranges' lists with !(s3 < t3 - d), t3 = the k-th best s3 over all of them, by
// k_topk_merge's filter / append / compact over batches of 256 keys with k_lx3t's keep rule (buffer keep + 256; more than keep
// inside the band: the row is marked overflowed); (2) the kept pairs through the exact chain, as k_pair_logit_rank does: 16 pairs per
// wave in the [rows][LDE] layout, mma_tile<1>'s k-order, the diagonal -- the float32 ader_logits_store writes for that pair, whatever
// its tile neighbours (here: the row's own rep in every column); (3) the best k by topk_key(exact score, id), unpacked as k_topk_merge does.  Every output is a function of
// sorted keys; LDS and global atomics only hand out slots and add up the diagnostics.
__global__ __launch_bounds__(256) void k_topk3_finish(TopkX3Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* E_l = smem;                                     // [keep rounded up to 16][LDE] table rows of the kept pairs
    float* R_l = E_l + ((a.keep + 15) & ~15) * LDE;        // [LDE] the row's rep: every pair's second operand (column stride 0)
    __shared__ u64 mb[TK3_KMAX + TK3_BANDMAX + 256];
    __shared__ u64 ek[64];
    __shared__ float mlo;
    __shared__ int mcnt, movf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int k = a.k, keep = a.keep, total = a.ranges * keep;
    const float d = a.delta[b];
    if (tid == 0) { mlo = -INFINITY; mcnt = 0; movf = a.status[b] != 0; }
    __syncthreads();
    for (int base = 0; base <= total; base += 256) {       // the pass at base >= total appends nothing: the final, sorting compaction
        const int i = base + tid;
        const bool last = base + 256 > total;
        u64 key = 0;
        if (i < total) { const int rg = i / keep; key = a.part3[((size_t)rg * a.Bp + b) * keep + (i - rg * keep)]; }
        int over = 0;
        if (key != 0 && !(topk_score(key) < mlo)) { const int p = atomicAdd(&mcnt, 1); mb[p] = key; over = (p >= keep); }
        if (__syncthreads_or(over | last)) {
            const int n = mcnt;                            // n <= keep + 256 <= 312: at most two keys per thread
            const u64 e0 = tid < n ? mb[tid] : 0, e1 = tid + 256 < n ? mb[tid + 256] : 0;
            int r0 = 0, r1 = 0;
#pragma unroll 8
            for (int j = 0; j < n; ++j) { const u64 x = mb[j]; r0 += x > e0; r1 += x > e1; }      // (unrolled: eight reads in flight)
            __syncthreads();
            if (tid < n && r0 == k - 1) mlo = topk_score(e0) - d;          // (fewer than k keys so far: the edge stays where it is)
            if (tid + 256 < n && r1 == k - 1) mlo = topk_score(e1) - d;
            __syncthreads();
            const float lo = mlo;
            const bool k0 = tid < n && !(topk_score(e0) < lo), k1 = tid + 256 < n && !(topk_score(e1) < lo);
            const int m = __syncthreads_count(k0) + __syncthreads_count(k1);
            if (k0 && r0 < keep) mb[r0] = e0;
            if (k1 && r1 < keep) mb[r1] = e1;
            if (tid == 0) { mcnt = min(m, keep); if (m > keep) movf = 1; }
            __syncthreads();
        }
        if (last) break;
    }
    const int n = mcnt;                                    // <= keep <= 56: one pass of 64 pairs
    if (movf) {                                            // (workgroup-uniform) the caller replaces this row
        if (tid == 0) { a.status[b] = 1; atomicAdd(a.diag + 1, 1); }
        for (int j = tid; j < k; j += 256) { a.items[(size_t)b * k + j] = 0; a.scores[(size_t)b * k + j] = -INFINITY; }
        return;
    }
    const int H = a.H, ksteps = (H + 3) >> 2;
    for (int i = tid; i < ((n + 15) & ~15) * LDE; i += 256) {
        const int r = i / LDE, c = i - r * LDE;
        E_l[i] = (r < n && c < H) ? a.emb1[(size_t)(topk_item(mb[r]) - 1) * H + c] : 0.0f;
    }
    for (int c = tid; c < LDE; c += 256) R_l[c] = c < H ? a.rep[(size_t)b * H + c] : 0.0f;
    __syncthreads();
    f32x4 acc[1];
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (wave * 16 < n)                                     // (wave-uniform) the same fma chain in k order whatever the neighbours
        mma_tile<1>(E_l + wave * 16 * LDE, LDE, 1, R_l, 1, 0, ksteps, acc, lane);
    const int col = lane & 15, q = lane >> 4;
    const int p = wave * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (q * 4 + r == col) {
            u64 e = 0;
            if (p < n) {
                const float s = acc[0][r], s3 = topk_score(mb[p]);
                e = topk_key(s, topk_item(mb[p]));
                const float err = d > 0.0f ? fabsf(s3 - s) / d : 0.0f;
                if (err > 0.0f) atomicMax(a.diag + 2, __float_as_int(err));
            }
            ek[p] = e;
        }
    __syncthreads();
    if (tid == 0) atomicAdd(a.diag, n);
    if (tid < n) {
        const u64 e = ek[tid];
        int r = 0;                                         // exact keys of a row are distinct: rank = number of larger keys
        for (int j = 0; j < n; ++j) r += ek[j] > e;
        if (r < k) { a.items[(size_t)b * k + r] = topk_item(e); a.scores[(size_t)b * k + r] = topk_score(e); }
    }
    for (int j = n + tid; j < k; j += 256) { a.items[(size_t)b * k + j] = 0; a.scores[(size_t)b * k + j] = -INFINITY; }
}

// in logits.hip: the exact-f32 target logits (k_target_logit) and the recheck of the listed pairs (k_pair_logit_rank)
int rank_target_logit_launch(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                             float* tlogit, void* stream);
int rank_pairs_launch(const float* rep, const float* emb, int B, int Bp, int H, int N, const int* target, const int* ncol,
                      const float* tlogit, const float* delta, const int* cand, int cap, int* diag, int* rank, void* stream);

extern "C" {

// emax[0] = max_n |E_n|_2 over items 1..N, rounded up: once per ranking call (after the table is final), not per chunk
int ader_rank_emax(const float* emb, int item_num, int H, int N, float* emax, void* stream) {
    if (N < 1 || N > item_num || H < 1 || H > HP) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(emax, 0, sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    const int g = (N + 3) / 4 < 2048 ? (N + 3) / 4 : 2048;
    hipLaunchKernelGGL(k_rank_emax, dim3(g), dim3(256), 0, st, emb + H, H, N, emax);
    HIP_LAUNCH_CHECK();
    return 0;
}

// ader_rank_targets on the bf16 matrix cores: the SAME ranks, ties included, wherever diag[0] <= cap afterwards (else the list
// overflowed: rank is short of the dropped pairs and the caller ranks the chunk with ader_rank_targets).  Bp % 128 == 0, Bp <= 1024,
// H as lx3f_supports (else -2).  Scratch: rep_hi, rep_lo Bp*168 bf16; tlogit, delta Bp floats; cand 3*cap ints; diag 2 ints.
int ader_rank_targets_x3(const float* rep, const float* emb, int item_num, int B, int Bp, int H, int N, const int* target,
                         const int* ncol, void* rep_hi, void* rep_lo, float* tlogit, float* delta, const float* emax, int* cand, int cap,
                         int* diag, int* rank, void* stream) {
    if (B <= 0) return 0;
    if (!x3_filter_shapes_ok(emb, item_num, B, Bp, H, N) || cap < 0) return -2;
    if (int e = ader_dyn_lds<k_lx3k>(3 * X3B_IMG_B)) return e;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(rank, 0, sizeof(int) * (size_t)Bp, st);
    if (e == hipSuccess) e = hipMemsetAsync(diag, 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (int rc = ader_lx3_prep(rep, rep_hi, rep_lo, B, Bp, H, stream)) return rc;
    if (int rc = rank_target_logit_launch(rep, emb, B, Bp, H, N, target, ncol, tlogit, stream)) return rc;
    hipLaunchKernelGGL(k_rank_delta, dim3(Bp / 4), dim3(256), 0, st, rep, B, Bp, H, emax, delta);
    RankX3Args a = {};
    a.emb1 = emb + H; a.vrows = item_num; a.rep_hi = (const bf16*)rep_hi; a.rep_lo = (const bf16*)rep_lo;
    a.Bp = Bp; a.H = H; a.N = N; a.ranges = ader_lbf_ranges(N, Bp);
    a.target = target; a.ncol = ncol; a.tlogit = tlogit; a.delta = delta; a.cand = cand; a.cap = cap; a.diag = diag; a.rank = rank;
    hipLaunchKernelGGL(k_lx3k, x3_grid(a.ranges, Bp), dim3(256), 3 * X3B_IMG_B, st, a);
    HIP_LAUNCH_CHECK();
    return rank_pairs_launch(rep, emb, B, Bp, H, N, target, ncol, tlogit, delta, cand, cap, diag, rank, stream);
}

// ader_topk_items on the bf16 matrix cores (k_lx3t + k_topk3_finish above).  ader_topk_x3_ranges: item ranges per 128-row chunk -- about
// one workgroup per CU over the Bp/128 chunks (every range emits k + band keys per row, so no more of them than fill the machine), a
// multiple of 8 (the block -> (range, chunk) mapping), so it may exceed the number of 32-item blocks: such ranges are empty.
int ader_topk_x3_kmax(void) { return TK3_KMAX; }
int ader_topk_x3_ranges(int N, int Bp) {
    const int nblk = (N + FB - 1) / FB;
    const int nchunk = Bp / G3_ROWS > 0 ? Bp / G3_ROWS : 1;
    int target = 256 / nchunk / 8 * 8;
    if (target < 8) target = 8;
    int r = (nblk + 7) / 8 * 8;
    if (r > target) r = target;
    if (r < 8) r = 8;
    return r;
}
// items / scores [B,k]: ader_topk_items' output, byte for byte, for every row with status[b] == 0 afterwards; a row with status[b] != 0
// (its kept set outgrew k + band keys, or an x3 score was a NaN) holds item 0 / -inf and the caller takes ader_topk_items' answer for it.
// emax: ader_rank_emax's output (once per call, after the table is final).  Scratch: rep_hi, rep_lo Bp*168 bf16; delta Bp floats; part3
// ader_topk_x3_ranges(N,Bp) * Bp * (k + band) keys.  status [Bp] and diag [3] are zeroed here.  Enqueue only.
int ader_topk_items_x3(const float* rep, const float* emb, int item_num, int B, int Bp, int H, int N, const int* ncol, const int* seen,
                       int seen_ld, int k, int band, void* rep_hi, void* rep_lo, float* delta, const float* emax,
                       unsigned long long* part3, int* status, int* diag, int* items, float* scores, void* stream) {
    if (k < 1 || k > TK3_KMAX || band < 0 || band > TK3_BANDMAX || !x3_filter_shapes_ok(emb, item_num, B, Bp, H, N) || (seen && seen_ld < 1))
        return -2;
    if (B <= 0) return 0;
    TopkX3Args a = {};
    a.rep = rep; a.emb1 = emb + H; a.vrows = item_num; a.rep_hi = (const bf16*)rep_hi; a.rep_lo = (const bf16*)rep_lo;
    a.B = B; a.Bp = Bp; a.H = H; a.N = N; a.ranges = ader_topk_x3_ranges(N, Bp); a.k = k; a.keep = k + band;
    a.ncol = ncol; a.seen = seen; a.seen_ld = seen_ld; a.delta = delta; a.part3 = part3; a.status = status; a.diag = diag;
    a.items = items; a.scores = scores;
    const size_t lds = 3 * X3B_IMG_B + (size_t)G3_ROWS * (a.keep + FB) * sizeof(u64) + G3_ROWS * sizeof(int);
    const size_t lds_fin = (size_t)((((a.keep + 15) & ~15) + 1) * LDE) * sizeof(float);
    if (int e = ader_dyn_lds<k_lx3t>(lds)) return e;
    if (int e = ader_dyn_lds<k_topk3_finish>(lds_fin)) return e;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)Bp, st);
    if (e == hipSuccess) e = hipMemsetAsync(diag, 0, 3 * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (int rc = ader_lx3_prep(rep, rep_hi, rep_lo, B, Bp, H, stream)) return rc;
    hipLaunchKernelGGL(k_rank_delta, dim3(Bp / 4), dim3(256), 0, st, rep, B, Bp, H, emax, delta);
    hipLaunchKernelGGL(k_lx3t, x3_grid(a.ranges, Bp), dim3(256), lds, st, a);
    hipLaunchKernelGGL(k_topk3_finish, dim3(B), dim3(256), lds_fin, st, a);
    HIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
