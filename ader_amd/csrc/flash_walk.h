// The flash forward of the logit kernels, the pieces that do not depend on how a table block lies in LDS: stated once for every
// grade and layout (logits_bf16.hip: k_lbf_fwd and its teacher readout on bf16 rows, k_lx3_fwd on hi/lo rows; logits_x3.hip: k_lx3g /
// k_lx3p / k_lx3r and the filters on the block images).  Reference: ADER.py:88-93, ADER.py:132-137.
//
// A workgroup = (item range, 128-row chunk) on one XCD, 32 batch rows per wave on v_mfma_f32_32x32x16_bf16; the range's 32-item
// blocks are streamed through LDS, and per block S^T = E.rep^T, the online softmax (FW_SOFTMAX_HEAD, FW_EXP_SUM), and the
// probabilities as the A operand of O += P^T.E (FW_PSPLIT).  Staging, operand reads and the MFMA phases are the including file's.
//
// Every piece is a macro over the kernel's locals, expanded in the kernel, and not a function: as functions the MFMA kernels compile
// to other instruction streams (profiles/logits_x3_refactor_isa.txt, profiles/flash_walk_refactor.txt).  Names a piece expects in
// scope are the ones the pieces before it define; the lane's batch row of the wave is r32 = lane & 31, its half hh = lane >> 5.
#pragma once
#include "lbf_common.h"

#define FB 32                      // items per streamed block

// ---- workgroup prologue.  FW_XCD_MAP: block -> (item range `range`, row chunk `bc` of nchunk_).  The row chunks of an item range
// sit on one XCD: the table block is fetched from HBM once and served to the others by that XCD's L2
#define FW_XCD_MAP(ranges_, nchunk_)                                                                      \
    const int nchunk = (nchunk_);                                                                         \
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;                                               \
    const int range = xcd + 8 * (slot / nchunk);                                                          \
    const int bc = slot % nchunk;                                                                         \
    if (range >= (ranges_)) return;
// FW_WG_SPAN: the range's span [blk_begin, blk_end) of the ncat_ items' 32-item blocks (the ranges partition the blocks of ncat_
// items), cut at the ncol_ columns these rows see; nb_blocks of them
#define FW_WG_SPAN(ranges_, ncat_, ncol_)                                                                 \
    const int nblk_all = ((ncat_) + FB - 1) / FB;                                                         \
    const int per = (nblk_all + (ranges_) - 1) / (ranges_);                                               \
    const int blk_begin = range * per, blk_end = min(((ncol_) + FB - 1) / FB, blk_begin + per);           \
    const int nb_blocks = max(0, blk_end - blk_begin);

// ---- the online softmax's head of block i0 (logits S of the chunk's N columns; running m_run, l_run, O): tail mask, running
// maximum, (rare) rescale of l and O.  Leaves nm = -m_run and the block's sum ls = 0 for the exp that follows.
// The two half-waves of a lane pair (l, l + 32) hold different items of the SAME batch row; m_run is kept equal in both, so the
// cross-half exchange is only needed on the (rare) rescale path
#define FW_SOFTMAX_HEAD()                                                                                 \
        if (i0 + FB > N) {                                 /* tail block: items >= N are outside the softmax */ \
            _Pragma("unroll") for (int j = 0; j < 16; ++j) if (i0 + acc_row(j, hh) >= N) S[j] = -INFINITY; \
        }                                                                                                 \
        float tmax = S[0];                                                                                \
        _Pragma("unroll") for (int j = 1; j < 16; ++j) tmax = fmaxf(tmax, S[j]);                          \
        float t2 = tmax * LOG2E;                                                                          \
        if (__any(t2 > m_run + RESCALE_THR)) {                                                            \
            t2 = fmaxf(t2, __shfl_xor(t2, 32, 64));                                                       \
            const float m_new = (t2 > m_run + RESCALE_THR) ? t2 : m_run;                                  \
            const float alpha = (m_new == -INFINITY) ? 1.0f : __builtin_amdgcn_exp2f(m_run - m_new);      \
            l_run *= alpha;                                                                               \
            m_run = m_new;                                                                                \
            _Pragma("unroll") for (int j = 0; j < 16; ++j) {                                              \
                const float ar = __shfl(alpha, acc_row(j, hh), 64);     /* O rows are batch rows */       \
                _Pragma("unroll") for (int nb = 0; nb < 5; ++nb) O[nb][j] *= ar;                          \
            }                                                                                             \
        }                                                                                                 \
        const float nm = -m_run;                                                                          \
        float ls = 0.0f;
// ... and the plain form of what follows it: S = the probabilities 2^(s log2e - m_run), their sum in element order into l_run
#define FW_EXP_SUM()                                                                                      \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) { S[j] = __builtin_amdgcn_exp2f(fmaf(S[j], LOG2E, nm)); ls += S[j]; } \
        l_run += ls;

// ---- the readout accumulator O (32 rows x 160 channels per wave) and the probabilities in S as its A operands: FW_PPACK pa0 / pa1
// (bf16 grade: hi only), FW_PSPLIT also pl0 / pl1 (lo)
#define FW_O_ZERO()                                                                                       \
    f32x16 O[5];                                                                                          \
    _Pragma("unroll") for (int nb = 0; nb < 5; ++nb)                                                      \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) O[nb][j] = 0.0f;
#define FW_PPACK() const bf16x8 pa0 = pack8(S, 0), pa1 = pack8(S, 1);
#define FW_PSPLIT()                                                                                       \
        FW_PPACK()                                                                                        \
        bf16x8 pl0, pl1;                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) { pl0[j] = (bf16)(S[j] - (float)pa0[j]); pl1[j] = (bf16)(S[8 + j] - (float)pa1[j]); }

// ---- epilogues: the wave's 32 rows of O to o_ [rows][HP]; a forward's (m, l) partials of its range
#define FW_STORE_O(o_)                                                                                    \
    {                                                                                                     \
        float* o = (o_);                                                                                  \
        _Pragma("unroll") for (int nb = 0; nb < 5; ++nb)                                                  \
            _Pragma("unroll") for (int j = 0; j < 16; ++j) o[(size_t)acc_row(j, hh) * HP + 32 * nb + r32] = O[nb][j]; \
    }
#define FW_STORE_ML()                                                                                     \
    {                                                                                                     \
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);                                            \
        if (hh == 0) {                                                                                    \
            a.pm[(size_t)range * a.Bp + b0 + r32] = m_run;                                                \
            a.pl[(size_t)range * a.Bp + b0 + r32] = l_tot;                                                \
        }                                                                                                 \
    }
