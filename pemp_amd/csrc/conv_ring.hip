// Split3 1x1 convs with fp32 activations and a long K on a THREE-deep activation ring (tile id 349; pemp_hip.h): the form of id 49
// (conv_dma2.hip: conv_dma2_s3p_body<256, 128, 8, 8>, persistent 256 x 128 tiles in 8 full-width wave strips) for the layers whose
// A operand is a pure HBM stream -- a 1x1 conv reads every activation line once, there are no tap re-reads that hit L2.
//
// Id 49's ring is two stages deep for both operands and its K step waits vmcnt(0): the last LDS-DMA piece issued under the second
// half of step kt has half a K step to land before the barrier of step kt + 1 drains it.  Here A has three stages, B keeps two:
//   * LDS: A [3][256][8] quads (fp32, the swizzle of conv_dma2.hip), B [2][128][12] quads (the packed split3 weights) = 147 456 B;
//   * behind the barrier of step s ("tail of s") a wave issues, one per MFMA slot of the step's second K16 slice, first the BL = 3
//     pieces of B(s + 2) into the B buffer step s has released and then the AL = 4 pieces of A(s + 3) into its A buffer -- in the
//     slice's first seven slots, in FRONT of the first fragment reads of step s + 1 (which have half a step to return): the DMAs'
//     landing window is what the next barrier waits for (measured: 1 .. 1.5 % over issuing them behind the 14 reads);
//   * vector memory operations of a wave retire in issue order, so the wait in front of a barrier is vmcnt(operations issued behind
//     the last one the next reads need).  The barrier of step s + 1 is followed by the first fragment reads of step s + 2: they need
//     A(s + 2), issued in the tail of s - 1, and B(s + 2), issued FIRST in the tail of s.  Behind B(s + 2) lie the AL pieces of
//     A(s + 3) and nothing else: ring_behind(RING_STEP) = AL.  A piece of A gets two K steps to land, a piece of B one;
//   * a stage is read one phase after the wait that retires it (wait, raw s_barrier, then the reads), and rewritten behind the
//     barrier that follows its last reads (those are retired by the lgkmcnt(0) of that wait).  Raw s_barrier throughout: a
//     __syncthreads() would drain the DMAs in flight.
//
// What the 1x1 / pad 0 restriction drops against id 49: tap state, tap masks, the padding vector and the scalar tap arithmetic of
// the K step -- a row's byte offset (stride inside it) is all a DMA needs, the K step only adds 128 bytes to the scalar offset.  A
// row behind M carries the offset 2^31: the descriptor's range check writes zeros and reads no memory (conv_dma2.hip's mechanism).
//
// Tile walk (XcdTileRange, conv_common.h; no counter, flag or atomic).  Steps are numbered THROUGH the walk: A(s) lives in A buffer
// s mod 3, B(s) in B buffer s mod 2, and the issue schedule above simply runs on into the next tile -- steps nk, nk + 1, nk + 2 of a
// tile ARE steps 0, 1, 2 of the next one.  With nk >= 4 K steps per tile, per tile:
//     tails of steps 0 .. nk - 4:  B(s + 2), A(s + 3) of this tile
//     -- the tile's last A piece is out: the row offsets become the next tile's --
//     tail of step nk - 3:         B(nk - 1), A'(0)
//     -- the tile's last B piece is out: the weight offsets become the next tile's --
//     tail of step nk - 2:         B'(0), A'(1)
//     step nk - 1:                 no tail, no next reads; its barrier waits for the LDS reads only, the next tile's stages fly on
//     epilogue:                    the scale / shift quads in one batch, the transpose patches in the A buffer the last step read
//                                  (one stage = 8 patches of 4 KB; A'(0), A'(1) and B'(0) are in the other buffers), NST stores
//     barrier, then the tail the last step did not issue: B'(1), A'(2) -- into the buffers of the last step
//     wait, barrier:               the first reads of the next tile need A'(0) and B'(0).  Behind B'(0): A'(1), the stores, B'(1),
//                                  A'(2): ring_behind(RING_FIRST) = AL + BL + AL (+ NST where the wave's rows are all inside M -- a
//                                  wave with rows behind M issues fewer stores and does not count them)
// From there the steady-state count holds again: the barrier of the next tile's step 0 needs A'(1) and B'(1), the AL pieces of
// A'(2) behind them may fly.  The block's first tile issues A(0), B(0), A(1), B(1), A(2) and waits ring_behind(RING_FIRST) without
// stores.  After the block's last tile the same DMAs go out with every offset at 2^31 (zeros into free buffers, no memory read): one
// form of the step, constant counts; they are drained before the block ends.
// (The epilogue's scale / shift quads are the youngest vector memory operations when they are needed, so waiting for them is a
// vmcnt(0) that also retires A'(0), A'(1) and B'(0) -- which hipcc places at their first use anyway; the kernel says it itself, for
// the waves that never use them.  A counted wait that finds less in flight than it allows returns at once: the counts above stay
// upper bounds, and the ring INSIDE a tile does not depend on it.)
//
// Arithmetic: the K16 slices ascending, per slice split3_bf16 of the A quads and split3_mma6's six products in its order, one
// accumulator per 32 x 32 sub-tile; the epilogue is conv_epilogue_s3p's (OUT 0: fp32, affine, per-image shift, ReLU, a channel
// window ldy != Cout; no residual -- none of the target layers has one, and its 16 quads are registers this kernel needs) or
// conv_epilogue_s3p_split's (OUT 1: PEMP_CONV_OUT_SPLIT3, the producer), statement for statement: BIT-IDENTICAL to ids 43 / 49.
#include "conv_tiles.h"

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int RING_BM = 256, RING_BN = 128, RING_NW = 8;
constexpr int RING_AQ = RING_BM * 8, RING_BQ = RING_BN * 12;                 // quads of one A / B stage
constexpr int RING_AL = RING_AQ / (RING_NW * 64), RING_BL = RING_BQ / (RING_NW * 64);      // DMA pieces per thread and stage: 4, 3
static_assert(RING_AQ % (RING_NW * 64) == 0 && RING_BQ % (RING_NW * 64) == 0, "whole DMA rounds");
constexpr size_t ring_lds() { return (size_t)(3 * RING_AQ + 2 * RING_BQ) * sizeof(v4f); }
static_assert(ring_lds() == 147456 && ring_lds() <= 160 * 1024, "LDS of a CU");
constexpr int RING_MIN_NK = 4;              // K steps per tile the walk needs (file header)

// Vector memory operations a wave has issued behind the last one a wait needs (the derivation in the file header).
//   RING_STEP:  in front of the barrier of a K step -- behind B(s + 2), the first of the tail, lie the pieces of A(s + 3)
//   RING_FIRST: in front of a tile's first fragment reads -- behind B'(0) lie A'(1), `stores` epilogue stores, B'(1), A'(2)
enum RingWait { RING_STEP, RING_FIRST };
constexpr int ring_behind(RingWait w, int stores = 0) { return w == RING_STEP ? RING_AL : RING_AL + stores + RING_BL + RING_AL; }

template <int OUT>
__global__ __launch_bounds__(RING_NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void conv_ring_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = RING_BM, BN = RING_BN, NW = RING_NW;
    constexpr int WM = BM / NW, TN = BN / 32;           // full-width wave strips: 32 rows x 128 columns, one row tile
    static_assert(WM == 32, "one 32-row strip per wave");
    constexpr int AL = RING_AL, BL = RING_BL, AQ = RING_AQ, BQ = RING_BQ;
    constexpr int NMF = 6 * TN, NDS = 2 + 3 * TN;       // per K16 slice: MFMAs, fragment reads
    static_assert(NDS + BL + AL <= NMF, "one LDS read / one DMA per MFMA slot");
    constexpr int NST = TN * (OUT == 0 ? 4 : 6);        // epilogue stores per thread of a wave tile inside the output
    static_assert(ring_behind(RING_FIRST, NST) <= 63, "vmcnt range");
    static_assert(NW * 256 <= AQ, "one 4 KB transpose patch per wave inside ONE A stage");

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                          // [3][BM][8]
    v4f* Bs = smem + 3 * AQ;                 // [2][BN][12]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = wave * WM;
    const int lr = lane & 31, lh = lane >> 5;

    // the block's tile sequence: tiles tr.first + j, j = tr.idx, tr.idx + tr.step, ... < tr.count
    const int ntn = a.Cout / BN;
    const XcdTileRange tr((a.M + BM - 1) / BM * ntn, (int)blockIdx.x, (int)gridDim.x);
    if (tr.idx >= tr.count) return;             // (the launch clamps the grid to the tile count: not expected)
    int j = tr.idx;
    int m0 = ((tr.first + j) / ntn) * BM, n0 = ((tr.first + j) % ntn) * BN;

    // loader role (conv_dma2.hip): thread (r, p) fetches, for rows r + 64 i, the quad that belongs at position p
    const int p = tid & 7;
    const int r = tid >> 3;
    const int sq = p ^ ((r >> 1) & 7);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);

    // per-tile byte offsets: conv_dma2_body's at pad 0 (ok_ false: behind the block's last tile, nothing reads memory)
    unsigned a_voff[AL], b_voff[BL];
    auto a_offsets = [&](const int m0_, const bool ok_) {
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int m = m0_ + r + NW * 8 * i;
            const bool in = ok_ && m < a.M;
            const int mm = in ? m : 0;
            const int img = mm / a.HoWo;
            const int rem = mm - img * a.HoWo;
            const int ho = rem / a.Wo;
            const int wo = rem - ho * a.Wo;
            a_voff[i] = in ? (unsigned)(((img * a.H + ho * a.stride) * a.W + wo * a.stride) * a.ldx + sq * 4) * 4u : 0x80000000u;
        }
    };
    auto b_offsets = [&](const int n0_, const bool ok_) {
#pragma unroll
        for (int i = 0; i < BL; ++i) {      // LDS quad q of the tile = row q / 12, position q % 12 = plane * 4 + (quad ^ ((row >> 2) & 3))
            const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
            const int src = PEMP_SPLIT3_SWZ(row, pos);
            b_voff[i] = ok_ ? (unsigned)((n0_ + row) * a.Kpad * 6 + src * 16) : 0x80000000u;
        }
    };
    a_offsets(m0, true);
    b_offsets(n0, true);
    const int nk = a.nk;

    // the AL pieces of A at K step k_ into the stage at quad offset ao_; the BL pieces of B likewise
#define PEMP_RING_DMA_A(ao_, k_)                                                                                  \
    do {                                                                                                          \
        const int so_ = __builtin_amdgcn_readfirstlane((k_) * 128);                                               \
        _Pragma("unroll") for (int i = 0; i < AL; ++i)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(As + (ao_) + i * NW * 64 + wave * 64), 16, a_voff[i], so_, 0, 0); \
    } while (0)
#define PEMP_RING_DMA_B(bo_, k_)                                                                                  \
    do {                                                                                                          \
        const int so_ = __builtin_amdgcn_readfirstlane((k_) * 192);                                               \
        _Pragma("unroll") for (int i = 0; i < BL; ++i)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bs + (bo_) + i * NW * 64 + wave * 64), 16, b_voff[i], so_, 0, 0); \
    } while (0)

    // fragment reads (conv_dma2.hip, S3): K16 slice j_ of a lane: fp32 quads 4 j + 2 lh and 4 j + 2 lh + 1 of its A row (position
    // quad ^ ((row >> 1) & 7)), quad 2 j + lh of each weight plane
    const int rsw = (lr >> 1) & 7;
    const int arow = (wm0 + lr) * 8;
    const int brow3 = lr * 12, bsw3 = (lr >> 2) & 3;
    v4f af3[2][2], bf3[2][TN][3];
#define PEMP_RING_READ(dst_, ao_, bo_, j_)                                                                        \
    do {                                                                                                          \
        const v4f* Ab_ = As + (ao_);                                                                              \
        const v4f* Bb_ = Bs + (bo_);                                                                              \
        const int p0_ = (4 * (j_) + 2 * lh) ^ rsw, p1_ = (4 * (j_) + 2 * lh + 1) ^ rsw;                           \
        const int pb_ = (2 * (j_) + lh) ^ bsw3;                                                                   \
        af3[dst_][0] = Ab_[arow + p0_];                                                                           \
        af3[dst_][1] = Ab_[arow + p1_];                                                                           \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                                         \
            _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                                      \
                bf3[dst_][ni][pl] = Bb_[brow3 + ni * 32 * 12 + pl * 4 + pb_];                                     \
    } while (0)

    // the K16 slice in registers src_: the row's split, then every accumulator's six products (split3_mma6's, in its order)
#define PEMP_RING_MMA(src_)                                                                                       \
    do {                                                                                                          \
        bf16x8 ah_, am_, al_;                                                                                     \
        split3_bf16(af3[src_][0], af3[src_][1], ah_, am_, al_);                                                   \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {                                                       \
            const bf16x8 bh_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][0]);                                      \
            const bf16x8 bm_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][1]);                                      \
            const bf16x8 bl_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][2]);                                      \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_, bh_, acc[ni], 0, 0, 0);                        \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, bl_, acc[ni], 0, 0, 0);                        \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, bm_, acc[ni], 0, 0, 0);                        \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_, bh_, acc[ni], 0, 0, 0);                        \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, bm_, acc[ni], 0, 0, 0);                        \
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_, bh_, acc[ni], 0, 0, 0);                        \
        }                                                                                                         \
    } while (0)

    // One K step on the stages (ao, bo); (an, bn): those of the next step.  TAIL_: behind the barrier B at K step kb into bo, then A
    // at K step ka into ao (both released by that barrier), and the first fragments of the next step; false: the tile's last step.
#define PEMP_RING_STEP(TAIL_)                                                                                     \
    do {                                                                                                          \
        PEMP_RING_READ(1, ao, bo, 1);                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PEMP_RING_MMA(0);                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        /* every LDS read of this step by this wave has returned; its pieces of what the next step reads have landed */ \
        __builtin_amdgcn_s_waitcnt(0xC07F);          /* lgkmcnt(0), visible to hipcc's own wait bookkeeping */    \
        if (TAIL_) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(ring_behind(RING_STEP)) : "memory");       \
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                   \
        __builtin_amdgcn_s_barrier();               /* ... everybody's */                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        if (TAIL_) {                                                                                              \
            PEMP_RING_DMA_B(bo, kb);                                                                              \
            PEMP_RING_DMA_A(ao, ka);                                                                              \
            PEMP_RING_READ(0, an, bn, 0);                                                                         \
        }                                                                                                         \
        PEMP_RING_MMA(1);               /* the second K16 slice covers the DMA issue / reads above: one per MFMA slot, the DMAs */ \
        if (TAIL_) {                    /* first -- their window is what the next barrier waits for, the reads have a half step */ \
            _Pragma("unroll") for (int k_ = 0; k_ < NMF; ++k_) {                                                  \
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                \
                if (k_ < BL + AL) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                              \
                else if (k_ < BL + AL + NDS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                   \
            }                                                                                                     \
        }                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        {                               /* the ring moves on */                                                   \
            const int t_ = ao;                                                                                    \
            ao = an;                                                                                              \
            an = ann;                                                                                             \
            ann = t_;                                                                                             \
            const int u_ = bo;                                                                                    \
            bo = bn;                                                                                              \
            bn = u_;                                                                                              \
        }                                                                                                         \
    } while (0)

    // the block's first tile: A(0), B(0), A(1), B(1), A(2)
    int ao = 0, an = AQ, ann = 2 * AQ, bo = 0, bn = BQ;     // quad offsets of the stages: this step's, the next one's (A: and the one after)
    PEMP_RING_DMA_A(ao, 0);
    PEMP_RING_DMA_B(bo, 0);
    PEMP_RING_DMA_A(an, 1);
    PEMP_RING_DMA_B(bn, 1);
    PEMP_RING_DMA_A(ann, 2);
    {
        constexpr int V0 = ring_behind(RING_FIRST);
        __builtin_amdgcn_s_waitcnt((V0 & 15) | 0x0F70 | ((V0 >> 4) << 14));
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(V0) : "memory");                         // A(0), B(0) have landed
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    const int c4_ = (lane & 7) * 4;
    for (;;) {
        f32x16 acc[TN];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
        const int jn = j + tr.step;
        const bool more = jn < tr.count;
        const int m0n = more ? ((tr.first + jn) / ntn) * BM : m0, n0n = more ? ((tr.first + jn) % ntn) * BN : n0;

        // the epilogue's operands, requested in one batch behind the last step's MFMAs (under them they cost the producer variant
        // 7 spilled registers): the scale / shift quads of the lane's channels (OUT 0: conv_epilogue_s3p's; OUT 1: conv_store_split3_to's 8 channels per lane)
        v4f scv[OUT == 0 ? TN : 1], shv[OUT == 0 ? TN : 1], sc8[OUT == 0 ? 1 : TN][2], sh8[OUT == 0 ? 1 : TN][2];
        const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
        auto epi_loads = [&]() {
            if constexpr (OUT == 0) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int n = n0 + ni * 32 + c4_;
                    scv[ni] = a.scale ? *(const v4f*)(a.scale + n) : v4f{1.f, 1.f, 1.f, 1.f};
                    shv[ni] = (a.shift && !per_img) ? *(const v4f*)(a.shift + n) : v4f{0.f, 0.f, 0.f, 0.f};
                }
            } else {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) conv_split3_affine(a, n0 + ni * 32 + (lane & 3) * 8, sc8[ni], sh8[ni]);
            }
        };

        PEMP_RING_READ(0, ao, bo, 0);
        int ka = 3, kb = 2;                      // the K steps the next tail issues
        for (int kt = 0; kt + 3 < nk; ++kt) {
            PEMP_RING_STEP(true);
            ++ka;
            ++kb;
        }
        a_offsets(m0n, more);                    // the tile's last A piece is out: the row offsets become the next tile's
        ka = 0;
        PEMP_RING_STEP(true);                    // B(nk - 1), A'(0)
        b_offsets(n0n, more);                    // the tile's last B piece is out
        ka = 1;
        kb = 0;
        PEMP_RING_STEP(true);                    // B'(0), A'(1)
        const int al_ = ao, bl_ = bo;            // the last step's stages: the transpose patches go to that A stage
        PEMP_RING_STEP(false);                   // the barrier waits for the LDS reads only: the next tile's stages fly on
        epi_loads();

        // The quads have to be there (they are the youngest vector memory operations, so this also retires A'(0), A'(1) and B'(0),
        // which have had one to two K steps).  Said to hipcc's bookkeeping as well: a wave whose rows all lie behind M never uses them,
        // and a load still pending in that bookkeeping costs a vmcnt(0) in front of the next tile's first fragment reads
        __builtin_amdgcn_s_waitcnt(0x0F70);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        float* patch = (float*)(As + al_ + wave * 256);
        if constexpr (OUT == 0) {                // conv_epilogue_s3p without a residual and bf16 output
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) {
                PEMP_CONV_PATCH_PUT(patch, acc[ni], lr, lh);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
                conv_patch_store_f32(a, patch, m0 + wm0, n0 + ni * 32, lane, scv[ni], shv[ni], per_img, nullptr, 0u);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
            }
        } else {                                 // conv_epilogue_s3p_split without the second output
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) {
                PEMP_CONV_PATCH_PUT(patch, acc[ni], lr, lh);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                conv_store_split3_to(a, (unsigned short*)a.y, patch, m0 + wm0, n0 + ni * 32, lane, sc8[ni], sh8[ni]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
        if (!more) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no LDS-DMA outlives the block
            break;
        }

        // the tail the last step did not issue, once every wave is done with its patch: B'(1), A'(2) into the last step's stages
        __builtin_amdgcn_s_barrier();
        PEMP_RING_DMA_B(bl_, 1);
        PEMP_RING_DMA_A(al_, 2);
        // (the builtin form as well: hipcc's own bookkeeping then knows the epilogue's stores as retired and puts no vmcnt(0) of its own
        // in front of the next tile's first fragment reads)
        constexpr int VF = ring_behind(RING_FIRST, NST), VP = ring_behind(RING_FIRST);
        if (m0 + wm0 + WM <= a.M) {
            __builtin_amdgcn_s_waitcnt((VF & 15) | 0x0F70 | ((VF >> 4) << 14));
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VF) : "memory");                     // A'(0), B'(0) have landed
        } else {
            __builtin_amdgcn_s_waitcnt((VP & 15) | 0x0F70 | ((VP >> 4) << 14));
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VP) : "memory");                     // (fewer stores than NST: do not count them)
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        j = jn;
        m0 = m0n;
        n0 = n0n;
    }
#endif
}
#undef PEMP_RING_STEP
#undef PEMP_RING_MMA
#undef PEMP_RING_READ
#undef PEMP_RING_DMA_B
#undef PEMP_RING_DMA_A

// what the id takes: a 1x1 conv without padding (any stride) on fp32 activations with ldx >= Cin, K = Cin in at least RING_MIN_NK
// steps of 32, Cout in whole 128-column tiles; the fp32 output (affine, per-image shift, ReLU, a channel window) or
// PEMP_CONV_OUT_SPLIT3; no residual, second output, pre-split input, strided residual, padding vector, statistics, DropBlock, bf16,
// stem, split-K or workspace
bool conv_ring_supported(const ConvArgs& a) {
    if (a.flags & (PEMP_CONV_IN_SPLIT3 | PEMP_CONV_OUT_SPLIT3_ALSO | PEMP_CONV_RES_S2 | PEMP_CONV_RES_HEVEN | PEMP_CONV_RES_WEVEN | PEMP_CONV_STEM4 |
                   PEMP_CONV_POOL3S2 | PEMP_CONV_BF16_IO))
        return false;
    if (a.res || a.padv || a.stats || a.rowmask || a.sk_S > 1 || a.sk_ws || a.bm_first) return false;
    if (a.KH != 1 || a.KW != 1 || a.pad != 0 || a.stride < 1) return false;
    if (a.Cin % 32 || a.Kpad != a.Cin || a.nk != a.Kpad / 32 || a.nk < RING_MIN_NK || a.ldx < a.Cin || a.Cout % RING_BN) return false;
    if ((a.flags & PEMP_CONV_OUT_SPLIT3) && a.ldy != a.Cout) return false;
    return conv_dma2_supported(a) && (long long)a.Cout * a.Kpad * 6 < (1ll << 31);
}

int launch_conv_ring(const ConvArgs& a, hipStream_t st) {
    if (!conv_ring_supported(a)) {
        set_error("conv split3 ring: unsupported (needs a 1x1 conv without padding on fp32 activations, Kpad == Cin >= %d, Cout %% 128 == 0, "
                  "the fp32 or PEMP_CONV_OUT_SPLIT3 output without residual / second output / padding value / workspace)", 32 * RING_MIN_NK);
        return -1;
    }
    const int tiles = cdiv(a.M, RING_BM) * (a.Cout / RING_BN);
    static int occ[2] = {0, 0};          // blocks per CU of the two instantiations
    int grid = 0;
    if (a.flags & PEMP_CONV_OUT_SPLIT3) {
        const int rc = persistent_grid(conv_ring_kernel<1>, RING_NW * 64, ring_lds(), tiles, occ[1], "conv split3 ring", grid);
        if (rc) return rc;
        return launch_with_lds(conv_ring_kernel<1>, grid, RING_NW * 64, ring_lds(), st, a, "conv_ring/out_split3");
    }
    const int rc = persistent_grid(conv_ring_kernel<0>, RING_NW * 64, ring_lds(), tiles, occ[0], "conv split3 ring", grid);
    if (rc) return rc;
    return launch_with_lds(conv_ring_kernel<0>, grid, RING_NW * 64, ring_lds(), st, a, "conv_ring");
}

}  // namespace pemp
