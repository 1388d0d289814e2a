// Split3 3x3 convs on pre-split activations, one A stage for the three taps of a kernel row (tile ids 246 / 249; pemp_hip.h).
//
// Ids 146 / 149 (conv_dma2.hip, A3) walk K as channel chunk outer, tap inner, and DMA a fresh 256-row A stage for every tap.  The
// three kw taps of one kh read the same activation rows displaced by -d, 0, +d pixels (stride 1, pad == dil == d: output row m
// is input pixel m), so two thirds of those bytes come twice.  Here ONE A stage serves a GROUP = one (chunk, kh) pair and its
// three kw steps:
//  * the stage holds the flat pixels [m0 - d, m0 + 256 + d) of the tile, each taken at image row h + (kh - 1) d, with d ZERO rows
//    inserted at every image-row boundary inside that range (a boundary between two images is an ordinary row boundary).  Stage
//    row s <-> (rr, cc) = divmod(s + c0, W + d), c0 the column of pixel m0 - d: cc >= W is a gap row, anything else is pixel
//    (R0 + rr) W + cc.  The output row m then sits at stage row s(m) = m - (m0 - d) + d (m / W - R0), and its kw tap at
//    s(m) + (kw - 1) d: a tap left of column 0 or right of column W - 1 lands in a gap row and reads zeros -- no masks in registers;
//  * gap rows, pixels outside [0, M), rows past the range and rows whose kh tap is outside the image get the offset 2^31: the
//    buffer range check writes zeros (conv_dma2.hip's mechanism).  That is one bit per stage row and kh, decided once per tile;
//  * capacity: ROW3_SR = 288 stage rows.  A range of 256 + 2 d pixels contains at most ceil((255 + 2 d) / W) row boundaries, so
//    the host takes the id where 256 + 2 d + d ceil((255 + 2 d) / W) <= 288 (conv_row3_supported) and refuses it elsewhere;
//  * 288 rows x 12 quads = 6.75 rounds of the block's 512 lanes.  The seventh round's upper two waves have no stage rows left;
//    they issue their piece all the same, with every offset out of range, into 2 KB of LDS behind the stages that nobody reads
//    (an exec-masked LDS-DMA is not an option, conv_dma2.hip's header; a branch would split the K step's basic block and give
//    the waves different wait counts).  LDS: 2 x 288 x 192 B of A, 2 x 24 KB of B, 2 KB = 161 792 B, one block per CU;
//  * a reader applies the swizzle of the row it reads: position plane * 4 + (quad ^ ((row >> 2) & 3)) with row = s(m) + (kw - 1) d.
//    The six fragment addresses per lane and K16 slice (2 row tiles x 3 kw) are computed once per tile.
// Tile (256 x 128, 8 waves as 4 x 2 of 64 x 64), weights (pemp_pack_split3_bf16, the B swizzle), the order of the K16 slices per
// accumulator (chunk, kh, kw ascending; inside a slice split3_mma6's products) and the epilogue (conv_epilogue_lds) are those of
// id 146: BIT-IDENTICAL to ids 146 / 149, and to id 43 on the fp32 tensor.
//
// Pipeline.  K step kt = 3 g + ph (group g, ph = kw).  B keeps its two-deep ring: B(kt + 2) goes out behind the barrier of step
// kt into the buffer that step frees.  The A buffer of group g + 1 is free from the barrier of step 3 g - 1 on (the last reads of
// group g - 1) and must have landed by the barrier of step 3 g + 2.  Behind the barrier of a step ("tail") a wave issues, one per
// MFMA slot of the step's second K16 slice, first the BL = 3 pieces of B and then row3_a_tail(ph) pieces of A:
//   tail of ph 2 (group g - 1):  B(3 g + 1),  A(g + 1) pieces 0..2
//   tail of ph 0 (group g):      B(3 g + 2),  A(g + 1) pieces 3..6
//   tail of ph 1:                B(3 g + 3)
// Vector memory operations of a wave retire in issue order, so the wait in front of a step's barrier is vmcnt(operations issued
// behind the last one it needs).  Step ph needs B(kt + 1), issued first in the tail of the step before; the A pieces behind it
// may fly on: row3_behind(ph) = row3_a_tail(ph - 1) = 3, 4.  Step ph 2 also needs all of A(g + 1), and nothing younger than B(kt + 1)
// has been issued: 0.  A piece of A thus gets one to two K steps to land, and two of three barriers no longer wait for
// everything in flight.  In front of the loop: A(0), B(0), then B(1), A(1) pieces 0..2 (the tail of a step "-1"); the first
// barrier waits past the last two, vmcnt(BL + row3_a_tail(2)).
// Stages past the last one are still issued, with every offset out of range (zeros into a free buffer, no memory read): one form
// of the step, constant counts.  They are drained (vmcnt(0) + barrier) before the transpose patches reuse the stage buffers.
//
// Persistent form (id 249): the tile walk of conv_dma2.hip's id 149 (XcdTileRange, conv_common.h).  Groups and steps are numbered THROUGH the walk (the buffer of a group / step
// is its running number's parity) and the (chunk, kh, kw) state wraps at the end of a tile, so the issue schedule above simply
// runs on into the next tile: A(g + 1), A(g + 2) and B(kt + 2) of a tile's last groups ARE the next tile's first stages, issued
// under its last steps with the next tile's offsets.  Those are exchanged in place where the current tile has issued its last
// piece of the kind: the A offsets between the tails of ph 0 and ph 2 of the second-to-last group, the B offsets between the
// tails of ph 0 and ph 1 of the last group (after the block's last tile: every offset out of range).  What differs at a tile's end:
//  * the last step issues nothing and reads no next fragments, and its barrier waits for the LDS reads only: the next tile's
//    A(0) and B(0) fly on under the epilogue, whose patches go to the A buffer that step read;
//  * the epilogue is conv_epilogue_s3p (conv_common.h) in its PLAIN form, without residual and per-image branches: the scale /
//    shift quads in one batch behind the last MFMAs, the stores back to back;
//  * B(1) and A(1) pieces 0..2 of the next tile -- the tail the last step did not issue; A(1) goes to the buffer the patches are
//    in -- follow a barrier behind the epilogue, and the wait in front of the next tile's first MFMA counts past them and past the
//    NST stores (a wave whose rows are not all inside M issues fewer stores and does not count them): vmcnt(row3_behind_first()
//    (+ NST)).  From there on the steady-state counts hold again: step 0 needs B(1), the three A pieces behind it may fly.
#include "conv_tiles.h"

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int ROW3_BM = 256, ROW3_BN = 128, ROW3_NW = 8, ROW3_WGM = 4;
constexpr int ROW3_SR = 288;                                    // stage rows of A
constexpr int ROW3_AQ = ROW3_SR * 12, ROW3_BQ = ROW3_BN * 12;   // quads of one A / B stage
constexpr int ROW3_AL = (ROW3_AQ + ROW3_NW * 64 - 1) / (ROW3_NW * 64);      // A pieces per thread and group: 7
constexpr int ROW3_BL = ROW3_BQ / (ROW3_NW * 64);                           // B pieces per thread and step: 3
constexpr int ROW3_SPARE = ROW3_AL * ROW3_NW * 64 - ROW3_AQ;                // quads the last round has no stage rows for
static_assert(ROW3_BQ % (ROW3_NW * 64) == 0 && ROW3_SPARE % 64 == 0 && ROW3_SPARE < ROW3_NW * 64, "whole waves in the last A round");
constexpr size_t row3_lds() { return (size_t)(2 * ROW3_AQ + 2 * ROW3_BQ + ROW3_SPARE) * sizeof(v4f); }
static_assert(row3_lds() <= 160 * 1024, "LDS of a CU");

// A pieces issued in the tail of a step of phase ph (behind its B pieces), and the first piece of that tail
constexpr int row3_a_tail(int ph) { return ph == 2 ? 3 : ph == 0 ? ROW3_AL - 3 : 0; }
constexpr int row3_a_first(int ph) { return ph == 0 ? 3 : 0; }
static_assert(row3_a_tail(0) + row3_a_tail(1) + row3_a_tail(2) == ROW3_AL, "a group's pieces over its window");
// vector memory operations behind the last one the barrier of a step of phase ph needs (the derivation in the file header)
constexpr int row3_behind(int ph) { return ph == 2 ? 0 : row3_a_tail((ph + 2) % 3); }
constexpr int row3_behind_first() { return ROW3_BL + row3_a_tail(2); }

__global__ __launch_bounds__(ROW3_NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void conv_row3_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = ROW3_BM, BN = ROW3_BN, NW = ROW3_NW, WGM = ROW3_WGM, WGN = NW / WGM;
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int AL = ROW3_AL, BL = ROW3_BL;
    constexpr int NMF = 6 * TM * TN, NDS = 3 * TM + 3 * TN;

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                          // [2][ROW3_SR][12]
    v4f* Bs = smem + 2 * ROW3_AQ;            // [2][BN][12]
    v4f* Sp = Bs + 2 * ROW3_BQ;              // the last A round's waves without stage rows write here

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
    const int lr = lane & 31, lh = lane >> 5;

    const int ntn = a.Cout / BN;
    const int tile_id = xcd_tile_order(blockIdx.x, gridDim.x);
    const int m0 = (tile_id / ntn) * BM, n0 = (tile_id % ntn) * BN;

    const int d = a.dil, W = a.W, Wd = W + d;
    const int f0 = m0 - d;                                           // the stage's first pixel (>= -d)
    const int R0 = f0 >= 0 ? f0 / W : -((W - 1 - f0) / W);           // floor(f0 / W)
    const int c0 = f0 - R0 * W;
    const int rowb = a.ldx * 6;                                      // bytes per pixel
    // the descriptor's base lies d rows + d pixels in front of x: offset of pixel f at kernel row kh = (f + d + kh d W) rowb >= 0
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x - (ptrdiff_t)(d * W + d) * rowb), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);

    // loader role: LDS quad q of the A stage = stage row q / 12, position q % 12 (the B image and swizzle)
    unsigned a_voff[AL], a_ok = 0, b_voff[BL];                       // a_ok: bit 3 i + kh = piece i reads memory at kernel row kh
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int q = i * NW * 64 + tid, srow = q / 12, pos = q - srow * 12;
        const int src = PEMP_SPLIT3_SWZ(srow, pos);
        const int t = srow + c0, rr = t / Wd, cc = t - rr * Wd;
        const int f = (R0 + rr) * W + cc;
        const bool pix = srow < ROW3_SR && cc < W && f >= 0 && f < a.M && f < m0 + BM + d;
        const int h = pix ? (R0 + rr) % a.H : 0;
        a_voff[i] = (unsigned)((f + d) * rowb + src * 16);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
            if (pix && (unsigned)(h + (kh - 1) * d) < (unsigned)a.H) a_ok |= 1u << (3 * i + kh);
    }
#pragma unroll
    for (int i = 0; i < BL; ++i) {
        const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
        const int src = PEMP_SPLIT3_SWZ(row, pos);
        b_voff[i] = (unsigned)((n0 + row) * a.Kpad * 6 + src * 16);
    }
    const int taph = d * W * rowb;
    const int NG = 3 * a.cin_steps, nkl = a.nk;

    // A piece i_ of the group (cb_, kh_) into stage buffer ab_ (ok_: the group exists)
#define PEMP_ROW3_DMA_A(i_, ab_, cb_, kh_, ok_)                                                                   \
    do {                                                                                                          \
        const int so_ = __builtin_amdgcn_readfirstlane((kh_) * taph + (cb_) * 192);                              \
        const bool in_ = (((a_ok & (0u - (unsigned)(ok_))) >> (3 * (i_) + (kh_))) & 1u) != 0u;   /* no branch: one basic block */ \
        v4f* dst_ = As + (ab_) * ROW3_AQ + (i_) * NW * 64 + wave * 64;                                            \
        if ((i_) == AL - 1 && ROW3_SPARE) dst_ = wave * 64 < NW * 64 - ROW3_SPARE ? dst_ : Sp + (wave * 64 - (NW * 64 - ROW3_SPARE)); \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)dst_, 16, in_ ? a_voff[i_] : 0x80000000u, so_, 0, 0); \
    } while (0)
    // the BL pieces of step (cb_, tap_) into stage buffer bb_
#define PEMP_ROW3_DMA_B(bb_, cb_, tap_, ok_)                                                                      \
    do {                                                                                                          \
        const int so_ = __builtin_amdgcn_readfirstlane(((tap_) * a.Cin + (cb_) * 32) * 6);                       \
        _Pragma("unroll") for (int i = 0; i < BL; ++i)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bs + (bb_) * ROW3_BQ + i * NW * 64 + wave * 64), 16, \
                                                     (ok_) ? b_voff[i] : 0x80000000u, so_, 0, 0);                 \
    } while (0)

    // fragment addresses (in quads): the lane's row of row tile mi at tap kw, K16 slice j: plane 0 of quad 2 j + lh
    int aidx[TM][3][2];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = m0 + wm0 + mi * 32 + lr;
        const int s = m - f0 + d * (m / W - R0);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int row = s + (kw - 1) * d, sw = (row >> 2) & 3;
            aidx[mi][kw][0] = row * 12 + (lh ^ sw);
            aidx[mi][kw][1] = row * 12 + ((2 + lh) ^ sw);
        }
    }
    const int brow3 = (wn0 + lr) * 12, bsw3 = (lr >> 2) & 3;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
    v4f aq3[2][TM][3], bf3[2][TN][3];

#define PEMP_ROW3_READ(dst_, ab_, bb_, kw_, j_)                                                                   \
    do {                                                                                                          \
        const v4f* Ab_ = As + (ab_) * ROW3_AQ;                                                                    \
        const v4f* Bb_ = Bs + (bb_) * ROW3_BQ;                                                                    \
        const int pb_ = (2 * (j_) + lh) ^ bsw3;                                                                   \
        _Pragma("unroll") for (int mi = 0; mi < TM; ++mi)                                                         \
            _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                                      \
                aq3[dst_][mi][pl] = Ab_[aidx[mi][kw_][j_] + pl * 4];                                              \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                                         \
            _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                                      \
                bf3[dst_][ni][pl] = Bb_[brow3 + ni * 32 * 12 + pl * 4 + pb_];                                     \
    } while (0)

    // the K16 slice in registers src_: every accumulator's six products (split3_mma6)
#define PEMP_ROW3_MMA(src_)                                                                                       \
    do {                                                                                                          \
        _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {     \
            const bf16x8 ah_ = __builtin_bit_cast(bf16x8, aq3[src_][mi][0]);                                      \
            const bf16x8 am_ = __builtin_bit_cast(bf16x8, aq3[src_][mi][1]);                                      \
            const bf16x8 al_ = __builtin_bit_cast(bf16x8, aq3[src_][mi][2]);                                      \
            const bf16x8 bh_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][0]);                                      \
            const bf16x8 bm_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][1]);                                      \
            const bf16x8 bl_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][2]);                                      \
            split3_mma6(acc[mi][ni], ah_, am_, al_, bh_, bm_, bl_);                                               \
        }                                                                                                         \
    } while (0)

    // One K step of phase PH_ (= kw) of the group with running number GG_ (A buffer GG_ & 1, B buffer (GG_ + PH_) & 1).  (cb, kh):
    // the group; (cbn, khn): group g + 1; (cbn2, khn2): group g + 2.  The tail issues B(kt + 2) and the phase's A pieces (file
    // header; OKB_ / OKA1_ / OKA2_: that step / group g + 1 / group g + 2 exists) and reads the first fragments of step kt + 1.
#define PEMP_ROW3_STEP(PH_, GG_, OKB_, OKA1_, OKA2_)                                                              \
    do {                                                                                                          \
        const int ab = (GG_) & 1, bb_ = ((GG_) + (PH_)) & 1;                                                      \
        PEMP_ROW3_READ(1, ab, bb_, PH_, 1);                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PEMP_ROW3_MMA(0);                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        /* every LDS read of this step by this wave has returned; its pieces of what step kt + 1 reads have landed */ \
        __builtin_amdgcn_s_waitcnt(0xC07F);          /* lgkmcnt(0), visible to hipcc's own wait bookkeeping */    \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(row3_behind(PH_)) : "memory");                        \
        __builtin_amdgcn_s_barrier();               /* ... everybody's */                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        if ((PH_) == 2) PEMP_ROW3_READ(0, ab ^ 1, bb_ ^ 1, 0, 0);                                                 \
        else PEMP_ROW3_READ(0, ab, bb_ ^ 1, (PH_) + 1, 0);                                                        \
        if ((PH_) == 0) PEMP_ROW3_DMA_B(bb_, cb, kh * 3 + 2, OKB_);                                               \
        else PEMP_ROW3_DMA_B(bb_, cbn, khn * 3 + (PH_) - 1, OKB_);                                                \
        _Pragma("unroll") for (int i = 0; i < row3_a_tail(PH_); ++i) {                                            \
            if ((PH_) == 2) PEMP_ROW3_DMA_A(row3_a_first(PH_) + i, ab, cbn2, khn2, OKA2_);                        \
            else PEMP_ROW3_DMA_A(row3_a_first(PH_) + i, ab ^ 1, cbn, khn, OKA1_);                                 \
        }                                                                                                         \
        PEMP_ROW3_MMA(1);               /* the second K16 slice covers the reads / DMA issue above: one per MFMA slot */ \
        _Pragma("unroll") for (int k_ = 0; k_ < NMF; ++k_) {                                                      \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                    \
            if (k_ < NDS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                      \
            else if (k_ < NDS + BL + row3_a_tail(PH_)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);         \
        }                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)
    static_assert(NDS + BL + ROW3_AL <= NMF, "one LDS read / one DMA per MFMA slot");

    // in front of the loop: A(0), B(0); B(1), A(1) pieces 0..2 -- the tail of a step in front of step 0
#pragma unroll
    for (int i = 0; i < AL; ++i) PEMP_ROW3_DMA_A(i, 0, 0, 0, true);
    PEMP_ROW3_DMA_B(0, 0, 0, true);
    PEMP_ROW3_DMA_B(1, 0, 1, true);
#pragma unroll
    for (int i = 0; i < row3_a_tail(2); ++i) PEMP_ROW3_DMA_A(i, 1, 0, 1, true);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(row3_behind_first()) : "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    PEMP_ROW3_READ(0, 0, 0, 0, 0);
    int cb = 0, kh = 0;
    for (int g = 0; g < NG; ++g) {
        const int cbn = kh == 2 ? cb + 1 : cb, khn = kh == 2 ? 0 : kh + 1;
        const int cbn2 = khn == 2 ? cbn + 1 : cbn, khn2 = khn == 2 ? 0 : khn + 1;
        PEMP_ROW3_STEP(0, g, 3 * g + 2 < nkl, g + 1 < NG, false);
        PEMP_ROW3_STEP(1, g, 3 * g + 3 < nkl, false, false);
        PEMP_ROW3_STEP(2, g, 3 * g + 4 < nkl, false, g + 2 < NG);
        cb = cbn;
        kh = khn;
    }

    // the stages past the last one (zeros) have landed and every wave is done with the stage buffers: the patches may go there
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    static_assert(NW * 1024 * sizeof(float) <= 2 * ROW3_AQ * sizeof(v4f), "one 4 KB transpose patch per wave");
    conv_epilogue_lds<TM, TN>(a, acc, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane);
#endif
}

// the persistent form (id 249; file header)
__global__ __launch_bounds__(ROW3_NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void conv_row3p_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = ROW3_BM, BN = ROW3_BN, NW = ROW3_NW, WGM = ROW3_WGM, WGN = NW / WGM;
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int AL = ROW3_AL, BL = ROW3_BL;
    constexpr int NMF = 6 * TM * TN, NDS = 3 * TM + 3 * TN;
    constexpr int NST = TM * TN * 4;            // epilogue stores per thread of a wave tile inside the output
    static_assert(row3_behind_first() + NST <= 63, "vmcnt range");

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                          // [2][ROW3_SR][12]
    v4f* Bs = smem + 2 * ROW3_AQ;            // [2][BN][12]
    v4f* Sp = Bs + 2 * ROW3_BQ;              // the last A round's waves without stage rows write here

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
    const int lr = lane & 31, lh = lane >> 5;

    // the block's tile sequence: tiles tr.first + j, j = tr.idx, tr.idx + tr.step, ... < tr.count
    const int ntn = a.Cout / BN;
    const XcdTileRange tr((a.M + BM - 1) / BM * ntn, (int)blockIdx.x, (int)gridDim.x);
    if (tr.idx >= tr.count) return;             // (the launch clamps the grid to the tile count: not expected)
    int j = tr.idx;
    int m0 = ((tr.first + j) / ntn) * BM, n0 = ((tr.first + j) % ntn) * BN;

    const int d = a.dil, W = a.W, Wd = W + d;
    const int rowb = a.ldx * 6;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x - (ptrdiff_t)(d * W + d) * rowb), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);

    // per-tile offsets: conv_row3_kernel's, expression for expression (ok_ false: behind the block's last tile, nothing reads memory)
    unsigned a_voff[AL], a_ok = 0, b_voff[BL];
    auto a_offsets = [&](const int m0_, const bool ok_) {
        const int f0 = m0_ - d;
        const int R0 = f0 >= 0 ? f0 / W : -((W - 1 - f0) / W);
        const int c0 = f0 - R0 * W;
        a_ok = 0;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int q = i * NW * 64 + tid, srow = q / 12, pos = q - srow * 12;
            const int src = PEMP_SPLIT3_SWZ(srow, pos);
            const int t = srow + c0, rr = t / Wd, cc = t - rr * Wd;
            const int f = (R0 + rr) * W + cc;
            const bool pix = ok_ && srow < ROW3_SR && cc < W && f >= 0 && f < a.M && f < m0_ + BM + d;
            const int h = pix ? (R0 + rr) % a.H : 0;
            a_voff[i] = (unsigned)((f + d) * rowb + src * 16);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
                if (pix && (unsigned)(h + (kh - 1) * d) < (unsigned)a.H) a_ok |= 1u << (3 * i + kh);
        }
    };
    auto b_offsets = [&](const int n0_, const bool ok_) {
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
            const int src = PEMP_SPLIT3_SWZ(row, pos);
            b_voff[i] = ok_ ? (unsigned)((n0_ + row) * a.Kpad * 6 + src * 16) : 0x80000000u;
        }
    };
    int aidx[TM][3][2];
    auto reader = [&](const int m0_) {
        const int f0 = m0_ - d;
        const int R0 = f0 >= 0 ? f0 / W : -((W - 1 - f0) / W);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            const int m = m0_ + wm0 + mi * 32 + lr;
            const int s = m - f0 + d * (m / W - R0);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int row = s + (kw - 1) * d, sw = (row >> 2) & 3;
                aidx[mi][kw][0] = row * 12 + (lh ^ sw);
                aidx[mi][kw][1] = row * 12 + ((2 + lh) ^ sw);
            }
        }
    };
    a_offsets(m0, true);
    b_offsets(n0, true);
    const int taph = d * W * rowb;
    const int NG = 3 * a.cin_steps, ncb = a.cin_steps;
    const int brow3 = (wn0 + lr) * 12, bsw3 = (lr >> 2) & 3;
    const int c4_ = (lane & 7) * 4;
    v4f aq3[2][TM][3], bf3[2][TN][3];

    // the block's first tile: A(0), B(0); B(1), A(1) pieces 0..2
#pragma unroll
    for (int i = 0; i < AL; ++i) PEMP_ROW3_DMA_A(i, 0, 0, 0, true);
    PEMP_ROW3_DMA_B(0, 0, 0, true);
    PEMP_ROW3_DMA_B(1, 0, 1, true);
#pragma unroll
    for (int i = 0; i < row3_a_tail(2); ++i) PEMP_ROW3_DMA_A(i, 1, 0, 1, true);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(row3_behind_first()) : "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    int gg = 0;                                  // running group number: group buffer gg & 1, step buffer (gg + ph) & 1
    int cb = 0, kh = 0;
    for (;;) {
        f32x16 acc[TM][TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
        const int jn = j + tr.step;
        const bool more = jn < tr.count;
        const int m0n = more ? ((tr.first + jn) / ntn) * BM : m0, n0n = more ? ((tr.first + jn) % ntn) * BN : n0;
        reader(m0);

        PEMP_ROW3_READ(0, gg & 1, gg & 1, 0, 0);
        // (cbn, khn), (cbn2, khn2): the next two groups, wrapping into the next tile's first ones
#define PEMP_ROW3_NEXT_GROUPS()                                                                                   \
        int cbn = kh == 2 ? cb + 1 : cb;                                                                          \
        const int khn = kh == 2 ? 0 : kh + 1;                                                                     \
        cbn = cbn == ncb ? 0 : cbn;                                                                               \
        int cbn2 = khn == 2 ? cbn + 1 : cbn;                                                                      \
        const int khn2 = khn == 2 ? 0 : khn + 1;                                                                  \
        cbn2 = cbn2 == ncb ? 0 : cbn2
        for (int g = 0; g < NG - 1; ++g, ++gg) {
            PEMP_ROW3_NEXT_GROUPS();
            PEMP_ROW3_STEP(0, gg, true, true, true);
            if (g == NG - 2) a_offsets(m0n, more);      // the tile's last A piece is out: the offsets become the next tile's
            PEMP_ROW3_STEP(1, gg, true, true, true);
            PEMP_ROW3_STEP(2, gg, true, true, true);
            cb = cbn;
            kh = khn;
        }
        const int abl = gg & 1;                  // the last group's buffer: the transpose patches go there
        {
            PEMP_ROW3_NEXT_GROUPS();
            PEMP_ROW3_STEP(0, gg, true, true, true);
            b_offsets(n0n, more);                // the tile's last B piece is out
            PEMP_ROW3_STEP(1, gg, true, true, true);
            // the tile's last step: no tail, and the barrier waits for the LDS reads only -- the next tile's stages fly on
            PEMP_ROW3_READ(1, abl, (gg + 2) & 1, 2, 1);
            __builtin_amdgcn_sched_barrier(0);
            PEMP_ROW3_MMA(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            PEMP_ROW3_MMA(1);
            __builtin_amdgcn_sched_barrier(0);
            cb = cbn;
            kh = khn;
            (void)cbn2;
            (void)khn2;
            ++gg;
        }
#undef PEMP_ROW3_NEXT_GROUPS
        v4f scv[TN], shv[TN];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int n = n0 + wn0 + ni * 32 + c4_;
            scv[ni] = a.scale ? *(const v4f*)(a.scale + n) : v4f{1.f, 1.f, 1.f, 1.f};
            shv[ni] = a.shift ? *(const v4f*)(a.shift + n) : v4f{0.f, 0.f, 0.f, 0.f};
        }
        static_assert(NW * 256 <= ROW3_AQ, "one 4 KB transpose patch per wave inside ONE stage buffer");
        conv_epilogue_s3p<TM, TN, true>(a, acc, (float*)(As + abl * ROW3_AQ + wave * 256), m0 + wm0, n0 + wn0, lane, nullptr, scv, shv);
        if (!more) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no LDS-DMA outlives the block
            break;
        }

        // the tail the last step did not issue, once every wave is done with its patch: B(1), A(1) pieces 0..2 of the next tile
        __builtin_amdgcn_s_barrier();
        PEMP_ROW3_DMA_B((gg + 1) & 1, 0, 1, true);
#pragma unroll
        for (int i = 0; i < row3_a_tail(2); ++i) PEMP_ROW3_DMA_A(i, (gg + 1) & 1, 0, 1, true);
        // (the builtin form as well: hipcc's own bookkeeping then knows the epilogue's stores as retired and puts no vmcnt(0) of its own
        // in front of the next tile's first fragment reads)
        constexpr int VF = row3_behind_first() + NST, VP = row3_behind_first();
        if (m0 + wm0 + WM <= a.M) {
            __builtin_amdgcn_s_waitcnt((VF & 15) | 0x0F70 | ((VF >> 4) << 14));
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VF) : "memory");                     // A(0), B(0) have landed
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
#undef PEMP_ROW3_STEP
#undef PEMP_ROW3_MMA
#undef PEMP_ROW3_READ
#undef PEMP_ROW3_DMA_B
#undef PEMP_ROW3_DMA_A

// stage rows a tile of this geometry can need: 256 + 2 d pixels and d gap rows per image-row boundary inside them
static long long row3_stage_rows(int W, int d) { return ROW3_BM + 2 * d + (long long)d * ((ROW3_BM - 1 + 2 * d + W - 1) / W); }

// what the id takes: 3x3, stride 1, pad == dil, pre-split input with ldx == Cin, the plain fp32 output (affine, ReLU) without a
// residual, padding vector, per-image shift or workspace, Cout in whole 128-column tiles, a stage of at most ROW3_SR rows
bool conv_row3_supported(const ConvArgs& a) {
    if (!(a.flags & PEMP_CONV_IN_SPLIT3) || (a.flags & (PEMP_CONV_OUT_SPLIT3 | PEMP_CONV_OUT_SPLIT3_ALSO | PEMP_CONV_SHIFT_PER_IMAGE | PEMP_CONV_STEM4 | PEMP_CONV_BF16_IO)))
        return false;
    if (a.res || a.padv || a.stats || a.rowmask || a.sk_S > 1 || a.sk_ws || a.bm_first) return false;
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != a.dil || a.ldx != a.Cin || a.Cin % 32 || a.Cout % ROW3_BN) return false;
    if (a.Kpad != 9 * a.Cin || a.nk != 9 * a.cin_steps) return false;
    if (row3_stage_rows(a.W, a.dil) > ROW3_SR) return false;
    return conv_dma2_supported(a) && (long long)a.Cout * a.Kpad * 6 < (1ll << 31);
}

int launch_conv_row3(bool persistent, const ConvArgs& a, hipStream_t st) {
    if (!conv_row3_supported(a)) {
        set_error("conv split3 row3: unsupported (needs a 3x3 / stride 1 / pad == dil conv on pre-split input, plain fp32 output without residual / "
                  "padding value / per-image shift / workspace, Cout %% 128 == 0, 256 + 2 d + d ceil((255 + 2 d) / W) <= %d stage rows)", ROW3_SR);
        return -1;
    }
    const int tiles = cdiv(a.M, ROW3_BM) * (a.Cout / ROW3_BN);
    if (!persistent) return launch_with_lds(conv_row3_kernel, tiles, ROW3_NW * 64, row3_lds(), st, a, "conv_row3");
    static int occ = 0;
    int grid = 0;
    const int rc = persistent_grid(conv_row3p_kernel, ROW3_NW * 64, row3_lds(), tiles, occ, "conv split3 row3 persistent", grid);
    if (rc) return rc;
    return launch_with_lds(conv_row3p_kernel, grid, ROW3_NW * 64, row3_lds(), st, a, "conv_row3/persistent");
}

}  // namespace pemp
