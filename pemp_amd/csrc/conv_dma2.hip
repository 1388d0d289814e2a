// Implicit-GEMM convolution, second LDS-DMA variant: the same GEMM view, LDS image, fragment reads, MFMA order and
// epilogue as conv_dma.hip (results are bit-identical), with the two things that kept the MFMA pipe idle there removed:
//
//  * Operand addressing.  conv_dma.hip rebuilds a 64-bit source pointer per row every K step (bounds tests, a 64-bit
//    multiply-add, a select against the zero block: ~100 VALU/SALU instructions per wave per step, executed by both
//    waves of a SIMD at the same moment right after the barrier).  Here both operands are fetched with
//    `buffer_load_dwordx4 ... offen lds`: a per-lane BYTE OFFSET that never changes during the K loop plus a
//    wave-uniform SGPR offset that carries the whole K-step dependence (tap displacement + channel chunk for the
//    activations, K offset for the weights).  Which taps of a row fall outside the image is decided ONCE per tile
//    (one bit per tap); an out-of-image tap replaces the lane's offset by 2^31, the buffer range check (num_records =
//    2 GiB) then makes the hardware write zeros -- zero padding without a zero block, 3 VALU instructions per row
//    and step.  (The base of the activation descriptor is moved back by pad rows + pad pixels so that every
//    in-image offset is non-negative.)
//
//  * Barrier placement.  One barrier per K step as before, but it sits BEFORE the last quarter of the step's MFMAs,
//    whose operands are already in registers: after the barrier a wave issues the first fragment reads of the next
//    step and the LDS-DMA of the step after that in the shadow of those 4*TM*TN MFMAs, instead of starting every
//    step with address arithmetic + a dozen LDS reads + a full wait while the matrix pipe drains.
//
// Not handled here (conv_dma.hip keeps them; conv_stem_pool.hip has the split3 stem fused with its max-pool): the NHWC4 stem (a K step spans 8 taps, the tap differs per lane), more
// than 32 taps, operands of 2 GiB or more, and a per-channel padding VALUE (padv) that does not lie behind the
// activations in the same 2 GiB window: the in-image and the out-of-image lanes of a piece must come through ONE
// descriptor (an exec-masked LDS-DMA does not leave the inactive lanes' 16-byte slots alone -- tried: two masked DMAs per
// piece give wrong data -- so a piece cannot be assembled from two).
#include <type_traits>
#include "conv_tiles.h"

#ifndef PEMP_SK_ACQUIRE
#define PEMP_SK_ACQUIRE 1     // 0: round 4's hand-off without the consumer acquire (A/B builds only)
#endif

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;

// The block's work: tile ``bid`` of the ``nblk`` blocks of one conv (the plain kernel passes blockIdx.x / gridDim.x; the
// grouped kernel below the block's index inside its member conv).
// BF16 (the side-figure variant, pemp_conv2d_bf16_nhwc): the operands are bf16 in memory.  The kernel is the same down to the
// byte -- a K step is still 128 bytes per row, staged, swizzled and read as 16-byte quads -- because the caller hands over
// Cin / ldx / Kpad in DWORDS (two bf16 each): a quad then holds 8 bf16 = the 8 K values one lane feeds into
// v_mfma_f32_32x32x16_bf16 (lanes 0-31: K 0..7, lanes 32-63: K 8..15 = quads 2j and 2j + 1, exactly the pair a fragment read
// of step j fetches), so one MFMA does the work of the four v_mfma_f32_32x32x2_f32 of the fp32 kernel at 8 cycles instead of
// 4 x 64.  Accumulation stays fp32; the epilogue writes bf16 (or fp32 for the last layer) -- PEMP_CONV_BF16_IO.
// R16 (tile id 28: 32 x 64 block, four waves of 16 x 32): the same K loop on v_mfma_f32_16x16x4_f32.  Measured on gfx950
// (scratch/mfma_eq): the fp32 MFMAs of every shape accumulate as ONE sequential fma chain in their k order -- 32x32x2, 16x16x4
// and fmaf() agree bit for bit -- so a 16-row wave tile that feeds the chain in the order of the 32-row kernels (per quarter j
// of a K step: k = 8j + {0, 4, 1, 5, 2, 6, 3, 7}) is BIT-IDENTICAL to them and may serve the exact evaluation path.  What it
// buys: granularity.  A one-episode step has 5202 output rows; a 256-channel conv is 1304 wave tiles of 32 x 32 on 1024 SIMDs --
// two rounds, the second 27 % full, 64 % of the chip's MFMA time at best -- and 2608 of 16 x 32 -- three rounds of half the
// length, 85 %.  It pays twice the LDS reads per flop for that, so it only wins where a launch is a few rounds long.
// S3 (tile ids 41..46 / 51..56, pemp_hip.h): fp32 operands on the bf16 MFMA pipe.  Every fp32 x is split exactly into three bf16
// pieces x = h + m + l (round to nearest at each stage: |m| <= 2^-8 |x|, |l| <= 2^-16 |x|); a product a b is taken as six bf16 x
// bf16 products in a fixed order (split3_mma6, conv_common.h).  The activations stay fp32 in memory and in LDS (same DMA, swizzle, tap masks and
// padding values as the fp32 kernels) and are split in registers after the fragment read; the weights come pre-split
// (pemp_pack_split3_bf16: per row and 32-channel K step, three 64-byte planes h, m, l), 192 bytes per row and K step in LDS.
// A K step is two K16 slices of v_mfma_f32_32x32x16_bf16 (lane half lh of slice s: channels 16 s + 8 lh .. + 7); every
// accumulator sees the slices in ascending K order, so all unsplit S3 variants are bit-identical to each other (not to the
// fp32-chain variants: a different, equally fp32-accurate, rounding sequence).
// A3 (tile ids 146 / 149, PEMP_CONV_IN_SPLIT3): S3 whose ACTIVATIONS come pre-split as well -- written by the producer conv's
// epilogue (PEMP_CONV_OUT_SPLIT3, conv_common.h) in the layout of the packed weights: per pixel and 32-channel K step three
// 64-byte planes h, m, l.  The A path is then the B path: 192 bytes per row and K step in LDS (12 quads, the B swizzle), DMA'd with
// the same tap / stride / dilation arithmetic at 6 bytes per element (out-of-image lanes read zeros -- three zero planes -- or the
// pre-split padding vector), three 16-byte fragment reads per half step that go straight into the MFMAs.  No split3_bf16 in the K
// loop; MFMA order, accumulators and epilogue are S3's, and the pieces are those split3_bf16 would have made: bit-identical.
template <int BM, int BN, int WGM, int NW, bool PADV, int EPI = 0, bool SK = false, bool BF16 = false, bool DB = false, bool R16 = false,
          bool S3 = false, bool A3 = false, bool ALSO = false, bool RS2 = false>
__device__ __forceinline__ void conv_dma2_body(const ConvArgs& a, const int bid, const int nblk) {
#if defined(__HIP_DEVICE_COMPILE__)     // the host pass only needs the launch stub (buffer-resource builtins / "s" asm operands are device-only)
    constexpr int WGN = NW / WGM;
    constexpr int RPI = NW * 8;                 // rows covered by one DMA instruction round of the block
    constexpr int WM = BM / WGM, WN = BN / WGN;
    static_assert(!R16 || (WM == 16 && WN % 16 == 0 && EPI == 0 && !SK && !BF16 && !DB), "R16: 16-row wave tiles, plain epilogue only");
    static_assert(!S3 || (EPI <= 1 && !BF16 && !DB && !R16), "S3: plain or statistics epilogue, fp32 operands");
    static_assert(!S3 || EPI == 0 || (!SK && !PADV && !A3), "S3 statistics: unsplit, zero padding, fp32 activations");
    static_assert(!A3 || (S3 && !SK && (BM * 12) % (NW * 64) == 0), "A3: an unsplit S3 form, whole A DMA rounds");
    static_assert(!ALSO || A3, "a second, pre-split output (PEMP_CONV_OUT_SPLIT3_ALSO; a.res is its pointer): the A3 forms only");
    constexpr int TM = R16 ? 1 : WM / 32, TN = R16 ? WN / 16 : WN / 32;      // R16: TN counts 16-column MFMA tiles
    constexpr int BQ = S3 ? 12 : 8;             // 16-byte quads of B per row and K step in LDS
    static_assert(!S3 || (BN * BQ) % (NW * 64) == 0, "S3: whole B DMA rounds");
    constexpr int AQ = A3 ? 12 : 8;             // ... of A
    constexpr int XB = A3 ? 6 : 4;              // bytes per activation element in memory
    constexpr int AL = A3 ? BM * AQ / (NW * 64) : BM / RPI, BL = S3 ? BN * BQ / (NW * 64) : BN / RPI; // DMA wave-instructions per thread per K step
    // per quarter step (S3: per half step): MFMAs, fragment reads; DMAs per step
    constexpr int NMF = S3 ? 6 * TM * TN : R16 ? 2 * TN : TM * TN * (BF16 ? 1 : 4), NDS = S3 ? (A3 ? 3 : 2) * TM + 3 * TN : R16 ? 1 + TN : TM + TN,
                  NDMA = AL + BL;
    constexpr int PER = (NDS + NDMA + NMF - 1) / NMF;

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                      // [2][BM][AQ]
    v4f* Bs = smem + 2 * BM * AQ;        // [2][BN][BQ]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WGN) * WM;
    const int wn0 = (wave % WGN) * WN;
    const int lr = lane & 31, lh = lane >> 5;

    const int ntn = a.Cout / BN;
    // SK: blocks [0, sk_full) compute whole tiles; behind them, sk_S consecutive blocks share one of the remaining tiles,
    // block `piece` of them running K steps [kt0, kt0 + nkl)
    int tile_id, kt0 = 0, nkl = a.nk, sk_r = -1, piece = 0;
    if constexpr (SK) {
        const int b = bid;
        if (b < a.sk_full) {
            tile_id = xcd_tile_order(b, a.sk_full);
        } else {
            const int rb = b - a.sk_full;
            sk_r = rb / a.sk_S;
            piece = rb - sk_r * a.sk_S;
            tile_id = a.sk_full + sk_r;
            kt0 = (int)((long long)piece * a.nk / a.sk_S);
            nkl = (int)((long long)(piece + 1) * a.nk / a.sk_S) - kt0;
        }
    } else {
        tile_id = xcd_tile_order(bid, nblk);
    }
    const int bm = a.bm_first + tile_id / ntn;
    const int bn = tile_id % ntn;
    const int m0 = bm * BM, n0 = bn * BN;

    // loader role: thread (r, p) fetches, for rows r + RPI i, the quad that belongs at position p (see conv_dma.hip)
    const int p = tid & 7;
    const int r = tid >> 3;
    const int sq = p ^ ((r >> 1) & 7);

    const int bias_pix = a.pad * a.W + a.pad;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x - (ptrdiff_t)bias_pix * a.ldx * XB), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);

    // PADV (ops.fold_input_affine: a BatchNorm in front of a zero-padded conv): out-of-image taps read a per-channel VALUE
    // instead of zero.  One descriptor must serve both kinds of lane, so this variant needs the [Cin] vector INSIDE the
    // activation descriptor's range, behind the tensor (the engine allocates it there); an out-of-image lane then gets
    // the offset of its channel quad of that vector, minus the tap displacement the SGPR offset is about to add.
    const unsigned padv_off = PADV ? (unsigned)((const char*)a.padv - ((const char*)a.x - (ptrdiff_t)bias_pix * a.ldx * XB)) + (A3 ? 0 : sq * 16) : 0x80000000u;
    // A3: six rows per thread instead of four -- the tap masks of two rows share a register (<= 16 taps), and the lane's (swizzled)
    // quad inside the row's 192 bytes, which differs per DMA round, is a_voff mod 192 (PADV reads it back from there)
    constexpr int AINV = A3 ? AL / 2 : AL;
    static_assert(!A3 || AL % 2 == 0, "A3: tap masks in pairs");
    unsigned a_voff[AL], a_inv[AINV], b_voff[BL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        int arow_ = r + RPI * i, asrc_ = sq * 16;
        if constexpr (A3) {     // LDS quad q of the A tile = row q / 12, position q % 12: the B tile's layout and swizzle
            const int q = i * NW * 64 + tid, pos = q % 12;
            arow_ = q / 12;
            asrc_ = PEMP_SPLIT3_SWZ(arow_, pos) * 16;
        }
        const int m = m0 + arow_;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int img = mm / a.HoWo;
        const int rem = mm - img * a.HoWo;
        const int ho = rem / a.Wo;
        const int wo = rem - ho * a.Wo;
        const int hi0 = ho * a.stride - a.pad;
        const int wi0 = wo * a.stride - a.pad;
        a_voff[i] = A3 ? (unsigned)(((img * a.H + hi0) * a.W + wi0 + bias_pix) * a.ldx * 6 + asrc_)
                           : (unsigned)(((img * a.H + hi0) * a.W + wi0 + bias_pix) * a.ldx + sq * 4) * 4u;
        unsigned mask = 0;
        int kh = 0, kw = 0;
        for (int t = 0; t < a.ntaps; ++t) {
            const int hi = hi0 + kh * a.dil, wi = wi0 + kw * a.dil;
            if (ok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W) mask |= 1u << t;
            if (++kw == a.KW) {
                kw = 0;
                ++kh;
            }
        }
        if constexpr (!A3) a_inv[i] = ~mask;
        else if (i & 1) a_inv[i >> 1] |= ~mask << 16;
        else a_inv[i >> 1] = ~mask & 0xFFFFu;
    }
#pragma unroll
    for (int i = 0; i < BL; ++i) {
        if constexpr (S3) {     // LDS quad q of the tile = row q / 12, position q % 12 = plane * 4 + (quad ^ ((row >> 2) & 3))
            const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
            const int src = PEMP_SPLIT3_SWZ(row, pos);
            b_voff[i] = (unsigned)((n0 + row) * a.Kpad * 6 + src * 16);
        } else {
            b_voff[i] = (unsigned)((n0 + r + RPI * i) * a.Kpad + sq * 4) * 4u;
        }
    }

    // wave-uniform K-step state.  Multi-tap convs: channel chunk OUTER, tap INNER (same order as every other conv
    // kernel of the library: variants stay bit-identical); 1x1: chunks in sequence.
    int tap = 0, cb = 0, kh_i = 0, kw_i = 0;
    if constexpr (SK) {
        if (kt0 > 0) {
            const int cb0 = a.ntaps > 1 ? kt0 / a.ntaps : kt0;
            const int tap0 = a.ntaps > 1 ? kt0 - cb0 * a.ntaps : 0;
            const int kh0 = tap0 / a.KW;
            cb = __builtin_amdgcn_readfirstlane(cb0);
            tap = __builtin_amdgcn_readfirstlane(tap0);
            kh_i = __builtin_amdgcn_readfirstlane(kh0);
            kw_i = __builtin_amdgcn_readfirstlane(tap0 - kh0 * a.KW);
        }
    }
    const int tapw = a.dil * a.ldx * XB, taph = a.dil * a.W * a.ldx * XB;     // byte displacement of one tap step

#define PEMP_DMA2(buf_)                                                                                           \
    do {                                                                                                          \
        v4f* Ad_ = As + (buf_) * BM * AQ + wave * 64;                                                             \
        v4f* Bd_ = Bs + (buf_) * BN * BQ + wave * 64;                                                             \
        const int sa_ = kh_i * taph + kw_i * tapw + cb * (32 * XB);                                               \
        const int sb_ = (tap * a.Cin + cb * 32) * (S3 ? 6 : 4);                                                   \
        const int sh_ = 31 - tap;                                                                                 \
        const unsigned oob_ = PADV ? padv_off - (unsigned)(kh_i * taph + kw_i * tapw) : 0x80000000u;              \
        _Pragma("unroll") for (int i = 0; i < AL; ++i) {                                                          \
            const bool inv_ = A3 ? (int)(a_inv[i >> 1] << (sh_ - ((i & 1) ? 16 : 0))) < 0 : (int)(a_inv[A3 ? 0 : i] << sh_) < 0;  \
            const unsigned vo_ = inv_ ? oob_ + (A3 && PADV ? a_voff[i] % 192u : 0u) : a_voff[i];                  \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(Ad_ + i * RPI * 8), 16, vo_, sa_, 0, 0);        \
        }                                                                                                         \
        _Pragma("unroll") for (int i = 0; i < BL; ++i)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bd_ + i * RPI * 8), 16, b_voff[i], sb_, 0, 0);  \
    } while (0)

    // branch-free and pinned to the scalar unit (inline asm: hipcc otherwise turns the selects into VALU code, the
    // SGPR offsets of the DMA instructions into VGPRs and every DMA into a readfirstlane loop); the steady-state
    // K step must stay one basic block
    // (the three loop-invariant inputs are produced by an asm statement with an "=s" result: hipcc has been seen to keep
    // a uniform value -- even the result of __builtin_amdgcn_readfirstlane -- in a VGPR and to print that VGPR into an
    // "s" operand)
    // HAZARDS the statement must cover itself (gfx940 / gfx950 wait-state rules that hipcc's hazard recogniser applies to the
    // instructions it schedules, NOT to the text of an inline-asm statement): "VALU writes a VGPR -> v_readlane /
    // v_readfirstlane reads it: 1 wait state" on the way in -- the "v" inputs are materialised by the compiler (v_mov /
    // v_cndmask from SGPRs) and may be the very instruction in front of the statement -- and "VALU writes an SGPR -> VALU reads it:
    // 2, v_readlane lane select: 4, VMEM reads it: 5 wait states" on the way out.  Hence the leading s_nop 0 and the trailing
    // s_nop 4.  Round 4's "tile 31" wrong results were exactly the first one: in ONE instantiation (128 x 128, 4 waves, padding
    // value, split-K) the scheduler put `v_cndmask_b32 v3, 0, 1, s[8:9]` (ntaps > 1 ? 1 : 0) directly in front of
    // `v_readfirstlane_b32 s8, v3`, the read returned v3's previous content, `multi` came out 0 and the K loop walked a 3 x 3
    // conv as if it were 1 x 1 (found round 5 by tracing the scalar state of the failing binary and inserting single s_nops
    // into its assembly: DESIGN.md section 4).
    int multi, s_kw, s_ntaps;
    asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %3\n\tv_readfirstlane_b32 %1, %4\n\tv_readfirstlane_b32 %2, %5\n\ts_nop 4"
                 : "=s"(multi), "=s"(s_kw), "=s"(s_ntaps)
                 : "v"(a.ntaps > 1 ? 1 : 0), "v"(a.KW), "v"(a.ntaps));
#define PEMP_ADVANCE2()                                                                                           \
    do {                                                                                                          \
        int wt_;                                                                                                  \
        asm volatile(                                                                                             \
            "s_add_u32 %0, %0, %5\n\t"      /* tap += multi                      */                                \
            "s_add_u32 %2, %2, %5\n\t"      /* kw  += multi                      */                                \
            "s_cmp_eq_u32 %2, %6\n\t"       /* kw == KW ?                        */                                \
            "s_cselect_b32 %2, 0, %2\n\t"   /*   kw = 0                          */                                \
            "s_addc_u32 %1, %1, 0\n\t"      /*   kh += 1                         */                                \
            "s_xor_b32 %4, %5, 1\n\t"       /* 1x1: wrap every step              */                                \
            "s_cmp_eq_u32 %0, %7\n\t"       /* tap == ntaps ?                    */                                \
            "s_cselect_b32 %4, 1, %4\n\t"                                                                          \
            "s_cmp_lg_u32 %4, 0\n\t"                                                                               \
            "s_cselect_b32 %0, 0, %0\n\t"   /*   tap = kh = kw = 0, next channel chunk */                          \
            "s_cselect_b32 %1, 0, %1\n\t"                                                                          \
            "s_cselect_b32 %2, 0, %2\n\t"                                                                          \
            "s_addc_u32 %3, %3, 0"                                                                                \
            : "+s"(tap), "+s"(kh_i), "+s"(kw_i), "+s"(cb), "=&s"(wt_)                                             \
            : "s"(multi), "s"(s_kw), "s"(s_ntaps)                                                    \
            : "scc");                                                                                             \
    } while (0)

    f32x16 acc[R16 ? 1 : TM][R16 ? 1 : TN];
#pragma unroll
    for (int mi = 0; mi < (R16 ? 1 : TM); ++mi)
#pragma unroll
        for (int ni = 0; ni < (R16 ? 1 : TN); ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
    v4f acc16[R16 ? TN : 1];             // R16: one 16 x 16 accumulator per column tile (rows 4 (lane >> 4) + e, column lane & 15)
#pragma unroll
    for (int ni = 0; ni < (R16 ? TN : 1); ++ni) acc16[ni] = v4f{0.f, 0.f, 0.f, 0.f};

    PEMP_DMA2(0);
    if (nkl > 1) {
        PEMP_ADVANCE2();
        PEMP_DMA2(1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");         // step 0 has landed, step 1 may still fly
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // fragment read positions: quad Q of row (.. + lr) sits at position Q ^ ((lr>>1)&7)
    const int rsw = (lr >> 1) & 7;
    const int arow = (wm0 + lr) * 8, brow = (wn0 + lr) * 8;
    v4f af[2][R16 ? 1 : TM], bf[2][R16 ? 1 : TN];
    // R16: lane (r16, g) feeds k slot g of v_mfma_f32_16x16x4_f32.  The two MFMAs of quarter j must see k = 8j + {0, 4, 1, 5} and
    // 8j + {2, 6, 3, 7} in their slots 0..3 (the chain order of the 32-row kernels): slot g reads quad 2j + (g & 1) of its row and
    // uses element (g >> 1) for the first MFMA, element 2 + (g >> 1) for the second -- one ds_read2_b32 (dwords +0, +2) per row.
    const int r16 = lane & 15, g16 = lane >> 4;
    const int rsw16 = (r16 >> 1) & 7;                 // wm0 / wn0 / 16 ni are multiples of 16: the row's swizzle is that of r16
    const int arow16 = (wm0 + r16) * 32 + (g16 >> 1), brow16 = (wn0 + r16) * 32 + (g16 >> 1);     // in floats
    float a16[2][2], b16[2][R16 ? TN : 1][2];
    // S3: half step j of a lane: fp32 quads 4 j + 2 lh and 4 j + 2 lh + 1 of its A rows, quad 2 j + lh of each weight plane
    v4f af3[2][S3 && !A3 ? TM : 1][2], bf3[2][S3 ? TN : 1][3];
    v4f aq3[2][A3 ? TM : 1][3];          // A3: the three planes of the A rows' quad, like bf3
    const int brow3 = (wn0 + lr) * 12, bsw3 = (lr >> 2) & 3, arow3 = (wm0 + lr) * 12;

#define PEMP_READ(dst_, buf_, j_)                                                                                 \
    do {                                                                                                          \
        const v4f* Ab_ = As + (buf_) * BM * AQ;                                                                   \
        const v4f* Bb_ = Bs + (buf_) * BN * BQ;                                                                   \
        if constexpr (S3) {                                                                                       \
            const int p0_ = (4 * (j_) + 2 * lh) ^ rsw, p1_ = (4 * (j_) + 2 * lh + 1) ^ rsw;                       \
            const int pb_ = (2 * (j_) + lh) ^ bsw3;                                                               \
            if constexpr (A3) {         /* the planes of the row's quad 2 j + lh, as for B (wm0 % 32 == 0: same swizzle) */ \
                _Pragma("unroll") for (int mi = 0; mi < TM; ++mi)                                                 \
                    _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                              \
                        aq3[dst_][mi][pl] = Ab_[arow3 + mi * 32 * 12 + pl * 4 + pb_];                             \
            } else                                                                                                \
            _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) {                                                   \
                af3[dst_][mi][0] = Ab_[arow + mi * 256 + p0_];                                                    \
                af3[dst_][mi][1] = Ab_[arow + mi * 256 + p1_];                                                    \
            }                                                                                                     \
            _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                                     \
                _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                                  \
                    bf3[dst_][ni][pl] = Bb_[brow3 + ni * 32 * 12 + pl * 4 + pb_];                                 \
        } else if constexpr (R16) {                                                                               \
            const int pos_ = ((2 * (j_) + (g16 & 1)) ^ rsw16) * 4;                                                \
            const float* pa_ = (const float*)Ab_ + arow16 + pos_;                                                 \
            a16[dst_][0] = pa_[0];                                                                                \
            a16[dst_][1] = pa_[2];                                                                                \
            _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {                                                   \
                const float* pb_ = (const float*)Bb_ + brow16 + ni * 512 + pos_;                                  \
                b16[dst_][ni][0] = pb_[0];                                                                        \
                b16[dst_][ni][1] = pb_[2];                                                                        \
            }                                                                                                     \
        } else {                                                                                                  \
            const int pos_ = (2 * (j_) + lh) ^ rsw;                                                               \
            _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) af[dst_][mi] = Ab_[arow + mi * 256 + pos_];         \
            _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) bf[dst_][ni] = Bb_[brow + ni * 256 + pos_];         \
        }                                                                                                         \
    } while (0)

#define PEMP_MMA(src_)                                                                                            \
    do {                                                                                                          \
        if constexpr (S3) {                                                                                       \
            bf16x8 ah_[TM], am_[TM], al_[TM];                                                                     \
            _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) {                                                   \
                if constexpr (A3) {                                                                               \
                    ah_[mi] = __builtin_bit_cast(bf16x8, aq3[src_][mi][0]);                                       \
                    am_[mi] = __builtin_bit_cast(bf16x8, aq3[src_][mi][1]);                                       \
                    al_[mi] = __builtin_bit_cast(bf16x8, aq3[src_][mi][2]);                                       \
                } else split3_bf16(af3[src_][mi][0], af3[src_][mi][1], ah_[mi], am_[mi], al_[mi]);                \
            }                                                                                                     \
            _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) { \
                const bf16x8 bh_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][0]);                                  \
                const bf16x8 bm_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][1]);                                  \
                const bf16x8 bl_ = __builtin_bit_cast(bf16x8, bf3[src_][ni][2]);                                  \
                /* split3_mma6's products, in its order (as a call of it the K loops of the fp32-activation kernels */ \
                /* come out with another schedule and other register counts) */                                   \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al_[mi], bh_, acc[mi][ni], 0, 0, 0);        \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_[mi], bl_, acc[mi][ni], 0, 0, 0);        \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_[mi], bm_, acc[mi][ni], 0, 0, 0);        \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am_[mi], bh_, acc[mi][ni], 0, 0, 0);        \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_[mi], bm_, acc[mi][ni], 0, 0, 0);        \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah_[mi], bh_, acc[mi][ni], 0, 0, 0);        \
            }                                                                                                     \
        } else if constexpr (R16) {      /* column tiles interleaved: no MFMA waits for the one in front of it */  \
            _Pragma("unroll") for (int h_ = 0; h_ < 2; ++h_) _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)    \
                acc16[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a16[src_][h_], b16[src_][ni][h_], acc16[ni], 0, 0, 0); \
        } else                                                                                                    \
        _Pragma("unroll") for (int mi = 0; mi < TM; ++mi) _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {     \
            const v4f av = af[src_][mi], bv = bf[src_][ni];                                                       \
            if constexpr (BF16) {                                                                                 \
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av),              \
                                                                      __builtin_bit_cast(bf16x8, bv), acc[mi][ni], 0, 0, 0); \
                continue;                                                                                         \
            }                                                                                                     \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[mi][ni], 0, 0, 0);                 \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[mi][ni], 0, 0, 0);                 \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[mi][ni], 0, 0, 0);                 \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[mi][ni], 0, 0, 0);                 \
        }                                                                                                         \
    } while (0)

    // One K step.  DMA_: issue the LDS-DMA of step kt+2 (into the buffer this step frees); NEXT_: read the first
    // fragments of step kt+1.  The steady-state body has both and no branch, so that the scheduler can place the reads
    // and the DMA issue between the MFMAs of the last quarter; the last two steps are peeled.
#define PEMP_STEP(buf_, DMA_, NEXT_) PEMP_STEP_X(buf_, DMA_, NEXT_, true, true)
    // (PEMP_STEP_X: ADV_ false = the DMA_ issue is the NEXT tile's step 0, its K state already reset -- the persistent S3
    // kernel below; WVM_ false = the barrier waits for LDS reads only, not for the vector memory counter)
#define PEMP_STEP_X(buf_, DMA_, NEXT_, ADV_, WVM_)                                                                \
    do {                                                                                                          \
        PEMP_READ(1, buf_, 1);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PEMP_MMA(0);                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        if constexpr (!S3) {            /* S3: two half steps, the first one above */                             \
            PEMP_READ(0, buf_, 2);                                                                                \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            PEMP_MMA(1);                                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            PEMP_READ(1, buf_, 3);                                                                                \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            PEMP_MMA(0);                                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
        }                                                                                                         \
        /* every LDS read of `buf` by this wave has returned; this wave's DMA pieces of step kt+1 have landed */  \
        if (WVM_) {                                                                                               \
            __builtin_amdgcn_s_waitcnt(0x0070);      /* vmcnt(0) lgkmcnt(0), visible to hipcc's own wait bookkeeping */ \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* (the LDS-DMA loads are not in that bookkeeping) */ \
        } else {                                                                                                  \
            __builtin_amdgcn_s_waitcnt(0xC07F);      /* lgkmcnt(0) only (vmcnt 63 = no wait) */                   \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                    \
        }                                                                                                         \
        __builtin_amdgcn_s_barrier();   /* ... everybody's: `buf` is free for step kt+2, `buf^1` holds step kt+1 */ \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        if (NEXT_) PEMP_READ(0, (buf_) ^ 1, 0);                                                                   \
        if (DMA_) {                                                                                               \
            if (ADV_) PEMP_ADVANCE2();                                                                            \
            PEMP_DMA2(buf_);                                                                                      \
        }                                                                                                         \
        PEMP_MMA(1);                    /* the last quarter of step kt covers the reads / DMA issue above */      \
        if (DMA_) {                     /* ... placed BETWEEN its MFMAs: one LDS read / one DMA per MFMA slot */    \
            _Pragma("unroll") for (int k_ = 0; k_ < NMF; ++k_) {                                                  \
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                \
                _Pragma("unroll") for (int q_ = 0; q_ < PER; ++q_) {                                              \
                    const int it_ = k_ * PER + q_;                                                                \
                    if (it_ < NDS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                             \
                    else if (it_ < NDS + NDMA) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                 \
                }                                                                                                 \
            }                                                                                                     \
        }                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    } while (0)

    int kt = 0;
    PEMP_READ(0, 0, 0);
    for (; kt + 2 < nkl; ++kt) {
        const int buf = kt & 1;
        PEMP_STEP(buf, true, true);
    }
    if (kt + 1 < nkl) {
        const int buf = kt & 1;
        PEMP_STEP(buf, false, true);
        ++kt;
    }
    // Residual (shortcut) quads of small tiles are requested HERE, in front of the last K step's MFMAs, instead of inside
    // the epilogue where every tile would wait out a full memory latency between its LDS transpose and its stores.
    constexpr bool PRE = !R16 && TM * TN <= 2;
    static_assert(!ALSO || !PRE, "ALSO: a.res is no residual");
    // RS2 (PEMP_CONV_RES_S2; conv_dma2_rs2_kernel): the residual lies on a grid twice as fine as the output -- the prefetch below is
    // the one place of this body that addresses it, so the variant is this prefetch with conv_res_s2_pixel for the row
    static_assert(!RS2 || (PRE && S3 && !A3 && !SK && !PADV && EPI == 0), "RS2: the prefetched residual of the plain unsplit S3 form");
    v4f rpre[PRE ? TM * TN * 4 : 1];
#pragma unroll
    for (int i = 0; i < (PRE ? TM * TN * 4 : 1); ++i) rpre[i] = v4f{0.f, 0.f, 0.f, 0.f};
    if constexpr (PRE) {
        if (a.res) {
            const int rr_ = lane >> 3, c4_ = (lane & 7) * 4;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = m0 + wm0 + mi * 32 + rr_ + 8 * i, n = n0 + wn0 + ni * 32 + c4_;
                        if constexpr (RS2) rpre[(mi * TN + ni) * 4 + i] = m < a.M ? *(const v4f*)(a.res + (size_t)conv_res_s2_pixel(a, m) * a.ldr + n) : v4f{0.f, 0.f, 0.f, 0.f};
                        else rpre[(mi * TN + ni) * 4 + i] = m < a.M ? load_quad(a.res, (size_t)m * a.ldr + n, a.flags & PEMP_CONV_BF16_IO) : v4f{0.f, 0.f, 0.f, 0.f};
                    }
        }
    }
    {
        const int buf = kt & 1;
        PEMP_STEP(buf, false, false);
    }
    // (the K-loop macros stay defined for conv_dma2_s3p_body below)

    if constexpr (SK) {
        if (sk_r >= 0) {
            // partial accumulators in register order: float4 q of tile (mi, ni) of every lane, 1 KB per wave-instruction
            v4f* part = (v4f*)a.sk_ws + ((size_t)(sk_r * a.sk_S + piece) * NW + wave) * (TM * TN * 4 * 64) + lane;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const v4f v = {acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
                        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(part + ((mi * TN + ni) * 4 + q) * 64), "v"(v) : "memory");
                    }
            // The hand-off.  Producer side: EVERY store of the handed-off bytes is a device-scope write-through store (`sc0 sc1`,
            // 16 B), every storing wave drains them (`s_waitcnt vmcnt(0)`), the workgroup's barrier, then ONE lane's returning
            // agent-scope atomic add on the tile's counter.  Consumer side (the workgroup whose add came last, told by the returned
            // value): that lane runs an AGENT-SCOPE ACQUIRE (`buffer_inv sc1`: this CU's vector L1) and waits for it before it
            // publishes the verdict through LDS, the other waves join it at the workgroup barrier, and every load of the bytes is
            // a `global_load_dwordx4 sc0 sc1` to registers.  That is MI355X_MICROARCH.md's "Consumer, always" form (one returned
            // atomic -> one agent acquire -> vmcnt(0) -> workgroup barrier -> loads) with the sc1-store producer form; the loads stay
            // sc1 on top of it.  Round 4 shipped this WITHOUT the acquire, claiming the guide's table of hand-offs measured with
            // sc1 loads in its place -- but that table's row is for hipMalloc memory at one workgroup per CU, and this workspace is
            // hipExtMallocWithFlags(uncached) with two workgroups per CU for the 128-row tiles: outside the row in two cells, so
            // the acquire stays (the guide's condition (4)).  It costs one L1 invalidate per SPLIT TILE in ONE workgroup --
            // measured (A/B of PEMP_SK_ACQUIRE, profiles/r05_splitk_acquire_ab.txt): +0.4 ... 1.1 us on the 35-70 us launches of a one-episode step, nothing at the training shapes --
            // not the release/acquire fence PAIR in every workgroup that round 2 measured at 118 -> 94 TFLOP/s.  (Rounds 2-3 used
            // plain stores and non-temporal loads on uncached memory, which held in every test until one launch of one run returned
            // a different tile: `nt` is not a coherent access.)  The workspace stays uncached device memory on top of that.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this thread's partial stores have been acknowledged
            __syncthreads();                                               // ... everybody's
            int* flag = (int*)smem;
            if (tid == 0) {
                const int v = __hip_atomic_fetch_add(a.sk_cnt + sk_r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // only now this block counts as arrived
#if PEMP_SK_ACQUIRE
                if (v == a.sk_S - 1) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the invalidate has completed before anybody is released
                }
#endif
                *flag = v;
            }
            __syncthreads();
            const int arrived = *flag;
            __syncthreads();
            if (arrived != a.sk_S - 1) return;        // not the last piece of this tile: done
            if (tid == 0) __hip_atomic_store(a.sk_cnt + sk_r, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
            for (int pc = 0; pc < a.sk_S; ++pc) {     // pieces in ascending order, whichever arrived last: deterministic
                const v4f* src = (const v4f*)a.sk_ws + ((size_t)(sk_r * a.sk_S + pc) * NW + wave) * (TM * TN * 4 * 64) + lane;
                // two 32 x 32 sub-tiles (8 coherent 16-byte loads) in flight per wait; a lane's quads of one sub-tile lie 1 KB apart
                constexpr int NST = TM * TN;
#pragma unroll
                for (int st = 0; st < NST; st += 2) {
                    v4f t[8];
                    const v4f* q0 = src + (st * 4) * 64;
                    if constexpr (NST >= 2) {
                        const v4f* q1 = q0 + 4 * 64;
                        asm volatile("global_load_dwordx4 %0, %8, off sc0 sc1\n\t"
                                     "global_load_dwordx4 %1, %8, off offset:1024 sc0 sc1\n\t"
                                     "global_load_dwordx4 %2, %8, off offset:2048 sc0 sc1\n\t"
                                     "global_load_dwordx4 %3, %8, off offset:3072 sc0 sc1\n\t"
                                     "global_load_dwordx4 %4, %9, off sc0 sc1\n\t"
                                     "global_load_dwordx4 %5, %9, off offset:1024 sc0 sc1\n\t"
                                     "global_load_dwordx4 %6, %9, off offset:2048 sc0 sc1\n\t"
                                     "global_load_dwordx4 %7, %9, off offset:3072 sc0 sc1\n\t"
                                     "s_waitcnt vmcnt(0)"
                                     : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])
                                     : "v"(q0), "v"(q1)
                                     : "memory");
                    } else {
                        asm volatile("global_load_dwordx4 %0, %4, off sc0 sc1\n\t"
                                     "global_load_dwordx4 %1, %4, off offset:1024 sc0 sc1\n\t"
                                     "global_load_dwordx4 %2, %4, off offset:2048 sc0 sc1\n\t"
                                     "global_load_dwordx4 %3, %4, off offset:3072 sc0 sc1\n\t"
                                     "s_waitcnt vmcnt(0)"
                                     : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])
                                     : "v"(q0)
                                     : "memory");
                    }
#pragma unroll
                    for (int u = 0; u < (NST >= 2 ? 2 : 1); ++u) {
                        const int mi = (st + u) / TN, ni = (st + u) % TN;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            acc[mi][ni][4 * q] += t[4 * u + q].x;
                            acc[mi][ni][4 * q + 1] += t[4 * u + q].y;
                            acc[mi][ni][4 * q + 2] += t[4 * u + q].z;
                            acc[mi][ni][4 * q + 3] += t[4 * u + q].w;
                        }
                    }
                }
            }
        }
    }

    // ---- epilogue: transpose through LDS.  No LDS read and no DMA is outstanding after the loop's last barrier. ----
    float* Rall = (float*)smem + NW * 1024;          // EPI: [NW][TN][2][8][32] sums of the waves, behind their transpose patches
    constexpr int LDSF = 8 * (AQ * BM + BQ * BN);    // floats of operand staging (fp32 chain: 64 (BM + BN); S3: 64 BM + 96 BN)
    static_assert(EPI == 0 || NW * 1024 + NW * TN * 512 <= LDSF, "LDS: statistics area");
    static_assert(NW * 1024 <= LDSF, "LDS: one 4 KB transpose patch per wave");
    if constexpr (R16) conv_epilogue_r16<TN>(a, acc16, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane);
    else if constexpr (PRE) conv_epilogue_lds_pre<TM, TN, TM * TN * 4, EPI, DB, S3 ? 1 : 0>(a, acc, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane, rpre, Rall + wave * TN * 512);
    else if constexpr (EPI != 0) {
        const v4f none[1] = {{0.f, 0.f, 0.f, 0.f}};
        conv_epilogue_lds_pre<TM, TN, 1, EPI>(a, acc, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane, none, Rall + wave * TN * 512);
    } else conv_epilogue_lds<TM, TN, DB, ALSO ? 2 : S3 ? 1 : 0>(a, acc, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane);
    if constexpr (EPI != 0) {
        __syncthreads();
        conv_stats_store<BN, WGM, NW, TN>(a, Rall, bm, n0, tid);
    }
#endif
}

template <int BM, int BN, int WGM, int NW, bool PADV, int EPI = 0, bool SK = false, bool BF16 = false, bool DB = false, bool R16 = false,
          bool S3 = false>
__global__ __launch_bounds__(NW * 64) void conv_dma2_kernel(ConvArgs a) {
    conv_dma2_body<BM, BN, WGM, NW, PADV, EPI, SK, BF16, DB, R16, S3>(a, blockIdx.x, gridDim.x);
}

// the plain split3 form with a strided residual (PEMP_CONV_RES_S2; a kernel of its own: the instantiations of conv_dma2_kernel keep
// their names and their code).  Instantiated for id 43's shape: the one-tile id that serves any M
template <int BM, int BN, int WGM, int NW>
__global__ __launch_bounds__(NW * 64) void conv_dma2_rs2_kernel(ConvArgs a) {
    conv_dma2_body<BM, BN, WGM, NW, false, 0, false, false, false, false, true, false, false, true>(a, blockIdx.x, gridDim.x);
}

// ---- persistent split3 form (tile ids 47, 49 = the shapes of 43, 46; pemp_hip.h).  (41's shape, 128 x 128 in 4 waves, needs
// scratch at 2 waves per SIMD in this form: no id.)  The grid is the number of blocks
// that are resident at once (persistent_grid), and every block walks a fixed sequence of tiles (XcdTileRange, conv_common.h).
// Each accumulator sees the same MFMAs in the same order as in ids 41..46, and the epilogue does the same arithmetic: bit-identical.
// What the loop buys: one block per tile starts cold (two DMA stages issued and waited for in full before its first MFMA) and
// ends with a serial epilogue (residual loads in series with the LDS transpose and the stores).  Here, inside a block,
//  * the NEXT tile's step-0 DMA is issued at the barrier of this tile's second-to-last K step, into the stage buffer that step
//    frees, slotted between the MFMAs of its last quarter like a steady-state step's DMA (the per-row offsets and tap masks of
//    the next tile are computed in front of that step: the current tile's last DMA is behind it);
//  * the last K step's barrier waits for the LDS reads only (not for that DMA), and the waves' transpose patches go to the
//    buffer the last step read (the other stage buffer): no extra LDS;
//  * the residual quads of the wave tile and the scale / shift quads are requested in one batch after the last K step (behind
//    its last quarter's MFMAs, not under them: registers), so the epilogue waits once (not once per 32 x 32 sub-tile), and its
//    stores then issue back to back;
//  * the next tile's step-1 DMA follows the epilogue's stores, and the wait before its first MFMA is counted past the stores
//    (vector memory operations retire in order: stage 0 -> residual / scale loads -> stores -> stage 1).
// (The epilogue of OUT 0 is conv_epilogue_s3p, conv_common.h.)
// OUT 1 / 2 (below): the tile goes out pre-split (conv_store_split3_to on every 32 x 32 sub-tile, the scale / shift quads of the lane's
// 8 channels given), with ALSO behind the sub-tile's fp32 stores (conv_patch_store_f32) -- no residual in either.
template <int TM, int TN, bool ALSO>
__device__ __forceinline__ void conv_epilogue_s3p_split(const ConvArgs& a, f32x16 (&acc)[TM][TN], float* S, int m_base, int n_base, int lane,
                                                        const v4f (&scv)[ALSO ? TN : 1], const v4f (&shv)[ALSO ? TN : 1],
                                                        const v4f (&sc8)[TN][2], const v4f (&sh8)[TN][2]) {
    const int lr = lane & 31, lh = lane >> 5;
    unsigned short* y3 = (unsigned short*)(ALSO ? (void*)a.res : (void*)a.y);
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            PEMP_CONV_PATCH_PUT(S, acc[mi][ni], lr, lh);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
            if constexpr (ALSO)
                conv_patch_store_f32(a, S, m_base + mi * 32, n_base + ni * 32, lane, scv[ni], shv[ni], a.flags & PEMP_CONV_SHIFT_PER_IMAGE, nullptr, 0);
            conv_store_split3_to(a, y3, S, m_base + mi * 32, n_base + ni * 32, lane, sc8[ni], sh8[ni]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
        }
    }
}

// OUT: what a tile's epilogue writes.  0: y as fp32 (+ residual), through conv_epilogue_s3p.  1 (PEMP_CONV_OUT_SPLIT3, the PRODUCER
// variant): y pre-split and nothing else; the kernel has no residual path at all -- no batched residual quads live across the tile
// loop, no a.res test -- which is what keeps the split store out of scratch (as a run-time branch of OUT 0 it cost the 256 x 128
// shape 9-23 spilled registers).  2 (PEMP_CONV_OUT_SPLIT3_ALSO): y as fp32 and the same values pre-split through a.res, no residual
// either.  Tiles, K order and MFMA order do not depend on OUT.
template <int BM, int BN, int WGM, int NW, bool PADV, bool A3 = false, int OUT = 0>
__device__ __forceinline__ void conv_dma2_s3p_body(const ConvArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool S3 = true, R16 = false, BF16 = false;       // the K-loop macros' switches
    constexpr int WGN = NW / WGM;
    constexpr int RPI = NW * 8;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int BQ = 12;
    static_assert((BN * BQ) % (NW * 64) == 0, "S3: whole B DMA rounds");
    constexpr int AQ = A3 ? 12 : 8, XB = A3 ? 6 : 4;
    static_assert(!A3 || (BM * 12) % (NW * 64) == 0, "A3: whole A DMA rounds");
    constexpr int AL = A3 ? BM * AQ / (NW * 64) : BM / RPI, BL = BN * BQ / (NW * 64);
    constexpr int NMF = 6 * TM * TN, NDS = (A3 ? 3 : 2) * TM + 3 * TN, NDMA = AL + BL;
    constexpr int PER = (NDS + NDMA + NMF - 1) / NMF;
    // epilogue stores per thread of a wave tile inside the output: per sub-tile 4 fp32 quads and / or 2 rows x 3 planes
    constexpr int NST = TM * TN * (OUT == 0 ? 4 : OUT == 1 ? 6 : 10);
    static_assert(NDMA + NST <= 63, "vmcnt range");
    static_assert(NW <= BM / 32 + 3 * BN / 64, "one 4 KB transpose patch per wave inside ONE stage buffer");

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                      // [2][BM][AQ]
    v4f* Bs = smem + 2 * BM * AQ;        // [2][BN][BQ]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave / WGN) * WM;
    const int wn0 = (wave % WGN) * WN;
    const int lr = lane & 31, lh = lane >> 5;

    // the block's tile sequence: tiles tr.first + j, j = tr.idx, tr.idx + tr.step, ... < tr.count
    const int ntn = a.Cout / BN;
    const XcdTileRange tr((a.M + BM - 1) / BM * ntn, (int)blockIdx.x, (int)gridDim.x);
    if (tr.idx >= tr.count) return;             // (the launch clamps the grid to the tile count: not expected)
    int j = tr.idx;
    int m0 = (a.bm_first + (tr.first + j) / ntn) * BM, n0 = ((tr.first + j) % ntn) * BN;

    const int p = tid & 7;
    const int r = tid >> 3;
    const int sq = p ^ ((r >> 1) & 7);
    const int bias_pix = a.pad * a.W + a.pad;
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.x - (ptrdiff_t)bias_pix * a.ldx * XB), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);
    const unsigned padv_off = PADV ? (unsigned)((const char*)a.padv - ((const char*)a.x - (ptrdiff_t)bias_pix * a.ldx * XB)) + (A3 ? 0 : sq * 16) : 0x80000000u;
    // A3: six rows per thread instead of four -- the tap masks of two rows share a register (<= 16 taps), and the lane's (swizzled)
    // quad inside the row's 192 bytes, which differs per DMA round, is a_voff mod 192 (PADV reads it back from there)
    constexpr int AINV = A3 ? AL / 2 : AL;
    static_assert(!A3 || AL % 2 == 0, "A3: tap masks in pairs");
    unsigned a_voff[AL], a_inv[AINV], b_voff[BL];
    // per-row byte offsets and tap masks of the tile at (m0_, n0_): conv_dma2_body's, expression for expression
    auto offsets = [&](const int m0_, const int n0_) {
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            int arow_ = r + RPI * i, asrc_ = sq * 16;
            if constexpr (A3) {     // LDS quad q of the A tile = row q / 12, position q % 12: the B tile's layout and swizzle
                const int q = i * NW * 64 + tid, pos = q % 12;
                arow_ = q / 12;
                asrc_ = PEMP_SPLIT3_SWZ(arow_, pos) * 16;
            }
            const int m = m0_ + arow_;
            const bool ok = m < a.M;
            const int mm = ok ? m : 0;
            const int img = mm / a.HoWo;
            const int rem = mm - img * a.HoWo;
            const int ho = rem / a.Wo;
            const int wo = rem - ho * a.Wo;
            const int hi0 = ho * a.stride - a.pad;
            const int wi0 = wo * a.stride - a.pad;
            a_voff[i] = A3 ? (unsigned)(((img * a.H + hi0) * a.W + wi0 + bias_pix) * a.ldx * 6 + asrc_)
                           : (unsigned)(((img * a.H + hi0) * a.W + wi0 + bias_pix) * a.ldx + sq * 4) * 4u;
            unsigned mask = 0;
            int kh = 0, kw = 0;
            for (int t = 0; t < a.ntaps; ++t) {
                const int hi = hi0 + kh * a.dil, wi = wi0 + kw * a.dil;
                if (ok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W) mask |= 1u << t;
                if (++kw == a.KW) {
                    kw = 0;
                    ++kh;
                }
            }
            if constexpr (!A3) a_inv[i] = ~mask;
            else if (i & 1) a_inv[i >> 1] |= ~mask << 16;
            else a_inv[i >> 1] = ~mask & 0xFFFFu;
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
            const int src = PEMP_SPLIT3_SWZ(row, pos);
            b_voff[i] = (unsigned)((n0_ + row) * a.Kpad * 6 + src * 16);
        }
    };
    offsets(m0, n0);

    int tap = 0, cb = 0, kh_i = 0, kw_i = 0;
    const int tapw = a.dil * a.ldx * XB, taph = a.dil * a.W * a.ldx * XB;
    int multi, s_kw, s_ntaps;
    asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %3\n\tv_readfirstlane_b32 %1, %4\n\tv_readfirstlane_b32 %2, %5\n\ts_nop 4"
                 : "=s"(multi), "=s"(s_kw), "=s"(s_ntaps)
                 : "v"(a.ntaps > 1 ? 1 : 0), "v"(a.KW), "v"(a.ntaps));
    const int nkl = a.nk;

    PEMP_DMA2(0);
    if (nkl > 1) {
        PEMP_ADVANCE2();
        PEMP_DMA2(1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    const int rsw = (lr >> 1) & 7;
    const int arow = (wm0 + lr) * 8, brow = (wn0 + lr) * 8;
    v4f af[2][1], bf[2][1];                      // (the macros' other variants: never used here)
    const int r16 = lane & 15, g16 = lane >> 4;
    const int rsw16 = (r16 >> 1) & 7;
    const int arow16 = (wm0 + r16) * 32 + (g16 >> 1), brow16 = (wn0 + r16) * 32 + (g16 >> 1);
    float a16[2][2], b16[2][1][2];
    v4f acc16[1];
    v4f af3[2][A3 ? 1 : TM][2], bf3[2][TN][3];
    v4f aq3[2][A3 ? TM : 1][3];
    const int brow3 = (wn0 + lr) * 12, bsw3 = (lr >> 2) & 3, arow3 = (wm0 + lr) * 12;
    const int rr_ = lane >> 3, c4_ = (lane & 7) * 4;

    int pb = 0;                                  // stage buffer of the tile's K step 0
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
        const int m0n = more ? (a.bm_first + (tr.first + jn) / ntn) * BM : m0, n0n = more ? ((tr.first + jn) % ntn) * BN : n0;

        int kt = 0;
        PEMP_READ(0, pb, 0);
        for (; kt + 2 < nkl; ++kt) {
            const int buf = (kt + pb) & 1;
            PEMP_STEP(buf, true, true);
        }
        // every DMA of this tile is issued: the offsets and the K state become the next tile's.  After the block's last tile the
        // step-0 DMA below still goes out (ONE form of the step: two would hold two sets of accumulators), with every offset
        // past the 2 GiB range: the hardware writes zeros into the free buffer and reads no memory
        if (more) {
            offsets(m0n, n0n);
        } else {
#pragma unroll
            for (int i = 0; i < AL; ++i) a_voff[i] = 0x80000000u;
#pragma unroll
            for (int i = 0; i < AINV; ++i) a_inv[i] = 0u;
#pragma unroll
            for (int i = 0; i < BL; ++i) b_voff[i] = 0x80000000u;
        }
        tap = 0;
        cb = 0;
        kh_i = 0;
        kw_i = 0;
        if (kt + 1 < nkl) {
            const int buf = (kt + pb) & 1;
            PEMP_STEP_X(buf, true, true, false, true);       // + the next tile's step 0, into `buf`
            ++kt;
        }
        const int bl = (kt + pb) & 1;            // the last step's buffer: the transpose patches go there
        v4f rres[OUT == 0 ? TM * TN * 4 : 1], scv[OUT == 1 ? 1 : TN], shv[OUT == 1 ? 1 : TN];
        v4f sc8[OUT == 0 ? 1 : TN][2], sh8[OUT == 0 ? 1 : TN][2];      // OUT != 0: the quads of conv_store_split3_to's 8 channels per lane
        auto epi_loads = [&]() {
            const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
            if constexpr (OUT != 1) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int n = n0 + wn0 + ni * 32 + c4_;
                    scv[ni] = a.scale ? *(const v4f*)(a.scale + n) : v4f{1.f, 1.f, 1.f, 1.f};
                    shv[ni] = (a.shift && !per_img) ? *(const v4f*)(a.shift + n) : v4f{0.f, 0.f, 0.f, 0.f};
                }
            }
            if constexpr (OUT != 0) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) conv_split3_affine(a, n0 + wn0 + ni * 32 + (lane & 3) * 8, sc8[ni], sh8[ni]);
                return;
            }
#pragma unroll
            for (int i = 0; i < (OUT == 0 ? TM * TN * 4 : 1); ++i) rres[i] = v4f{0.f, 0.f, 0.f, 0.f};
            if (a.res) {
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int m = m0 + wm0 + mi * 32 + rr_ + 8 * i, n = n0 + wn0 + ni * 32 + c4_;
                            rres[(mi * TN + ni) * 4 + i] = m < a.M ? load_quad(a.res, (size_t)m * a.ldr + n, a.flags & PEMP_CONV_BF16_IO)
                                                                   : v4f{0.f, 0.f, 0.f, 0.f};
                        }
            }
        };
        PEMP_STEP_X(bl, false, false, true, false);      // the barrier waits for LDS reads only: the next tile's DMA flies on
        epi_loads();             // behind the last step's MFMAs: in front of that step they would cost 64 x 64 its fourth wave per
                                 // SIMD (scratch at 128 VGPRs), and 256 x 128 has no registers left under them

        float* patch = wave < BM / 32 ? (float*)(As + bl * BM * AQ + wave * 256) : (float*)(Bs + bl * BN * BQ + (wave - BM / 32) * 256);
        if constexpr (OUT == 0) conv_epilogue_s3p<TM, TN>(a, acc, patch, m0 + wm0, n0 + wn0, lane, rres, scv, shv);
        else conv_epilogue_s3p_split<TM, TN, OUT == 2>(a, acc, patch, m0 + wm0, n0 + wn0, lane, scv, shv, sc8, sh8);
        if (!more) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no LDS-DMA outlives the block
            break;
        }

        // the next tile: its step 1 goes into `bl` once every wave is done with its patch
        const int pbn = (pb + nkl) & 1;
        __builtin_amdgcn_s_barrier();
        if (nkl > 1) {
            PEMP_ADVANCE2();
            PEMP_DMA2(bl);
            if (m0 + wm0 + WM <= a.M) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA + NST) : "memory");   // step 0 has landed
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");     // (fewer stores than NST: do not count them)
        } else {
            PEMP_DMA2(pbn);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        j = jn;
        m0 = m0n;
        n0 = n0n;
        pb = pbn;
    }
#endif
}

// (waves per SIMD: 43's shape is held to 4 by its LDS -- the registers must not take that below 4)
template <int BM, int BN, int WGM, int NW, bool PADV>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(BM == 64 ? 4 : 2))) void conv_dma2_s3p_kernel(ConvArgs a) {
    conv_dma2_s3p_body<BM, BN, WGM, NW, PADV>(a);
}

// pre-split activations (A3): the one-tile and the persistent form, ids 146 / 149 (kernels of their own: the instantiations of
// conv_dma2_kernel / conv_dma2_s3p_kernel keep their names)
template <int BM, int BN, int WGM, int NW, bool PADV>
__global__ __launch_bounds__(NW * 64) void conv_dma2_a3_kernel(ConvArgs a) {
    conv_dma2_body<BM, BN, WGM, NW, PADV, 0, false, false, false, false, true, true>(a, blockIdx.x, gridDim.x);
}

template <int BM, int BN, int WGM, int NW, bool PADV>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void conv_dma2_a3p_kernel(ConvArgs a) {
    conv_dma2_s3p_body<BM, BN, WGM, NW, PADV, true>(a);
}

// the variants that store pre-split (kernels of their own again): the producer forms of 47 / 49 (conv_dma2_s3po_kernel, OUT 1) and
// of 149 (conv_dma2_a3po_kernel, OUT 1), and 146 / 149 with the second, pre-split output (conv_dma2_a3o_kernel; _a3po_, OUT 2)
template <int BM, int BN, int WGM, int NW, bool PADV, int OUT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(BM == 64 ? 4 : 2))) void conv_dma2_s3po_kernel(ConvArgs a) {
    conv_dma2_s3p_body<BM, BN, WGM, NW, PADV, false, OUT>(a);
}

template <int BM, int BN, int WGM, int NW, bool PADV, int OUT>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void conv_dma2_a3po_kernel(ConvArgs a) {
    conv_dma2_s3p_body<BM, BN, WGM, NW, PADV, true, OUT>(a);
}

template <int BM, int BN, int WGM, int NW, bool PADV>
__global__ __launch_bounds__(NW * 64) void conv_dma2_a3o_kernel(ConvArgs a) {
    conv_dma2_body<BM, BN, WGM, NW, PADV, 0, false, false, false, false, true, true, true>(a, blockIdx.x, gridDim.x);
}
#undef PEMP_STEP_X
#undef PEMP_STEP
#undef PEMP_DMA2
#undef PEMP_ADVANCE2
#undef PEMP_READ
#undef PEMP_MMA

// Several INDEPENDENT convs of the same tile shape in ONE launch: member i owns the blocks [first[i], first[i] + nblk[i]) (the
// first[] are multiples of 8, so that a block's XCD is the same function of its index inside the member as in a launch of its
// own; the few blocks in between return at once).  A one-episode step has 5202 feature rows -- 41 to 82 tiles per conv on 256
// CUs -- and convs that do not depend on each other (the dilated ASPP branches; a stage's downsample conv beside its conv1):
// together they fill the chip without splitting K and without one launch + drain per member.  Same tiles, same K order: every
// member's result is bit-identical to its own launch.
template <int BM, int BN, int WGM, int NW, bool PADV, bool R16 = false, bool S3 = false>
__global__ __launch_bounds__(NW * 64) void conv_dma2_group_kernel(ConvGroupArgs g) {
    int which = 0;
#pragma unroll
    for (int i = 1; i < CONV_GROUP_MAX; ++i) which += (i < g.n && (int)blockIdx.x >= g.first[i]) ? 1 : 0;
    const int bid = (int)blockIdx.x - g.first[which];
    if (bid >= g.nblk[which]) return;
    conv_dma2_body<BM, BN, WGM, NW, PADV, 0, false, false, false, R16, S3>(g.a[which], bid, g.nblk[which]);
}

// ---- host side.  Every launch entry takes a SHAPE index (a row of conv_tiles.h's table), picks its kernel through
// with_tile<family> and launches it through launch_with_lds. ----

// the kernel of shape T with the variant switches of conv_dma2_kernel
template <class T, bool PADV, int EPI = 0, bool SK = false, bool BF16 = false, bool DB = false, bool R16 = false, bool S3 = false>
constexpr auto dma2_kernel = conv_dma2_kernel<T::BM, T::BN, T::WGM, T::NW, PADV, EPI, SK, BF16, DB, R16, S3>;

// fp32 chain: statistics / BatchNorm-backward epilogue, padding vector or plain
template <class T, bool SK>
static auto dma2_fp32_kernel(const ConvArgs& a) {
    return a.stats ? (a.bz ? dma2_kernel<T, false, 2, SK> : dma2_kernel<T, false, 1, SK>)
                   : a.padv ? dma2_kernel<T, true, 0, SK> : dma2_kernel<T, false, 0, SK>;
}

template <class T, bool R16 = false, bool S3 = false>
static int launch_dma2_group(ConvGroupArgs& g, hipStream_t st) {
    auto kern = g.a[0].padv ? conv_dma2_group_kernel<T::BM, T::BN, T::WGM, T::NW, true, R16, S3>
                            : conv_dma2_group_kernel<T::BM, T::BN, T::WGM, T::NW, false, R16, S3>;
    int grid = 0;
    for (int i = 0; i < g.n; ++i) {
        g.first[i] = grid;
        g.nblk[i] = tile_grid<T>(g.a[i]);
        grid += (g.nblk[i] + 7) & ~7;
    }
    g.first[g.n] = grid;
    return launch_with_lds(kern, grid, T::NW * 64, S3 ? tile_lds_s3<T>() : tile_lds<T>(), st, g, "conv_dma2/group");
}

// Hybrid launch (tile id 29) for convs of a FEW rounds: 32 x 32 wave tiles are the efficient shape, but T of them on 1024 SIMDs
// take ceil(T / 1024) rounds (a one-episode 256-channel conv: 1304 tiles, two rounds, the second 27 % full).  Here the rows that
// fill whole rounds go to the 64 x 64 tile and the remaining rows to 16-row wave tiles (half the work per K step) in the SAME
// grid: the SIMDs that would have taken a second 32 x 32 tile take a 16 x 32 one beside their first, 1.5 instead of 2 units per
// K step.  Both members run the K loop in the same order: bit-identical to every other variant.
static int g_simds_of[64] = {0};     // SIMD count per device id (filled on first use; racing fills write the same value)

template <bool PADV>
__global__ __launch_bounds__(256) void conv_dma2_hybrid_kernel(ConvGroupArgs g) {
    const int bid = (int)blockIdx.x;
    if (bid < g.first[1]) {
        if (bid < g.nblk[0]) conv_dma2_body<64, 64, 2, 4, PADV, 0, false, false, false, false>(g.a[0], bid, g.nblk[0]);
    } else {
        conv_dma2_body<32, 64, 2, 4, PADV, 0, false, false, false, true>(g.a[1], bid - g.first[1], g.nblk[1]);
    }
}

// SIMDs of the current device (4 per CU; filled on first use)
int conv_dma2_simds() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;        // no device (CPU-side query): the MI355X count
    if (!g_simds_of[dev]) {
        int cus = 0;
        if (dev == 63 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        g_simds_of[dev] = 4 * cus;
    }
    return g_simds_of[dev];
}

// rows of an M x Cout conv that go to the 64 x 64 tile in the hybrid launch (the rest: 16-row tiles); 0 = no such split
int conv_dma2_hybrid_rows(int M, int Cout) {
    const int g_simds = conv_dma2_simds();
    if (M <= 0 || Cout < 64 || Cout % 64) return 0;
    const int per32 = Cout / 32;                                 // 32 x 32 wave tiles per 32 output rows
    const int rounds = (int)(((long long)M / 32 * per32) / g_simds);        // whole rounds the 32-row tiles fill
    if (rounds < 1 || rounds > 8) return 0;                      // (many rounds: the quantisation loss is small anyway)
    const int rows_a = ((long long)rounds * g_simds / per32) * 32 / 64 * 64;
    const int rest = M - rows_a;
    if (rows_a <= 0 || rest <= 0 || (long long)cdiv(rest, 16) * per32 > g_simds) return 0;
    return rows_a;
}

int launch_conv_dma2_hybrid(const ConvArgs& a, hipStream_t st) {
    if (a.stats || (a.flags & PEMP_CONV_BF16_IO)) return -2;
    const int rows_a = conv_dma2_hybrid_rows(a.M, a.Cout);
    if (!rows_a) return -2;
    const int rest = a.M - rows_a;
    ConvGroupArgs g;
    g.n = 2;
    g.a[0] = a;
    g.a[0].M = rows_a;
    g.a[1] = a;
    g.a[1].bm_first = rows_a / 32;
    for (int i = 2; i < CONV_GROUP_MAX; ++i) g.a[i] = a;
    g.nblk[0] = (rows_a / 64) * (a.Cout / 64);
    g.nblk[1] = cdiv(rest, 32) * (a.Cout / 64);
    g.first[0] = 0;
    g.first[1] = (g.nblk[0] + 7) & ~7;
    g.first[2] = g.first[1] + g.nblk[1];
    auto kern = a.padv ? conv_dma2_hybrid_kernel<true> : conv_dma2_hybrid_kernel<false>;
    return launch_with_lds(kern, g.first[2], 256, tile_lds<Tile<3>>(), st, g, "conv_dma2/hybrid");
}

int launch_conv_dma2_group(int shape, ConvGroupArgs& g, hipStream_t st) {
    return with_tile<FamGroup>(shape, [&](auto t) { return launch_dma2_group<decltype(t), decltype(t)::BM == 32>(g, st); });
}

int launch_conv_dma2_bf16(int shape, const ConvArgs& a, hipStream_t st) {
    return with_tile<FamFp32>(shape, [&](auto t) {
        using T = decltype(t);
        auto kern = a.padv ? dma2_kernel<T, true, 0, false, true> : dma2_kernel<T, false, 0, false, true>;
        return launch_with_lds(kern, tile_grid<T>(a), T::NW * 64, tile_lds<T>(), st, a, "conv_dma2/bf16");
    });
}

// The tiles of a launch are dealt to the 256 CUs in rounds; T mod 256 tiles are left for a last, partly filled round (8 images
// of 51 x 51 pixels: 326 tiles of 128 x 128 for 256 output channels -- the chip is busy for two rounds and does the work
// of 1.27).  Those remainder tiles are split along K into as many pieces as keep the piece count <= 256, so that the last
// round is short instead of partly filled.
SplitKPlan conv_dma2_splitk_plan(int shape, const ConvArgs& a) {
    SplitKPlan p = {0, 0, 1, 0};
    if (!in_family<FamSplitK>(shape)) return p;
    const int bm = kTileShapes[shape].bm, bn = kTileShapes[shape].bn;
    const int T = cdiv(a.M, bm) * (a.Cout / bn);
    const int rem = T % 256;
    p.full = T;
    if (rem == 0 || rem > 128) return p;
    int pieces = 256 / rem;
    if (pieces > a.nk / 4) pieces = a.nk / 4;
    if (pieces > 16) pieces = 16;
    if (pieces < 2) return p;
    p.full = T - rem;
    p.split = rem;
    p.pieces = pieces;
    p.ws_bytes = 1024 + (size_t)rem * pieces * bm * bn * sizeof(float);     // counters (<= 128 ints), then the partial tiles
    return p;
}

// conv + DropBlock2D's row scaling in the epilogue (pemp_conv2d_dropblock_nhwc_f32): DB instantiations, unsplit and split-K
int launch_conv_dma2_db(int shape, ConvArgs a, void* ws, size_t ws_bytes, bool split, hipStream_t st) {
    const SplitKPlan p = split ? conv_dma2_splitk_plan(shape, a) : SplitKPlan{0, 0, 1, 0};
    const int sk_grid = p.pieces >= 2 ? bind_splitk(a, p, ws, ws_bytes) : 0;
    if (sk_grid < 0) return -1;
    return with_tile<FamFp32>(shape, [&](auto t) {
        using T = decltype(t);
        auto kern = sk_grid ? dma2_kernel<T, false, 0, true, false, true> : dma2_kernel<T, false, 0, false, false, true>;
        return launch_with_lds(kern, sk_grid ? sk_grid : tile_grid<T>(a), T::NW * 64, tile_lds<T>(), st, a, "conv_dma2/dropblock");
    });
}

int launch_conv_dma2_splitk(int shape, ConvArgs a, void* ws, size_t ws_bytes, hipStream_t st) {
    const SplitKPlan p = conv_dma2_splitk_plan(shape, a);
    if (p.pieces < 2 || (a.padv && a.stats)) return launch_conv_dma2(shape, a, st);       // nothing to split: the plain variant
    const int grid = bind_splitk(a, p, ws, ws_bytes);
    if (grid < 0) return -1;
    return with_tile<FamSplitK>(shape, [&](auto t) {
        using T = decltype(t);
        return launch_with_lds(dma2_fp32_kernel<T, true>(a), grid, T::NW * 64, tile_lds<T>(), st, a, "conv_dma2/splitk");
    });
}

// ---- split3 family: the S3 body on the shapes 1..4 and 6 (shape 5, 128 x 64 in 8 waves, has no whole B DMA rounds at
// 192 bytes per row; shape 7, 256 x 256, would need all 160 KiB of LDS).
// Wave grids (the table's wgm3): the A fragment is split (split3_bf16, ~9 VALU per element pair) by every wave that reads it, and
// the pieces feed 6 TN MFMAs.  So ids 41, 42 and 46 give each wave a FULL-WIDTH strip (WGM = NW: 32 rows x BN columns, TN = BN / 32),
// and every activation row of a block is split once instead of once per wave column: 41 / 46 go from ~4.0 to ~2.2 VALU per MFMA in
// the K loop (scratch/s3_isa_mix.py).  43 (64 x 64, 4 waves) and 44 (128 x 128, 8 waves) have fewer 32-row strips than waves and keep
// two wave columns.  The MFMA sequence each accumulator sees does not depend on the grid: every id stays bit-identical. ----
static int split3_check(bool shape_ok, int shape, const ConvArgs& a) {       // a shape of the family, the plain epilogue
    if (shape_ok && !a.stats && !a.rowmask && !(a.flags & PEMP_CONV_BF16_IO)) return 0;
    set_error("conv split3: tile %d / epilogue outside the family", shape);
    return -1;
}

int launch_conv_dma2_split3(int shape, ConvArgs a, void* ws, size_t ws_bytes, bool split, hipStream_t st) {
    if (split3_check(in_family<FamSplit3>(shape), shape, a)) return -1;
    const SplitKPlan p = split ? conv_dma2_splitk_plan(shape, a) : SplitKPlan{0, 0, 1, 0};
    const int sk_grid = p.pieces >= 2 ? bind_splitk(a, p, ws, ws_bytes) : 0;
    if (sk_grid < 0) return -1;
    if (a.flags & PEMP_CONV_RES_S2) {    // the residual on a grid twice as fine: id 43's shape, unsplit, zero padding
        if (shape != 3 || split || a.padv || !a.res || a.Hr < 1 || a.Wr < 1) {
            set_error("conv split3: PEMP_CONV_RES_S2 needs the 64 x 64 tile (id 43), unsplit, with a residual and no padding value");
            return -1;
        }
        using T = Tile<3, true>;
        return launch_with_lds(conv_dma2_rs2_kernel<T::BM, T::BN, T::WGM, T::NW>, tile_grid<T>(a), T::NW * 64, tile_lds_s3<T>(), st, a,
                               "conv_dma2/split3/res_s2");
    }
    return with_tile<FamSplit3>(shape, [&](auto t) {
        using T = decltype(t);
        auto kern = sk_grid ? (a.padv ? dma2_kernel<T, true, 0, true, false, false, false, true> : dma2_kernel<T, false, 0, true, false, false, false, true>)
                            : (a.padv ? dma2_kernel<T, true, 0, false, false, false, false, true> : dma2_kernel<T, false, 0, false, false, false, false, true>);
        return launch_with_lds(kern, sk_grid ? sk_grid : tile_grid<T>(a), T::NW * 64, tile_lds_s3<T>(), st, a,
                               sk_grid ? "conv_dma2/split3/splitk" : "conv_dma2/split3");
    });
}

// ... with the statistics epilogue (EPI 1; pemp_split3_conv2d_stats_nhwc_f32): the K loop and the MFMA order of the plain form, so
// z is bit-identical to launch_conv_dma2_split3 of the same shape; the partial rows are conv_stats_store's.  Unsplit, zero
// padding, no affine / residual -- the frozen trunks of the head trainers.  FamSplit3Stats (conv_tiles.h) lists the shapes.
bool conv_dma2_split3_stats_shape(int shape) { return in_family<FamSplit3Stats>(shape); }

int launch_conv_dma2_split3_stats(int shape, const ConvArgs& a, hipStream_t st) {
    if (!a.stats || a.bz || a.padv || a.res || a.rowmask || a.scale || a.shift || a.flags) {
        set_error("conv split3 statistics: plain conv with a partials buffer only");
        return -1;
    }
    return with_tile<FamSplit3Stats>(shape, [&](auto t) {
        using T = decltype(t);
        return launch_with_lds(dma2_kernel<T, false, 1, false, false, false, false, true>, tile_grid<T>(a), T::NW * 64, tile_lds_s3<T>(), st, a,
                               "conv_dma2/split3/stats");
    });
}

// persistent forms (ids 47, 49; A3: 149): grid = resident blocks (occupancy of the instantiation x CUs, taken once), at most the tile count
template <class T, bool A3 = false, int OUT = 0>
static int launch_dma2_s3p(const ConvArgs& a, hipStream_t st) {
    constexpr size_t lds = A3 ? tile_lds_a3<T>() : tile_lds_s3<T>();
    auto s3p_kernel = [](auto padv) {
        if constexpr (OUT != 0 && A3) return conv_dma2_a3po_kernel<T::BM, T::BN, T::WGM, T::NW, decltype(padv)::value, OUT>;
        else if constexpr (OUT != 0) return conv_dma2_s3po_kernel<T::BM, T::BN, T::WGM, T::NW, decltype(padv)::value, OUT>;
        else if constexpr (A3) return conv_dma2_a3p_kernel<T::BM, T::BN, T::WGM, T::NW, decltype(padv)::value>;
        else return conv_dma2_s3p_kernel<T::BM, T::BN, T::WGM, T::NW, decltype(padv)::value>;
    };
    auto kern = a.padv ? s3p_kernel(std::true_type{}) : s3p_kernel(std::false_type{});
    static int occ[2] = {0, 0};          // blocks per CU of the two instantiations
    int grid = 0;
    const int rc = persistent_grid(kern, T::NW * 64, lds, tile_grid<T>(a), occ[a.padv ? 1 : 0], "conv split3 persistent", grid);
    if (rc) return rc;
    return launch_with_lds(kern, grid, T::NW * 64, lds, st, a, "conv_dma2/split3/persistent");
}

// the shapes whose persistent form has a producer variant (PEMP_CONV_OUT_SPLIT3): both -- 64 x 64 keeps its 128 registers
struct FamPersistOut { static constexpr unsigned shapes = shape_bits({3, 6}); static constexpr bool s3 = true; };
bool conv_dma2_persist_out_split3(int shape) { return in_family<FamPersistOut>(shape); }

int launch_conv_dma2_split3_persist(int shape, const ConvArgs& a, hipStream_t st) {
    if (split3_check(true, shape, a)) return -1;
    if (a.flags & PEMP_CONV_OUT_SPLIT3) return with_tile<FamPersistOut>(shape, [&](auto t) { return launch_dma2_s3p<decltype(t), false, 1>(a, st); });
    return with_tile<FamPersist>(shape, [&](auto t) { return launch_dma2_s3p<decltype(t)>(a, st); });
}

struct TileA3 { static constexpr int BM = 256, BN = 128, NW = 8, WGM = 4; };
// pre-split activations (ids 146 / 149): the 256 x 128 8-wave shape only.  (128 x 128 would hold 2 x 12 x 256 quads = 96 KiB of
// LDS per block: one block per CU, where its fp32-input form has two -- no id.)
int launch_conv_dma2_split3_pre(int shape, bool persistent, const ConvArgs& a, hipStream_t st) {
    if (split3_check(shape == 6, shape, a)) return -1;
    // the wave grid: 4 x 2 waves of 64 x 64, not the fp32-input form's 8 full-width strips of 32 x 128 -- those exist to split each
    // activation once per block; with nothing to split, the squarer wave tile reads 24 KB of LDS per K step instead of 30
    using T = TileA3;
    static_assert(T::BM == kTileShapes[6].bm && T::BN == kTileShapes[6].bn && T::NW == kTileShapes[6].nw, "shape 6");
    const bool also = a.flags & PEMP_CONV_OUT_SPLIT3_ALSO;
    if (persistent) return also ? launch_dma2_s3p<T, true, 2>(a, st) : (a.flags & PEMP_CONV_OUT_SPLIT3) ? launch_dma2_s3p<T, true, 1>(a, st) : launch_dma2_s3p<T, true>(a, st);
    auto kern = also ? (a.padv ? conv_dma2_a3o_kernel<T::BM, T::BN, T::WGM, T::NW, true> : conv_dma2_a3o_kernel<T::BM, T::BN, T::WGM, T::NW, false>)
                     : (a.padv ? conv_dma2_a3_kernel<T::BM, T::BN, T::WGM, T::NW, true> : conv_dma2_a3_kernel<T::BM, T::BN, T::WGM, T::NW, false>);
    return launch_with_lds(kern, tile_grid<T>(a), T::NW * 64, tile_lds_a3<T>(), st, a, "conv_dma2/split3/presplit");
}

int launch_conv_dma2_group_split3(int shape, ConvGroupArgs& g, hipStream_t st) {
    if (shape == 5) {
        set_error("conv split3: no 128 x 64 8-wave form");
        return -1;
    }
    return with_tile<FamSplit3>(shape, [&](auto t) { return launch_dma2_group<decltype(t), false, true>(g, st); });
}

// [Cout][Kpad] fp32 -> [Cout][Kpad / 32][3][32] bf16: per row and 32-channel K step the h, m and l planes of split3_bf16
__global__ __launch_bounds__(256) void pack_split3_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // one 8-channel octet (= one quad of each plane)
    if (i >= n8) return;
    const v4f x0 = *(const v4f*)(w + i * 8), x1 = *(const v4f*)(w + i * 8 + 4);
    bf16x8 h, m, l;
    split3_bf16(x0, x1, h, m, l);
    const long long step = i >> 2;                   // (row, K step): 4 octets each
    unsigned short* o = out + step * 96 + (i & 3) * 8;
    *(bf16x8*)o = h;
    *(bf16x8*)(o + 32) = m;
    *(bf16x8*)(o + 64) = l;
}

int pack_split3(const float* w, void* out, int cout, int kpad, hipStream_t st) {
    const long long n8 = (long long)cout * kpad / 8;
    hipLaunchKernelGGL(pack_split3_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, w, (unsigned short*)out, n8);
    return launch_status("pack_split3");
}

// true when the geometry / operands fit this variant (the caller falls back to conv_dma.hip otherwise)
bool conv_dma2_supported(const ConvArgs& a) {
    if ((a.flags & PEMP_CONV_STEM4) || a.ntaps > 32 || (a.stats && a.padv)) return false;
    const long long eb = (a.flags & PEMP_CONV_IN_SPLIT3) ? 6 : 4;       // bytes per activation element (pre-split: three bf16)
    const long long xbytes = ((long long)a.N * a.H * a.W + (long long)a.pad * a.W + a.pad + (long long)a.dil * (a.KH - 1) * a.W +
                              (long long)a.dil * (a.KW - 1)) * a.ldx * eb;
    const long long wbytes = (long long)a.Cout * a.Kpad * 4;
    if (a.padv) {           // the padding vector must sit behind the activations, inside the 2 GiB window of their descriptor,
                            // and far enough in that subtracting the largest tap displacement leaves a non-negative offset
        const long long behind = (const char*)a.padv - (const char*)a.x - (long long)a.N * a.H * a.W * a.ldx * eb;
        const long long d = (const char*)a.padv - (const char*)a.x + ((long long)a.pad * a.W + a.pad) * a.ldx * eb;
        const long long tapmax = ((long long)a.dil * (a.KH - 1) * a.W + (long long)a.dil * (a.KW - 1)) * a.ldx * eb;
        if (behind < 0 || d < tapmax || d + (long long)a.Cin * eb >= (1ll << 31)) return false;
    }
    return xbytes < (1ll << 31) && wbytes < (1ll << 31);
}

// shape 8: the 16-row variant (32 x 64 block, 16 x 32 wave tiles on v_mfma_f32_16x16x4_f32); plain epilogue only
static int launch_dma2_r16(const ConvArgs& a, hipStream_t st) {
    if (a.stats) {
        set_error("conv_dma2: the 16-row tile has no statistics epilogue");
        return -1;
    }
    using T = Tile<8>;
    auto kern = a.padv ? dma2_kernel<T, true, 0, false, false, false, true> : dma2_kernel<T, false, 0, false, false, false, true>;
    return launch_with_lds(kern, tile_grid<T>(a), T::NW * 64, tile_lds<T>(), st, a, "conv_dma2/r16");
}

int launch_conv_dma2(int shape, const ConvArgs& a, hipStream_t st) {
    if (shape == 8) return launch_dma2_r16(a, st);
    return with_tile<FamFp32>(shape, [&](auto t) {
        using T = decltype(t);
        return launch_with_lds(dma2_fp32_kernel<T, false>(a), tile_grid<T>(a), T::NW * 64, tile_lds<T>(), st, a, "conv_dma2");
    });
}

}  // namespace pemp
