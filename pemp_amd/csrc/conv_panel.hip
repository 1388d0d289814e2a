// Split3 1x1 convs with a short K (Kpad <= 256): activation-stationary, weight-streaming (tile ids 71, 72; pemp_hip.h).
//
// The tile-per-block split3 kernels (conv_dma2.hip) fetch and split the same activation panel once per tile COLUMN: for 256 -> 1024
// that is 8 times, ~2.2 VALU per MFMA in a K loop of at most 8 steps, followed by a serial epilogue.  Here a block of NW waves owns
// 32 NW consecutive output rows for ALL of Cout:
//  * every wave loads its 32 rows x K of fp32 activations ONCE, straight into the MFMA operand layout (lane half lh of K16 slice s
//    holds channels 16 s + 8 lh .. + 7 of row lane & 31: the lane -> k mapping of the S3 kernels), splits them once (split3_bf16)
//    and keeps the h / m / l fragments in registers for the block's lifetime: 12 VGPRs per slice, 192 at K = 256.  The conv's
//    stride and the input's channel stride go into the row offset (a stride-2 downsample is a row gather); rows >= M read zeros
//    through the buffer range check;
//  * the block then walks the N tiles (BN columns each).  Only the packed weights stream through LDS: one stage = the 32-channel
//    K step of BN weight rows in the S3 image of conv_dma2.hip (12 quads per row, same swizzle, same LDS-DMA), NS stages in a
//    ring (panel_stages), the DMA of stage t + NS issued behind the barrier in the middle of stage t.  The K loop is MFMAs, B
//    fragment reads and DMA issue: no A reads, no split;
//  * per accumulator the order is K16 slices ascending, inside a slice split3_mma6's: BIT-IDENTICAL to ids 41..49 (the
//    accumulators of one slice are interleaved product by product, so that consecutive MFMAs do not depend on each other);
//  * the epilogue is PEMP_CONV_PATCH_PUT and conv_affine_quad on the patch's quads.  Its stores are buffer stores that are ALWAYS
//    issued (a row >= M gets an offset behind the descriptor's range and is dropped), so that their number is a constant and the
//    wait for a weight stage can be counted past them: they drain under the MFMAs of tile n + 1.
// Vector memory operations of a wave retire in issue order (the persistent kernels of conv_dma2.hip count on the same), so the
// wait in the middle of stage t, which wants DMA(t + 1), is vmcnt(everything issued behind DMA(t + 1)).  DMA(t + 1) went out in
// the middle of step t + 1 - NS; the steps u = t + 1 - NS .. t - 1 have since put behind it (panel_behind):
//   BL DMAs of stage u + NS    for every u but the first (whose DMA is the one waited for),
//   NST stores                 after every u that is the last K step of its tile.
// The number depends on t through kt = t % NK alone.  The loads of a tile's residual / scale / shift quads are conditional and
// stay out of the count wherever they are issued: a count that is too small only waits longer, for the oldest operations behind
// DMA(t + 1) as well.
//  * NK < 4 (layer1's K = 64: at the HBM bound, too few steps per tile) keeps three stages and asks for those quads behind the
//    barrier of the tile's LAST K step, in front of the DMA: vmcnt(BL + NST) in K steps 0 and 1, vmcnt(BL + 2 NST) at NK == 1,
//    vmcnt(BL) elsewhere.
//  * NK >= 4 asks for them in K step 0 of the tile that uses them, behind that step's DMA: a whole tile ahead of the epilogue
//    instead of half a K step.  Its ring is 5 to 8 stages deep (panel_stages: what LDS and the 6 bits of vmcnt allow), so that
//    a store has NS - 1 K steps to retire before a weight wait sits behind it, not 2.  Its vector memory instructions of a K
//    step -- the stage's DMAs, in K step 0 the residual loads behind them -- go out one behind each MFMA of the step's second
//    K16 slice: issued in a burst behind the barrier, by four waves at once, they held every wave's MFMAs up while the address
//    unit worked through them (residual loads issued for nothing cost 2 - 3 % of a 256 -> 1024 launch).
// The first NS stages are waited for in full before the loop.  That covers the steps t <= NS - 2, whose window reaches in front
// of step 0 and whose count names operations that were never issued: their stage has landed whatever the count says.  From
// t = NS - 1 on every step of the window is a real one and issues exactly the operations above.
// Stages past the last one are still issued, with every offset behind the range: the hardware writes zeros into a free buffer
// and reads no memory -- one form of the step, constant counts.
#include "conv_tiles.h"

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) unsigned int v4u;

// the long-K schedule: epilogue operands a tile ahead, a deep ring, vector memory instructions issued between the MFMAs
template <int NK> constexpr bool panel_early() { return NK >= 4; }
// two blocks per CU (registers and LDS): the 64-column form up to K = 128
template <int NK, int BN> constexpr bool panel_two_blocks() { return BN == 64 && NK <= 4; }
// stages in the ring: stages are 12 KB (BN = 64) / 24 KB (BN = 128), the patches 16 KB, a CU has 160 KB; and panel_behind <= 63
template <int NK, int BN> constexpr int panel_stages() {
    if (!panel_early<NK>()) return 3;
    if (NK == 4) return 5;                          // BN = 64: two blocks of 76 KB each; a tile is 4 steps long
    return BN == 64 ? 8 : 6;                        // 112 KB; 160 KB
}
// vector memory operations behind DMA(t + 1) at the wait of K step kt = t % NK (the derivation in the file header)
template <int NK, int NS, int BL, int NST>
constexpr int panel_behind(int kt) {
    int c = 0;
    for (int u = kt + 1 - NS; u <= kt - 1; ++u) {
        const int ku = ((u % NK) + NK) % NK;
        if (u > kt + 1 - NS) c += BL;
        if (ku == NK - 1) c += NST;
    }
    return c;
}
template <int NK, int NS, int BL, int NST>
constexpr int panel_behind_max() {
    int m = 0;
    for (int kt = 0; kt < NK; ++kt) m = panel_behind<NK, NS, BL, NST>(kt) > m ? panel_behind<NK, NS, BL, NST>(kt) : m;
    return m;
}
// every LDS read of this wave has returned; its pieces of stage t + 1 have landed
template <int NK, int NS, int BL, int NST, int KT = 0>
__device__ __forceinline__ void panel_wait(int kt) {
    if constexpr (KT < NK) {
        if (kt == KT) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(panel_behind<NK, NS, BL, NST>(KT)) : "memory");
        else panel_wait<NK, NS, BL, NST, KT + 1>(kt);
    }
}

// RS2 (PEMP_CONV_RES_S2, a compile-time variant: conv_panel_rs2_kernel): the residual lies on a grid twice as fine as the output.
// A lane's four epilogue rows are the same for every N tile, so their residual pixels (conv_res_s2_pixel) are worked out once per
// block, where the dense form multiplies the row by ldr; the K loop and the epilogue are the dense form's.
template <int NK, int BN, int NW, bool RS2 = false>
__device__ __forceinline__ void conv_panel_body(const ConvArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int TN = BN / 32;
    constexpr int SQ = BN * 12;                     // quads of one weight stage
    static_assert(SQ % (NW * 64) == 0, "whole DMA rounds");
    constexpr int BL = SQ / (NW * 64);              // DMA instructions per thread and stage
    constexpr int NST = TN * 4;                     // stores per thread and N tile
    constexpr int NS = panel_stages<NK, BN>();      // stages in the ring
    constexpr bool EARLY = panel_early<NK>();
    static_assert(panel_behind_max<NK, NS, BL, NST>() <= 63, "vmcnt range");
    static_assert(NK >= 4 || (panel_behind<NK, NS, BL, NST>(0) == BL + (NK == 1 ? 2 : 1) * NST && panel_behind<NK, NS, BL, NST>(NK - 1) == BL + (NK == 1 ? 2 : NK == 2 ? 1 : 0) * NST),
                  "the short-K counts");

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* Bs = smem;                                 // [NS][BN][12]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* patch = (float*)(smem + NS * SQ) + wave * 1024;      // one 4 KB transpose patch per wave
    const int lr = lane & 31, lh = lane >> 5;
    const int m_wave = ((int)blockIdx.x * NW + wave) * 32;
    const int ntn = a.Cout / BN;
    const int T = ntn * NK;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)(a.res ? a.res : a.y), 0, 0x80000000u, 0x00020000);

    // weight stage (n, kt): LDS quad q of the stage = row q / 12, position q % 12 = plane * 4 + (quad ^ ((row >> 2) & 3))
    unsigned b_voff[BL];
#pragma unroll
    for (int i = 0; i < BL; ++i) {
        const int q = i * NW * 64 + tid, row = q / 12, pos = q - row * 12;
        const int src = PEMP_SPLIT3_SWZ(row, pos);
        b_voff[i] = (unsigned)(row * a.Kpad * 6 + src * 16);
    }
    const int tile_bytes = BN * a.Kpad * 6;         // weight bytes of one N tile
    // stage t_ = (n_, kt_) into ring buffer buf_: the stage's constants, then its BL instructions one by one
#define PEMP_PANEL_DMA_SETUP(buf_, t_, n_, kt_)                                                                   \
    v4f* const Bd_ = Bs + (buf_) * SQ + wave * 64;                                                                \
    const int so_ = __builtin_amdgcn_readfirstlane((t_) < T ? (n_) * tile_bytes + (kt_) * 192 : 0);              \
    const bool in_ = (t_) < T
#define PEMP_PANEL_DMA_ONE(i_) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bd_ + (i_) * NW * 64), 16, in_ ? b_voff[i_] : 0x80000000u, so_, 0, 0)
#define PEMP_PANEL_DMA(buf_, t_, n_, kt_)                                                                         \
    do {                                                                                                          \
        PEMP_PANEL_DMA_SETUP(buf_, t_, n_, kt_);                                                                  \
        _Pragma("unroll") for (int i = 0; i < BL; ++i) PEMP_PANEL_DMA_ONE(i);                                     \
    } while (0)

    // the first NS stages fly while the activation panel is loaded and split
#pragma unroll
    for (int t = 0; t < NS; ++t) PEMP_PANEL_DMA(t, t, t / NK, t % NK);

    // ---- the activation panel: row m_wave + lr, channels 16 s + 8 lh .. + 7 of every K16 slice s ----
    bf16x8 ah[2 * NK], am[2 * NK], al[2 * NK];
    {
        const int m = m_wave + lr;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int img = mm / a.HoWo;
        const int rem = mm - img * a.HoWo;
        const int ho = rem / a.Wo;
        const int wo = rem - ho * a.Wo;
        const unsigned off = ok ? (unsigned)(((img * a.H + ho * a.stride) * a.W + wo * a.stride) * a.ldx + 8 * lh) * 4u : 0x80000000u;
        v4f x0[2 * NK], x1[2 * NK];
#pragma unroll
        for (int s = 0; s < 2 * NK; ++s) {
            x0[s] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rx, off + s * 64, 0, 0));
            x1[s] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rx, off + s * 64 + 16, 0, 0));
        }
#pragma unroll
        for (int s = 0; s < 2 * NK; ++s) split3_bf16(x0[s], x1[s], ah[s], am[s], al[s]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the first NS stages have landed (this thread's pieces)
    __builtin_amdgcn_s_barrier();                              // ... everybody's
    __builtin_amdgcn_sched_barrier(0);

    const int brow3 = lr * 12, bsw3 = (lr >> 2) & 3;
    v4f bfr[2][TN][3];
    // half step j_ of the stage in ring buffer buf_: quad 2 j_ + lh of each weight plane of the wave's BN rows
#define PEMP_PANEL_READ(dst_, buf_, j_)                                                                           \
    do {                                                                                                          \
        const v4f* Bb_ = Bs + (buf_) * SQ;                                                                        \
        const int pb_ = (2 * (j_) + lh) ^ bsw3;                                                                   \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni)                                                         \
            _Pragma("unroll") for (int pl = 0; pl < 3; ++pl)                                                      \
                bfr[dst_][ni][pl] = Bb_[brow3 + ni * 32 * 12 + pl * 4 + pb_];                                     \
    } while (0)
    // K16 slice s_: product pr of split3_mma6's order (conv_common.h) for each of the TN accumulators in turn -- not a call of it: the
    // accumulators take turns product by product, with HOOK_(j) behind MFMA j of the slice.
#define PEMP_PANEL_MMA_HOOKED(src_, s_, HOOK_)                                                                    \
    do {                                                                                                          \
        _Pragma("unroll") for (int pr = 0; pr < 6; ++pr)                                                          \
            _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {                                                   \
                const bf16x8 av_ = pr == 0 ? al[s_] : (pr == 2 || pr == 3) ? am[s_] : ah[s_];                     \
                const bf16x8 bv_ = __builtin_bit_cast(bf16x8, bfr[src_][ni][pr == 1 ? 2 : (pr == 2 || pr == 4) ? 1 : 0]); \
                acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av_, bv_, acc[ni], 0, 0, 0);                    \
                HOOK_(pr * TN + ni);                                                                              \
            }                                                                                                     \
    } while (0)
#define PEMP_PANEL_HOOK_NONE(j_)
#define PEMP_PANEL_MMA(src_, s_) PEMP_PANEL_MMA_HOOKED(src_, s_, PEMP_PANEL_HOOK_NONE)
    // the stage's DMA instructions, one behind each of the slice's first MFMAs: a wave's vector memory instructions issue under
    // its own MFMAs instead of in a burst of all four waves behind the barrier, during which the MFMA pipes stand still
#define PEMP_PANEL_HOOK_DMA(j_)                                                                                   \
    if ((j_) < BL) {                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        PEMP_PANEL_DMA_ONE((j_) < BL ? (j_) : 0);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    // ... and behind them the residual quads of the tile, one per MFMA
#define PEMP_PANEL_HOOK_DMA_RES(j_)                                                                               \
    PEMP_PANEL_HOOK_DMA(j_)                                                                                       \
    else if ((j_) - BL < NST && a.res) {                                                                          \
        const int k_ = (j_) - BL < NST ? (j_) - BL : 0;                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
        rres[k_] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rr, r_off[k_ & 3] + (unsigned)(n * BN + (k_ >> 2) * 32) * 4u, 0, 0)); \
        __builtin_amdgcn_sched_barrier(0);                                                                        \
    }
    static_assert(BL + NST <= 6 * TN, "one instruction per MFMA of a slice");

    f32x16 acc[TN];
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;

    const bool relu = a.flags & PEMP_CONV_RELU;
    const int er = lane >> 3, c4 = (lane & 7) * 4;           // epilogue role: rows er + 8 i, channels c4 .. c4 + 3 of a sub-tile
    unsigned y_off[4], r_off[4];                               // byte offsets of the lane's four rows (behind the range: row >= M)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m_wave + er + 8 * i;
        y_off[i] = m < a.M ? (unsigned)(m * a.ldy + c4) * 4u : 0x80000000u;
        if constexpr (RS2) r_off[i] = m < a.M ? (unsigned)(conv_res_s2_pixel(a, m) * a.ldr + c4) * 4u : 0x80000000u;
        else r_off[i] = m < a.M ? (unsigned)(m * a.ldr + c4) * 4u : 0x80000000u;
    }

    // the scale / shift quads of N tile n_
#define PEMP_PANEL_AFFINE(n_)                                                                                     \
    do {                                                                                                          \
        _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {                                                       \
            const int c = (n_) * BN + ni * 32 + c4;                                                               \
            scv[ni] = a.scale ? *(const v4f*)(a.scale + c) : v4f{1.f, 1.f, 1.f, 1.f};                             \
            shv[ni] = a.shift ? *(const v4f*)(a.shift + c) : v4f{0.f, 0.f, 0.f, 0.f};                             \
        }                                                                                                         \
    } while (0)

    int cur = 0;                                               // ring buffer of the current stage
    PEMP_PANEL_READ(0, 0, 0);
    for (int n = 0; n < ntn; ++n) {
        v4f rres[NST], scv[TN], shv[TN];
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) {
            const int nxt = cur == NS - 1 ? 0 : cur + 1;
            PEMP_PANEL_READ(1, cur, 1);
            __builtin_amdgcn_sched_barrier(0);
            PEMP_PANEL_MMA(0, 2 * kt);
            __builtin_amdgcn_sched_barrier(0);
            panel_wait<NK, NS, BL, NST>(kt);
            __builtin_amdgcn_s_barrier();       // ... everybody's: `cur` is free for stage t + NS, `nxt` holds stage t + 1
            __builtin_amdgcn_sched_barrier(0);
            PEMP_PANEL_READ(0, nxt, 0);
            const int t3 = n * NK + kt + NS;                        // the stage that goes into `cur`
            const int n3 = n + (kt + NS) / NK, k3 = (kt + NS) % NK;
            if constexpr (!EARLY) {
                if (kt == NK - 1) {             // the tile's epilogue operands: in front of the DMA, so behind it in no count
                    PEMP_PANEL_AFFINE(n);
#pragma unroll
                    for (int i = 0; i < NST; ++i) rres[i] = v4f{0.f, 0.f, 0.f, 0.f};
                    if (a.res) {
#pragma unroll
                        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                rres[ni * 4 + i] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rr, r_off[i] + (unsigned)(n * BN + ni * 32) * 4u, 0, 0));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                PEMP_PANEL_DMA(cur, t3, n3, k3);
                __builtin_amdgcn_sched_barrier(0);
                PEMP_PANEL_MMA(1, 2 * kt + 1);
            } else {
                PEMP_PANEL_DMA_SETUP(cur, t3, n3, k3);
                if (kt == 0) PEMP_PANEL_AFFINE(n);                  // a whole tile ahead of the epilogue
                __builtin_amdgcn_sched_barrier(0);
                if (kt == 0) PEMP_PANEL_MMA_HOOKED(1, 2 * kt + 1, PEMP_PANEL_HOOK_DMA_RES);
                else PEMP_PANEL_MMA_HOOKED(1, 2 * kt + 1, PEMP_PANEL_HOOK_DMA);
            }
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
        // ---- epilogue of N tile n: conv_epilogue_lds_pre's EPI 0 without a per-image shift, every store issued ----
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            PEMP_CONV_PATCH_PUT(patch, acc[ni], lr, lh);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = er + 8 * i;
                const v4f v = *(const v4f*)(patch + row * 32 + c4);
                v4f add = shv[ni];
                if (a.res) add += rres[ni * 4 + i];
                const v4f o = conv_affine_quad(v, scv[ni], add, relu);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, o), ry, y_off[i] + (unsigned)(n * BN + ni * 32) * 4u, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // no LDS-DMA outlives the block
#undef PEMP_PANEL_DMA_SETUP
#undef PEMP_PANEL_DMA_ONE
#undef PEMP_PANEL_DMA
#undef PEMP_PANEL_AFFINE
#undef PEMP_PANEL_READ
#undef PEMP_PANEL_MMA_HOOKED
#undef PEMP_PANEL_HOOK_NONE
#undef PEMP_PANEL_HOOK_DMA
#undef PEMP_PANEL_HOOK_DMA_RES
#undef PEMP_PANEL_MMA
#endif
}

// waves per SIMD: one block of 4 waves per CU = 1; the 64-column form up to K = 128 fits two blocks (registers and LDS)
template <int NK, int BN, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(panel_two_blocks<NK, BN>() ? 2 : 1))) void conv_panel_kernel(ConvArgs a) {
    conv_panel_body<NK, BN, NW>(a);
}

// the strided-residual variant (a kernel of its own: the instantiations of conv_panel_kernel keep their names and their code);
// K = 64 and 128 only, the two-blocks-per-CU forms included
template <int NK, int BN, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(panel_two_blocks<NK, BN>() ? 2 : 1))) void conv_panel_rs2_kernel(ConvArgs a) {
    conv_panel_body<NK, BN, NW, true>(a);
}

constexpr int PANEL_NW = 4;
template <int NK, int BN> constexpr size_t panel_lds() { return (size_t)(panel_stages<NK, BN>() * BN * 12 + PANEL_NW * 256) * sizeof(v4f); }
static_assert(panel_lds<8, 128>() <= 160 * 1024 && 2 * panel_lds<4, 64>() <= 160 * 1024, "LDS of a CU");

template <int BN, int NK = 1>
static int launch_panel_nk(const ConvArgs& a, hipStream_t st) {
    if constexpr (NK > 8) {
        set_error("conv split3 panel: Kpad=%d above 256", a.Kpad);
        return -1;
    } else {
        if (a.nk == NK)
            return launch_with_lds(conv_panel_kernel<NK, BN, PANEL_NW>, cdiv(a.M, 32 * PANEL_NW), PANEL_NW * 64, panel_lds<NK, BN>(), st, a,
                                   "conv_panel");
        return launch_panel_nk<BN, NK + 1>(a, st);
    }
}

template <int BN, int NK>
static int launch_panel_rs2(const ConvArgs& a, hipStream_t st) {
    return launch_with_lds(conv_panel_rs2_kernel<NK, BN, PANEL_NW>, cdiv(a.M, 32 * PANEL_NW), PANEL_NW * 64, panel_lds<NK, BN>(), st, a,
                           "conv_panel/res_s2");
}

// what the family takes: 1x1, no padding, Kpad <= 256, plain epilogue without a per-image shift, operands whose byte offsets fit
// the 2 GiB window of a buffer descriptor (a strided residual: all of its own grid); PEMP_CONV_RES_S2 at Kpad 64 and 128 only
bool conv_panel_supported(const ConvArgs& a) {
    if (a.KH != 1 || a.KW != 1 || a.pad != 0 || a.nk < 1 || a.nk > 8 || a.Kpad != a.Cin || (a.flags & (PEMP_CONV_STEM4 | PEMP_CONV_SHIFT_PER_IMAGE | PEMP_CONV_BF16_IO)))
        return false;
    if (a.padv || a.stats || a.rowmask || a.sk_S > 1 || a.bm_first) return false;
    const bool rs2 = a.flags & PEMP_CONV_RES_S2;
    if (rs2 && (!a.res || a.Hr < 1 || a.Wr < 1 || (a.nk != 2 && a.nk != 4))) return false;      // (launch_conv_panel: 128 columns at K = 64 only)
    const long long lim = 1ll << 31;
    const long long res_rows = rs2 ? (long long)a.N * a.Hr * a.Wr : a.M;
    return (long long)a.N * a.H * a.W * a.ldx * 4 < lim && (long long)a.M * a.ldy * 4 < lim && (!a.res || res_rows * a.ldr * 4 < lim) &&
           (long long)a.Cout * a.Kpad * 6 < lim;
}

int launch_conv_panel(int shape, const ConvArgs& a, hipStream_t st) {
    if (!conv_panel_supported(a)) {
        set_error("conv split3 panel: needs a 1x1 conv without padding, Kpad <= 256 (64 or 128 with PEMP_CONV_RES_S2), no padding value / per-image shift, operands < 2 GiB");
        return -1;
    }
    if (a.flags & PEMP_CONV_RES_S2) {
        // <4, 128> is not instantiated: like its dense form it would hold 16 VGPRs in AGPRs (counted as spilled), and a new
        // instantiation may have none -- id 71 refuses the flag at K = 128
        if (kTileShapes[shape].bn == 128) {
            if (a.nk == 2) return launch_panel_rs2<128, 2>(a, st);
            set_error("conv split3 panel: PEMP_CONV_RES_S2 on tile 71 needs Kpad 64 (Kpad 128: tile 72 or 43)");
            return -1;
        }
        return a.nk == 2 ? launch_panel_rs2<64, 2>(a, st) : launch_panel_rs2<64, 4>(a, st);
    }
    return kTileShapes[shape].bn == 128 ? launch_panel_nk<128>(a, st) : launch_panel_nk<64>(a, st);
}

}  // namespace pemp
