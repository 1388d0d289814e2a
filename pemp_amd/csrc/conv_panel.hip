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
//    K step of BN weight rows in the S3 image of conv_dma2.hip (12 quads per row, same swizzle, same LDS-DMA), three stages in a
//    ring, the DMA of stage t + 3 issued behind the barrier in the middle of stage t.  The K loop is MFMAs, B fragment reads and
//    DMA issue: no A reads, no split;
//  * per accumulator the order is K16 slices ascending, inside a slice lh, hl, mm, mh, hm, hh: BIT-IDENTICAL to ids 41..49 (the
//    accumulators of one slice are interleaved product by product, so that consecutive MFMAs do not depend on each other);
//  * the epilogue is conv_epilogue_lds_pre's arithmetic, statement for statement.  The residual / scale / shift quads of N tile n
//    are requested behind the barrier of its last K step; its stores are buffer stores that are ALWAYS issued (a row >= M gets an
//    offset behind the descriptor's range and is dropped), so that their number is a constant and the wait for a weight stage
//    can be counted past them: they drain under the MFMAs of tile n + 1.
// Vector memory operations of a wave retire in order (the persistent kernels of conv_dma2.hip count on the same), in issue
// order:  DMA(t+1) | .. | DMA(t+2) | .. | <- the wait in the middle of stage t wants everything up to DMA(t+1):
//   K step 0 of a tile, or its K step 1:  one batch of NST stores of the previous tile lies behind DMA(t+1)  -> vmcnt(BL + NST)
//   NK == 1:                              two batches                                                         -> vmcnt(BL + 2 NST)
//   any other step:                                                                                           -> vmcnt(BL)
// (loads of the epilogue lie in front of the stores that use them and may be left out of the count: that only waits longer.
// The first three stages are waited for in full before the loop, which covers the steps that have no such history yet.)
// Stages past the last one are still issued, with every offset behind the range: the hardware writes zeros into a free buffer
// and reads no memory -- one form of the step, constant counts.
#include "conv_tiles.h"

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) unsigned int v4u;

template <int NK, int BN, int NW>
__device__ __forceinline__ void conv_panel_body(const ConvArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int TN = BN / 32;
    constexpr int SQ = BN * 12;                     // quads of one weight stage
    static_assert(SQ % (NW * 64) == 0, "whole DMA rounds");
    constexpr int BL = SQ / (NW * 64);              // DMA instructions per thread and stage
    constexpr int NST = TN * 4;                     // stores per thread and N tile
    constexpr int NS = 3;                           // stages in the ring
    static_assert(BL + 2 * NST <= 63, "vmcnt range");

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
        const int src = (pos & ~3) | ((pos & 3) ^ ((row >> 2) & 3));
        b_voff[i] = (unsigned)(row * a.Kpad * 6 + src * 16);
    }
    const int tile_bytes = BN * a.Kpad * 6;         // weight bytes of one N tile
    // stage t_ = (n_, kt_) into ring buffer buf_
#define PEMP_PANEL_DMA(buf_, t_, n_, kt_)                                                                         \
    do {                                                                                                          \
        v4f* Bd_ = Bs + (buf_) * SQ + wave * 64;                                                                  \
        const int so_ = __builtin_amdgcn_readfirstlane((t_) < T ? (n_) * tile_bytes + (kt_) * 192 : 0);          \
        const bool in_ = (t_) < T;                                                                                \
        _Pragma("unroll") for (int i = 0; i < BL; ++i)                                                            \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bd_ + i * NW * 64), 16, in_ ? b_voff[i] : 0x80000000u, so_, 0, 0); \
    } while (0)

    // the first three stages fly while the activation panel is loaded and split
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // stages 0..2 have landed (this thread's pieces)
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
    // K16 slice s_: per accumulator lh, hl, mm, mh, hm, hh; the TN accumulators take turns
#define PEMP_PANEL_MMA(src_, s_)                                                                                  \
    do {                                                                                                          \
        _Pragma("unroll") for (int pr = 0; pr < 6; ++pr)                                                          \
            _Pragma("unroll") for (int ni = 0; ni < TN; ++ni) {                                                   \
                const bf16x8 av_ = pr == 0 ? al[s_] : (pr == 2 || pr == 3) ? am[s_] : ah[s_];                     \
                const bf16x8 bv_ = __builtin_bit_cast(bf16x8, bfr[src_][ni][pr == 1 ? 2 : (pr == 2 || pr == 4) ? 1 : 0]); \
                acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av_, bv_, acc[ni], 0, 0, 0);                    \
            }                                                                                                     \
    } while (0)

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
        r_off[i] = m < a.M ? (unsigned)(m * a.ldr + c4) * 4u : 0x80000000u;
    }

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
            // every LDS read of `cur` by this wave has returned; this wave's pieces of the next stage have landed
            if constexpr (NK == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BL + 2 * NST) : "memory");
            else if (kt <= 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BL + NST) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BL) : "memory");
            __builtin_amdgcn_s_barrier();       // ... everybody's: `cur` is free for stage t + 3, `nxt` holds stage t + 1
            __builtin_amdgcn_sched_barrier(0);
            PEMP_PANEL_READ(0, nxt, 0);
            if (kt == NK - 1) {                 // the tile's epilogue operands: in front of the DMA, so behind it in no count
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int c = n * BN + ni * 32 + c4;
                    scv[ni] = a.scale ? *(const v4f*)(a.scale + c) : v4f{1.f, 1.f, 1.f, 1.f};
                    shv[ni] = a.shift ? *(const v4f*)(a.shift + c) : v4f{0.f, 0.f, 0.f, 0.f};
                }
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
            {
                const int t3 = n * NK + kt + NS;                    // the stage that goes into `cur`
                const int n3 = n + (kt + NS) / NK, k3 = (kt + NS) % NK;
                PEMP_PANEL_DMA(cur, t3, n3, k3);
            }
            __builtin_amdgcn_sched_barrier(0);
            PEMP_PANEL_MMA(1, 2 * kt + 1);
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
        // ---- epilogue of N tile n: conv_epilogue_lds_pre's arithmetic (EPI 0, no per-image shift, no DropBlock) ----
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const v4f sc = scv[ni], sh = shv[ni];
#pragma unroll
            for (int e = 0; e < 16; ++e) patch[((e & 3) + 8 * (e >> 2) + 4 * lh) * 32 + lr] = acc[ni][e];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = er + 8 * i;
                const v4f v = *(const v4f*)(patch + row * 32 + c4);
                v4f add = sh;
                if (a.res) add += rres[ni * 4 + i];
                v4f o;
                o.x = __builtin_fmaf(v.x, sc.x, add.x);      // explicit: every epilogue variant must round identically
                o.y = __builtin_fmaf(v.y, sc.y, add.y);
                o.z = __builtin_fmaf(v.z, sc.z, add.z);
                o.w = __builtin_fmaf(v.w, sc.w, add.w);
                if (relu) {
                    o.x = fmaxf(o.x, 0.f);
                    o.y = fmaxf(o.y, 0.f);
                    o.z = fmaxf(o.z, 0.f);
                    o.w = fmaxf(o.w, 0.f);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, o), ry, y_off[i] + (unsigned)(n * BN + ni * 32) * 4u, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // no LDS-DMA outlives the block
#undef PEMP_PANEL_DMA
#undef PEMP_PANEL_READ
#undef PEMP_PANEL_MMA
#endif
}

// waves per SIMD: one block of 4 waves per CU = 1; the 64-column form up to K = 128 fits two blocks (registers and LDS)
template <int NK, int BN, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu((BN == 64 && NK <= 4) ? 2 : 1))) void conv_panel_kernel(ConvArgs a) {
    conv_panel_body<NK, BN, NW>(a);
}

constexpr int PANEL_NW = 4;
template <int BN> constexpr size_t panel_lds() { return (size_t)(3 * BN * 12 + PANEL_NW * 256) * sizeof(v4f); }

template <int BN, int NK = 1>
static int launch_panel_nk(const ConvArgs& a, hipStream_t st) {
    if constexpr (NK > 8) {
        set_error("conv split3 panel: Kpad=%d above 256", a.Kpad);
        return -1;
    } else {
        if (a.nk == NK)
            return launch_with_lds(conv_panel_kernel<NK, BN, PANEL_NW>, cdiv(a.M, 32 * PANEL_NW), PANEL_NW * 64, panel_lds<BN>(), st, a,
                                   "conv_panel");
        return launch_panel_nk<BN, NK + 1>(a, st);
    }
}

// what the family takes: 1x1, no padding, Kpad <= 256, plain epilogue without a per-image shift, operands whose byte offsets fit
// the 2 GiB window of a buffer descriptor
bool conv_panel_supported(const ConvArgs& a) {
    if (a.KH != 1 || a.KW != 1 || a.pad != 0 || a.nk < 1 || a.nk > 8 || a.Kpad != a.Cin || (a.flags & (PEMP_CONV_STEM4 | PEMP_CONV_SHIFT_PER_IMAGE | PEMP_CONV_BF16_IO)))
        return false;
    if (a.padv || a.stats || a.rowmask || a.sk_S > 1 || a.bm_first) return false;
    const long long lim = 1ll << 31;
    return (long long)a.N * a.H * a.W * a.ldx * 4 < lim && (long long)a.M * a.ldy * 4 < lim && (!a.res || (long long)a.M * a.ldr * 4 < lim) &&
           (long long)a.Cout * a.Kpad * 6 < lim;
}

int launch_conv_panel(int shape, const ConvArgs& a, hipStream_t st) {
    if (!conv_panel_supported(a)) {
        set_error("conv split3 panel: needs a 1x1 conv without padding, Kpad <= 256, no padding value / per-image shift, operands < 2 GiB");
        return -1;
    }
    return kTileShapes[shape].bn == 128 ? launch_panel_nk<128>(a, st) : launch_panel_nk<64>(a, st);
}

}  // namespace pemp
