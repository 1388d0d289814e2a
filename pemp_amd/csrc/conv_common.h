// Shared between the conv engine's translation units.
#pragma once
#include "common.h"

namespace pemp {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float v4f;   // first-class vector: loads/stores never become memcpy
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// internal flag (not part of pemp_hip.h's desc flags): y and the residual are bf16 tensors (strides in bf16 elements)
#define PEMP_CONV_BF16_IO 0x100u

// four consecutive channels at element offset ``off`` of a tensor that is fp32 or (bf16 != 0) bf16, as fp32
__device__ __forceinline__ v4f load_quad(const float* base, size_t off, unsigned bf16) {
    if (!bf16) return *(const v4f*)(base + off);
    const u32x2 r = *(const u32x2*)((const unsigned short*)base + off);
    return v4f{__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.x & 0xFFFF0000u),
               __builtin_bit_cast(float, r.y << 16), __builtin_bit_cast(float, r.y & 0xFFFF0000u)};
}

// fp32 -> bf16, round to nearest even (NaN stays NaN: the quiet bit is forced)
__device__ __forceinline__ unsigned int bf16_bits(float f) {
    const unsigned int u = __builtin_bit_cast(unsigned int, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// x = h + m + l exactly, for the 8 fp32 values of two quads: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), each rounded to
// nearest even (the differences are exact in fp32).  The split3 conv kernels (conv_dma2.hip, S3) and pemp_pack_split3_bf16.
__device__ __forceinline__ void split3_bf16(const v4f& x0, const v4f& x1, bf16x8& h, bf16x8& m, bf16x8& l) {
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 he = (__bf16)x[e];
        const float r = x[e] - (float)he;
        const __bf16 me = (__bf16)r;
        h[e] = he;
        m[e] = me;
        l[e] = (__bf16)(r - (float)me);
    }
}

__device__ __forceinline__ void store_quad(float* base, size_t off, const v4f& o, unsigned bf16) {
    if (!bf16) {
        *(v4f*)(base + off) = o;
        return;
    }
    u32x2 r;
    r.x = bf16_bits(o.x) | (bf16_bits(o.y) << 16);
    r.y = bf16_bits(o.z) | (bf16_bits(o.w) << 16);
    *(u32x2*)((unsigned short*)base + off) = r;
}

// The epilogue's rounding contract, one quad of it: o = fmaf(v, scale, add), then max with 0 -- v the accumulator, add the shift
// with whatever the variant adds to it (per-image shift, residual), in that variant's order.  The fma is explicit: written as
// v * sc + add the contraction would be hipcc's choice per call site, and every epilogue variant must round identically (the
// bit identity of the tile ids rests on it).  conv_stem_pool.hip applies the same expression per scalar (lane = channel).
__device__ __forceinline__ v4f conv_affine_quad(const v4f& v, const v4f& sc, const v4f& add, bool relu) {
    v4f o;
    o.x = __builtin_fmaf(v.x, sc.x, add.x);
    o.y = __builtin_fmaf(v.y, sc.y, add.y);
    o.z = __builtin_fmaf(v.z, sc.z, add.z);
    o.w = __builtin_fmaf(v.w, sc.w, add.w);
    if (relu) {
        o.x = fmaxf(o.x, 0.f);
        o.y = fmaxf(o.y, 0.f);
        o.z = fmaxf(o.z, 0.f);
        o.w = fmaxf(o.w, 0.f);
    }
    return o;
}

// The split3 product of one K16 slice: a b with a = ah + am + al, b = bh + bm + bl (split3_bf16) is taken as the six bf16 x bf16
// products whose size is above one fp32 rounding of it, in the FIXED order lh, hl, mm, mh, hm, hh -- smallest first, each exact in
// the MFMA's fp32 sum.  The order is what makes every split3 tile id bit-identical to id 43; it is defined here.
// (Two K loops write it out instead of calling this: conv_panel.hip interleaves the products of its accumulators, one hooked
// instruction per MFMA slot, and picks product pr of this order by index; conv_dma2.hip's PEMP_MMA keeps its six lines because
// the fp32-activation kernels come out with another schedule when they call it.)
__device__ __forceinline__ void split3_mma6(f32x16& acc, bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 bh, bf16x8 bm, bf16x8 bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// LDS image of a split3 operand stage: a row holds 12 quads, position = plane * 4 + quad, and the quad is XORed with bits 2..3 of
// the row.  -> the position of the row's 192 bytes in memory that belongs at LDS position ``pos`` (the map is its own inverse).
// (A macro, like PEMP_CONV_PATCH_PUT below: as functions the two are simplified on their own before they are inlined, and the
// address arithmetic of every kernel comes out differently -- other registers, in some kernels more of them.)
#define PEMP_SPLIT3_SWZ(row_, pos_) (((pos_) & ~3) | (((pos_) & 3) ^ (((row_) >> 2) & 3)))

// A 32 x 32 accumulator (lane (lr_, lh_) = (lane & 31, lane >> 5): column lr_, 16 registers = rows (e & 3) + 8 (e >> 2) + 4 lh_)
// into the wave's 4 KB transpose patch S_, row-major.  The caller waits for the writes (lgkmcnt(0)) before it reads the patch.
#define PEMP_CONV_PATCH_PUT(S_, acc_, lr_, lh_) \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) (S_)[((e & 3) + 8 * (e >> 2) + 4 * (lh_)) * 32 + (lr_)] = (acc_)[e]

struct ConvArgs {
    const float* x;
    const float* w;
    float* y;
    const float* scale;
    const float* shift;
    const float* res;
    const float* padv;      // per-input-channel value of out-of-image taps (NULL: zero padding)
    float* stats;           // [ceil(M/BM)][2][Cout] per-row-tile partial sums (NULL: none; conv_dma2.hip only): of y and y^2, or,
                            // with bz set, of g and g*xhat (BatchNorm backward; see pemp_conv2d_bnbwd_nhwc_f32)
    const uint32_t* bmask;  // sign bits of the BatchNorm's output (NULL: no ReLU)
    const float* bz;        // the BatchNorm's input, per-pixel stride ldbz
    const float* bmean;
    const float* binvstd;
    int ldbz;
    // DropBlock2D behind the conv (pemp_conv2d_dropblock_nhwc_f32): every output row m is multiplied by rowmask[m] * M / *rowcnt
    // (the layer's two statements, in its order and rounding: ((y * mask) * numel) / sum(mask)); NULL: none
    const float* rowmask;
    const int* rowcnt;
    // split-K of the remainder tiles (conv_dma2.hip, SK kernels): tiles >= sk_full are computed by sk_S blocks each, every block
    // over 1/sk_S of the K steps; partial accumulators go to sk_ws, the last block to arrive adds them in piece order
    float* sk_ws;
    int* sk_cnt;            // one arrival counter per split tile: zero on entry, left zero
    int sk_full, sk_S;
    int N, H, W, Cin, ldx, Ho, Wo, Cout, ldy, KH, KW, stride, pad, dil, ldr, Kpad;
    unsigned flags;
    int M, HoWo, cin_steps, nk, ntaps;
    int bm_first = 0;       // conv_dma2.hip: the launch's first row tile (in units of its BM; 0 except in the hybrid launch's second member)
    int Hr = 0, Wr = 0;     // PEMP_CONV_RES_S2: the residual's own grid [N][Hr][Wr] (0: dense, the residual lies on the output grid)
};

// PEMP_CONV_RES_S2: the residual pixel of output row m = (img, ho, wo) -- pixel (img, 2 ho, 2 wo) of the [N][Hr][Wr] grid; its
// element offset is this times ldr.  (101 != 2 x 51: not affine in m, so no ldr fakes it.  The kernels that take the flag do this
// once per row they own, as a compile-time variant: conv_panel.hip and conv_dma2.hip, RS2.)
__device__ __forceinline__ int conv_res_s2_pixel(const ConvArgs& a, int m) {
    const int img = m / a.HoWo;
    const int rem = m - img * a.HoWo;
    const int ho = rem / a.Wo;
    const int wo = rem - ho * a.Wo;
    return (img * a.Hr + 2 * ho) * a.Wr + 2 * wo;
}

// up to CONV_GROUP_MAX independent convs of one tile shape in one launch (conv_dma2.hip: conv_dma2_group_kernel)
constexpr int CONV_GROUP_MAX = 4;
struct ConvGroupArgs {
    ConvArgs a[CONV_GROUP_MAX];
    int first[CONV_GROUP_MAX + 1];   // first block of member i (multiples of 8); first[n] = grid size
    int nblk[CONV_GROUP_MAX];        // tiles of member i
    int n;
};

// XCD-aware tile order.  Hardware deals consecutive block ids round-robin over the 8 XCDs (each
// with a private 4 MiB L2).  Tiles that share an A row-panel (same M tile, different N tiles) and
// neighbouring M tiles (3x3 halos) should therefore get ids that are congruent mod 8.  This
// bijection hands every XCD one contiguous range of the logical (M-major, N-minor) tile order.
// Placement only affects speed, never results.
// XcdTileRange: XCD (bid & 7)'s range [first, first + count) of ``tiles`` tiles in that order, and block ``bid``'s place in it: it
// is block ``idx`` of the ``step`` blocks of its XCD in a grid of ``nblk``.  One tile per block (nblk == tiles): tile first + idx,
// which is xcd_tile_order (below, in its own words: the one-tile kernels keep their emitted code).
// The persistent kernels (a resident grid, nblk <= tiles): tiles first + j for j = idx, idx + step, ... < count -- no counter, flag
// or atomic; which block computes a tile, and when, is all that changes.
struct XcdTileRange {
    int first, count, step, idx;
    __device__ __forceinline__ XcdTileRange(int tiles, int bid, int nblk) {
        const int xcd = bid & 7;
        idx = bid >> 3;
        const int q8 = tiles >> 3, r8 = tiles & 7;
        first = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
        count = q8 + (xcd < r8 ? 1 : 0);
        step = (nblk - xcd + 7) >> 3;
    }
};

__device__ __forceinline__ int xcd_tile_order(int bid, int nblk) {
    const int x = bid & 7, idx = bid >> 3;
    const int q = nblk >> 3, rem = nblk & 7;
    return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + idx;
}

// Wave-level epilogue through LDS.  The 32x32 accumulator tile sits "column per lane" (lane = channel,
// 16 registers = pixels), which would mean 16 scalar residual loads + 16 scalar stores per lane.  Each
// wave transposes its tile through a private 4 KB LDS patch so that a lane owns 4 consecutive channels
// of one pixel: float4 residual loads and float4 stores, 8 lanes = one 128-B row segment.  Same
// arithmetic, in the same order, as the scalar form:  v = acc * scale + (shift (+ per-image) (+ res)).
// ``pre`` (optional): the residual quads of the wave's tiles, loaded by the caller ahead of time in the order
// [mi][ni][i] (row = (lane >> 3) + 8 i of tile (mi, ni), channels (lane & 7) * 4 ..) -- conv_dma2.hip issues those loads
// under its last K step so that their latency is not exposed here.
// EPI 1: per-channel sums of the stored values and of their squares over the wave's rows, left in R ([TN][2][8][32] floats of
// LDS per wave: one row of 32 channel sums per lane group; the kernel adds the lane groups and the waves of a block in a fixed
// order and writes one partial row per row tile: the batch statistics of the BatchNorm behind the conv; fixed layout, fixed
// order -> deterministic).
// EPI 2: the stored value is g = o masked by the sign bits of the BatchNorm output this gradient belongs to, the sums are
// those of g and g * xhat (first half of that BatchNorm's backward; the expression of colsum_kernel<1> in train_ops.hip).
// DB: DropBlock2D's scaling of the output rows (a.rowmask / a.rowcnt) -- a compile-time variant, instantiated for the kernels of
// pemp_conv2d_dropblock_nhwc_f32 only: it keeps the four instructions out of every other epilogue.  (Round 4 made it one because
// the run-time branch "broke" one kernel; the cause was an unrelated wait-state hazard in conv_dma2.hip's inline asm that the
// branch merely re-scheduled into view -- DESIGN.md section 4, scratch/t31/README.md.)
// PEMP_CONV_OUT_SPLIT3: the 32 x 32 sub-tile in the wave's patch S (rows m_base .., channels n32 ..) goes out PRE-SPLIT -- bf16
// [M][Cout / 32][3][32], per row and 32-channel group the planes h, m, l of split3_bf16 -- for a split3 conv that reads it with
// PEMP_CONV_IN_SPLIT3 (conv_dma2.hip, A3).  A lane owns 8 consecutive channels of one row (4 lanes per row, 16 rows per pass), so
// that every plane goes out as one 16-byte store and a row's 192 bytes are written by 4 neighbouring lanes.  The value that is
// split is conv_affine_quad's, of the accumulator and the shift (+ per-image shift; no residual: the entry refuses one).
// (conv_split3_affine: the scale / shift quads of the lane's 8 channels n .. n + 7; conv_store_split3_to: the store itself, to y3,
// with those quads given -- the persistent kernels load them once per tile, beside their other epilogue loads)
__device__ __forceinline__ void conv_split3_affine(const ConvArgs& a, int n, v4f (&sc)[2], v4f (&sh)[2]) {
    const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        sc[u] = v4f{1.f, 1.f, 1.f, 1.f};
        sh[u] = v4f{0.f, 0.f, 0.f, 0.f};
        if (a.scale) sc[u] = *(const v4f*)(a.scale + n + 4 * u);
        if (a.shift && !per_img) sh[u] = *(const v4f*)(a.shift + n + 4 * u);
    }
}

__device__ __forceinline__ void conv_store_split3_to(const ConvArgs& a, unsigned short* y3, const float* S, int m_base, int n32, int lane,
                                                     const v4f (&sc)[2], const v4f (&sh)[2]) {
    const bool relu = a.flags & PEMP_CONV_RELU;
    const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
    const int r4 = lane >> 2, c8 = (lane & 3) * 8, n = n32 + c8;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = r4 + 16 * i;
        const int m = m_base + row;
        v4f o[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const v4f v = *(const v4f*)(S + row * 32 + c8 + 4 * u);
            v4f add = sh[u];
            if (per_img && m < a.M) add += *(const v4f*)(a.shift + (size_t)(m / a.HoWo) * a.Cout + n + 4 * u);
            o[u] = conv_affine_quad(v, sc[u], add, relu);
        }
        if (m < a.M) {
            bf16x8 h, md, l;
            split3_bf16(o[0], o[1], h, md, l);
            unsigned short* y = y3 + ((size_t)m * (a.Cout >> 5) + (n32 >> 5)) * 96 + c8;
            *(bf16x8*)y = h;
            *(bf16x8*)(y + 32) = md;
            *(bf16x8*)(y + 64) = l;
        }
    }
}

__device__ __forceinline__ void conv_store_split3(const ConvArgs& a, const float* S, int m_base, int n32, int lane) {
    v4f sc[2], sh[2];
    conv_split3_affine(a, n32 + (lane & 3) * 8, sc, sh);
    conv_store_split3_to(a, (unsigned short*)a.y, S, m_base, n32, lane, sc, sh);
}

// OS3 1: the kernel may be asked for a pre-split output (PEMP_CONV_OUT_SPLIT3: a run-time, wave-uniform branch per sub-tile -- the
// split3 kernels only, so that the fp32-chain instantiations do not carry it).
// OS3 2 (PEMP_CONV_OUT_SPLIT3_ALSO, a compile-time variant): y is written as fp32 AND the same values go out pre-split, through
// the pointer that arrives in a.res -- which is therefore never read as a residual.  After a sub-tile's fp32 stores the patch is
// still intact (until the trailing lgkmcnt(0)), and conv_store_split3_to recomputes the stored value from it, same statements.
template <int TM, int TN, int NPRE, int EPI = 0, bool DB = false, int OS3 = 0>
__device__ __forceinline__ void conv_epilogue_lds_pre(const ConvArgs& a, f32x16 (&acc)[TM][TN], float* S, int m_base,
                                                      int n_base, int lane, const v4f (&pre)[NPRE], float* R = nullptr) {
    constexpr bool PRE = NPRE == TM * TN * 4;       // (an array of 1 = "no prefetched residual": registers, never scratch)
    const bool relu = a.flags & PEMP_CONV_RELU;
    const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
    float db_sum = 1.f, db_numel = 1.f;
    if constexpr (DB) {
        db_sum = (float)*a.rowcnt;
        db_numel = (float)a.M;
    }
    const int lr = lane & 31, lh = lane >> 5;
    const int rr = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
        const int n = n_base + ni * 32 + c4;
        v4f sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (a.scale) sc = *(const v4f*)(a.scale + n);
        if (a.shift && !per_img) sh = *(const v4f*)(a.shift + n);
        v4f bmu = {0.f, 0.f, 0.f, 0.f}, bis = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EPI == 2) {
            bmu = *(const v4f*)(a.bmean + n);
            bis = *(const v4f*)(a.binvstd + n);
        }
        v4f t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};      // EPI: sums over the wave's TM row groups, ascending
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            v4f zt[4];
            uint32_t mw[4];
            if constexpr (EPI == 2) {                              // issued before the accumulators go through LDS
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m_base + mi * 32 + rr + 8 * i;
                    zt[i] = v4f{0.f, 0.f, 0.f, 0.f};
                    mw[i] = 0xFFFFFFFFu;
                    if (m < a.M) {
                        zt[i] = *(const v4f*)(a.bz + (size_t)m * a.ldbz + n);
                        if (a.bmask) mw[i] = a.bmask[(size_t)m * (a.Cout >> 5) + (n >> 5)];
                    }
                }
            }
            PEMP_CONV_PATCH_PUT(S, acc[mi][ni], lr, lh);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
            v4f s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
            if (OS3 == 1 && EPI == 0 && !DB && (a.flags & PEMP_CONV_OUT_SPLIT3)) conv_store_split3(a, S, m_base + mi * 32, n_base + ni * 32, lane);
            else
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rr + 8 * i;
                const int m = m_base + mi * 32 + row;
                const v4f v = *(const v4f*)(S + row * 32 + c4);
                if (m < a.M) {
                    v4f add = sh;
                    if (per_img) add += *(const v4f*)(a.shift + (size_t)(m / a.HoWo) * a.Cout + n);
                    if (OS3 != 2 && a.res) {
                        if constexpr (PRE) add += pre[(mi * TN + ni) * 4 + i];
                        else add += load_quad(a.res, (size_t)m * a.ldr + n, a.flags & PEMP_CONV_BF16_IO);
                    }
                    v4f o = conv_affine_quad(v, sc, add, relu);
                    if constexpr (DB) {                           // DropBlock2D.forward / its backward, fused (dropout.hip: pixel_scale_kernel)
                        const float k = a.rowmask[m];
                        o.x = __fdiv_rn(__fmul_rn(__fmul_rn(o.x, k), db_numel), db_sum);
                        o.y = __fdiv_rn(__fmul_rn(__fmul_rn(o.y, k), db_numel), db_sum);
                        o.z = __fdiv_rn(__fmul_rn(__fmul_rn(o.z, k), db_numel), db_sum);
                        o.w = __fdiv_rn(__fmul_rn(__fmul_rn(o.w, k), db_numel), db_sum);
                    }
                    if constexpr (EPI == 2) {
                        const uint32_t b = mw[i] >> c4;
                        o.x = (b & 1u) ? o.x : 0.f;
                        o.y = (b & 2u) ? o.y : 0.f;
                        o.z = (b & 4u) ? o.z : 0.f;
                        o.w = (b & 8u) ? o.w : 0.f;
                    }
                    store_quad(a.y, (size_t)m * a.ldy + n, o, a.flags & PEMP_CONV_BF16_IO);
                    if constexpr (EPI == 1) {
                        s1 += o;
                        s2 += o * o;
                    }
                    if constexpr (EPI == 2) {
                        s1 += o;
                        s2 += o * ((zt[i] - bmu) * bis);
                    }
                }
            }
            if constexpr (EPI != 0) {       // per lane: its 4 rows of this row group, then the wave's row groups in ascending order
                t1 += s1;
                t2 += s2;
            }
            if constexpr (OS3 == 2) {
                static_assert(EPI == 0 && !DB && !PRE, "the second, pre-split output: plain epilogue");
                v4f sc8[2], sh8[2];
                conv_split3_affine(a, n_base + ni * 32 + (lane & 3) * 8, sc8, sh8);
                conv_store_split3_to(a, (unsigned short*)a.res, S, m_base + mi * 32, n_base + ni * 32, lane, sc8, sh8);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
        }
        if constexpr (EPI != 0) {
            // The 8 lanes that share a channel quad (lane bits 3..5 = the row inside an 8-row group) leave their sums side by side
            // in LDS; conv_stats_store adds them in a fixed order.  (Round 3 reduced them here with a three-level shuffle butterfly
            // per 32 x 32 sub-tile: 24 cross-lane operations each, 20 us of a 105 us launch on the 256 -> 1024 layers.)
            *(v4f*)(R + ((ni * 2 + 0) * 8 + rr) * 32 + c4) = t1;
            *(v4f*)(R + ((ni * 2 + 1) * 8 + rr) * 32 + c4) = t2;
        }
    }
}

// Block-level finish of the EPI sums: the waves that cover the same columns (WGM of them, one per row band of the tile) are
// added in ascending row order and the tile's partial row goes to a.stats[bm].  Rall: the R areas of all waves
// ([NW][TN][2][8][32]); call after a block barrier.
template <int BN, int WGM, int NW, int TN>
__device__ __forceinline__ void conv_stats_store(const ConvArgs& a, const float* Rall, int bm, int n0, int tid) {
    constexpr int WGN = NW / WGM, WN = BN / WGN;
    if (tid < 2 * BN) {
        const int st = tid / BN, col = tid - st * BN;
        const int wni = col / WN, ni = (col - wni * WN) >> 5, c = col & 31;
        float s = 0.f;
#pragma unroll
        for (int wmi = 0; wmi < WGM; ++wmi)
#pragma unroll
            for (int g = 0; g < 8; ++g) s += Rall[((((wmi * WGN + wni) * TN + ni) * 2 + st) * 8 + g) * 32 + c];
        a.stats[((size_t)bm * 2 + st) * a.Cout + n0 + col] = s;
    }
}

template <int TM, int TN, bool DB = false, int OS3 = 0>
__device__ __forceinline__ void conv_epilogue_lds(const ConvArgs& a, f32x16 (&acc)[TM][TN], float* S, int m_base,
                                                  int n_base, int lane) {
    const v4f none[1] = {{0.f, 0.f, 0.f, 0.f}};
    static_assert(TM * TN * 4 != 1, "tile");
    conv_epilogue_lds_pre<TM, TN, 1, 0, DB, OS3>(a, acc, S, m_base, n_base, lane, none);
}

// The fp32 stores of one 32 x 32 sub-tile (rows m_base .., channels n32 ..) from the wave's patch S, for the persistent kernels,
// whose operands are in registers already: sc / sh = the scale / shift quads of the lane's channels n32 + 4 (lane & 7) .., res =
// the residual quads of its four rows (lane >> 3) + 8 i, requested by the caller ahead of time (nullptr: the kernel has no
// residual path).  conv_epilogue_lds_pre's EPI 0 arithmetic, in its order: shift, per-image shift, residual.
__device__ __forceinline__ void conv_patch_store_f32(const ConvArgs& a, const float* S, int m_base, int n32, int lane, const v4f& sc,
                                                     const v4f& sh, bool per_img, const v4f* res, unsigned bf16) {
    const bool relu = a.flags & PEMP_CONV_RELU;
    const int rr = lane >> 3, c4 = (lane & 7) * 4, n = n32 + c4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = rr + 8 * i;
        const int m = m_base + row;
        const v4f v = *(const v4f*)(S + row * 32 + c4);
        if (m < a.M) {
            v4f add = sh;
            if (per_img) add += *(const v4f*)(a.shift + (size_t)(m / a.HoWo) * a.Cout + n);
            if (res && a.res) add += res[i];
            store_quad(a.y, (size_t)m * a.ldy + n, conv_affine_quad(v, sc, add, relu), bf16);
        }
    }
}

// Epilogue of the persistent split3 kernels (conv_dma2.hip: conv_dma2_s3p_body; conv_row3.hip): the residual quads of the wave tile
// (order [mi][ni][i]) and the scale / shift quads of every column group were loaded by the caller in one batch, so the epilogue
// waits once and its stores issue back to back.  PLAIN: no residual, per-image shift or bf16 output (the entry refuses them).
template <int TM, int TN, bool PLAIN = false>
__device__ __forceinline__ void conv_epilogue_s3p(const ConvArgs& a, f32x16 (&acc)[TM][TN], float* S, int m_base, int n_base,
                                                  int lane, const v4f* pre, const v4f (&scv)[TN], const v4f (&shv)[TN]) {
    const bool per_img = !PLAIN && (a.flags & PEMP_CONV_SHIFT_PER_IMAGE);
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            PEMP_CONV_PATCH_PUT(S, acc[mi][ni], lr, lh);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
            conv_patch_store_f32(a, S, m_base + mi * 32, n_base + ni * 32, lane, scv[ni], shv[ni], per_img,
                                 PLAIN ? nullptr : pre + (mi * TN + ni) * 4, PLAIN ? 0u : a.flags & PEMP_CONV_BF16_IO);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // reads done before the patch is rewritten
        }
    }
}

// Epilogue of the 16-row wave tiles (conv_dma2.hip, R16): TN accumulators of 16 x 16 (rows 4 (lane >> 4) + e, column lane & 15) go
// through a 16 x (16 TN) LDS patch (row stride + 4 floats: the four lane groups write different banks) so that a lane owns 4
// consecutive channels of one pixel; shift, per-image shift and residual are added in conv_epilogue_lds_pre's order.
template <int TN>
__device__ __forceinline__ void conv_epilogue_r16(const ConvArgs& a, v4f (&acc)[TN], float* S, int m_base, int n_base, int lane) {
    constexpr int WN = TN * 16, LD = WN + 4, QPR = WN / 4;
    static_assert(16 * LD * 4 <= 4096 && (16 * QPR) % 64 == 0, "R16 epilogue patch");
    const bool relu = a.flags & PEMP_CONV_RELU;
    const bool per_img = a.flags & PEMP_CONV_SHIFT_PER_IMAGE;
    const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int e = 0; e < 4; ++e) S[(4 * g + e) * LD + ni * 16 + r16] = acc[ni][e];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's writes have landed (DS is in-order per wave)
    const int c4 = (lane % QPR) * 4, n = n_base + c4;
    v4f sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (a.scale) sc = *(const v4f*)(a.scale + n);
    if (a.shift && !per_img) sh = *(const v4f*)(a.shift + n);
#pragma unroll
    for (int i = 0; i < 16 * QPR / 64; ++i) {
        const int row = (lane + 64 * i) / QPR;
        const int m = m_base + row;
        const v4f v = *(const v4f*)(S + row * LD + c4);
        if (m < a.M) {
            v4f add = sh;
            if (per_img) add += *(const v4f*)(a.shift + (size_t)(m / a.HoWo) * a.Cout + n);
            if (a.res) add += load_quad(a.res, (size_t)m * a.ldr + n, a.flags & PEMP_CONV_BF16_IO);
            store_quad(a.y, (size_t)m * a.ldy + n, conv_affine_quad(v, sc, add, relu), a.flags & PEMP_CONV_BF16_IO);
        }
    }
}

// The launch entries below take a SHAPE index 1..9 (conv_tiles.h: the table and decode_tile, which turns a tile id into one).
// conv_dma.hip
int launch_conv_dma(int shape, const ConvArgs& a, hipStream_t st);
// conv_dma2.hip
bool conv_dma2_supported(const ConvArgs& a);
int launch_conv_dma2(int shape, const ConvArgs& a, hipStream_t st);
int launch_conv_dma2_group(int shape, ConvGroupArgs& g, hipStream_t st);      // fills g.first / g.nblk
int launch_conv_dma2_hybrid(const ConvArgs& a, hipStream_t st);             // shape 9; -2: the geometry has no hybrid split
int conv_dma2_hybrid_rows(int M, int Cout);                               // rows on the 64 x 64 tile in that launch (0: no split)
int launch_conv_dma2_bf16(int shape, const ConvArgs& a, hipStream_t st);     // bf16 operands (Cin / ldx / Kpad in dwords)
int launch_conv_dma2_db(int shape, ConvArgs a, void* ws, size_t ws_bytes, bool split, hipStream_t st);   // + DropBlock row scaling
// split-K plan of a shape for this geometry: number of unsplit tiles, split tiles, pieces per split tile (pieces == 1: the
// variant runs unsplit) and the workspace the launch needs (counters first, then the partial tiles)
struct SplitKPlan { int full, split, pieces; size_t ws_bytes; };
SplitKPlan conv_dma2_splitk_plan(int shape, const ConvArgs& a);
int launch_conv_dma2_splitk(int shape, ConvArgs a, void* ws, size_t ws_bytes, hipStream_t st);
// split3 family (a.w = the weights from pemp_pack_split3_bf16); split: the split-K form (ws as for launch_conv_dma2_splitk)
int launch_conv_dma2_split3(int shape, ConvArgs a, void* ws, size_t ws_bytes, bool split, hipStream_t st);
int launch_conv_dma2_group_split3(int shape, ConvGroupArgs& g, hipStream_t st);
// ... with the statistics epilogue (a.stats; unsplit, zero padding, no affine / residual); whether a shape has that form
int launch_conv_dma2_split3_stats(int shape, const ConvArgs& a, hipStream_t st);
bool conv_dma2_split3_stats_shape(int shape);
// its persistent forms (shapes 3 and 6): a resident grid walks the tiles
int launch_conv_dma2_split3_persist(int shape, const ConvArgs& a, hipStream_t st);
// (with PEMP_CONV_OUT_SPLIT3: the producer variant of the shape, which has no residual path; whether a shape has one)
bool conv_dma2_persist_out_split3(int shape);
// ... and the forms whose activations come pre-split (PEMP_CONV_IN_SPLIT3; shape 6 only), one tile per block or persistent; with
// PEMP_CONV_OUT_SPLIT3 / _ALSO in a.flags the variants that store pre-split (_ALSO: the second output's pointer in a.res)
int launch_conv_dma2_split3_pre(int shape, bool persistent, const ConvArgs& a, hipStream_t st);
// conv_panel.hip: the activation-stationary split3 form of short-K 1x1 convs (shapes 1 and 2 = 128 / 64 columns at a time)
bool conv_panel_supported(const ConvArgs& a);
int launch_conv_panel(int shape, const ConvArgs& a, hipStream_t st);
// conv_row3.hip: 3x3 / stride 1 / pad == dil convs on pre-split activations, one A stage per (chunk, kh) group (tile ids 246 /
// 249: one tile per block / persistent)
bool conv_row3_supported(const ConvArgs& a);
int launch_conv_row3(bool persistent, const ConvArgs& a, hipStream_t st);
// conv_ring.hip: the persistent 256 x 128 form of 1x1 / pad 0 convs on fp32 activations with a three-deep activation ring (tile id 349)
bool conv_ring_supported(const ConvArgs& a);
int launch_conv_ring(const ConvArgs& a, hipStream_t st);
int conv_dma2_simds();                                                     // SIMDs of the current device (4 per CU)
int pack_split3(const float* w, void* out, int cout, int kpad, hipStream_t st);
// conv_stem_pool.hip: the 7x7 / 2 / 3 NHWC4 stem (split3 weights) + its 3 / 2 / 1 ceil-mode max-pool in one launch (PEMP_CONV_POOL3S2)
int launch_conv_stem_pool(const ConvArgs& a, hipStream_t st);
int conv_stem_pool_out(int i);

// Grid of a persistent kernel (XcdTileRange's walk): the blocks that are resident at once -- the occupancy of the kernel, asked
// for once and kept in ``occ_cache`` (zero on entry; one per instantiation; racing fills write the same value), times the CUs --
// at least 8 (every XCD's range needs a block), at most ``tiles``.  -> 0 and the grid, or an error (set; ``what`` names the kernel).
template <class Kern> int allow_lds(Kern kern, size_t lds);      // conv_tiles.h
template <class Kern>
int persistent_grid(Kern kern, int threads, size_t lds, long long tiles, int& occ_cache, const char* what, int& grid_out) {
    if (!occ_cache) {
        const int rc = allow_lds(kern, lds);        // the occupancy query wants what the launch will have
        if (rc) return rc;
        int v = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, (const void*)kern, threads, lds);
        if (e != hipSuccess || v <= 0) {
            set_error("%s: occupancy query failed (%s, %d blocks)", what, hipGetErrorString(e), v);
            return -1;
        }
        occ_cache = v;
    }
    long long grid = (long long)occ_cache * (conv_dma2_simds() / 4);
    if (grid < 8) grid = 8;
    if (grid > tiles) grid = tiles;
    grid_out = (int)grid;
    return 0;
}

}  // namespace pemp
