// Implicit-GEMM convolution for gfx950 on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulate: bit-for-bit an fmaf chain, so parity with the fp32 reference is limited only by
// summation order).
//
//   GEMM view:  D[m][n] = sum_k A[m][k] * B[k][n]
//     m = (image, ho, wo) output pixel        M = N*Ho*Wo
//     n = output channel                      (Cout)
//     k = (kh, kw, ci), ci fastest            K = KH*KW*Cin      (NHWC input, KRSC weights)
//
//   Block = 256 threads = 4 waves, block tile BM x BN, K step 32 floats (= 8 "quads" of 4).
//   Each wave owns a (BM/WGM) x (BN/WGN) sub-tile made of 32x32 MFMA tiles.
//
//   LDS image (double buffered): A as float4 As[8 quads][BM rows], B as float4 Bs[8][BN];
//   element [q][r] holds k = 4q..4q+3 of row r and is stored at [q][r ^ q]: the 8 lanes that
//   stage one row's 128 contiguous bytes (q = 0..7) land on 8 different 16-B slots
//   (ds_write_b128 conflict-free), and a wave's ds_read_b128 of 32 consecutive rows of one quad
//   still covers 32 distinct slots.
//
//   MFMA operand order: lane l = (h = l>>5, r = l&31) reads quad 2j+h of row r and feeds its 4
//   floats to 4 consecutive MFMAs, i.e. MFMA e of pair j contracts k = {8j+e, 8j+4+e}.  A and B
//   use the same pairing, so the result is the plain dot product in a fixed, deterministic
//   order.
//
//   Staging: global -> registers (issued before the MFMAs of the current step) -> LDS buffer
//   b^1 after them; one __syncthreads per K step.
#include "conv_tiles.h"

namespace pemp {


template <int BM, int BN, int WGM, bool STEM>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvArgs a) {
    constexpr int WGN = 4 / WGM;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int AL = BM / 32, BL = BN / 32;  // v4f loads per thread per K step
    static_assert(TM >= 1 && TN >= 1, "wave tile");

    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* As = smem;                    // [2][8][BM]
    v4f* Bs = smem + 2 * 8 * BM;       // [2][8][BN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave / WGN) * WM;
    const int wn0 = (wave % WGN) * WN;
    const int lr = lane & 31, lh = lane >> 5;

    // n tiles vary fastest so that consecutive blocks reuse one A row-panel from L2
    const int ntn = a.Cout / BN;
    const int tile_id = xcd_tile_order(blockIdx.x, gridDim.x);
    const int bm = tile_id / ntn;
    const int bn = tile_id % ntn;
    const int m0 = bm * BM, n0 = bn * BN;

    // ---- staging roles: thread (q, r) moves quad q of rows r + 32 i --------------------------
    const int q = tid & 7;
    const int r = tid >> 3;

    int a_pix[AL];   // element offset of (image, hi0, wi0) *without* ldx scaling: img*H*W + hi0*W + wi0
    int a_hi0[AL], a_wi0[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        int m = m0 + r + 32 * i;
        bool ok = m < a.M;
        int mm = ok ? m : 0;
        int img = mm / a.HoWo;
        int rem = mm - img * a.HoWo;
        int ho = rem / a.Wo;
        int wo = rem - ho * a.Wo;
        int hi0 = ho * a.stride - a.pad;
        int wi0 = wo * a.stride - a.pad;
        a_hi0[i] = ok ? hi0 : -(1 << 28);   // invalid rows fail every bounds test
        a_wi0[i] = wi0;
        a_pix[i] = img * a.H * a.W + hi0 * a.W + wi0;
    }
    const float* wrow[BL];
#pragma unroll
    for (int i = 0; i < BL; ++i) wrow[i] = a.w + (size_t)(n0 + r + 32 * i) * a.Kpad + q * 4;

    v4f ra[AL], rb[BL];
    unsigned okmask = 0;   // bit i: ra[i] holds real data (else it is zeroed before staging)

    // Source cursor of the generic path: K steps walk (tap outer, 32-channel chunk inner).  Inside
    // a tap every row pointer just advances by 32 floats; only a tap change re-derives pointers and
    // bounds (that keeps the per-step VALU/SALU work next to nothing).  Out-of-image taps point at
    // the tensor base (a harmless valid address) and are zeroed at staging time, so no load is
    // conditional per lane and the wave never waits on memory before its MFMAs.
    const float* pa[AL];
    const float* pb[BL];
#pragma unroll
    for (int i = 0; i < BL; ++i) pb[i] = wrow[i];
    int cur_tap = 0, cur_cb = 0;
#define PEMP_SET_TAP(tap_, cb_)                                                                      \
    do {                                                                                             \
        const int tap__ = (tap_);                                                                    \
        const int coff__ = (cb_) * 32 + q * 4;                                                       \
        const int kh = tap__ / a.KW, kw = tap__ - kh * a.KW;                                         \
        const int dh = kh * a.dil, dw = kw * a.dil;                                                  \
        const bool tok = tap__ < a.ntaps;                                                            \
        const bool pv__ = a.padv && tok;              /* out-of-image taps read the padding vector */ \
        const float* const oob__ = pv__ ? a.padv + coff__ : a.x;                                     \
        okmask = 0;                                                                                  \
        _Pragma("unroll") for (int i = 0; i < AL; ++i) {                                             \
            const int hi = a_hi0[i] + dh, wi = a_wi0[i] + dw;                                        \
            const bool ok = tok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;     \
            pa[i] = ok ? a.x + (ptrdiff_t)(a_pix[i] + dh * a.W + dw) * a.ldx + coff__ : oob__;       \
            okmask |= ((ok || pv__) ? 1u : 0u) << i;                                                 \
        }                                                                                            \
    } while (0)

    // loads of the CURRENT cursor position (generic) / of K step kt_ (stem)
#define PEMP_GLOAD(kt_)                                                                              \
    do {                                                                                             \
        if constexpr (STEM) {                                                                        \
            const int tap = (kt_) * 8 + q;                                                           \
            const int kh = tap / a.KW, kw = tap - kh * a.KW;                                         \
            const bool tok = tap < a.ntaps;                                                          \
            const int dh = kh * a.dil, dw = kw * a.dil;                                              \
            okmask = 0;                                                                              \
            _Pragma("unroll") for (int i = 0; i < AL; ++i) {                                         \
                const int hi = a_hi0[i] + dh, wi = a_wi0[i] + dw;                                    \
                const bool ok = tok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W; \
                const float* p = ok ? a.x + (ptrdiff_t)(a_pix[i] + dh * a.W + dw) * 4 : a.x;         \
                ra[i] = *(const v4f*)p;                                                              \
                okmask |= (ok ? 1u : 0u) << i;                                                       \
            }                                                                                        \
        } else {                                                                                     \
            _Pragma("unroll") for (int i = 0; i < AL; ++i) ra[i] = *(const v4f*)pa[i];              \
        }                                                                                            \
        _Pragma("unroll") for (int i = 0; i < BL; ++i) rb[i] = *(const v4f*)pb[i];                   \
    } while (0)

    // move the cursor one K step forward
#define PEMP_ADVANCE()                                                                               \
    do {                                                                                             \
        if constexpr (STEM) {                                                                        \
            _Pragma("unroll") for (int i = 0; i < BL; ++i) pb[i] += 32;                              \
        } else if (a.ntaps > 1) {                                                                    \
            /* multi-tap convs: channel chunk outer, tap inner (same order as conv_dma.hip: the taps \
               of one chunk re-read the same lines back to back -> L2 hits) */                       \
            if (++cur_tap == a.ntaps) {                                                              \
                cur_tap = 0;                                                                         \
                ++cur_cb;                                                                            \
            }                                                                                        \
            PEMP_SET_TAP(cur_tap, cur_cb);                                                           \
            const int koff = cur_tap * a.Cin + cur_cb * 32;                                          \
            _Pragma("unroll") for (int i = 0; i < BL; ++i) pb[i] = wrow[i] + koff;                   \
        } else {                                                                                     \
            _Pragma("unroll") for (int i = 0; i < BL; ++i) pb[i] += 32;                              \
            _Pragma("unroll") for (int i = 0; i < AL; ++i) pa[i] += 32;                              \
        }                                                                                            \
    } while (0)

#define PEMP_LSTORE(buf_)                                                                            \
    do {                                                                                             \
        v4f* Ab_ = As + (buf_) * 8 * BM + q * BM;                                                 \
        v4f* Bb_ = Bs + (buf_) * 8 * BN + q * BN;                                                 \
        _Pragma("unroll") for (int i = 0; i < AL; ++i) {                                             \
            v4f v = ra[i];                                                                        \
            if (!((okmask >> i) & 1u)) v = v4f{0.f, 0.f, 0.f, 0.f};                          \
            Ab_[(r + 32 * i) ^ q] = v;                                                               \
        }                                                                                            \
        _Pragma("unroll") for (int i = 0; i < BL; ++i) Bb_[(r + 32 * i) ^ q] = rb[i];                \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    if constexpr (!STEM) PEMP_SET_TAP(0, 0);
    PEMP_GLOAD(0);
    PEMP_LSTORE(0);
    __syncthreads();

    const int arow = wm0 + lr, brow = wn0 + lr;
#ifndef PEMP_ABLATE
#define PEMP_ABLATE 0   // 1: no global loads in the loop, 2: + no LDS staging/barrier, 3: + no LDS reads (timing builds only)
#endif
    for (int kt = 0; kt < a.nk; ++kt) {
        const int buf = (PEMP_ABLATE >= 2) ? 0 : (kt & 1);
        if (PEMP_ABLATE < 1 && kt + 1 < a.nk) {   // wave-uniform branch; the last step re-stages stale registers (unused)
            PEMP_ADVANCE();
            PEMP_GLOAD(kt + 1);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the MFMAs (hipcc sinks them to their use)

        const v4f* Ab = As + buf * 8 * BM;
        const v4f* Bb = Bs + buf * 8 * BN;
        v4f af[2][TM], bf[2][TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) af[0][mi] = Ab[lh * BM + ((arow + mi * 32) ^ lh)];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) bf[0][ni] = Bb[lh * BN + ((brow + ni * 32) ^ lh)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < 3) {   // prefetch the next quad pair while this one is in the matrix pipe
                const int qq = 2 * (j + 1) + lh;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) af[(j + 1) & 1][mi] = Ab[qq * BM + ((arow + mi * 32) ^ qq)];
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) bf[(j + 1) & 1][ni] = Bb[qq * BN + ((brow + ni * 32) ^ qq)];
            }
            __builtin_amdgcn_sched_barrier(0);   // reads of pair j+1 stay in front of the MFMAs of pair j
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const v4f av = af[j & 1][mi], bv = bf[j & 1][ni];
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[mi][ni], 0, 0, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (PEMP_ABLATE < 2) {
            PEMP_LSTORE(buf ^ 1);
            __syncthreads();
        }
    }
#undef PEMP_GLOAD
#undef PEMP_ADVANCE
#undef PEMP_SET_TAP
#undef PEMP_LSTORE

    // ---- epilogue: transpose through LDS (staging buffers are free after the loop's last barrier) ----
    conv_epilogue_lds<TM, TN>(a, acc, (float*)smem + wave * 1024, m0 + wm0, n0 + wn0, lane);
}

// the register-staged kernels (ids 1..3: the 4-wave shapes of the table)
static int launch_conv(int shape, const ConvArgs& a, hipStream_t st) {
    return with_tile<FamIgemm>(shape, [&](auto t) {
        using T = decltype(t);
        auto kern = (a.flags & PEMP_CONV_STEM4) ? conv_igemm_kernel<T::BM, T::BN, T::WGM, true> : conv_igemm_kernel<T::BM, T::BN, T::WGM, false>;
        return launch_with_lds(kern, tile_grid<T>(a), 256, tile_lds<T>(), st, a, "conv_igemm");
    });
}

}  // namespace pemp

using namespace pemp;

extern "C" int pemp_conv2d_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                                    const float* scale, const float* shift, const float* residual,
                                    void* stream) {
    return pemp_conv2d_padv_nhwc_f32(d, x, w, y, scale, shift, residual, nullptr, stream);
}

static int conv2d_impl(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale, const float* shift,
                       const float* residual, const float* pad_value, void* ws, size_t ws_bytes, void* stream);

extern "C" int pemp_conv2d_padv_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                                         const float* scale, const float* shift, const float* residual,
                                         const float* pad_value, void* stream) {
    PEMP_REQUIRE(!d || !decode_tile(d->tile).splitk,
                 "conv2d: the split-K tile ids 31..37 / 51..56 need pemp_conv2d_splitk_nhwc_f32 (workspace)");
    return conv2d_impl(d, x, w, y, scale, shift, residual, pad_value, nullptr, 0, stream);
}

extern "C" int pemp_conv2d_splitk_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                                           const float* scale, const float* shift, const float* residual, void* ws,
                                           size_t ws_bytes, void* stream) {
    return conv2d_impl(d, x, w, y, scale, shift, residual, nullptr, ws, ws_bytes, stream);
}

extern "C" int pemp_conv2d_padv_splitk_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                                                const float* scale, const float* shift, const float* residual,
                                                const float* pad_value, void* ws, size_t ws_bytes, void* stream) {
    PEMP_REQUIRE(pad_value, "conv2d_padv_splitk: pad_value is null");
    return conv2d_impl(d, x, w, y, scale, shift, residual, pad_value, ws, ws_bytes, stream);
}

// argument checks of one conv + its ConvArgs (``any_taps``: a padding value may accompany a 1x1 conv -- it is never read)
static int conv_fill(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale, const float* shift,
                     const float* residual, const float* pad_value, ConvArgs& a, bool any_taps = false, bool pooled = false) {
    PEMP_REQUIRE(d && x && w && y, "conv2d: null pointer");
    PEMP_REQUIRE(pooled || !(d->flags & (PEMP_CONV_OUT_SPLIT3 | PEMP_CONV_IN_SPLIT3 | PEMP_CONV_OUT_SPLIT3_ALSO)),
                 "conv2d: pre-split activations belong to pemp_conv2d_nhwc_f32 / _padv_ (no grouped / dropblock / statistics / bf16 form)");
    PEMP_REQUIRE(pooled || !(d->flags & PEMP_CONV_POOL3S2), "conv2d: PEMP_CONV_POOL3S2 belongs to pemp_conv2d_nhwc_f32 (no grouped / dropblock / statistics / bf16 form)");
    PEMP_REQUIRE(pooled || !(d->flags & (PEMP_CONV_RES_S2 | PEMP_CONV_RES_HEVEN | PEMP_CONV_RES_WEVEN)),
                 "conv2d: PEMP_CONV_RES_S2 belongs to pemp_conv2d_nhwc_f32 (no grouped / dropblock / statistics / bf16 form)");
    PEMP_REQUIRE(!pad_value || (!(d->flags & PEMP_CONV_STEM4) && (any_taps || d->KH * d->KW > 1) && ((uintptr_t)pad_value & 15) == 0),
                 "conv2d: pad_value needs a multi-tap non-stem conv and a 16-byte aligned [Cin] vector");
    PEMP_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "conv2d: bad dims");
    PEMP_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->dil > 0 && d->pad >= 0, "conv2d: bad kernel geometry");
    const int ho = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
    const int wo = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
    PEMP_REQUIRE(ho == d->Ho && wo == d->Wo, "conv2d: Ho/Wo (%d,%d) do not match geometry (%d,%d)", d->Ho, d->Wo, ho, wo);
    PEMP_REQUIRE(d->Cout % 64 == 0, "conv2d: Cout=%d must be a multiple of 64", d->Cout);
    PEMP_REQUIRE(d->ldy >= d->Cout && d->ldy % 4 == 0 && ((uintptr_t)y & 15) == 0, "conv2d: ldy must be >= Cout and a multiple of 4, y 16-byte aligned");
    PEMP_REQUIRE(!scale || ((uintptr_t)scale & 15) == 0, "conv2d: scale must be 16-byte aligned");
    PEMP_REQUIRE(!shift || ((uintptr_t)shift & 15) == 0, "conv2d: shift must be 16-byte aligned");
    PEMP_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "conv2d: x/w must be 16-byte aligned");
    const bool stem = d->flags & PEMP_CONV_STEM4;
    const int ntaps = d->KH * d->KW;
    if (stem) {
        PEMP_REQUIRE(d->Cin == 4 && d->ldx == 4, "conv2d: STEM4 needs NHWC4 input (Cin=ldx=4)");
        PEMP_REQUIRE(d->Kpad % 32 == 0 && d->Kpad >= ntaps * 4, "conv2d: STEM4 Kpad=%d too small / not x32", d->Kpad);
    } else {
        PEMP_REQUIRE(d->Cin % 32 == 0, "conv2d: Cin=%d must be a multiple of 32 (or use STEM4)", d->Cin);
        PEMP_REQUIRE(d->ldx >= d->Cin && d->ldx % 4 == 0, "conv2d: ldx=%d must be >= Cin and a multiple of 4", d->ldx);
        PEMP_REQUIRE(d->Kpad == ntaps * d->Cin, "conv2d: Kpad=%d must equal KH*KW*Cin=%d", d->Kpad, ntaps * d->Cin);
    }
    const long long in_elems = (long long)d->N * d->H * d->W * d->ldx;
    const long long out_elems = (long long)d->N * d->Ho * d->Wo * (long long)(d->ldy > d->ldr ? d->ldy : d->ldr);
    PEMP_REQUIRE(in_elems < (1ll << 31) && out_elems < (1ll << 31), "conv2d: tensor too large for 32-bit indexing");

    a.x = x; a.w = w; a.y = y; a.scale = scale; a.shift = shift; a.res = residual; a.padv = pad_value; a.stats = nullptr; a.bz = nullptr;
    a.bmask = nullptr; a.bmean = nullptr; a.binvstd = nullptr; a.ldbz = 0;
    a.rowmask = nullptr; a.rowcnt = nullptr;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.ldx = d->ldx; a.Ho = d->Ho; a.Wo = d->Wo;
    a.Cout = d->Cout; a.ldy = d->ldy; a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
    a.dil = d->dil; a.ldr = d->ldr; a.Kpad = d->Kpad; a.flags = d->flags;
    a.HoWo = d->Ho * d->Wo;
    a.M = d->N * a.HoWo;
    a.ntaps = ntaps;
    a.cin_steps = stem ? 1 : d->Cin / 32;
    a.nk = d->Kpad / 32;
    if (residual && !(d->flags & PEMP_CONV_OUT_SPLIT3_ALSO)) PEMP_REQUIRE(d->ldr >= d->Cout && d->ldr % 4 == 0 && ((uintptr_t)residual & 15) == 0, "conv2d: ldr must be >= Cout and x4, residual 16-byte aligned");
    a.sk_ws = nullptr; a.sk_cnt = nullptr; a.sk_full = 0; a.sk_S = 1;
    a.bm_first = 0;
    return 0;
}

static int conv2d_impl(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale, const float* shift,
                       const float* residual, const float* pad_value, void* ws, size_t ws_bytes, void* stream) {
    ConvArgs a;
    const int rc = conv_fill(d, x, w, y, scale, shift, residual, pad_value, a, false, true);
    if (rc) return rc;
    const bool stem = d->flags & PEMP_CONV_STEM4;
    int tile = d->tile;
    if (tile == 0) {
        // Measured on MI355X (scratch/conv_tune.py): at these problem sizes (M <= ~80k rows) the 64x64
        // tile wins or ties everywhere -- waves per SIMD matter more than operand reuse for the
        // 64-cycle fp32 MFMA.  Callers that know better (engine autotune) pass an explicit tile.
        tile = 3;
    }
    TileId t = decode_tile(tile);
    if (t.ring) {                        // conv_ring.hip: same results as 43 / 49 where it applies, an error elsewhere
        PEMP_REQUIRE(!ws && !pad_value && conv_ring_supported(a),
                     "conv2d: tile %d unsupported: needs a 1x1 conv without padding on fp32 activations with Kpad == Cin >= 128 and Cout %% 128 == 0, the "
                     "fp32 output or PEMP_CONV_OUT_SPLIT3 (ldy == Cout); no residual, PEMP_CONV_OUT_SPLIT3_ALSO, PEMP_CONV_IN_SPLIT3, PEMP_CONV_RES_S2, "
                     "padding value, stem, split-K or workspace; operands < 2 GiB", tile);
        return launch_conv_ring(a, (hipStream_t)stream);
    }
    // y: bf16 [M][Cout / 32][3][32].  The persistent ids 47 / 49 / 149 run their producer variants (compile-time: no residual path,
    // which is what leaves registers for the split); a persistent shape without one would run as the id it walks -- same tiles,
    // same results (conv_dma2_persist_out_split3)
    const bool out_split3 = d->flags & PEMP_CONV_OUT_SPLIT3;
    if (out_split3)
        PEMP_REQUIRE(t.family == TILE_SPLIT3 && !t.splitk && !t.panel && !ws && !stem && !residual && a.Cout % 32 == 0 && a.ldy == a.Cout,
                     "conv2d: PEMP_CONV_OUT_SPLIT3 needs an unsplit split3 tile id (41..44, 46, 47, 49, 146, 149), ldy == Cout, no residual / workspace");
    // y fp32 as without the flag, and the same values pre-split, bf16 [M][Cout / 32][3][32], through `residual` (never read)
    const bool also_split3 = d->flags & PEMP_CONV_OUT_SPLIT3_ALSO;
    if (also_split3) {
        PEMP_REQUIRE(t.presplit && !out_split3 && !ws && !stem && a.Cout % 32 == 0,
                     "conv2d: PEMP_CONV_OUT_SPLIT3_ALSO needs tile id 146 / 149, no PEMP_CONV_OUT_SPLIT3 / split-K / workspace / stem");
        PEMP_REQUIRE(residual && ((uintptr_t)residual & 15) == 0,
                     "conv2d: PEMP_CONV_OUT_SPLIT3_ALSO takes the pre-split tensor (16-byte aligned) in the residual argument; a residual is never read");
        const char *y0 = (const char*)y, *y1 = y0 + ((size_t)(a.M - 1) * a.ldy + a.Cout) * 4;
        const char *s0 = (const char*)residual, *s1 = s0 + (size_t)a.M * a.Cout * 6;
        PEMP_REQUIRE(y1 <= s0 || s1 <= y0, "conv2d: PEMP_CONV_OUT_SPLIT3_ALSO: y and the pre-split tensor overlap");
    }
    // the residual on a grid twice as fine, [N][Hr][Wr] (row (n, ho, wo) adds pixel (n, 2 ho, 2 wo)): compile-time variants of ids
    // 71 / 72 at Kpad 64 / 128 (conv_panel_rs2_kernel) and of id 43 (conv_dma2_rs2_kernel); nothing else reads a residual that way
    const bool res_s2 = d->flags & PEMP_CONV_RES_S2;
    PEMP_REQUIRE(res_s2 || !(d->flags & (PEMP_CONV_RES_HEVEN | PEMP_CONV_RES_WEVEN)), "conv2d: PEMP_CONV_RES_HEVEN / _WEVEN come with PEMP_CONV_RES_S2");
    if (res_s2) {
        PEMP_REQUIRE(residual && !out_split3 && !also_split3 && !(d->flags & PEMP_CONV_IN_SPLIT3) && !ws && !stem && !pad_value,
                     "conv2d: PEMP_CONV_RES_S2 needs a residual, no pre-split operands / PEMP_CONV_OUT_SPLIT3_ALSO / split-K / workspace / stem / padding value");
        PEMP_REQUIRE(t.family == TILE_SPLIT3 && t.exists && !t.splitk && !t.persistent && !t.presplit &&
                         (t.panel ? (a.nk == 2 || (a.nk == 4 && t.shape == 2)) : t.shape == 3),
                     "conv2d: PEMP_CONV_RES_S2 needs tile id 43, 72 with Kpad 64 or 128, or 71 with Kpad 64 (tile %d, Kpad %d: the persistent, split-K, "
                     "pre-split and fp32-chain ids have no strided-residual form)", tile, a.Kpad);
        a.Hr = 2 * a.Ho - 1 + ((d->flags & PEMP_CONV_RES_HEVEN) ? 1 : 0);
        a.Wr = 2 * a.Wo - 1 + ((d->flags & PEMP_CONV_RES_WEVEN) ? 1 : 0);
        PEMP_REQUIRE((long long)a.N * a.Hr * a.Wr * a.ldr < (1ll << 31), "conv2d: PEMP_CONV_RES_S2: residual too large for 32-bit indexing");
    }
    if (d->flags & PEMP_CONV_POOL3S2) {     // the fused stem (conv_stem_pool.hip): y is the pooled tensor
        PEMP_REQUIRE(stem && t.family == TILE_SPLIT3 && !t.splitk && !t.panel && !residual && !pad_value,
                     "conv2d: PEMP_CONV_POOL3S2 needs PEMP_CONV_STEM4 with split3 weights (a tile id 41..49), no residual, no padding value");
        return launch_conv_stem_pool(a, (hipStream_t)stream);
    }
    PEMP_REQUIRE(tile != 33 && tile != 53, "conv2d: no split-K variant of the 64 x 64 tile");
    PEMP_REQUIRE(tile != 45 && tile != 55, "conv2d: no split3 form of the 128 x 64 8-wave tile");
    PEMP_REQUIRE(tile != 48, "conv2d: no persistent split3 form of the 128 x 128 4-wave tile");
    PEMP_REQUIRE(t.exists, "conv2d: unknown tile id %d", tile);
    hipStream_t st = (hipStream_t)stream;
    PEMP_REQUIRE(t.presplit == ((d->flags & PEMP_CONV_IN_SPLIT3) != 0), "conv2d: tile ids 146 / 149 and PEMP_CONV_IN_SPLIT3 come together (tile %d)", tile);
    if (t.presplit) {                    // conv_dma2.hip, A3: x bf16 [N][H][W][Cin / 32][3][32], w from pemp_pack_split3_bf16
        PEMP_REQUIRE(!stem && !ws && a.ntaps > 1 && a.ntaps <= 16 && a.ldx == a.Cin && !(d->flags & PEMP_CONV_SHIFT_PER_IMAGE),
                     "conv2d: tile %d takes convs of 2..16 taps with ldx == Cin, no per-image shift, no workspace", tile);
        PEMP_REQUIRE(conv_dma2_supported(a) && (long long)a.Cout * a.Kpad * 6 < (1ll << 31),
                     "conv2d: tile %d needs <= 32 taps and operands < 2 GiB (a padding value behind the activations)", tile);
        PEMP_REQUIRE_COUT("conv2d", t.shape, a.Cout);
        if (t.row3) {                    // conv_row3.hip: same results as 146 / 149 where it applies, an error elsewhere
            PEMP_REQUIRE(conv_row3_supported(a),
                         "conv2d: tile %d unsupported: needs a 3x3 / stride 1 / pad == dil conv, the plain fp32 output without residual / padding value, "
                         "and a stage of at most 288 rows (256 + 2 d + d ceil((255 + 2 d) / W))", tile);
            return launch_conv_row3(t.persistent, a, st);
        }
        return launch_conv_dma2_split3_pre(t.shape, t.persistent, a, st);      // (+ the variants of both ids that store pre-split)
    }
    if (t.family == TILE_SPLIT3) {       // conv_dma2.hip, S3: w from pemp_pack_split3_bf16
        PEMP_REQUIRE(!stem && conv_dma2_supported(a) && (long long)a.Cout * a.Kpad * 6 < (1ll << 31),
                     "conv2d: split3 tile %d needs a geometry of the buffer-addressed kernels (no stem, <= 32 taps, operands < 2 GiB)", tile);
        PEMP_REQUIRE_COUT("conv2d", t.shape, a.Cout);
        if (t.panel) {                   // conv_panel.hip: same results as 41..49 where it applies, an error elsewhere
            PEMP_REQUIRE(!ws && conv_panel_supported(a),
                         "conv2d: tile %d needs a 1x1 conv without padding, Kpad <= 256, no padding value / per-image shift / workspace, operands < 2 GiB", tile);
            return launch_conv_panel(t.shape, a, st);
        }
        if (t.persistent && (!out_split3 || conv_dma2_persist_out_split3(t.shape))) return launch_conv_dma2_split3_persist(t.shape, a, st);      // same results as the id it walks
        return launch_conv_dma2_split3(t.shape, a, ws, ws_bytes, t.splitk, st);
    }
    // the fp32 chain: every id falls back towards the pointer-addressed kernels where its own do not apply (same results)
    if (t.family == TILE_DMA2 && t.splitk) {      // the last round of tiles split along K
        if (conv_dma2_supported(a)) {
            PEMP_REQUIRE_COUT("conv2d", t.shape, a.Cout);
            return launch_conv_dma2_splitk(t.shape, a, ws, ws_bytes, st);
        }
        t.splitk = false;                // 3x -> 2x
    }
    if (t.family == TILE_DMA2 && t.shape == 9) {  // hybrid: whole rounds of 32 x 32 wave tiles + the remaining rows on 16-row tiles, one grid
        if (conv_dma2_supported(a)) {
            const int rc2 = launch_conv_dma2_hybrid(a, st);
            if (rc2 != -2) return rc2;
        }
        t.shape = 3;                     // no hybrid split for this geometry: 29 -> 23
    }
    if (t.family == TILE_DMA2) {         // buffer-addressed LDS-DMA + barrier inside the MFMA stream
        if (conv_dma2_supported(a)) {
            PEMP_REQUIRE_COUT("conv2d", t.shape, a.Cout);
            return launch_conv_dma2(t.shape, a, st);
        }
        t.family = TILE_DMA;             // stem / padding value / > 32 taps / >= 2 GiB operands: 2x -> 1x, and 28 -> 13
        if (t.shape == 8) t.shape = 3;
    }
    if (t.family == TILE_DMA) {          // LDS-DMA staging, pointer-addressed (conv_dma.hip)
        PEMP_REQUIRE_COUT("conv2d", t.shape, a.Cout);
        return launch_conv_dma(t.shape, a, st);
    }
    PEMP_REQUIRE(t.shape != 1 || a.Cout % 128 == 0, "conv2d: tile 128x128 needs Cout %% 128 == 0");
    return launch_conv(t.shape, a, st);      // register staging (this file)
}


extern "C" int pemp_conv2d_group_nhwc_f32(int n, const pemp_conv_desc* d, const float* const* x, const float* const* w,
                                          float* const* y, const float* const* scale, const float* const* shift,
                                          const float* const* residual, const float* const* pad_value, void* stream) {
    PEMP_REQUIRE(n >= 1 && n <= CONV_GROUP_MAX && d && x && w && y, "conv2d_group: 1..%d member convs", CONV_GROUP_MAX);
    ConvGroupArgs g;
    g.n = n;
    const int tile = d[0].tile;
    const TileId t = decode_tile(tile);
    const bool s3 = t.family == TILE_SPLIT3 && t.exists && !t.splitk && !t.persistent && !t.panel && !t.presplit;
    PEMP_REQUIRE((t.family == TILE_DMA2 && !t.splitk && t.shape <= 8) || s3, "conv2d_group: tile must be one of the buffer-addressed variants 21..28 or 41..44, 46, got %d", tile);
    for (int i = 0; i < n; ++i) {
        PEMP_REQUIRE(d[i].tile == tile, "conv2d_group: every member must name the same tile variant");
        PEMP_REQUIRE(!pad_value || (pad_value[i] != nullptr) == (pad_value[0] != nullptr), "conv2d_group: pad_value for every member or for none");
        const int rc = conv_fill(&d[i], x[i], w[i], y[i], scale ? scale[i] : nullptr, shift ? shift[i] : nullptr,
                                 residual ? residual[i] : nullptr, pad_value ? pad_value[i] : nullptr, g.a[i], true);
        if (rc) return rc;
        PEMP_REQUIRE(conv_dma2_supported(g.a[i]), "conv2d_group: member %d lies outside the buffer-addressed kernels (stem / > 32 taps / 2 GiB operands / padding vector not behind the activations)", i);
        PEMP_REQUIRE_COUT("conv2d_group", t.shape, g.a[i].Cout);
        PEMP_REQUIRE(!s3 || (long long)g.a[i].Cout * g.a[i].Kpad * 6 < (1ll << 31), "conv2d_group: split3 weights of 2 GiB or more");
    }
    // members run beside each other in one grid: no member may write what another one writes or reads.  Two tensors that interleave
    // in one buffer (the ASPP branches write channel slices of the concat buffer: equal per-pixel stride, disjoint channel windows)
    // are fine; any other overlap of the byte ranges is refused.
    auto clash = [](const float* pa, long long rows_a, int ld_a, int c_a, const float* pb, long long rows_b, int ld_b, int c_b) {
        if (!pa || !pb) return false;
        const char *a0 = (const char*)pa, *a1 = a0 + ((rows_a - 1) * ld_a + c_a) * 4;
        const char *b0 = (const char*)pb, *b1 = b0 + ((rows_b - 1) * ld_b + c_b) * 4;
        if (a1 <= b0 || b1 <= a0) return false;                       // disjoint ranges
        if (ld_a != ld_b) return true;
        const long long delta = (b0 - a0) / 4, r = ((delta % ld_a) + ld_a) % ld_a;      // b's window inside a's pixel
        return !(r >= c_a && r + c_b <= ld_a);
    };
    for (int i = 0; i < n; ++i) {
        const long long Mi = (long long)g.a[i].N * g.a[i].Ho * g.a[i].Wo;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const long long Mj = (long long)g.a[j].N * g.a[j].Ho * g.a[j].Wo, Pj = (long long)g.a[j].N * g.a[j].H * g.a[j].W;
            PEMP_REQUIRE(j > i || !clash(g.a[i].y, Mi, g.a[i].ldy, g.a[i].Cout, g.a[j].y, Mj, g.a[j].ldy, g.a[j].Cout),
                         "conv2d_group: members %d and %d write the same output", i, j);
            PEMP_REQUIRE(!clash(g.a[i].y, Mi, g.a[i].ldy, g.a[i].Cout, g.a[j].x, Pj, g.a[j].ldx, g.a[j].Cin),
                         "conv2d_group: member %d writes what member %d reads as its input", i, j);
            PEMP_REQUIRE(!clash(g.a[i].y, Mi, g.a[i].ldy, g.a[i].Cout, g.a[j].res, Mj, g.a[j].ldr, g.a[j].Cout),
                         "conv2d_group: member %d writes what member %d reads as its residual", i, j);
        }
    }
    for (int i = n; i < CONV_GROUP_MAX; ++i) g.a[i] = g.a[0];
    return s3 ? launch_conv_dma2_group_split3(t.shape, g, (hipStream_t)stream) : launch_conv_dma2_group(t.shape, g, (hipStream_t)stream);
}

extern "C" int pemp_pack_split3_bf16(const float* w, void* out, int cout, int kpad, void* stream) {
    PEMP_REQUIRE(w && out && cout > 0 && kpad > 0 && kpad % 32 == 0, "pack_split3: null pointer or Kpad not a multiple of 32");
    PEMP_REQUIRE((((uintptr_t)w | (uintptr_t)out) & 15) == 0, "pack_split3: pointers must be 16-byte aligned");
    return pack_split3(w, out, cout, kpad, (hipStream_t)stream);
}


// conv (+ affine, residual, ReLU) followed by DropBlock2D's scaling of the output rows, in one launch: the buffer-addressed
// kernels only (tiles 21..27, or 31..37 with a split-K workspace)
extern "C" int pemp_conv2d_dropblock_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale,
                                              const float* shift, const float* residual, const float* rowmask, const int* kept_count,
                                              void* ws, size_t ws_bytes, void* stream) {
    PEMP_REQUIRE(rowmask && kept_count, "conv2d_dropblock: null mask / count");
    ConvArgs a;
    const int rc = conv_fill(d, x, w, y, scale, shift, residual, nullptr, a);
    if (rc) return rc;
    const TileId t = decode_tile(d->tile);
    PEMP_REQUIRE(t.family == TILE_DMA2 && t.exists && t.shape <= 7,
                 "conv2d_dropblock: tile must be 21..27 or 31..37 (no 33), got %d", d->tile);
    PEMP_REQUIRE(conv_dma2_supported(a), "conv2d_dropblock: geometry / operand size outside the buffer-addressed kernels");
    a.rowmask = rowmask;
    a.rowcnt = kept_count;
    PEMP_REQUIRE_COUT("conv2d_dropblock", t.shape, a.Cout);
    return launch_conv_dma2_db(t.shape, a, ws, ws_bytes, t.splitk, (hipStream_t)stream);
}


// The side-figure variant: bf16 operands, fp32 accumulation (conv_dma2.hip, BF16).  The descriptor is in ELEMENTS like every
// other; the kernel is handed Cin / ldx / Kpad in dwords (two bf16 each), which is all it needs to address bf16 rows.
extern "C" int pemp_conv2d_bf16_nhwc(const pemp_conv_desc* d, const void* x, const void* w, void* y, const float* scale,
                                     const float* shift, const void* residual, const void* pad_value, int out_f32, void* stream) {
    PEMP_REQUIRE(d && x && w && y, "conv2d_bf16: null pointer");
    PEMP_REQUIRE(!(d->flags & (PEMP_CONV_STEM4 | PEMP_CONV_BF16_IO | PEMP_CONV_POOL3S2 | PEMP_CONV_OUT_SPLIT3_ALSO)), "conv2d_bf16: no stem variant; unknown flags");
    PEMP_REQUIRE(d->Cin % 64 == 0 && d->ldx % 8 == 0 && d->ldx >= d->Cin && d->Kpad == d->KH * d->KW * d->Cin,
                 "conv2d_bf16: Cin must be a multiple of 64, ldx of 8 (bf16 elements), Kpad = KH*KW*Cin");
    PEMP_REQUIRE(!residual || !out_f32, "conv2d_bf16: a residual comes with a bf16 output");
    const TileId t = decode_tile(d->tile == 0 ? 24 : d->tile);
    PEMP_REQUIRE(t.family == TILE_DMA2 && !t.splitk && t.shape <= 7, "conv2d_bf16: tile must be 0 or 21..27");
    pemp_conv_desc h = *d;
    h.Cin = d->Cin / 2;
    h.ldx = d->ldx / 2;
    h.Kpad = d->Kpad / 2;
    ConvArgs a;
    // (the fp32 checks apply to the halved descriptor: Cin % 32, ldx % 4, 16-byte aligned operands; y / residual strides % 4)
    const int rc = conv_fill(&h, (const float*)x, (const float*)w, (float*)y, scale, shift, (const float*)residual,
                             (const float*)pad_value, a);
    if (rc) return rc;
    if (!out_f32) a.flags |= PEMP_CONV_BF16_IO;
    PEMP_REQUIRE(conv_dma2_supported(a), "conv2d_bf16: geometry / operand size outside the buffer-addressed kernels");
    PEMP_REQUIRE_COUT("conv2d_bf16", t.shape, a.Cout);
    return launch_conv_dma2_bf16(t.shape, a, (hipStream_t)stream);
}


// the id of a statistics / BatchNorm-backward launch: 0 runs as 23
static TileId stats_tile(const pemp_conv_desc* d) { return decode_tile(d->tile == 0 ? 23 : d->tile); }

static int conv_stats_fill(const char* what, const pemp_conv_desc* d, ConvArgs& a) {
    PEMP_REQUIRE(!(d->flags & (PEMP_CONV_STEM4 | PEMP_CONV_RELU | PEMP_CONV_SHIFT_PER_IMAGE | PEMP_CONV_POOL3S2 | PEMP_CONV_OUT_SPLIT3 | PEMP_CONV_IN_SPLIT3 | PEMP_CONV_OUT_SPLIT3_ALSO | PEMP_CONV_RES_S2 | PEMP_CONV_RES_HEVEN | PEMP_CONV_RES_WEVEN)), "%s: plain conv only (no stem / ReLU / per-image shift)", what);
    PEMP_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0 && d->stride > 0 && d->dil > 0 && d->pad >= 0,
                 "%s: bad geometry", what);
    const int ho = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
    const int wo = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
    PEMP_REQUIRE(ho == d->Ho && wo == d->Wo, "%s: Ho/Wo do not match geometry", what);
    PEMP_REQUIRE(d->Cout % 64 == 0 && d->Cin % 32 == 0 && d->ldx >= d->Cin && d->ldx % 4 == 0 && d->ldy >= d->Cout && d->ldy % 4 == 0,
                 "%s: Cout %% 64, Cin %% 32, strides %% 4", what);
    PEMP_REQUIRE(d->Kpad == d->KH * d->KW * d->Cin, "%s: Kpad must equal KH*KW*Cin", what);
    a.scale = nullptr; a.shift = nullptr; a.padv = nullptr; a.rowmask = nullptr; a.rowcnt = nullptr;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.ldx = d->ldx; a.Ho = d->Ho; a.Wo = d->Wo;
    a.Cout = d->Cout; a.ldy = d->ldy; a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
    a.dil = d->dil; a.ldr = d->ldr; a.Kpad = d->Kpad; a.flags = d->flags;
    a.HoWo = d->Ho * d->Wo;
    a.M = d->N * a.HoWo;
    a.ntaps = d->KH * d->KW;
    a.cin_steps = d->Cin / 32;
    a.nk = d->Kpad / 32;
    a.sk_ws = nullptr; a.sk_cnt = nullptr; a.sk_full = 0; a.sk_S = 1;
    a.bm_first = 0;
    if (!conv_dma2_supported(a)) {
        set_error("%s: geometry / operand size outside the buffer-addressed kernels", what);
        return -2;
    }
    const TileId t = stats_tile(d);
    PEMP_REQUIRE(t.family == TILE_DMA2 && t.exists && t.shape <= 7, "%s: tile must be 0, 21..27 or 31..37 (no 33)", what);
    PEMP_REQUIRE_COUT(what, t.shape, a.Cout);
    return 0;
}

static int conv_stats_common(const char* what, const pemp_conv_desc* d, ConvArgs& a, void* ws, size_t ws_bytes, hipStream_t st) {
    const int rc = conv_stats_fill(what, d, a);
    if (rc) return rc;
    const TileId t = stats_tile(d);
    return t.splitk ? launch_conv_dma2_splitk(t.shape, a, ws, ws_bytes, st) : launch_conv_dma2(t.shape, a, st);
}

extern "C" int pemp_conv2d_hybrid_rows(const pemp_conv_desc* d) {
    if (!d || d->N <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Cout <= 0) return 0;
    return conv_dma2_hybrid_rows(d->N * d->Ho * d->Wo, d->Cout);
}

extern "C" int pemp_conv2d_tile_shape(int id, int* bm, int* bn) {
    const TileId t = decode_tile(id);
    if (!t.exists) return 0;
    if (bm) *bm = kTileShapes[t.shape].bm;
    if (bn) *bn = kTileShapes[t.shape].bn;
    return 1;
}

extern "C" int pemp_conv2d_stats_rows(const pemp_conv_desc* d) {
    if (!d || d->N <= 0 || d->Ho <= 0 || d->Wo <= 0) return 0;
    const TileId t = stats_tile(d);          // by shape alone: a refused id of the two decades (33) answers like its shape
    if (t.family != TILE_DMA2 || t.shape > 7) return 0;      // 28 / 29 (16-row and hybrid launches) have no statistics epilogue
    return cdiv(d->N * d->Ho * d->Wo, kTileShapes[t.shape].bm);
}

extern "C" size_t pemp_conv2d_splitk_workspace_bytes(const pemp_conv_desc* d) {
    const TileId t = decode_tile(d ? d->tile : 0);      // 3x: fp32 chain; 5x: split3 (same plan)
    if (!t.splitk || !t.exists || d->N <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Cout <= 0 || d->Kpad < 32) return 0;
    ConvArgs a;
    a.M = d->N * d->Ho * d->Wo;
    a.Cout = d->Cout;
    a.nk = d->Kpad / 32;
    return conv_dma2_splitk_plan(t.shape, a).ws_bytes;
}

extern "C" int pemp_conv2d_stats_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, float* stats,
                                          void* ws, size_t ws_bytes, void* stream) {
    PEMP_REQUIRE(d && x && w && y && stats, "conv2d_stats: null pointer");
    PEMP_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)stats) & 15) == 0, "conv2d_stats: pointers must be 16-byte aligned");
    ConvArgs a;
    a.x = x; a.w = w; a.y = y; a.res = nullptr; a.stats = stats;
    a.bmask = nullptr; a.bz = nullptr; a.bmean = nullptr; a.binvstd = nullptr; a.ldbz = 0;
    return conv_stats_common("conv2d_stats", d, a, ws, ws_bytes, (hipStream_t)stream);
}

// ---- the statistics epilogue on the split3 family (conv_dma2.hip: launch_conv_dma2_split3_stats).  Entry points of their own:
// pemp_conv2d_stats_nhwc_f32 / pemp_conv2d_stats_rows keep answering for the fp32 chain only.
// the id of such a launch (0 runs as 43) -> its shape; 0 for an id the form does not take (persistent, panel, pre-split, split-K
// ids; another family's; a shape whose statistics form is not offered)
static int stats_split3_shape(const pemp_conv_desc* d) {
    const int id = d->tile == 0 ? 43 : d->tile;
    const TileId t = decode_tile(id);
    if (id < 41 || id > 46 || t.family != TILE_SPLIT3 || !t.exists || t.persistent || t.splitk || t.panel || t.presplit) return 0;
    return conv_dma2_split3_stats_shape(t.shape) ? t.shape : 0;
}

extern "C" int pemp_conv2d_stats_split3_rows(const pemp_conv_desc* d) {
    if (!d || d->N <= 0 || d->Ho <= 0 || d->Wo <= 0) return 0;
    const int shape = stats_split3_shape(d);
    return shape ? cdiv(d->N * d->Ho * d->Wo, kTileShapes[shape].bm) : 0;
}

extern "C" int pemp_split3_conv2d_stats_nhwc_f32(const pemp_conv_desc* d, const float* x, const void* w3, float* y, float* stats, void* stream) {
    PEMP_REQUIRE(d && x && w3 && y && stats, "conv2d_stats_split3: null pointer");
    PEMP_REQUIRE((((uintptr_t)x | (uintptr_t)w3 | (uintptr_t)y | (uintptr_t)stats) & 15) == 0, "conv2d_stats_split3: pointers must be 16-byte aligned");
    const int shape = stats_split3_shape(d);
    PEMP_REQUIRE(shape, "conv2d_stats_split3: tile %d has no split3 statistics form (0 or an unsplit id of 41..46 that pemp_conv2d_stats_split3_rows answers for)", d->tile);
    PEMP_REQUIRE(d->flags == 0, "conv2d_stats_split3: plain conv only (no flags: stem / ReLU / per-image shift / pre-split operands)");
    PEMP_REQUIRE(d->Cout > 0 && d->Cout >= kTileShapes[shape].bn, "conv2d_stats_split3: Cout=%d below the tile's %d columns", d->Cout, kTileShapes[shape].bn);
    ConvArgs a;
    a.x = x; a.w = (const float*)w3; a.y = y; a.res = nullptr; a.stats = stats;
    a.bmask = nullptr; a.bz = nullptr; a.bmean = nullptr; a.binvstd = nullptr; a.ldbz = 0;
    pemp_conv_desc f = *d;
    f.tile = 20 + shape;                 // conv_stats_fill's rules are those of the fp32-chain id of the same shape
    const int rc = conv_stats_fill("conv2d_stats_split3", &f, a);
    if (rc) return rc;
    if ((long long)a.Cout * a.Kpad * 6 >= (1ll << 31)) {     // (conv_dma2_supported counts 4 bytes per weight)
        set_error("conv2d_stats_split3: split3 weights of 2 GiB or more");
        return -2;
    }
    return launch_conv_dma2_split3_stats(shape, a, (hipStream_t)stream);
}

extern "C" int pemp_conv2d_bnbwd_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* residual,
                                          const uint32_t* mask, const float* z, int ldz, const float* mean, const float* invstd,
                                          float* stats, void* ws, size_t ws_bytes, void* stream) {
    PEMP_REQUIRE(d && x && w && y && z && mean && invstd && stats, "conv2d_bnbwd: null pointer");
    PEMP_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)stats | (uintptr_t)z | (uintptr_t)residual | (uintptr_t)mean |
                   (uintptr_t)invstd) & 15) == 0 && ((uintptr_t)mask & 3) == 0, "conv2d_bnbwd: pointers must be 16-byte aligned");
    PEMP_REQUIRE(ldz >= d->Cout && ldz % 4 == 0 && (!residual || (d->ldr >= d->Cout && d->ldr % 4 == 0)), "conv2d_bnbwd: ldz / ldr");
    ConvArgs a;
    a.x = x; a.w = w; a.y = y; a.res = residual; a.stats = stats;
    a.bmask = mask; a.bz = z; a.bmean = mean; a.binvstd = invstd; a.ldbz = ldz;
    return conv_stats_common("conv2d_bnbwd", d, a, ws, ws_bytes, (hipStream_t)stream);
}
