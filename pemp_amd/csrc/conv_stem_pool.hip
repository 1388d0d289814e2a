// The ResNet stem in one launch: 7x7 / stride 2 / pad 3 conv over an NHWC4 input (split3 arithmetic: conv_dma2.hip, S3) + folded
// affine + ReLU + the 3x3 / stride 2 / pad 1 ceil-mode max-pool behind it.  Only the pooled tensor goes to memory: the conv's own
// output (four times the pooled size) never leaves the CU.
//
// Tiling.  A block owns an 8 x 8 patch of POOL outputs of one image and 64 output channels.  The patch needs the 17 x 17 conv
// pixels (2 ph0 - 1 .. 2 ph0 + 15, likewise columns: one halo row and column, shared with the neighbouring patches and computed by
// both), which in turn read 39 x 39 input pixels.  289 conv pixels are 10 strips of 32 GEMM rows -- one wave each, 32 x 64
// accumulators -- so 320 rows are computed per 256 conv pixels a patch would need without the halo: 1.25 x.
//
// Operands.  The 39 x 39 input quads (16 bytes: one NHWC4 pixel) are fetched ONCE per block by LDS-DMA, out-of-image pixels as
// zeros through the buffer range check (the conv's zero padding).  There is no im2col image: the A fragment of GEMM row (cy, cx),
// tap (kh, kw) IS the quad at [2 cy + kh][2 cx + kw] of that patch, a per-lane base plus a compile-time tap offset.  A K step is
// 8 taps x 4 channels, taps ascending (conv_dma.hip's STEM order = the order of the [Cout][Kpad] weight pack), two K16 slices of
// v_mfma_f32_32x32x16_bf16 each: lane half lh of slice s feeds taps 8 kt + 4 s + 2 lh, + 1.  The weights come from
// pemp_pack_split3_bf16 (192 bytes per row and K step), one K step per stage buffer, double buffered; LDS image, swizzle and
// fragment reads are conv_dma2.hip's.  Every accumulator sees the slices in ascending K order and per slice the six products in
// the family's order (split3_mma6), so the result does not depend on tile, batch or grid.  Taps 49..55 are padding
// (zero weights); the activations fed for them are zeros, and the last slice (taps 52..55: nothing but padding) is not issued.
//
// Epilogue.  scale / shift / ReLU on the accumulators (conv_affine_quad's rule, conv_common.h, per scalar: lane = channel),
// the 17 x 17 x 64 fp32 conv patch goes to LDS over the operand buffers, and every thread takes the maximum of the IN-IMAGE
// conv pixels of one pool window for four channels (a pixel outside the conv's Ho x Wo is skipped by its coordinates, never read
// as a value) and stores one 16-byte quad: 16 lanes = the 256 contiguous bytes of a pooled pixel.
#include "conv_common.h"

namespace pemp {

typedef __attribute__((address_space(3))) void* lptr_t;

namespace {
constexpr int SP_PH = 8, SP_PW = 8;                                 // pool outputs of a block
constexpr int SP_CH = 2 * SP_PH + 1, SP_CW = 2 * SP_PW + 1;         // conv pixels it computes
constexpr int SP_IH = 2 * (SP_CH - 1) + 7, SP_IW = 2 * (SP_CW - 1) + 7;   // input pixels they read
constexpr int SP_ROWS = SP_CH * SP_CW;
constexpr int SP_NW = (SP_ROWS + 31) / 32;                          // one wave per strip of 32 GEMM rows
constexpr int SP_TAPS = 49, SP_NK = 7;
constexpr int SP_XQ = SP_IH * SP_IW;                                // input quads
constexpr int SP_XI = (SP_XQ + 63) / 64;                            // ... in DMA wave-instructions
constexpr int SP_BQ = 64 * 12;                                      // weight quads of one K step
constexpr int SP_LDS_OPS = (SP_XI * 64 + 2 * SP_BQ) * 16, SP_LDS_EPI = SP_ROWS * 64 * 4;
constexpr int SP_LDS = SP_LDS_OPS > SP_LDS_EPI ? SP_LDS_OPS : SP_LDS_EPI;
static_assert(SP_NW * 64 <= 1024 && SP_LDS <= 80 * 1024, "two blocks per CU");

__host__ __device__ constexpr int sp_tap_off(int tap) { return (tap / 7) * SP_IW + tap % 7; }   // in quads of the input patch
}  // namespace

__global__ __launch_bounds__(SP_NW * 64) void conv_stem_pool_kernel(ConvArgs a, int Hp, int Wp, int nph, int npw) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) v4f smem[];
    v4f* Xs = smem;                      // [SP_IH][SP_IW]
    v4f* Bs = smem + SP_XI * 64;         // [2][64][12]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;

    // block -> (image, patch, column group); neighbouring patches (shared input halo) sit on one XCD
    const int ntn = a.Cout / 64;
    int t = xcd_tile_order(blockIdx.x, gridDim.x);
    const int n0 = (t % ntn) * 64;
    t /= ntn;
    const int pxb = t % npw;
    t /= npw;
    const int pyb = t % nph, img = t / nph;
    const int ph0 = pyb * SP_PH, pw0 = pxb * SP_PW;
    const int cy0 = 2 * ph0 - 1, cx0 = 2 * pw0 - 1;        // first conv pixel of the patch (pool pad 1)
    const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;        // first input pixel (conv pad 3)

    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (size_t)img * a.H * a.W * 4), 0, 0x80000000u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x80000000u, 0x00020000);

    // input patch: quad q of the LDS image = input pixel (iy0 + q / SP_IW, ix0 + q % SP_IW); outside the image (and behind the
    // patch's last quad) the offset lies past the descriptor's range and the hardware writes zeros
    for (int i = wave; i < SP_XI; i += SP_NW) {
        const int q = i * 64 + lane;
        const int py = q / SP_IW, px = q - py * SP_IW;
        const int iy = iy0 + py, ix = ix0 + px;
        const bool ok = q < SP_XQ && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        const unsigned vo = ok ? (unsigned)(iy * a.W + ix) * 16u : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(Xs + i * 64), 16, vo, 0, 0, 0);
    }
    // weights of K step kt_: LDS quad q of the stage = row q / 12, position q % 12 = plane * 4 + (quad ^ ((row >> 2) & 3))
#define PEMP_SP_DMA_B(kt_, buf_)                                                                                  \
    for (int i = wave; i < SP_BQ / 64; i += SP_NW) {                                                              \
        const int q = i * 64 + lane, row = q / 12, pos = q - row * 12;                                            \
        const int src = PEMP_SPLIT3_SWZ(row, pos);                                                                \
        const unsigned vo = (unsigned)((n0 + row) * a.Kpad * 6 + src * 16);                                       \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Bs + (buf_) * SP_BQ + i * 64), 16, vo, (kt_) * 192, 0, 0); \
    }
    PEMP_SP_DMA_B(0, 0);

    // the lane's GEMM row: conv pixel (cy, cx) of the patch (rows behind the patch's last pixel compute pixel 0 and are dropped)
    const int m = wave * 32 + lr;
    const int mc = m < SP_ROWS ? m : 0;
    const int cy = mc / SP_CW, cx = mc - cy * SP_CW;
    const v4f* Ax = Xs + 2 * cy * SP_IW + 2 * cx;
    const v4f* Bw = Bs + lr * 12;
    const int bsw = (lr >> 2) & 3;
    const v4f zero4 = {0.f, 0.f, 0.f, 0.f};

    f32x16 acc[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;

#pragma unroll
    for (int kt = 0; kt < SP_NK; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's DMA pieces of step kt (and of the input patch) have landed
        __syncthreads();                                       // ... everybody's, and every read of the other stage is done
        if (kt + 1 < SP_NK) PEMP_SP_DMA_B(kt + 1, (kt + 1) & 1);
        const v4f* Bb = Bw + (kt & 1) * SP_BQ;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int tap0 = kt * 8 + s * 4;                   // this slice: taps tap0 .. tap0 + 3, two per lane half
            if (tap0 >= SP_TAPS) continue;
            const bool v00 = tap0 < SP_TAPS, v01 = tap0 + 1 < SP_TAPS, v10 = tap0 + 2 < SP_TAPS, v11 = tap0 + 3 < SP_TAPS;
            const int o00 = v00 ? sp_tap_off(tap0) : 0, o01 = v01 ? sp_tap_off(tap0 + 1) : 0;
            const int o10 = v10 ? sp_tap_off(tap0 + 2) : 0, o11 = v11 ? sp_tap_off(tap0 + 3) : 0;
            v4f x0 = Ax[lh ? o10 : o00], x1 = Ax[lh ? o11 : o01];
            if (!(lh ? v10 : v00)) x0 = zero4;
            if (!(lh ? v11 : v01)) x1 = zero4;
            bf16x8 ah, am, al;
            split3_bf16(x0, x1, ah, am, al);
            const int pb = (2 * s + lh) ^ bsw;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bf16x8 bh = __builtin_bit_cast(bf16x8, Bb[ni * 32 * 12 + pb]);
                const bf16x8 bm = __builtin_bit_cast(bf16x8, Bb[ni * 32 * 12 + 4 + pb]);
                const bf16x8 bl = __builtin_bit_cast(bf16x8, Bb[ni * 32 * 12 + 8 + pb]);
                split3_mma6(acc[ni], ah, am, al, bh, bm, bl);
            }
        }
    }
#undef PEMP_SP_DMA_B

    // ---- epilogue: affine + ReLU in registers (lane = channel), conv patch to LDS, 3x3 / 2 maximum, quad stores ----
    __syncthreads();                                           // the operand buffers are free
    float* Cs = (float*)smem;                                  // [SP_ROWS][64]
    const bool relu = a.flags & PEMP_CONV_RELU;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int n = n0 + ni * 32 + lr;
        const float sc = a.scale ? a.scale[n] : 1.f, sh = a.shift ? a.shift[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            float o = __builtin_fmaf(acc[ni][e], sc, sh);
            if (relu) o = fmaxf(o, 0.f);
            if (row < SP_ROWS) Cs[row * 64 + ni * 32 + lr] = o;
        }
    }
    __syncthreads();
    for (int i = tid; i < SP_PH * SP_PW * 16; i += SP_NW * 64) {
        const int c4 = i & 15, pp = i >> 4;
        const int py = pp / SP_PW, px = pp - py * SP_PW;
        const int ph = ph0 + py, pw = pw0 + px;
        if (ph >= Hp || pw >= Wp) continue;
        v4f mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ly = 2 * py + dy;
            if ((unsigned)(cy0 + ly) >= (unsigned)a.Ho) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int lx = 2 * px + dx;
                if ((unsigned)(cx0 + lx) >= (unsigned)a.Wo) continue;
                const v4f v = *(const v4f*)(Cs + (ly * SP_CW + lx) * 64 + c4 * 4);
                mx.x = fmaxf(mx.x, v.x);
                mx.y = fmaxf(mx.y, v.y);
                mx.z = fmaxf(mx.z, v.z);
                mx.w = fmaxf(mx.w, v.w);
            }
        }
        *(v4f*)(a.y + ((size_t)(img * Hp + ph) * Wp + pw) * a.ldy + n0 + c4 * 4) = mx;
    }
#endif
}

// output size of the 3 / 2 / 1 ceil-mode pool (ATen's rule: the last window starts inside the input or its left padding)
int conv_stem_pool_out(int i) {
    int o = (i + 2 - 3 + 1) / 2 + 1;
    if ((o - 1) * 2 >= i + 1) --o;
    return o;
}

int launch_conv_stem_pool(const ConvArgs& a, hipStream_t st) {
    if (!(a.flags & PEMP_CONV_STEM4) || a.KH != 7 || a.KW != 7 || a.stride != 2 || a.pad != 3 || a.dil != 1 || a.Kpad != SP_NK * 32) {
        set_error("conv2d: POOL3S2 needs the 7x7 / stride 2 / pad 3 NHWC4 stem (Kpad %d)", SP_NK * 32);
        return -1;
    }
    if (a.res || a.padv || a.stats || a.rowmask || (a.flags & (PEMP_CONV_SHIFT_PER_IMAGE | PEMP_CONV_BF16_IO))) {
        set_error("conv2d: POOL3S2 takes no residual, padding value, per-image shift or statistics");
        return -1;
    }
    const int Hp = conv_stem_pool_out(a.Ho), Wp = conv_stem_pool_out(a.Wo);
    const int nph = cdiv(Hp, SP_PH), npw = cdiv(Wp, SP_PW);
    const long long grid = (long long)a.N * nph * npw * (a.Cout / 64);
    if ((long long)a.H * a.W * 16 >= (1ll << 31) || (long long)a.Cout * a.Kpad * 6 >= (1ll << 31) || grid >= (1ll << 31) ||
        (long long)a.N * Hp * Wp * a.ldy >= (1ll << 31)) {
        set_error("conv2d: POOL3S2 operands outside 32-bit addressing");
        return -1;
    }
    static_assert(SP_LDS > 64 * 1024, "dynamic LDS attribute");
    hipError_t e = hipFuncSetAttribute((const void*)conv_stem_pool_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SP_LDS);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(lds=%d): %s", SP_LDS, hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(conv_stem_pool_kernel, dim3((unsigned)grid), dim3(SP_NW * 64), SP_LDS, st, a, Hp, Wp, nph, npw);
    return launch_status("conv_stem_pool");
}

}  // namespace pemp
