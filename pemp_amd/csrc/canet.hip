// CANet inference kernels (reference: networks/canet.py, entry/canet.py): the support vector of the dense comparison
// (:175-178), the support half of the zero-padded dilated layer55 (:179-181), the input of the pre-activation residual blocks
// with the history channels (:103-104,193) and the softmax that becomes a later step's history (entry/canet.py:52,77-80).
// All fp32, fixed summation orders (no atomics): results are bit-stable run to run.
#include "common.h"
#include "head_common.h"

namespace pemp {
namespace {

constexpr int SV_Q = 16;        // support vector: float4 channel lanes per block (64 channels)
constexpr int SV_P = 64;        // ... and pixel lanes
constexpr float SV_EPS = 1e-5f;

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }

// z[b][c] = mean_s( sum_p f[bs][p][c] m[bs][p] / (sum_p m[bs][p] + 1e-5) ), m = plane 0 of the [B*S][2][H][W] support mask
// sampled nearest to h x w (canet.py:175-178).  Block = 16 float4 channel lanes x 64 pixel lanes; the 64 partial sums of a
// channel are added in lane order, the shots in order 0..S-1.
__global__ __launch_bounds__(SV_Q* SV_P) void support_vector_kernel(const float* __restrict__ f, int ldf, const float* __restrict__ mask,
                                                                    float* __restrict__ out, int S, int h, int w, int H, int W,
                                                                    int C) {
    __shared__ float4 pf[SV_P][SV_Q];
    __shared__ float pm[SV_P];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c = (blockIdx.x * SV_Q + tx) * 4, b = blockIdx.y, HW = h * w;
    const bool live = c < C;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int si = 0; si < S; ++si) {
        const int n = b * S + si;
        const float* mp = mask + (size_t)n * 2 * H * W;
        float4 sf = make_float4(0.f, 0.f, 0.f, 0.f);
        float sm = 0.f;
        for (int p = ty; p < HW; p += SV_P) {
            const int y = p / w, x = p - y * w;
            const float mv = mp[(size_t)nearest_src(y, H, h) * W + nearest_src(x, W, w)];
            sm = __fadd_rn(sm, mv);
            if (live) {
                const float4 v = ld4(f + ((size_t)n * HW + p) * ldf + c);
                sf.x = __fmaf_rn(v.x, mv, sf.x);
                sf.y = __fmaf_rn(v.y, mv, sf.y);
                sf.z = __fmaf_rn(v.z, mv, sf.z);
                sf.w = __fmaf_rn(v.w, mv, sf.w);
            }
        }
        pf[ty][tx] = sf;
        if (tx == 0) pm[ty] = sm;
        __syncthreads();
        if (ty == 0 && live) {
            float4 tf = make_float4(0.f, 0.f, 0.f, 0.f);
            float tm = 0.f;
            for (int j = 0; j < SV_P; ++j) {
                const float4 v = pf[j][tx];
                tf.x = __fadd_rn(tf.x, v.x);
                tf.y = __fadd_rn(tf.y, v.y);
                tf.z = __fadd_rn(tf.z, v.z);
                tf.w = __fadd_rn(tf.w, v.w);
                tm = __fadd_rn(tm, pm[j]);
            }
            const float den = __fadd_rn(tm, SV_EPS);
            const float4 g = make_float4(__fdiv_rn(tf.x, den), __fdiv_rn(tf.y, den), __fdiv_rn(tf.z, den), __fdiv_rn(tf.w, den));
            acc = si == 0 ? g : make_float4(__fadd_rn(acc.x, g.x), __fadd_rn(acc.y, g.y), __fadd_rn(acc.z, g.z), __fadd_rn(acc.w, g.w));
        }
        __syncthreads();
    }
    if (ty == 0 && live) {
        if (S > 1) {
            const float fs = (float)S;
            acc = make_float4(__fdiv_rn(acc.x, fs), __fdiv_rn(acc.y, fs), __fdiv_rn(acc.z, fs), __fdiv_rn(acc.w, fs));
        }
        *(float4*)(out + (size_t)b * C + c) = acc;
    }
}

// T[b][tap][co] = sum_ci wz[tap][co][ci] z[b][ci]: one wave per (tap, co) row, float4 per lane along ci, the lane partials
// summed by the fixed butterfly of wave_sum.
__global__ __launch_bounds__(256) void zterm_gemv_kernel(const float* __restrict__ wz, const float* __restrict__ z,
                                                         float* __restrict__ T, int rows, int Cin) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (row >= rows) return;                                  // whole waves leave together: no shuffle below is split
    const float* wr = wz + (size_t)row * Cin;
    const float* zb = z + (size_t)b * Cin;
    float s = 0.f;
    for (int k = lane * 4; k < Cin; k += 256) {
        const float4 a = ld4(wr + k), v = ld4(zb + k);
        s = __fmaf_rn(a.w, v.w, __fmaf_rn(a.z, v.z, __fmaf_rn(a.y, v.y, __fmaf_rn(a.x, v.x, s))));
    }
    s = wave_sum(s);
    if (lane == 0) T[(size_t)b * rows + row] = s;
}

// R[b][y][x][co] = sum over the taps (ky, kx) of a 3x3 conv of dilation dil whose source pixel lies inside the h x w image,
// in tap order 0..8, of T[b][tap][co] (the zero padding drops the others).  One thread per (pixel, 4 channels).
__global__ void zterm_spread_kernel(const float* __restrict__ T, float* __restrict__ R, int ldr, int B, int h, int w, int Cout,
                                    int dil) {
    const int cq = Cout / 4;
    const long long total = (long long)B * h * w * cq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % cq);
        long long t = i / cq;
        const int x = (int)(t % w);
        t /= w;
        const int y = (int)(t % h);
        const int b = (int)(t / h);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int sy = y + (tap / 3 - 1) * dil, sx = x + (tap % 3 - 1) * dil;
            if (sy < 0 || sy >= h || sx < 0 || sx >= w) continue;
            const float4 v = ld4(T + ((size_t)b * 9 + tap) * Cout + q * 4);
            acc.x = __fadd_rn(acc.x, v.x);
            acc.y = __fadd_rn(acc.y, v.y);
            acc.z = __fadd_rn(acc.z, v.z);
            acc.w = __fadd_rn(acc.w, v.w);
        }
        *(float4*)(R + (((size_t)b * h + y) * w + x) * ldr + q * 4) = acc;
    }
}

// y[b][p][0..C) = relu(x[b][p][:]); nhist == 2: also y[b][p][C], y[b][p][C + 1] = relu(hist[row][0..1][p]), row = b (hist is a
// [B][2][HW] tensor) or slot[b] (hist is a table of nslots such rows; a slot outside 0..nslots-1 means "no history": zeros,
// data_kits/pascal_voc.py:423-424); hist == NULL: zeros.
__global__ void block_input_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ hist, const int* __restrict__ slot,
                                   int nslots, float* __restrict__ y, int ldy, int B, int HW, int C, int nhist) {
    const int cq = C / 4;
    const long long total = (long long)B * HW * cq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % cq);
        const long long px = i / cq;
        const float4 v = ld4(x + px * ldx + q * 4);
        float* yp = y + px * ldy;
        *(float4*)(yp + q * 4) = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        if (nhist && q == 0) {
            const int b = (int)(px / HW), p = (int)(px - (long long)b * HW);
            const int row = slot ? slot[b] : b;
            float h0 = 0.f, h1 = 0.f;
            if (hist && row >= 0 && row < nslots) {
                const float* hp = hist + (size_t)row * 2 * HW + p;
                h0 = fmaxf(hp[0], 0.f);
                h1 = fmaxf(hp[HW], 0.f);
            }
            yp[C] = h0;
            yp[C + 1] = h1;
        }
    }
}

// F.softmax over the two channels of logits [B][2][HW] (max-subtracted, as ATen) -> row slot[b] of the table (0 <= slot[b] <
// nslots; other values: not written) and / or row b of a [B][2][HW] tensor.
__global__ void history_update_kernel(const float* __restrict__ logits, float* __restrict__ table, const int* __restrict__ slot,
                                      int nslots, float* __restrict__ out, int B, int HW) {
    const long long total = (long long)B * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
        const float* lp = logits + (size_t)b * 2 * HW + p;
        const float l0 = lp[0], l1 = lp[HW];
        const float m = fmaxf(l0, l1);
        const float e0 = expf(__fsub_rn(l0, m)), e1 = expf(__fsub_rn(l1, m));
        const float den = __fadd_rn(e0, e1);
        const float p0 = __fdiv_rn(e0, den), p1 = __fdiv_rn(e1, den);
        const int row = table ? slot[b] : -1;
        if (row >= 0 && row < nslots) {
            float* tp = table + (size_t)row * 2 * HW + p;
            tp[0] = p0;
            tp[HW] = p1;
        }
        if (out) {
            float* op = out + (size_t)b * 2 * HW + p;
            op[0] = p0;
            op[HW] = p1;
        }
    }
}

int grid_of(long long total) { return (int)std::min<long long>((total + 255) / 256, 8192); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" int pemp_canet_support_vector_f32(const float* feat, int ldf, const float* mask, float* out, int B, int S, int h, int w,
                                             int H, int W, int C, void* stream) {
    PEMP_REQUIRE(feat && mask && out, "canet_support_vector: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && B <= 65535, "canet_support_vector: bad sizes");
    PEMP_REQUIRE(C % 4 == 0 && ldf >= C && ldf % 4 == 0 && aligned16(feat) && aligned16(out),
                 "canet_support_vector: C and ldf must be multiples of 4, ldf >= C, feat / out 16-byte aligned");
    hipLaunchKernelGGL(support_vector_kernel, dim3(cdiv(C, 4 * SV_Q), B), dim3(SV_Q, SV_P), 0, (hipStream_t)stream, feat, ldf, mask,
                       out, S, h, w, H, W, C);
    return launch_status("canet_support_vector");
}

extern "C" int pemp_canet_zterm_f32(const float* wz, const float* z, float* T, float* R, int ldr, int B, int h, int w, int Cin,
                                    int Cout, int dil, void* stream) {
    PEMP_REQUIRE(wz && z && T && R, "canet_zterm: null pointer");
    PEMP_REQUIRE(B > 0 && h > 0 && w > 0 && Cin > 0 && Cout > 0 && dil > 0 && B <= 65535, "canet_zterm: bad sizes");
    PEMP_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && ldr >= Cout && ldr % 4 == 0 && aligned16(wz) && aligned16(z) && aligned16(T) &&
                     aligned16(R),
                 "canet_zterm: Cin, Cout and ldr must be multiples of 4, ldr >= Cout, operands 16-byte aligned");
    const int rows = 9 * Cout;
    hipLaunchKernelGGL(zterm_gemv_kernel, dim3(cdiv(rows, 4), B), dim3(256), 0, (hipStream_t)stream, wz, z, T, rows, Cin);
    hipLaunchKernelGGL(zterm_spread_kernel, dim3(grid_of((long long)B * h * w * (Cout / 4))), dim3(256), 0, (hipStream_t)stream, T, R,
                       ldr, B, h, w, Cout, dil);
    return launch_status("canet_zterm");
}

extern "C" int pemp_canet_block_input_f32(const float* x, int ldx, const float* hist, const int* slot, int nslots, float* y, int ldy,
                                          int B, int HW, int C, int nhist, void* stream) {
    PEMP_REQUIRE(x && y, "canet_block_input: null pointer");
    PEMP_REQUIRE((nhist == 0 && !hist && !slot) || (nhist == 2 && (hist || !slot)), "canet_block_input: nhist is 0 (no history "
                 "source) or 2; slots need a table");
    PEMP_REQUIRE(B > 0 && HW > 0 && C > 0 && nslots >= 0 && (!hist || nslots >= (slot ? 1 : B)), "canet_block_input: bad sizes");
    PEMP_REQUIRE(C % 4 == 0 && ldx >= C && ldx % 4 == 0 && ldy >= C + nhist && ldy % 4 == 0 && aligned16(x) && aligned16(y),
                 "canet_block_input: C, ldx and ldy must be multiples of 4, ldx >= C, ldy >= C + nhist, x / y 16-byte aligned");
    hipLaunchKernelGGL(block_input_kernel, dim3(grid_of((long long)B * HW * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, ldx, hist,
                       slot, nslots, y, ldy, B, HW, C, nhist);
    return launch_status("canet_block_input");
}

extern "C" int pemp_canet_history_update_f32(const float* logits, float* table, const int* slot, int nslots, float* out, int B,
                                             int HW, void* stream) {
    PEMP_REQUIRE(logits && (table || out), "canet_history_update: null pointer");
    PEMP_REQUIRE(!table == !slot && (!table || nslots > 0), "canet_history_update: a history table, its slots and its row count "
                 "come together");
    PEMP_REQUIRE(B > 0 && HW > 0, "canet_history_update: bad sizes");
    hipLaunchKernelGGL(history_update_kernel, dim3(grid_of((long long)B * HW)), dim3(256), 0, (hipStream_t)stream, logits, table, slot,
                       nslots, out, B, HW);
    return launch_status("canet_history_update");
}
