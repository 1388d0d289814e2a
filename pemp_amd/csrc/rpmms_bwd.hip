// RPMMs head training (reference: networks/rpmms.py:237-251 under autograd): layer55 over the ten prototype columns with one
// Dropout2d draw per column, its adjoint, and the adjoint of the softmax that hands a pass's prediction to the next pass as
// history.  Only the query carries a gradient (the prototypes are constants of the step, rpmms.py:73,126).  All fp32, NHWC with
// a leading dimension, C = 256.  No atomics: every cross-block sum is a two-stage partial sum of fixed shape and order through
// a workspace of the caller, so two runs give the same bits.
#include "rpmms_common.h"

namespace pemp {
namespace {

constexpr int PS_PIX = 16;            // pixels per block of the per-pixel kernels (64 channel lanes x 4 pixel lanes), as rpmms.hip
constexpr int PB_WAVES = 4;           // waves per block of the tap-sum kernel: one wave per pixel, float4 per lane
constexpr int PB_MAX_BLOCKS = 16;     // pixel blocks per (image, column) of the tap-sum kernel (the second stage adds them in order)

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
    return make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w));
}
// m where pre > 0, else 0, times d: a column's share of the gradient at its pre-activation
__device__ __forceinline__ float4 gate4(float4 pre, float4 m, float4 d) {
    return make_float4(pre.x > 0.f ? __fmul_rn(m.x, d.x) : 0.f, pre.y > 0.f ? __fmul_rn(m.y, d.y) : 0.f,
                       pre.z > 0.f ? __fmul_rn(m.z, d.z) : 0.f, pre.w > 0.f ? __fmul_rn(m.w, d.w) : 0.f);
}
__device__ __forceinline__ void fma4(float4& a, float s, const float4& v) {
    a.x = __fmaf_rn(s, v.x, a.x);
    a.y = __fmaf_rn(s, v.y, a.y);
    a.z = __fmaf_rn(s, v.z, a.z);
    a.w = __fmaf_rn(s, v.w, a.w);
}
__device__ __forceinline__ bool interior_px(int y, int x, int h, int w, int dil) {
    return y >= dil && y + dil < h && x >= dil && x + dil < w;
}

int tap_blocks(int HW) { return std::min(PB_MAX_BLOCKS, cdiv(HW, PB_WAVES)); }

// ---- forward ---------------------------------------------------------------------------------------------------------------
// proto_sum_kernel of rpmms.hip with a multiplier per (image, column, channel) on each column's ReLU output:
// out_g[b][p][c] = sum_{i in mixture g, ascending} m[b][i][c] * relu(base[b][p][c] + bias[c] + R_i[p][c]).  The same tap order and
// the same sum: with every m = 1 the products are exact and the result is that kernel's, bit for bit.  Nothing is kept per
// column: the backward recomputes.  grid (chunks of 16 pixels, B).
__global__ __launch_bounds__(256) void proto_sum_train_kernel(const float* __restrict__ base, int ldb, const float* __restrict__ bias,
                                                              const float* __restrict__ T, const float* __restrict__ mult,
                                                              float* __restrict__ out, int ldo, long long gstride, int h, int w,
                                                              int dil) {
    const int c = 4 * (threadIdx.x & 63), ty = threadIdx.x >> 6, b = blockIdx.y, HW = h * w;
    const float* Tb = T + (size_t)b * RP_J * 9 * RP_C + c;
    const float* mb = mult + (size_t)b * RP_J * RP_C + c;
    float4 full[RP_J];
#pragma unroll
    for (int i = 0; i < RP_J; ++i) full[i] = full_taps(Tb + (size_t)i * 9 * RP_C);
    const float4 bv = ld4(bias + c);
    const int p_end = min((blockIdx.x + 1) * PS_PIX, HW);
    for (int p = blockIdx.x * PS_PIX + ty; p < p_end; p += 4) {
        const int y = p / w, x = p - y * w;
        const bool interior = interior_px(y, x, h, w, dil);
        const size_t px = (size_t)b * HW + p;
        const float4 bb = add4(ld4(base + px * ldb + c), bv);
        float4 g0, g1, g2;
#pragma unroll
        for (int i = 0; i < RP_J; ++i) {
            float4 R = full[i];
            if (!interior) R = border_taps(Tb + (size_t)i * 9 * RP_C, y, x, h, w, dil);
            const float4 v = mul4(ld4(mb + i * RP_C), relu4(add4(bb, R)));
            if (i == 0) g0 = v;
            else if (i == 1) g1 = v;
            else if (i < 4) g1 = add4(g1, v);
            else if (i == 4) g2 = v;
            else g2 = add4(g2, v);
        }
        float* op = out + px * ldo + c;
        *(float4*)op = g0;
        *(float4*)(op + gstride) = g1;
        *(float4*)(op + 2 * gstride) = g2;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// dbase[b][p][c] = sum_g sum_{i in g} m_i 1[pre_i > 0] dout_g[b][p][c], columns ascending, pre_i recomputed exactly as the forward
// computes it.  One pass, a thread writes what it sums.  grid (chunks of 16 pixels, B).
__global__ __launch_bounds__(256) void proto_dbase_kernel(const float* __restrict__ dout, int ldd, long long gstride,
                                                          const float* __restrict__ base, int ldb, const float* __restrict__ bias,
                                                          const float* __restrict__ T, const float* __restrict__ mult,
                                                          float* __restrict__ dbase, int lddb, int h, int w, int dil) {
    const int c = 4 * (threadIdx.x & 63), ty = threadIdx.x >> 6, b = blockIdx.y, HW = h * w;
    const float* Tb = T + (size_t)b * RP_J * 9 * RP_C + c;
    const float* mb = mult + (size_t)b * RP_J * RP_C + c;
    float4 full[RP_J];
#pragma unroll
    for (int i = 0; i < RP_J; ++i) full[i] = full_taps(Tb + (size_t)i * 9 * RP_C);
    const float4 bv = ld4(bias + c);
    const int p_end = min((blockIdx.x + 1) * PS_PIX, HW);
    for (int p = blockIdx.x * PS_PIX + ty; p < p_end; p += 4) {
        const int y = p / w, x = p - y * w;
        const bool interior = interior_px(y, x, h, w, dil);
        const size_t px = (size_t)b * HW + p;
        const float4 bb = add4(ld4(base + px * ldb + c), bv);
        const float* dp = dout + px * ldd + c;
        const float4 d0 = ld4(dp), d1 = ld4(dp + gstride), d2 = ld4(dp + 2 * gstride);
        float4 s = zero4();
#pragma unroll
        for (int i = 0; i < RP_J; ++i) {
            float4 R = full[i];
            if (!interior) R = border_taps(Tb + (size_t)i * 9 * RP_C, y, x, h, w, dil);
            s = add4(s, gate4(add4(bb, R), ld4(mb + i * RP_C), i == 0 ? d0 : i < 4 ? d1 : d2));
        }
        *(float4*)(dbase + px * lddb + c) = s;
    }
}

// part[b][i][blk][tap][c] = sum over the block's pixels whose tap (ky, kx) lands inside the image of column i's gated gradient
// m_i 1[pre_i > 0] dout_g(i) -- never stored per pixel.  Row y serves ky = 0 when y >= dil, ky = 1 always, ky = 2 when y < h - dil
// (columns alike): nine clipped-rectangle sums, an empty rectangle stays exactly 0.  A thread whose four multipliers are all
// zero (its channels dropped in this column) skips the pixels.  grid (blocks, B, 10 columns).
__global__ __launch_bounds__(64 * PB_WAVES) void proto_tap_sums_kernel(const float* __restrict__ dout, int ldd, long long gstride,
                                                                        const float* __restrict__ base, int ldb,
                                                                        const float* __restrict__ bias, const float* __restrict__ T,
                                                                        const float* __restrict__ mult, float* __restrict__ part,
                                                                        int h, int w, int dil, int nblk) {
    __shared__ float4 red[PB_WAVES][9][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, i = blockIdx.z;
    const int c = 4 * lane, HW = h * w;
    const float* Ti = T + ((size_t)b * RP_J + i) * 9 * RP_C + c;
    const float4 mv = ld4(mult + ((size_t)b * RP_J + i) * RP_C + c);
    const float4 full = full_taps(Ti), bv = ld4(bias + c);
    const float* dg = dout + (i == 0 ? 0 : i < 4 ? 1 : 2) * gstride + c;
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = zero4();
    if (mv.x != 0.f || mv.y != 0.f || mv.z != 0.f || mv.w != 0.f) {
        for (int p = blockIdx.x * PB_WAVES + wave; p < HW; p += nblk * PB_WAVES) {
            const int y = p / w, x = p - y * w;
            const size_t px = (size_t)b * HW + p;
            float4 R = full;
            if (!interior_px(y, x, h, w, dil)) R = border_taps(Ti, y, x, h, w, dil);
            const float4 v = gate4(add4(add4(ld4(base + px * ldb + c), bv), R), mv, ld4(dg + px * ldd));
            const bool ry[3] = {y >= dil, true, y < h - dil}, rx[3] = {x >= dil, true, x < w - dil};
#pragma unroll
            for (int t = 0; t < 9; ++t)
                if (ry[t / 3] && rx[t % 3]) acc[t] = add4(acc[t], v);
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave == 0) {
        float* pb = part + (((size_t)b * RP_J + i) * nblk + blockIdx.x) * 9 * RP_C + c;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            float4 s = red[0][t][lane];
            for (int k = 1; k < PB_WAVES; ++k) s = add4(s, red[k][t][lane]);
            *(float4*)(pb + (size_t)t * RP_C) = s;
        }
    }
}

// G[slab][j] = sum over k = 0..nparts-1, in that order, of part[slab][k][j]  (slab = (image, column), j over [9][256])
__global__ __launch_bounds__(256) void proto_sum_partials_kernel(const float* __restrict__ part, int nparts, int len, float* __restrict__ G) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    const float* p = part + (size_t)blockIdx.y * nparts * len + j;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s = __fadd_rn(s, p[(size_t)k * len]);
    G[(size_t)blockIdx.y * len + j] = s;
}

// The prototype half of layer55's weight gradient, straight into its column slice of the KRSC gradient:
// dW[(co * 9 + tap) * ldw + ci] = sum_b sum_i G[b][i][tap][co] mu[b][0][i][ci], b then i ascending: one thread per (row, 4 input
// channels) -- canet_bwd.hip's zterm_dw_kernel with ten columns per image instead of one.
__global__ __launch_bounds__(256) void proto_dw_kernel(const float* __restrict__ G, const float* __restrict__ mu, float* __restrict__ dW,
                                                       int ldw, int B) {
    const int cq = RP_C / 4;
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= 9 * RP_C * cq) return;
    const int q = i0 % cq, r = i0 / cq;
    const int co = r / 9, tap = r - co * 9;
    float4 acc = zero4();
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < RP_J; ++i)
            fma4(acc, G[(((size_t)b * RP_J + i) * 9 + tap) * RP_C + co], ld4(mu + ((size_t)b * 2 * RP_J + i) * RP_C + q * 4));
    *(float4*)(dW + (size_t)r * ldw + q * 4) = acc;
}

// layer55's bias gradient = the sum of dbase over images and pixels.  The centre tap is inside the image at every pixel, so
// G[b][i][4][c] already is column i's sum over the pixels: db[c] = sum_b sum_i G[b][i][4][c], b then i ascending.  One block.
__global__ __launch_bounds__(RP_C) void proto_dbias_kernel(const float* __restrict__ G, float* __restrict__ db, int B) {
    float s = 0.f;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < RP_J; ++i) s = __fadd_rn(s, G[(((size_t)b * RP_J + i) * 9 + 4) * RP_C + threadIdx.x]);
    db[threadIdx.x] = s;
}

// Adjoint of the two-class softmax that made the history: dpred[b][k][p] += prob_k (dh_k - sum_j prob_j dh_j), dh NHWC with two
// channels (ldh), prob / dpred [B][2][HW].  One thread per pixel.
__global__ __launch_bounds__(256) void history_bwd_kernel(const float* __restrict__ dh, int ldh, const float* __restrict__ prob,
                                                          float* __restrict__ dpred, int B, int HW) {
    const long long m = blockIdx.x * 256LL + threadIdx.x;
    if (m >= (long long)B * HW) return;
    const int b = (int)(m / HW), p = (int)(m - (long long)b * HW);
    const float d0 = dh[(size_t)m * ldh], d1 = dh[(size_t)m * ldh + 1];
    const size_t o = ((size_t)b * 2) * HW + p;
    const float p0 = prob[o], p1 = prob[o + HW];
    const float s = __fmaf_rn(p1, d1, __fmul_rn(p0, d0));
    dpred[o] = __fmaf_rn(p0, __fsub_rn(d0, s), dpred[o]);
    dpred[o + HW] = __fmaf_rn(p1, __fsub_rn(d1, s), dpred[o + HW]);
}

}  // namespace
}  // namespace pemp

using namespace pemp;

#define RPB_SIZES(who)                                                                                                       \
    PEMP_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && (long long)h * w < (1 << 24) && dil > 0, who ": bad sizes");      \
    PEMP_REQUIRE(C == RP_C, who ": the kernels are built for C = 256")

extern "C" int pemp_rpmms_proto_sum_train_f32(const float* wz, const float* mu, const float* base, int ldb, const float* bias,
                                              const float* mult, float* T, float* out, int ldo, long long gstride, int B, int h,
                                              int w, int C, int dil, void* stream) {
    PEMP_REQUIRE(wz && mu && base && bias && mult && T && out, "rpmms_proto_sum_train: null pointer");
    RPB_SIZES("rpmms_proto_sum_train");
    PEMP_REQUIRE(ldb >= C && ldb % 4 == 0 && ldo >= C && ldo % 4 == 0 && gstride >= 0 && gstride % 4 == 0 && aligned16(wz) &&
                     aligned16(mu) && aligned16(base) && aligned16(bias) && aligned16(mult) && aligned16(T) && aligned16(out),
                 "rpmms_proto_sum_train: ldb, ldo and gstride must be multiples of 4, ldb / ldo >= C, operands 16-byte aligned");
    const int rows = 9 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tap_gemv_kernel, dim3(cdiv(rows, 4), B), dim3(256), 0, st, wz, mu, T, rows);
    hipLaunchKernelGGL(proto_sum_train_kernel, dim3(cdiv(h * w, PS_PIX), B), dim3(256), 0, st, base, ldb, bias, (const float*)T, mult,
                       out, ldo, gstride, h, w, dil);
    return launch_status("rpmms_proto_sum_train");
}

extern "C" size_t pemp_rpmms_proto_sum_bwd_work_floats(int B, int h, int w, int C) {
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0) return 0;
    return (size_t)B * RP_J * tap_blocks(h * w) * 9 * C;
}

extern "C" int pemp_rpmms_proto_sum_bwd_f32(const float* dout, int ldd, long long gstride, const float* base, int ldb,
                                            const float* bias, const float* T, const float* mult, const float* mu, float* dbase,
                                            int lddb, float* G, float* dW, int ldw, float* dbias, float* work, size_t work_floats,
                                            int B, int h, int w, int C, int dil, void* stream) {
    PEMP_REQUIRE(dout && base && bias && T && mult && dbase && G && work, "rpmms_proto_sum_bwd: null pointer");
    PEMP_REQUIRE(!dW || mu, "rpmms_proto_sum_bwd: the weight gradient needs mu");
    RPB_SIZES("rpmms_proto_sum_bwd");
    PEMP_REQUIRE(ldd >= C && ldd % 4 == 0 && gstride >= 0 && gstride % 4 == 0 && ldb >= C && ldb % 4 == 0 && lddb >= C && lddb % 4 == 0 &&
                     aligned16(dout) && aligned16(base) && aligned16(bias) && aligned16(T) && aligned16(mult) && aligned16(dbase) &&
                     aligned16(G) && aligned16(work),
                 "rpmms_proto_sum_bwd: ldd, gstride, ldb and lddb must be multiples of 4, ldd / ldb / lddb >= C, operands 16-byte aligned");
    PEMP_REQUIRE(!dW || (ldw >= C && ldw % 4 == 0 && aligned16(dW) && aligned16(mu)),
                 "rpmms_proto_sum_bwd: ldw must be a multiple of 4 and >= C, dW / mu 16-byte aligned");
    PEMP_REQUIRE(work_floats >= pemp_rpmms_proto_sum_bwd_work_floats(B, h, w, C), "rpmms_proto_sum_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int HW = h * w, nblk = tap_blocks(HW), len = 9 * C;
    hipLaunchKernelGGL(proto_dbase_kernel, dim3(cdiv(HW, PS_PIX), B), dim3(256), 0, st, dout, ldd, gstride, base, ldb, bias, T, mult,
                       dbase, lddb, h, w, dil);
    hipLaunchKernelGGL(proto_tap_sums_kernel, dim3(nblk, B, RP_J), dim3(64 * PB_WAVES), 0, st, dout, ldd, gstride, base, ldb, bias, T,
                       mult, work, h, w, dil, nblk);
    hipLaunchKernelGGL(proto_sum_partials_kernel, dim3(cdiv(len, 256), B * RP_J), dim3(256), 0, st, (const float*)work, nblk, len, G);
    if (dW)
        hipLaunchKernelGGL(proto_dw_kernel, dim3(cdiv(9 * C * (C / 4), 256)), dim3(256), 0, st, (const float*)G, mu, dW, ldw, B);
    if (dbias) hipLaunchKernelGGL(proto_dbias_kernel, dim3(1), dim3(RP_C), 0, st, (const float*)G, dbias, B);
    return launch_status("rpmms_proto_sum_bwd");
}

extern "C" int pemp_rpmms_history_bwd_f32(const float* dh, int ldh, const float* prob, float* dpred, int B, int HW, void* stream) {
    PEMP_REQUIRE(dh && prob && dpred, "rpmms_history_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && HW > 0 && (long long)B * HW < (1LL << 30) && ldh >= 2, "rpmms_history_bwd: bad sizes");
    hipLaunchKernelGGL(history_bwd_kernel, dim3((unsigned)(((long long)B * HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dh, ldh,
                       prob, dpred, B, HW);
    return launch_status("rpmms_history_bwd");
}
