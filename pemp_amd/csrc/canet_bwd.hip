// CANet head training: the adjoints of the kernels of canet.hip and the backward of the 2-class classifier (reference:
// networks/canet.py:175-181,197-209 under autograd).  All fp32, NHWC with a leading dimension.  Every reduction is a two-stage
// partial sum of fixed shape and order (no atomics): two runs give the same bits.
#include "common.h"
#include "head_common.h"

namespace pemp {
namespace {

constexpr int CB_WAVES = 4;           // waves per block of the streaming kernels: one wave per pixel, float4 per lane (256 channels)
constexpr int CB_MAX_BLOCKS = 64;     // pixel blocks of a partial-sum pass (the second stage adds them in order)
constexpr int DZ_GROUPS = 16;         // row groups of the dz GEMV block
constexpr float SV_EPS = 1e-5f;

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void add4(float4& a, const float4& v) {
    a.x = __fadd_rn(a.x, v.x);
    a.y = __fadd_rn(a.y, v.y);
    a.z = __fadd_rn(a.z, v.z);
    a.w = __fadd_rn(a.w, v.w);
}
__device__ __forceinline__ void fma4(float4& a, float s, const float4& v) {
    a.x = __fmaf_rn(s, v.x, a.x);
    a.y = __fmaf_rn(s, v.y, a.y);
    a.z = __fmaf_rn(s, v.z, a.z);
    a.w = __fmaf_rn(s, v.w, a.w);
}

int blocks_of(int pixels) { return std::min(CB_MAX_BLOCKS, cdiv(pixels, CB_WAVES)); }

// out[i] = sum over k = 0..nparts-1, in that order, of part[k * len + i]  (one slab of nparts * len floats per blockIdx.y)
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, int nparts, int len, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const float* p = part + (size_t)blockIdx.y * nparts * len + i;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s = __fadd_rn(s, p[(size_t)k * len]);
    out[(size_t)blockIdx.y * len + i] = s;
}

// ---- (a) adjoint of canet_zterm -------------------------------------------------------------------------------------------
// part[b][blk][tap][c] = sum over the block's pixels whose tap (ky, kx) lands inside the image of g[b][y][x][c].  Tap (ky, kx)
// reads (y + (ky - 1) dil, x + (kx - 1) dil): row y serves ky = 0 when y >= dil, ky = 1 always, ky = 2 when y < h - dil (columns
// alike), so the nine sums are clipped-rectangle sums and an empty rectangle stays exactly 0.  grid (blocks, B, C / 256).
__global__ __launch_bounds__(64 * CB_WAVES) void tap_sums_kernel(const float* __restrict__ g, int ldg, float* __restrict__ part,
                                                                  int h, int w, int C, int dil, int nblk) {
    __shared__ float4 red[CB_WAVES][9][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int c = (blockIdx.z * 64 + lane) * 4, HW = h * w;
    const bool live = c < C;
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = zero4();
    for (int p = blockIdx.x * CB_WAVES + wave; p < HW; p += nblk * CB_WAVES) {
        const int y = p / w, x = p - y * w;
        const float4 v = live ? ld4(g + ((size_t)b * HW + p) * ldg + c) : zero4();
        const bool ry[3] = {y >= dil, true, y < h - dil}, rx[3] = {x >= dil, true, x < w - dil};
#pragma unroll
        for (int t = 0; t < 9; ++t)
            if (ry[t / 3] && rx[t % 3]) add4(acc[t], v);
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) red[wave][t][lane] = acc[t];
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            float4 s = red[0][t][lane];
            for (int k = 1; k < CB_WAVES; ++k) add4(s, red[k][t][lane]);
            *(float4*)(part + (((size_t)b * nblk + blockIdx.x) * 9 + t) * C + c) = s;
        }
    }
}

// dz[b][ci] = sum over rows r = co * 9 + tap of W[r * ldw + ci] * G[b][tap][co]: 64 ci lanes x DZ_GROUPS row groups per block
// (group k takes rows k, k + DZ_GROUPS, ...), the groups added in order.  grid (Cin / 64, B).
__global__ __launch_bounds__(64 * DZ_GROUPS) void zterm_dz_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ G,
                                                                   float* __restrict__ dz, int Cin, int Cout) {
    __shared__ float red[DZ_GROUPS][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, b = blockIdx.y;
    const int ci = blockIdx.x * 64 + lane, rows = 9 * Cout;
    float s = 0.f;
    if (ci < Cin)
        for (int r = grp; r < rows; r += DZ_GROUPS) {
            const int co = r / 9, tap = r - co * 9;
            s = __fmaf_rn(W[(size_t)r * ldw + ci], G[((size_t)b * 9 + tap) * Cout + co], s);
        }
    red[grp][lane] = s;
    __syncthreads();
    if (grp == 0 && ci < Cin) {
        float t = red[0][lane];
        for (int k = 1; k < DZ_GROUPS; ++k) t = __fadd_rn(t, red[k][lane]);
        dz[(size_t)b * Cin + ci] = t;
    }
}

// dW[(co * 9 + tap) * ldw + ci] = sum_b G[b][tap][co] z[b][ci], b in order: one thread per (row, 4 input channels).
__global__ __launch_bounds__(256) void zterm_dw_kernel(const float* __restrict__ G, const float* __restrict__ z, float* __restrict__ dW,
                                                       int ldw, int B, int Cin, int Cout) {
    const int cq = Cin / 4;
    const long long total = (long long)9 * Cout * cq;
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % cq), r = (int)(i / cq);
    const int co = r / 9, tap = r - co * 9;
    float4 acc = zero4();
    for (int b = 0; b < B; ++b) fma4(acc, G[((size_t)b * 9 + tap) * Cout + co], ld4(z + (size_t)b * Cin + q * 4));
    *(float4*)(dW + (size_t)r * ldw + q * 4) = acc;
}

// ---- (b) adjoint of canet_support_vector ----------------------------------------------------------------------------------
// df[n][p][c] = dz[b][c] * (m[n][p] / (S * (sum_p m[n][p] + 1e-5))), n = b * S + s, m = plane 0 of the mask sampled nearest to
// h x w as the forward samples it.  Every block re-adds its image's mask in the forward's order (64 strided lanes, then the 64
// partials in lane order): the denominator is the forward's, bit for bit.  grid (pixel blocks, B * S).
__global__ __launch_bounds__(64 * CB_WAVES) void support_vector_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ mask,
                                                                            float* __restrict__ df, int ldd, int S, int h, int w,
                                                                            int H, int W, int C) {
    __shared__ float pm[64];
    __shared__ float den_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, b = n / S, HW = h * w;
    const float* mp = mask + (size_t)n * 2 * H * W;
    if (wave == 0) {
        float sm = 0.f;
        for (int p = lane; p < HW; p += 64) {
            const int y = p / w, x = p - y * w;
            sm = __fadd_rn(sm, mp[(size_t)nearest_src(y, H, h) * W + nearest_src(x, W, w)]);
        }
        pm[lane] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tm = 0.f;
        for (int j = 0; j < 64; ++j) tm = __fadd_rn(tm, pm[j]);
        den_s = __fmul_rn((float)S, __fadd_rn(tm, SV_EPS));
    }
    __syncthreads();
    const float den = den_s;
    for (int p = blockIdx.x * CB_WAVES + wave; p < HW; p += gridDim.x * CB_WAVES) {
        const int y = p / w, x = p - y * w;
        const float coef = __fdiv_rn(mp[(size_t)nearest_src(y, H, h) * W + nearest_src(x, W, w)], den);
        float* dp = df + ((size_t)n * HW + p) * ldd;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 v = ld4(dz + (size_t)b * C + c);
            *(float4*)(dp + c) = make_float4(__fmul_rn(v.x, coef), __fmul_rn(v.y, coef), __fmul_rn(v.z, coef), __fmul_rn(v.w, coef));
        }
    }
}

// ---- (c) backward of the 2-class 1x1 classifier ---------------------------------------------------------------------------
// One pass over x [B][HW][C] and dpred [B][2][HW]: dx[b][p][:] = dpred[b][0][p] W[0][:] + dpred[b][1][p] W[1][:], and the block's
// share of dW[k][c] = sum dpred[b][k][p] x[b][p][c], db[k] = sum dpred[b][k][p] -> part[blk][2 * C + 2].  grid (blocks, C / 256).
__global__ __launch_bounds__(64 * CB_WAVES) void cls_bwd_kernel(const float* __restrict__ dpred, const float* __restrict__ x, int ldx,
                                                                 const float* __restrict__ Wt, float* __restrict__ dx, int lddx,
                                                                 float* __restrict__ part, int B, int HW, int C, int nblk) {
    __shared__ float4 red[CB_WAVES][2][64];
    __shared__ float redb[CB_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (blockIdx.y * 64 + lane) * 4;
    const bool live = c < C;
    const long long M = (long long)B * HW;
    const float4 w0 = live ? ld4(Wt + c) : zero4(), w1 = live ? ld4(Wt + C + c) : zero4();
    float4 a0 = zero4(), a1 = zero4();
    float b0 = 0.f, b1 = 0.f;
    for (long long m = blockIdx.x * CB_WAVES + wave; m < M; m += (long long)nblk * CB_WAVES) {
        const int b = (int)(m / HW), p = (int)(m - (long long)b * HW);
        const float d0 = dpred[((size_t)b * 2 + 0) * HW + p], d1 = dpred[((size_t)b * 2 + 1) * HW + p];
        b0 = __fadd_rn(b0, d0);
        b1 = __fadd_rn(b1, d1);
        if (live) {
            const float4 v = ld4(x + (size_t)m * ldx + c);
            fma4(a0, d0, v);
            fma4(a1, d1, v);
            float4 o = make_float4(__fmul_rn(d0, w0.x), __fmul_rn(d0, w0.y), __fmul_rn(d0, w0.z), __fmul_rn(d0, w0.w));
            fma4(o, d1, w1);
            *(float4*)(dx + (size_t)m * lddx + c) = o;
        }
    }
    red[wave][0][lane] = a0;
    red[wave][1][lane] = a1;
    if (lane == 0) {
        redb[wave][0] = b0;
        redb[wave][1] = b1;
    }
    __syncthreads();
    float* pr = part + (size_t)blockIdx.x * (2 * C + 2);
    if (wave == 0 && live) {
        for (int k = 0; k < 2; ++k) {
            float4 s = red[0][k][lane];
            for (int j = 1; j < CB_WAVES; ++j) add4(s, red[j][k][lane]);
            pr[k * C + c + 0] = s.x;          // (a slab starts 2 * C + 2 floats after the last: not 16-byte aligned)
            pr[k * C + c + 1] = s.y;
            pr[k * C + c + 2] = s.z;
            pr[k * C + c + 3] = s.w;
        }
    }
    if (threadIdx.x < 2 && blockIdx.y == 0) {
        float s = redb[0][threadIdx.x];
        for (int j = 1; j < CB_WAVES; ++j) s = __fadd_rn(s, redb[j][threadIdx.x]);
        pr[2 * C + threadIdx.x] = s;
    }
}

// dW [2][C] and db [2] from the summed slab [2 * C + 2]
__global__ __launch_bounds__(256) void cls_bwd_store_kernel(const float* __restrict__ sum, float* __restrict__ dW, float* __restrict__ db,
                                                            int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * C) dW[i] = sum[i];
    else if (i < 2 * C + 2) db[i - 2 * C] = sum[i];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" size_t pemp_canet_zterm_bwd_workspace_bytes(int B, int h, int w, int Cout) {
    if (B <= 0 || h <= 0 || w <= 0 || Cout <= 0) return 0;
    return (size_t)B * blocks_of(h * w) * 9 * Cout * sizeof(float);
}

extern "C" int pemp_canet_zterm_bwd_f32(const float* g, int ldg, const float* W, int ldw, const float* z, float* G, float* dz,
                                        float* dW, void* ws, size_t ws_bytes, int B, int h, int w, int Cin, int Cout, int dil,
                                        void* stream) {
    PEMP_REQUIRE(g && W && z && G && dz && dW && ws, "canet_zterm_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && h > 0 && w > 0 && Cin > 0 && Cout > 0 && dil > 0 && B <= 65535 && (long long)h * w < (1LL << 30),
                 "canet_zterm_bwd: bad sizes");
    PEMP_REQUIRE(Cin % 4 == 0 && Cout % 4 == 0 && Cout <= 256 * 65535 && ldg >= Cout && ldg % 4 == 0 && ldw >= Cin && ldw % 4 == 0 &&
                     aligned16(g) && aligned16(W) && aligned16(z) && aligned16(G) && aligned16(dW) && aligned16(ws),
                 "canet_zterm_bwd: Cin, Cout, ldg and ldw must be multiples of 4, ldg >= Cout, ldw >= Cin, operands 16-byte aligned");
    PEMP_REQUIRE(ws_bytes >= pemp_canet_zterm_bwd_workspace_bytes(B, h, w, Cout), "canet_zterm_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = blocks_of(h * w);
    hipLaunchKernelGGL(tap_sums_kernel, dim3(nblk, B, cdiv(Cout, 256)), dim3(64 * CB_WAVES), 0, st, g, ldg, (float*)ws, h, w, Cout, dil,
                       nblk);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(cdiv(9 * Cout, 256), B), dim3(256), 0, st, (const float*)ws, nblk, 9 * Cout, G);
    hipLaunchKernelGGL(zterm_dz_kernel, dim3(cdiv(Cin, 64), B), dim3(64 * DZ_GROUPS), 0, st, W, ldw, (const float*)G, dz, Cin, Cout);
    hipLaunchKernelGGL(zterm_dw_kernel, dim3((unsigned)(((long long)9 * Cout * (Cin / 4) + 255) / 256)), dim3(256), 0, st,
                       (const float*)G, z, dW, ldw, B, Cin, Cout);
    return launch_status("canet_zterm_bwd");
}

extern "C" int pemp_canet_support_vector_bwd_f32(const float* dz, const float* mask, float* df, int ldd, int B, int S, int h, int w,
                                                 int H, int W, int C, void* stream) {
    PEMP_REQUIRE(dz && mask && df, "canet_support_vector_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && (long long)B * S <= 65535 &&
                     (long long)h * w < (1LL << 30),
                 "canet_support_vector_bwd: bad sizes");
    PEMP_REQUIRE(C % 4 == 0 && ldd >= C && ldd % 4 == 0 && aligned16(dz) && aligned16(df),
                 "canet_support_vector_bwd: C and ldd must be multiples of 4, ldd >= C, dz / df 16-byte aligned");
    hipLaunchKernelGGL(support_vector_bwd_kernel, dim3(blocks_of(h * w), B * S), dim3(64 * CB_WAVES), 0, (hipStream_t)stream, dz, mask,
                       df, ldd, S, h, w, H, W, C);
    return launch_status("canet_support_vector_bwd");
}

extern "C" size_t pemp_canet_cls_bwd_workspace_bytes(int M, int C) {
    if (M <= 0 || C <= 0) return 0;
    return ((size_t)blocks_of(M) + 1) * (2 * (size_t)C + 2) * sizeof(float);
}

extern "C" int pemp_canet_cls_bwd_f32(const float* dpred, const float* x, int ldx, const float* W, float* dx, int lddx, float* dW,
                                      float* db, void* ws, size_t ws_bytes, int B, int HW, int C, void* stream) {
    PEMP_REQUIRE(dpred && x && W && dx && dW && db && ws, "canet_cls_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && HW > 0 && C > 0 && (long long)B * HW < (1LL << 30) && C <= 256 * 65535, "canet_cls_bwd: bad sizes");
    PEMP_REQUIRE(C % 4 == 0 && ldx >= C && ldx % 4 == 0 && lddx >= C && lddx % 4 == 0 && aligned16(x) && aligned16(W) && aligned16(dx),
                 "canet_cls_bwd: C, ldx and lddx must be multiples of 4 and >= C, x / W / dx 16-byte aligned");
    PEMP_REQUIRE(ws_bytes >= pemp_canet_cls_bwd_workspace_bytes(B * HW, C), "canet_cls_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = blocks_of(B * HW), len = 2 * C + 2;
    float* part = (float*)ws;
    float* sum = part + (size_t)nblk * len;
    hipLaunchKernelGGL(cls_bwd_kernel, dim3(nblk, cdiv(C, 256)), dim3(64 * CB_WAVES), 0, st, dpred, x, ldx, W, dx, lddx, part, B, HW, C,
                       nblk);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(cdiv(len, 256), 1), dim3(256), 0, st, (const float*)part, nblk, len, sum);
    hipLaunchKernelGGL(cls_bwd_store_kernel, dim3(cdiv(len, 256)), dim3(256), 0, st, (const float*)sum, dW, db, C);
    return launch_status("canet_cls_bwd");
}
