// What rpmms.hip (inference) and rpmms_bwd.hip (head training) share: the column layout of the three mixtures and the tap
// products / tap sums of layer55's prototype half.  The training forward must give the inference kernel's bits when every
// Dropout2d multiplier is 1, so both read T and add its taps through the code below.
#pragma once
#include "common.h"

namespace pemp {
namespace {

constexpr int RP_C = 256;                    // channels: one per thread of a block
constexpr int RP_J = 10;                     // columns of the three mixtures side by side: K = 1 | 3 | 6

__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 relu4(float4 a) { return make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)); }

// first column and width of mixture g
__device__ __forceinline__ int group_first(int g) { return g == 0 ? 0 : g == 1 ? 1 : 4; }
__device__ __forceinline__ int group_size(int g) { return g == 0 ? 1 : g == 1 ? 3 : 6; }

// T[b][i][tap][co] = sum_ci wz[tap][co][ci] mu[b][0][i][ci] for the ten foreground prototypes: one wave per (tap, co) row reads
// the row once, float4 per lane along ci, and meets the ten prototypes with it; the lane partials are summed by the fixed
// butterfly of wave_sum.  grid (rows / 4, B).
__global__ __launch_bounds__(256) void tap_gemv_kernel(const float* __restrict__ wz, const float* __restrict__ mu,
                                                       float* __restrict__ T, int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (row >= rows) return;                                  // whole waves leave together: no shuffle below is split
    const float4 a = ld4(wz + (size_t)row * RP_C + 4 * lane);
    const float* zb = mu + (size_t)b * 2 * RP_J * RP_C + 4 * lane;
#pragma unroll
    for (int i = 0; i < RP_J; ++i) {
        const float4 v = ld4(zb + i * RP_C);
        const float s = wave_sum(__fmaf_rn(a.w, v.w, __fmaf_rn(a.z, v.z, __fmaf_rn(a.y, v.y, __fmaf_rn(a.x, v.x, 0.f)))));
        if (lane == 0) T[((size_t)b * RP_J + i) * rows + row] = s;
    }
}

// The in-image taps of one prototype at a border pixel, in tap order (kept out of line: the ring is a small share of the pixels
// and its 90 loads must not cost the interior path its registers).
__device__ __noinline__ float4 border_taps(const float* __restrict__ Ti, int y, int x, int h, int w, int dil) {
    float4 R = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int tap = 0; tap < 9; ++tap) {
        const int sy = y + (tap / 3 - 1) * dil, sx = x + (tap % 3 - 1) * dil;
        if (sy < 0 || sy >= h || sx < 0 || sx >= w) continue;
        R = add4(R, ld4(Ti + (size_t)tap * RP_C));
    }
    return R;
}

// The sum of all nine taps of prototype i, in tap order: R_i of every interior pixel.
__device__ __forceinline__ float4 full_taps(const float* __restrict__ Ti) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) s = add4(s, ld4(Ti + (size_t)tap * RP_C));
    return s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace pemp
