// PFENet head training: the adjoints of the streaming kernels of pfenet.hip (reference: networks/pfenet.py:15-20,229-268 under
// autograd).  All fp32.  One wave per pixel of the tensor that is written, float4 per lane over the channels; every output
// element is written exactly once by one thread that gathers its terms in a fixed order, every reduction is a two-stage
// partial sum of fixed shape (no atomics): two runs give the same bits.
#include "common.h"
#include "head_common.h"

namespace pemp {
namespace {

constexpr int PB_WAVES = 4;           // waves per block: one wave per pixel
constexpr int PB_MAX_BLOCKS = 64;     // pixel blocks of a partial-sum pass (the second stage adds them in order)
constexpr int PB_MAX_BINS = 4;        // pyramid bins served by one launch
constexpr int DS_GROUPS = 16;         // row groups of the dsvec GEMV block

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

struct BinArgs {                      // the pyramid bins of one launch: g_k NHWC [B][h_k][w_k][.] with pixel stride ld_k
    const float* g[PB_MAX_BINS];
    int ld[PB_MAX_BINS], h[PB_MAX_BINS], w[PB_MAX_BINS];
    int n;
};
struct MergeArgs {                    // support columns of the init_merge weights and of their gradients (row stride ldw)
    const float* W[PB_MAX_BINS];
    float* dW[PB_MAX_BINS];
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
long long grid_pixels(long long pixels) { return (pixels + PB_WAVES - 1) / PB_WAVES; }

// ---- (a) adjoint of weighted_gap ----------------------------------------------------------------------------------------
// df[n][p][c] = dvec[b][c] * (m[n][p] / area[n] / S), n = b * S + s, area = fl(fl(fl(sum m / HW) * h) * w) + 0.0005 with the
// mask re-added in the forward's order (16 strided lanes, then the 16 partials in lane order): the forward's denominator, bit
// for bit.  An all-zero mask gives coef = 0 / 0.0005 = 0: exact zeros.  grid (pixel blocks, B * S).
__global__ __launch_bounds__(64 * PB_WAVES) void weighted_gap_bwd_kernel(const float* __restrict__ dvec, const float* __restrict__ mask,
                                                                          float* __restrict__ df, int ldd, int S, int h, int w, int C) {
    __shared__ float pm[16];
    __shared__ float area_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y, b = n / S, HW = h * w;
    const float* mp = mask + (size_t)n * HW;
    if (threadIdx.x < 16) {
        float sm = 0.f;
        for (int p = threadIdx.x; p < HW; p += 16) sm = __fadd_rn(sm, mp[p]);
        pm[threadIdx.x] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tm = 0.f;
        for (int j = 0; j < 16; ++j) tm = __fadd_rn(tm, pm[j]);
        area_s = __fadd_rn(__fmul_rn(__fmul_rn(__fdiv_rn(tm, (float)HW), (float)h), (float)w), 0.0005f);
    }
    __syncthreads();
    const float area = area_s;
    for (int p = blockIdx.x * PB_WAVES + wave; p < HW; p += gridDim.x * PB_WAVES) {
        float coef = __fdiv_rn(mp[p], area);
        if (S > 1) coef = __fdiv_rn(coef, (float)S);
        float* dp = df + ((size_t)n * HW + p) * ldd;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 v = ld4(dvec + (size_t)b * C + c);
            *(float4*)(dp + c) = make_float4(__fmul_rn(v.x, coef), __fmul_rn(v.y, coef), __fmul_rn(v.z, coef), __fmul_rn(v.w, coef));
        }
    }
}

// ---- (b) adjoint of adaptive_avgpool, up to four bins summed -----------------------------------------------------------
// dx[n][y][x][c] = sum over the bins in index order, within a bin over the windows that contain (y, x) in row-major order, of
// g_k[n][oy][ox][c] / kh / kw.  Window oy covers rows [floor(oy H / Ho), ceil((oy + 1) H / Ho)) (the forward's rule), so the
// windows over row y are oy = floor(y Ho / H) .. floor(((y + 1) Ho - 1) / H).  One wave per input pixel; written once.
__global__ __launch_bounds__(64 * PB_WAVES) void avgpool_bwd_multi_kernel(BinArgs a, float* __restrict__ dx, int lddx, long long npix,
                                                                           int H, int W, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long i = (long long)blockIdx.x * PB_WAVES + wave; i < npix; i += (long long)gridDim.x * PB_WAVES) {
        const int x = (int)(i % W);
        const long long t = i / W;
        const int y = (int)(t % H), n = (int)(t / H);
        for (int c = lane * 4; c < C; c += 256) {
            float4 acc = zero4();
            for (int k = 0; k < a.n; ++k) {
                const int Ho = a.h[k], Wo = a.w[k];
                const int oy0 = (y * Ho) / H, oy1 = ((y + 1) * Ho - 1) / H;
                const int ox0 = (x * Wo) / W, ox1 = ((x + 1) * Wo - 1) / W;
                for (int oy = oy0; oy <= oy1; ++oy) {
                    const float kh = (float)(((oy + 1) * H + Ho - 1) / Ho - (oy * H) / Ho);
                    for (int ox = ox0; ox <= ox1; ++ox) {
                        const float kw = (float)(((ox + 1) * W + Wo - 1) / Wo - (ox * W) / Wo);
                        const float4 v = ld4(a.g[k] + (((size_t)n * Ho + oy) * Wo + ox) * a.ld[k] + c);
                        add4(acc, make_float4(__fdiv_rn(__fdiv_rn(v.x, kh), kw), __fdiv_rn(__fdiv_rn(v.y, kh), kw),
                                              __fdiv_rn(__fdiv_rn(v.z, kh), kw), __fdiv_rn(__fdiv_rn(v.w, kh), kw)));
                    }
                }
            }
            *(float4*)(dx + (size_t)i * lddx + c) = acc;
        }
    }
}

// ---- (c) adjoint of resize_ac -------------------------------------------------------------------------------------------
// dx[n][y][x][c] = add[n][y][x][c] + sum over the output pixels (Y, X), row-major, whose stencil touches (y, x) of
// wy(Y, y) wx(X, x) dy[n][Y][X][c]; hi x wi is the size of dx (the forward's input), ho x wo of dy.  Output row Y reads rows
// i0 = min(int(s Y), hi - 1) and i1 with weights 1 - l and l (head_common.h bilin, the forward's): it touches y iff
// y - 1 < s Y < y + 1, so the scan runs over [(y - 1) / s, (y + 1) / s] widened by one row for the float rounding of s Y and
// tests every row with bilin itself.  That holds for s > 1 (down-sampling: at most a few rows) as for s < 1; s == 0 (a
// one-row side) scans everything.  Element (n, pixel, c) of a tensor lives at n * tn + pixel * ld + c * tc.
// V = 4: unit channel strides, float4 per lane; V = 1: any strides, one channel per lane.  `add` may alias dx (read, then
// written, by the same thread).
struct Wgt {
    int lo, hi;
};
__device__ __forceinline__ Wgt scan_range(int y, int in, int out) {
    const float s = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    Wgt r;
    if (s > 0.f) {
        r.lo = max(0, (int)floorf((float)(y - 1) / s) - 1);
        r.hi = min(out - 1, (int)ceilf((float)(y + 1) / s) + 1);
    } else {
        r.lo = 0;
        r.hi = out - 1;
    }
    return r;
}
__device__ __forceinline__ float tap_weight(int Y, int y, int in, int out) {
    const Bilin b = bilin(Y, in, out);
    // i1 == i0 only on the last row, where l == 0 (or the side has one row): both taps land on it
    return (b.i0 == y ? 1.f - b.l : 0.f) + (b.i1 == y ? b.l : 0.f);
}

template <int V>
__global__ __launch_bounds__(64 * PB_WAVES) void resize_ac_bwd_kernel(const float* __restrict__ dy, long long dyn, int lddy, int dyc,
                                                                       const float* add, long long addn, int ldadd, int addc,
                                                                       float* dx, long long dxn, int lddx, int dxc, long long npix, int C,
                                                                       int hi, int wi, int ho, int wo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long i = (long long)blockIdx.x * PB_WAVES + wave; i < npix; i += (long long)gridDim.x * PB_WAVES) {
        const int x = (int)(i % wi);
        const long long t = i / wi;
        const int y = (int)(t % hi), n = (int)(t / hi);
        const Wgt ry = scan_range(y, hi, ho), rx = scan_range(x, wi, wo);
        const float* dyp = dy + n * dyn;
        const long long pix = (long long)y * wi + x;
        if (V == 4) {
            for (int c = lane * 4; c < C; c += 256) {
                float4 acc = zero4();
                for (int Y = ry.lo; Y <= ry.hi; ++Y) {
                    const float wy = tap_weight(Y, y, hi, ho);
                    if (wy == 0.f) continue;
                    for (int X = rx.lo; X <= rx.hi; ++X) {
                        const float wx = tap_weight(X, x, wi, wo);
                        if (wx == 0.f) continue;
                        fma4(acc, __fmul_rn(wy, wx), ld4(dyp + ((long long)Y * wo + X) * lddy + c));
                    }
                }
                if (add) add4(acc, ld4(add + n * addn + pix * ldadd + c));
                *(float4*)(dx + n * dxn + pix * lddx + c) = acc;
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                float acc = 0.f;
                for (int Y = ry.lo; Y <= ry.hi; ++Y) {
                    const float wy = tap_weight(Y, y, hi, ho);
                    if (wy == 0.f) continue;
                    for (int X = rx.lo; X <= rx.hi; ++X) {
                        const float wx = tap_weight(X, x, wi, wo);
                        if (wx == 0.f) continue;
                        acc = __fmaf_rn(__fmul_rn(wy, wx), dyp[((long long)Y * wo + X) * lddy + (long long)c * dyc], acc);
                    }
                }
                if (add) acc = __fadd_rn(acc, add[n * addn + pix * ldadd + (long long)c * addc]);
                dx[n * dxn + pix * lddx + (long long)c * dxc] = acc;
            }
        }
    }
}

// ---- (d) the support half of the init_merge convs ---------------------------------------------------------------------------
// part[k][b][blk][c] = sum over block blk's pixels of g_k[b][p][c]; every bin uses PB_MAX_BLOCKS blocks (one without pixels
// writes zeros), so the second stage has one shape.  grid (PB_MAX_BLOCKS, B, bins * C / 256).
__global__ __launch_bounds__(64 * PB_WAVES) void colsum_bins_kernel(BinArgs a, float* __restrict__ part, int B, int C) {
    __shared__ float4 red[PB_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const int cchunks = (C + 255) / 256, k = blockIdx.z / cchunks, c = ((blockIdx.z - k * cchunks) * 64 + lane) * 4;
    const bool live = c < C;
    const int HW = a.h[k] * a.w[k];
    float4 acc = zero4();
    if (live)
        for (int p = blockIdx.x * PB_WAVES + wave; p < HW; p += PB_MAX_BLOCKS * PB_WAVES)
            add4(acc, ld4(a.g[k] + ((size_t)b * HW + p) * a.ld[k] + c));
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
        float4 s = red[0][lane];
        for (int j = 1; j < PB_WAVES; ++j) add4(s, red[j][lane]);
        *(float4*)(part + (((size_t)k * B + b) * PB_MAX_BLOCKS + blockIdx.x) * C + c) = s;
    }
}

// out[i] = sum over k = 0..nparts-1, in that order, of part[k * len + i]  (one slab of nparts * len floats per blockIdx.y)
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, int nparts, int len, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const float* p = part + (size_t)blockIdx.y * nparts * len + i;
    float s = 0.f;
    for (int k = 0; k < nparts; ++k) s = __fadd_rn(s, p[(size_t)k * len]);
    out[(size_t)blockIdx.y * len + i] = s;
}

// dsvec[b][ci] = sum over rows r = k * Cout + co of W_k[co * ldw + ci] * csum[k][b][co]: 64 ci lanes x DS_GROUPS row groups per
// block (group j takes rows j, j + DS_GROUPS, ...), the groups added in order.  grid (Cin / 64, B).
__global__ __launch_bounds__(64 * DS_GROUPS) void merge_dsvec_kernel(MergeArgs m, int ldw, const float* __restrict__ csum,
                                                                      float* __restrict__ dsvec, int nbins, int B, int Cin, int Cout) {
    __shared__ float red[DS_GROUPS][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, b = blockIdx.y;
    const int ci = blockIdx.x * 64 + lane, rows = nbins * Cout;
    float s = 0.f;
    if (ci < Cin)
        for (int r = grp; r < rows; r += DS_GROUPS) {
            const int k = r / Cout, co = r - k * Cout;
            s = __fmaf_rn(m.W[k][(size_t)co * ldw + ci], csum[((size_t)k * B + b) * Cout + co], s);
        }
    red[grp][lane] = s;
    __syncthreads();
    if (grp == 0 && ci < Cin) {
        float t = red[0][lane];
        for (int j = 1; j < DS_GROUPS; ++j) t = __fadd_rn(t, red[j][lane]);
        dsvec[(size_t)b * Cin + ci] = t;
    }
}

// dW_k[co * ldw + ci] = sum_b csum[k][b][co] svec[b][ci], b in order: one thread per (bin, co, ci).  The rows of the 513-column
// weight are not 16-byte aligned: scalar stores, coalesced over ci.
__global__ __launch_bounds__(256) void merge_dw_kernel(MergeArgs m, int ldw, const float* __restrict__ csum, const float* __restrict__ svec,
                                                       int nbins, int B, int Cin, int Cout) {
    const long long total = (long long)nbins * Cout * Cin;
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i % Cin);
    const int r = (int)(i / Cin), k = r / Cout, co = r - k * Cout;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = __fmaf_rn(csum[((size_t)k * B + b) * Cout + co], svec[(size_t)b * Cin + ci], acc);
    m.dW[k][(size_t)co * ldw + ci] = acc;
}

int fill_bins(BinArgs& a, const char* what, int nbins, const float* const* g, const int* ldg, const int* bh, const int* bw, int C) {
    PEMP_REQUIRE(nbins >= 1 && nbins <= PB_MAX_BINS && g && ldg && bh && bw, "%s: 1..4 bins with their tables are needed", what);
    a = BinArgs{};
    a.n = nbins;
    for (int k = 0; k < nbins; ++k) {
        PEMP_REQUIRE(g[k] && aligned16(g[k]) && ldg[k] >= C && ldg[k] % 4 == 0 && bh[k] > 0 && bw[k] > 0 && bh[k] <= 4096 && bw[k] <= 4096,
                     "%s: bin %d: null or unaligned pointer, ld < C or not a multiple of 4, or a side outside 1..4096", what, k);
        a.g[k] = g[k];
        a.ld[k] = ldg[k];
        a.h[k] = bh[k];
        a.w[k] = bw[k];
    }
    return 0;
}

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" int pemp_weighted_gap_bwd_f32(const float* dvec, const float* mask, float* dfeat, int ldd, int B, int S, int h, int w, int C,
                                         void* stream) {
    PEMP_REQUIRE(dvec && mask && dfeat, "weighted_gap_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && C > 0 && (long long)B * S <= 65535 && (long long)h * w < (1LL << 30),
                 "weighted_gap_bwd: bad sizes");
    PEMP_REQUIRE(C % 4 == 0 && ldd >= C && ldd % 4 == 0 && aligned16(dvec) && aligned16(dfeat),
                 "weighted_gap_bwd: C and ldd must be multiples of 4, ldd >= C, dvec / dfeat 16-byte aligned");
    const int nblk = (int)std::min<long long>(PB_MAX_BLOCKS, grid_pixels((long long)h * w));
    hipLaunchKernelGGL(weighted_gap_bwd_kernel, dim3(nblk, B * S), dim3(64 * PB_WAVES), 0, (hipStream_t)stream, dvec, mask, dfeat, ldd, S,
                       h, w, C);
    return launch_status("weighted_gap_bwd");
}

extern "C" int pemp_adaptive_avgpool_bwd_multi_nhwc_f32(int nbins, const float* const* g, const int* ldg, const int* bin_h,
                                                        const int* bin_w, float* dx, int lddx, int N, int H, int W, int C,
                                                        void* stream) {
    PEMP_REQUIRE(dx, "adaptive_avgpool_bwd_multi: null pointer");
    PEMP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && H <= 4096 && W <= 4096 && (long long)N * H * W < (1LL << 40),
                 "adaptive_avgpool_bwd_multi: bad sizes (sides up to 4096)");
    PEMP_REQUIRE(C % 4 == 0 && lddx >= C && lddx % 4 == 0 && aligned16(dx),
                 "adaptive_avgpool_bwd_multi: C and lddx must be multiples of 4, lddx >= C, dx 16-byte aligned");
    BinArgs a;
    if (int rc = fill_bins(a, "adaptive_avgpool_bwd_multi", nbins, g, ldg, bin_h, bin_w, C)) return rc;
    const long long npix = (long long)N * H * W;
    hipLaunchKernelGGL(avgpool_bwd_multi_kernel, dim3((unsigned)std::min<long long>(grid_pixels(npix), 65535)), dim3(64 * PB_WAVES), 0,
                       (hipStream_t)stream, a, dx, lddx, npix, H, W, C);
    return launch_status("adaptive_avgpool_bwd_multi");
}

extern "C" int pemp_resize_bilinear_ac_bwd_nhwc_f32(const float* dy, long long dyn, int lddy, int dyc, const float* add, long long addn,
                                                    int ldadd, int addc, float* dx, long long dxn, int lddx, int dxc, int N, int C,
                                                    int hi, int wi, int ho, int wo, void* stream) {
    PEMP_REQUIRE(dy && dx, "resize_bilinear_ac_bwd: null pointer");
    PEMP_REQUIRE(N > 0 && C > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0 && hi <= 32768 && wi <= 32768 && ho <= 32768 && wo <= 32768 &&
                     lddy > 0 && dyc > 0 && dyn >= 0 && lddx > 0 && dxc > 0 && dxn >= 0 &&
                     (!add || (ldadd > 0 && addc > 0 && addn >= 0)),
                 "resize_bilinear_ac_bwd: bad sizes or strides");
    const bool vec = C % 4 == 0 && dyc == 1 && dxc == 1 && lddy % 4 == 0 && lddx % 4 == 0 && dyn % 4 == 0 && dxn % 4 == 0 &&
                     aligned16(dy) && aligned16(dx) && (!add || (addc == 1 && ldadd % 4 == 0 && addn % 4 == 0 && aligned16(add)));
    const long long npix = (long long)N * hi * wi;
    const dim3 grid((unsigned)std::min<long long>(grid_pixels(npix), 65535)), block(64 * PB_WAVES);
    if (vec)
        hipLaunchKernelGGL(resize_ac_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, dy, dyn, lddy, dyc, add, addn, ldadd, addc, dx, dxn,
                           lddx, dxc, npix, C, hi, wi, ho, wo);
    else
        hipLaunchKernelGGL(resize_ac_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, dy, dyn, lddy, dyc, add, addn, ldadd, addc, dx, dxn,
                           lddx, dxc, npix, C, hi, wi, ho, wo);
    return launch_status("resize_bilinear_ac_bwd");
}

extern "C" size_t pemp_pfenet_merge_support_bwd_workspace_bytes(int nbins, int B, int Cout) {
    if (nbins <= 0 || B <= 0 || Cout <= 0) return 0;
    return (size_t)nbins * B * (PB_MAX_BLOCKS + 1) * Cout * sizeof(float);      // part[k][b][blk][co], then csum[k][b][co]
}

extern "C" int pemp_pfenet_merge_support_bwd_f32(int nbins, const float* const* g, const int* ldg, const int* bin_h, const int* bin_w,
                                                 const float* const* W, float* const* dW, int ldw, const float* svec, float* dsvec,
                                                 void* ws, size_t ws_bytes, int B, int Cin, int Cout, void* stream) {
    PEMP_REQUIRE(W && dW && svec && dsvec && ws, "pfenet_merge_support_bwd: null pointer");
    PEMP_REQUIRE(B > 0 && B <= 65535 && Cin > 0 && Cout > 0 && Cout % 4 == 0 && ldw >= Cin && aligned16(ws) &&
                     (long long)nbins * cdiv(Cout, 256) <= 65535 && (long long)nbins * B <= 65535,
                 "pfenet_merge_support_bwd: bad sizes (Cout %% 4 == 0, ldw >= Cin)");
    BinArgs a;
    if (int rc = fill_bins(a, "pfenet_merge_support_bwd", nbins, g, ldg, bin_h, bin_w, Cout)) return rc;
    MergeArgs m = {};
    for (int k = 0; k < nbins; ++k) {
        PEMP_REQUIRE(W[k] && dW[k], "pfenet_merge_support_bwd: bin %d: null weight or weight-gradient pointer", k);
        m.W[k] = W[k];
        m.dW[k] = dW[k];
    }
    PEMP_REQUIRE(ws_bytes >= pemp_pfenet_merge_support_bwd_workspace_bytes(nbins, B, Cout), "pfenet_merge_support_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    float* csum = part + (size_t)nbins * B * PB_MAX_BLOCKS * Cout;
    hipLaunchKernelGGL(colsum_bins_kernel, dim3(PB_MAX_BLOCKS, B, nbins * cdiv(Cout, 256)), dim3(64 * PB_WAVES), 0, st, a, part, B, Cout);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(cdiv(Cout, 256), nbins * B), dim3(256), 0, st, (const float*)part, PB_MAX_BLOCKS, Cout,
                       csum);
    hipLaunchKernelGGL(merge_dsvec_kernel, dim3(cdiv(Cin, 64), B), dim3(64 * DS_GROUPS), 0, st, m, ldw, (const float*)csum, dsvec, nbins, B,
                       Cin, Cout);
    hipLaunchKernelGGL(merge_dw_kernel, dim3((unsigned)(((long long)nbins * Cout * Cin + 255) / 256)), dim3(256), 0, st, m, ldw,
                       (const float*)csum, svec, nbins, B, Cin, Cout);
    return launch_status("pfenet_merge_support_bwd");
}
