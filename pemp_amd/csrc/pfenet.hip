// PFENet inference kernels (reference: networks/pfenet.py): the prior mask (:201-226), the FEM's adaptive pooling and
// bilinear resizes on NHWC maps (:238-268), Weighted_GAP (:15-20) and the masked support input of layer 4 (:190-193).
#include "common.h"
#include "head_common.h"

namespace pemp {
namespace {

constexpr int PT = 64;          // prior tile: 64 support pixels x 64 query pixels per block
constexpr int PK = 32;          // K (channels) staged per step
// LDS row stride of the k-major operand images.  The staging stores (lane l of a 32-lane group writes row r + (l >> 3),
// k row 4 (l & 7) + j) hit bank (4 (l & 7) PLD + r) mod 32: PT + 1 spreads them over all 32 banks (PT + 4 put 32 lanes
// on 8 banks); the MFMA operand reads take 32 consecutive floats of one k row, conflict-free for any stride.
constexpr int PLD = PT + 1;
constexpr float COS_EPS = 1e-7f;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// One (episode-shot, support tile, query tile) block: sim[p][q] = dot(m_p s_p, q) / (|m_p s_p| |q| + eps) on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered fma chain), the norms accumulated from the same staged operands,
// the max over the tile's support pixels taken in the epilogue -> part[bs][p tile][q].  Four waves, 2 x 2 tiles of 32 x 32.
__global__ __launch_bounds__(256) void prior_tile_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ s, int lds,
                                                         const float* __restrict__ mask, float* __restrict__ part, int S, int HW,
                                                         int C) {
    __shared__ float As[PK][PLD];       // support operand, k-major
    __shared__ float Bs[PK][PLD];       // query operand, k-major
    __shared__ float nrm[2][PT];        // |m s| per support pixel, |q| per query pixel
    __shared__ float red[2][PT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wp = wave & 1, wq = wave >> 1;
    const int bs = blockIdx.z, b = bs / S;
    const int q0 = blockIdx.x * PT, p0 = blockIdx.y * PT;
    const int r = t >> 3, kc = (t & 7) * 4;             // rows r and r + 32 of both tiles, channels kc..kc+3 of a step

    const float* sp[2];
    const float* qp[2];
    float mk[2];
    for (int i = 0; i < 2; ++i) {
        const int p = p0 + r + 32 * i, qq = q0 + r + 32 * i;
        sp[i] = p < HW ? s + ((size_t)bs * HW + p) * lds + kc : nullptr;
        mk[i] = p < HW ? mask[(size_t)bs * HW + p] : 0.f;
        qp[i] = qq < HW ? q + ((size_t)b * HW + qq) * ldq + kc : nullptr;
    }
    float4 ra[2], rb[2];
    float ssa[2] = {0.f, 0.f}, ssb[2] = {0.f, 0.f};
    auto load = [&](int k0) {
        for (int i = 0; i < 2; ++i) {
            float4 v = sp[i] ? *(const float4*)(sp[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
            // the mask multiply on operand load: fl(m * s), the reference's operand (pfenet.py:199)
            ra[i] = make_float4(__fmul_rn(v.x, mk[i]), __fmul_rn(v.y, mk[i]), __fmul_rn(v.z, mk[i]), __fmul_rn(v.w, mk[i]));
            rb[i] = qp[i] ? *(const float4*)(qp[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    f32x16 acc = {};
    load(0);
    for (int k0 = 0; k0 < C; k0 += PK) {
        __syncthreads();
        for (int i = 0; i < 2; ++i) {
            const int row = r + 32 * i;
            As[kc + 0][row] = ra[i].x; As[kc + 1][row] = ra[i].y; As[kc + 2][row] = ra[i].z; As[kc + 3][row] = ra[i].w;
            Bs[kc + 0][row] = rb[i].x; Bs[kc + 1][row] = rb[i].y; Bs[kc + 2][row] = rb[i].z; Bs[kc + 3][row] = rb[i].w;
            ssa[i] = __fmaf_rn(ra[i].w, ra[i].w, __fmaf_rn(ra[i].z, ra[i].z, __fmaf_rn(ra[i].y, ra[i].y, __fmaf_rn(ra[i].x, ra[i].x, ssa[i]))));
            ssb[i] = __fmaf_rn(rb[i].w, rb[i].w, __fmaf_rn(rb[i].z, rb[i].z, __fmaf_rn(rb[i].y, rb[i].y, __fmaf_rn(rb[i].x, rb[i].x, ssb[i]))));
        }
        __syncthreads();
        if (k0 + PK < C) load(k0 + PK);
#pragma unroll
        for (int kk = 0; kk < PK / 2; ++kk) {
            const float a = As[2 * kk + (lane >> 5)][wp * 32 + (lane & 31)];
            const float bq = Bs[2 * kk + (lane >> 5)][wq * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
        }
    }
    // norms: the 8 lanes of a row hold its partial sums of squares (lanes 8j .. 8j+7), fixed butterfly order
    for (int i = 0; i < 2; ++i) {
        float xa = ssa[i], xb = ssb[i];
        xa += __shfl_xor(xa, 1, 64); xb += __shfl_xor(xb, 1, 64);
        xa += __shfl_xor(xa, 2, 64); xb += __shfl_xor(xb, 2, 64);
        xa += __shfl_xor(xa, 4, 64); xb += __shfl_xor(xb, 4, 64);
        if ((t & 7) == 0) {
            nrm[0][r + 32 * i] = __fsqrt_rn(xa);
            nrm[1][r + 32 * i] = __fsqrt_rn(xb);
        }
    }
    __syncthreads();
    // epilogue: C/D of 32x32x2: column (query) = lane & 31, row (support) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int qc = wq * 32 + (lane & 31);
    const float nq = nrm[1][qc];
    float mx = -INFINITY;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int pr = wp * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (p0 + pr < HW) {
            const float v = __fdiv_rn(acc[reg], __fadd_rn(__fmul_rn(nrm[0][pr], nq), COS_EPS));
            mx = fmaxf(mx, v);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lane < 32) red[wp][qc] = mx;
    __syncthreads();
    if (t < PT && q0 + t < HW) part[((size_t)bs * gridDim.y + blockIdx.y) * HW + q0 + t] = fmaxf(red[0][t], red[1][t]);
}

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* sh) {
    // max / min of a 1024-thread block (exact, order-free); sh: 16 floats
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : fminf(v, u);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    v = sh[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) v = is_max ? fmaxf(v, sh[i]) : fminf(v, sh[i]);
    return v;
}

// sim[bs][q] = max over the support tiles of part (exact, order-free): one thread per (shot, query pixel).
__global__ __launch_bounds__(256) void prior_tilemax_kernel(const float* __restrict__ part, float* __restrict__ sim, int HW,
                                                            int nbp) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x, bs = blockIdx.y;
    if (q >= HW) return;
    const float* pp = part + (size_t)bs * nbp * HW + q;
    float v = pp[0];
    for (int j = 1; j < nbp; ++j) v = fmaxf(v, pp[(size_t)j * HW]);
    sim[(size_t)bs * HW + q] = v;
}

// One block per episode: per shot, sim min-max normalised over the query pixels with (sim - min) / (max - min + eps)
// (pfenet.py:217-218); the shots added in order 0..S-1, then / S (:227).
__global__ __launch_bounds__(1024) void prior_finish_kernel(const float* __restrict__ sim, float* __restrict__ out, int S,
                                                            int HW) {
    __shared__ float sh[16];
    const int b = blockIdx.x;
    for (int si = 0; si < S; ++si) {
        const float* sp = sim + (size_t)(b * S + si) * HW;
        float lo = INFINITY, hi = -INFINITY;
        for (int q = threadIdx.x; q < HW; q += blockDim.x) {
            lo = fminf(lo, sp[q]);
            hi = fmaxf(hi, sp[q]);
        }
        lo = block_reduce(lo, false, sh);
        hi = block_reduce(hi, true, sh);
        const float den = __fadd_rn(__fsub_rn(hi, lo), COS_EPS);
        for (int q = threadIdx.x; q < HW; q += blockDim.x) {
            const float nv = __fdiv_rn(__fsub_rn(sp[q], lo), den);
            float* o = out + (size_t)b * HW + q;
            *o = si == 0 ? nv : __fadd_rn(*o, nv);
            if (si == S - 1 && S > 1) *o = __fdiv_rn(*o, (float)S);
        }
    }
}

// -- support banks: the support side of the prior GEMM stored once per (class, shot), met by any number of queries ---------------
// Pack: one block per support image.  The pixels with m != 0 are compacted in pixel order (chunks of 256 pixels, an integer
// ballot / popcount scan: exact, the same layout on every run); row j of the slot is fl(m_p s_p), its norm is accumulated with
// prior_tile_kernel's own partial sums (lane t & 7 owns channels 4 (t & 7) .. + 3 of every 32-channel step, fma chain x y z w,
// xor-1/2/4 butterfly, __fsqrt_rn), so the stored norm is the number that kernel forms for the pixel.  One all-zero row follows
// when a pixel with m == 0 exists.  rows == nullptr: only the count is written.  Rows at or beyond cap are not written.
__global__ __launch_bounds__(256) void prior_bank_pack_kernel(const float* __restrict__ s, int lds, const float* __restrict__ mask,
                                                              float* __restrict__ rows, float* __restrict__ norms,
                                                              int* __restrict__ count, int HW, int C, int cap) {
    __shared__ int src[256];
    __shared__ int wtot[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t img = blockIdx.x;
    const float* mp = mask + img * HW;
    const int g = t >> 3, kc = (t & 7) * 4;
    int run = 0;
    for (int c0 = 0; c0 < HW; c0 += 256) {
        const int p = c0 + t;
        const bool fg = p < HW && mp[p] != 0.f;
        const unsigned long long bal = __ballot(fg);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();                                // the previous chunk's readers of src / wtot are done
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int base = 0;
        for (int i = 0; i < wave; ++i) base += wtot[i];
        const int tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        if (fg) src[base + pre] = p;
        __syncthreads();
        if (rows) {
            for (int j0 = 0; j0 < tot; j0 += 32) {      // 32 rows per pass, 8 lanes per row
                const int j = j0 + g, dst = run + j;
                const bool ok = j < tot && dst < cap;
                const int sp = ok ? src[j] : 0;
                const float m = ok ? mp[sp] : 0.f;
                const float* in = s + (img * HW + sp) * lds + kc;
                float* o = rows + (img * cap + (ok ? dst : 0)) * C + kc;
                float ss = 0.f;
                for (int k0 = 0; k0 < C; k0 += PK) {
                    if (ok) {
                        const float4 v = *(const float4*)(in + k0);
                        const float4 a = make_float4(__fmul_rn(v.x, m), __fmul_rn(v.y, m), __fmul_rn(v.z, m), __fmul_rn(v.w, m));
                        *(float4*)(o + k0) = a;
                        ss = __fmaf_rn(a.w, a.w, __fmaf_rn(a.z, a.z, __fmaf_rn(a.y, a.y, __fmaf_rn(a.x, a.x, ss))));
                    }
                }
                ss += __shfl_xor(ss, 1, 64);
                ss += __shfl_xor(ss, 2, 64);
                ss += __shfl_xor(ss, 4, 64);
                if (ok && (t & 7) == 0) norms[img * cap + dst] = __fsqrt_rn(ss);
            }
        }
        run += tot;
    }
    if (rows && run < HW && run < cap) {                // the one row that stands for every pixel with m == 0
        for (int i = t; i < C; i += 256) rows[(img * cap + run) * C + i] = 0.f;
        if (t == 0) norms[img * cap + run] = 0.f;
    }
    if (t == 0) count[img] = run + (run < HW ? 1 : 0);
}

// One (query tile, shot, query-class pair) block: prior_tile_kernel's arithmetic with the support operand and its norms read from
// the bank.  The block walks the ceil(count / 64) support tiles of its slot itself and keeps the running max in registers
// -> sim[pair * S + shot][q]; every similarity is its own k-ordered MFMA chain, so the tile a row sits in does not matter.
// index != nullptr: pair n meets class index[n] (clamped into 0..K-1); nullptr: pair n * K + k meets class k.
__global__ __launch_bounds__(256) void prior_bank_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ rows,
                                                         const float* __restrict__ norms, const int* __restrict__ count,
                                                         const int* __restrict__ index, float* __restrict__ sim, int K, int S,
                                                         int HW, int C, int cap) {
    __shared__ float As[PK][PLD];       // support operand, k-major
    __shared__ float Bs[PK][PLD];       // query operand, k-major
    __shared__ float nrm[2][PT];        // |m s| per stored row, |q| per query pixel
    __shared__ float red[2][PT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wp = wave & 1, wq = wave >> 1;
    const int si = blockIdx.y, pair = blockIdx.z;
    const int n = index ? pair : pair / K;
    const int k = index ? min(max(index[pair], 0), K - 1) : pair % K;
    const size_t slot = (size_t)k * S + si;
    const int cnt = min(max(count[slot], 1), cap);
    const float* rbase = rows + slot * cap * C;
    const float* nbase = norms + slot * cap;
    const int q0 = blockIdx.x * PT;
    const int r = t >> 3, kc = (t & 7) * 4;             // rows r and r + 32 of both tiles, channels kc..kc+3 of a step

    const float* sp[2];
    const float* qp[2];
    for (int i = 0; i < 2; ++i) {
        const int qq = q0 + r + 32 * i;
        qp[i] = qq < HW ? q + ((size_t)n * HW + qq) * ldq + kc : nullptr;
    }
    float4 ra[2], rb[2];
    float ssb[2] = {0.f, 0.f};
    auto load = [&](int k0) {
        for (int i = 0; i < 2; ++i) {
            ra[i] = sp[i] ? *(const float4*)(sp[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[i] = qp[i] ? *(const float4*)(qp[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    const int qc = wq * 32 + (lane & 31);
    float mx = -INFINITY;
    for (int p0 = 0; p0 < cnt; p0 += PT) {
        for (int i = 0; i < 2; ++i) {
            const int p = p0 + r + 32 * i;
            sp[i] = p < cnt ? rbase + (size_t)p * C + kc : nullptr;
        }
        f32x16 acc = {};
        load(0);
        for (int k0 = 0; k0 < C; k0 += PK) {
            __syncthreads();
            if (k0 == 0 && t < PT) nrm[0][t] = p0 + t < cnt ? nbase[p0 + t] : 0.f;
            for (int i = 0; i < 2; ++i) {
                const int row = r + 32 * i;
                As[kc + 0][row] = ra[i].x; As[kc + 1][row] = ra[i].y; As[kc + 2][row] = ra[i].z; As[kc + 3][row] = ra[i].w;
                Bs[kc + 0][row] = rb[i].x; Bs[kc + 1][row] = rb[i].y; Bs[kc + 2][row] = rb[i].z; Bs[kc + 3][row] = rb[i].w;
                if (p0 == 0)
                    ssb[i] = __fmaf_rn(rb[i].w, rb[i].w, __fmaf_rn(rb[i].z, rb[i].z, __fmaf_rn(rb[i].y, rb[i].y, __fmaf_rn(rb[i].x, rb[i].x, ssb[i]))));
            }
            __syncthreads();
            if (k0 + PK < C) load(k0 + PK);
#pragma unroll
            for (int kk = 0; kk < PK / 2; ++kk) {
                const float a = As[2 * kk + (lane >> 5)][wp * 32 + (lane & 31)];
                const float bq = Bs[2 * kk + (lane >> 5)][wq * 32 + (lane & 31)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
            }
        }
        if (p0 == 0) {                  // the query norms: once, in prior_tile_kernel's summation order
            for (int i = 0; i < 2; ++i) {
                float xb = ssb[i];
                xb += __shfl_xor(xb, 1, 64);
                xb += __shfl_xor(xb, 2, 64);
                xb += __shfl_xor(xb, 4, 64);
                if ((t & 7) == 0) nrm[1][r + 32 * i] = __fsqrt_rn(xb);
            }
        }
        __syncthreads();
        const float nq = nrm[1][qc];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = wp * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (p0 + pr < cnt) {
                const float v = __fdiv_rn(acc[reg], __fadd_rn(__fmul_rn(nrm[0][pr], nq), COS_EPS));
                mx = fmaxf(mx, v);
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lane < 32) red[wp][qc] = mx;
    __syncthreads();
    if (t < PT && q0 + t < HW) sim[((size_t)pair * S + si) * HW + q0 + t] = fmaxf(red[0][t], red[1][t]);
}

// dst[n] = src[index[n]] (index clamped into 0..K-1), or without an index dst[n * K + k] = src[k]: rows of C floats.
__global__ void bank_gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ index, float* __restrict__ dst,
                                        int P, int K, int C) {
    const long long total = (long long)P * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C), pr = (int)(i / C);
        const int k = index ? min(max(index[pr], 0), K - 1) : pr % K;
        dst[i] = src[(size_t)k * C + c];
    }
}

// nn.AdaptiveAvgPool2d on NHWC: window rows [floor(i in / out), ceil((i + 1) in / out)), sum row by row, / kh / kw.
__global__ void adaptive_avgpool_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int N, int H, int W,
                                        int C, int Ho, int Wo) {
    const long long total = (long long)N * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long t = i / C;
        const int ox = (int)(t % Wo);
        t /= Wo;
        const int oy = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const int ys = (oy * H) / Ho, ye = ((oy + 1) * H + Ho - 1) / Ho;
        const int xs = (ox * W) / Wo, xe = ((ox + 1) * W + Wo - 1) / Wo;
        float sum = 0.f;
        for (int yy = ys; yy < ye; ++yy)
            for (int xx = xs; xx < xe; ++xx) sum = __fadd_rn(sum, x[(((size_t)n * H + yy) * W + xx) * ldx + c]);
        y[(((size_t)n * Ho + oy) * Wo + ox) * ldy + c] = __fdiv_rn(__fdiv_rn(sum, (float)(ye - ys)), (float)(xe - xs));
    }
}

// F.interpolate(bilinear, align_corners=True) between any two sizes; element (n, pixel, c) of x at n * xn + pixel * ldx + c * xc
// (NHWC slices: xc = 1; a mask plane of a [B][S][2][H][W] tensor: ldx = 1, xn = 2 H W).  flags & 1: read x as (x == 1).
__global__ void resize_ac_kernel(const float* __restrict__ x, long long xn, int ldx, int xc, float* __restrict__ y, long long yn,
                                 int ldy, int yc, int N, int C, int hi, int wi, int ho, int wo, int flags) {
    const long long total = (long long)N * ho * wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long t = i / C;
        const int ox = (int)(t % wo);
        t /= wo;
        const int oy = (int)(t % ho);
        const int n = (int)(t / ho);
        const Bilin by = bilin(oy, hi, ho), bx = bilin(ox, wi, wo);
        const float* p = x + n * xn + (long long)c * xc;
        float v00 = p[(size_t)(by.i0 * wi + bx.i0) * ldx], v01 = p[(size_t)(by.i0 * wi + bx.i1) * ldx];
        float v10 = p[(size_t)(by.i1 * wi + bx.i0) * ldx], v11 = p[(size_t)(by.i1 * wi + bx.i1) * ldx];
        if (flags & 1) {
            v00 = v00 == 1.f ? 1.f : 0.f; v01 = v01 == 1.f ? 1.f : 0.f;
            v10 = v10 == 1.f ? 1.f : 0.f; v11 = v11 == 1.f ? 1.f : 0.f;
        }
        const float h0 = 1.f - by.l, w0 = 1.f - bx.l;       // same rounding points as head_common.h bilerp
        const float top = __fmaf_rn(bx.l, v01, __fmul_rn(w0, v00));
        const float bot = __fmaf_rn(bx.l, v11, __fmul_rn(w0, v10));
        y[n * yn + (long long)(oy * wo + ox) * ldy + (long long)c * yc] = __fmaf_rn(by.l, bot, __fmul_rn(h0, top));
    }
}

// Weighted_GAP (pfenet.py:15-20) of every shot, averaged over the shots (:229-233).  Block (64 channels, 16 pixel lanes) per
// (channel chunk, episode); the 16 partial sums are added in lane order.
__global__ __launch_bounds__(1024) void weighted_gap_kernel(const float* __restrict__ f, int ldf, const float* __restrict__ m,
                                                            float* __restrict__ out, int S, int h, int w, int C) {
    __shared__ float pf[16][64];
    __shared__ float pm[16][64];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int c = blockIdx.x * 64 + tx, b = blockIdx.y, HW = h * w;
    float acc = 0.f;
    for (int si = 0; si < S; ++si) {
        const int n = b * S + si;
        float sf = 0.f, sm = 0.f;
        if (c < C) {
            for (int p = ty; p < HW; p += 16) {
                const float mv = m[(size_t)n * HW + p];
                sf = __fadd_rn(sf, __fmul_rn(f[((size_t)n * HW + p) * ldf + c], mv));
                sm = __fadd_rn(sm, mv);
            }
        }
        pf[ty][tx] = sf;
        pm[ty][tx] = sm;
        __syncthreads();
        if (ty == 0 && c < C) {
            float tf = 0.f, tm = 0.f;
            for (int j = 0; j < 16; ++j) {
                tf = __fadd_rn(tf, pf[j][tx]);
                tm = __fadd_rn(tm, pm[j][tx]);
            }
            // avg_pool2d(.) * h * w, and area = avg_pool2d(mask) * h * w + 0.0005
            const float num = __fmul_rn(__fmul_rn(__fdiv_rn(tf, (float)HW), (float)h), (float)w);
            const float area = __fadd_rn(__fmul_rn(__fmul_rn(__fdiv_rn(tm, (float)HW), (float)h), (float)w), 0.0005f);
            const float g = __fdiv_rn(num, area);
            acc = si == 0 ? g : __fadd_rn(acc, g);
        }
        __syncthreads();
    }
    if (ty == 0 && c < C) out[(size_t)b * C + c] = S > 1 ? __fdiv_rn(acc, (float)S) : acc;
}

// y = x * m[pixel] (m optional) + r (r optional), NHWC rows with their own strides
__global__ void scale_add_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ m, const float* __restrict__ r,
                                 int ldr, float* __restrict__ y, int ldy, long long npix, int C) {
    const long long total = npix * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long p = i / C;
        float v = x[p * ldx + c];
        if (m) v = __fmul_rn(v, m[p]);
        if (r) v = __fadd_rn(v, r[p * ldr + c]);
        y[p * ldy + c] = v;
    }
}

int grid_of(long long total) { return (int)std::min<long long>((total + 255) / 256, 8192); }

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" size_t pemp_prior_mask_workspace_bytes(int B, int S, int HW) {
    if (B <= 0 || S <= 0 || HW <= 0) return 0;
    return (size_t)B * S * (cdiv(HW, PT) + 1) * HW * sizeof(float);      // part[bs][tile][q], then sim[bs][q]
}

extern "C" int pemp_prior_mask_f32(const float* q, int ldq, const float* s, int lds, const float* mask, float* out, void* ws,
                                   size_t ws_bytes, int B, int S, int HW, int C, void* stream) {
    PEMP_REQUIRE(q && s && mask && out && ws, "prior_mask: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && HW > 0 && C > 0 && C % PK == 0, "prior_mask: bad sizes (C %% 32 == 0 required)");
    PEMP_REQUIRE(ldq >= C && lds >= C && ldq % 4 == 0 && lds % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)s & 15) == 0,
                 "prior_mask: ldq/lds must be >= C, multiples of 4, operands 16-byte aligned");
    PEMP_REQUIRE(ws_bytes >= pemp_prior_mask_workspace_bytes(B, S, HW), "prior_mask: workspace too small");
    PEMP_REQUIRE(B * S <= 65535, "prior_mask: too many support images");
    const int nbt = cdiv(HW, PT);
    float* part = (float*)ws;
    hipLaunchKernelGGL(prior_tile_kernel, dim3(nbt, nbt, B * S), dim3(256), 0, (hipStream_t)stream, q, ldq, s, lds, mask, part, S,
                       HW, C);
    float* sim = part + (size_t)B * S * nbt * HW;
    hipLaunchKernelGGL(prior_tilemax_kernel, dim3(cdiv(HW, 256), B * S), dim3(256), 0, (hipStream_t)stream, part, sim, HW, nbt);
    hipLaunchKernelGGL(prior_finish_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, sim, out, S, HW);
    return launch_status("prior_mask");
}

extern "C" int pemp_prior_bank_pack_f32(const float* s, int lds, const float* mask, float* rows, float* norms, int32_t* count,
                                        int KS, int HW, int C, int cap, void* stream) {
    PEMP_REQUIRE(mask && count, "prior_bank_pack: null pointer");
    PEMP_REQUIRE((rows != nullptr) == (norms != nullptr) && (!rows || s), "prior_bank_pack: rows, norms and s go together");
    PEMP_REQUIRE(KS > 0 && HW > 0, "prior_bank_pack: bad sizes");
    if (rows) {
        PEMP_REQUIRE(C > 0 && C % PK == 0, "prior_bank_pack: bad sizes (C %% 32 == 0 required)");
        PEMP_REQUIRE(cap > 0 && cap % PT == 0, "prior_bank_pack: cap must be a positive multiple of 64");
        PEMP_REQUIRE(lds >= C && lds % 4 == 0 && ((uintptr_t)s & 15) == 0 && ((uintptr_t)rows & 15) == 0,
                     "prior_bank_pack: lds must be >= C and a multiple of 4, s and rows 16-byte aligned");
    }
    hipLaunchKernelGGL(prior_bank_pack_kernel, dim3(KS), dim3(256), 0, (hipStream_t)stream, s, lds, mask, rows, norms, count, HW, C,
                       cap);
    return launch_status("prior_bank_pack");
}

extern "C" size_t pemp_prior_bank_workspace_bytes(int pairs, int S, int HW) {
    if (pairs <= 0 || S <= 0 || HW <= 0) return 0;
    return (size_t)pairs * S * HW * sizeof(float);                           // sim[pair * S + shot][q]
}

extern "C" int pemp_prior_bank_f32(const float* q, int ldq, const float* rows, const float* norms, const int32_t* count,
                                   const int32_t* index, float* out, void* ws, size_t ws_bytes, int N, int K, int S, int HW, int C,
                                   int cap, void* stream) {
    PEMP_REQUIRE(q && rows && norms && count && out && ws, "prior_bank: null pointer");
    PEMP_REQUIRE(N > 0 && K > 0 && S > 0 && HW > 0 && C > 0 && C % PK == 0, "prior_bank: bad sizes (C %% 32 == 0 required)");
    PEMP_REQUIRE(cap > 0 && cap % PT == 0, "prior_bank: cap must be a positive multiple of 64");
    PEMP_REQUIRE(ldq >= C && ldq % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)rows & 15) == 0,
                 "prior_bank: ldq must be >= C and a multiple of 4, q and rows 16-byte aligned");
    const long long pairs = index ? N : (long long)N * K;
    PEMP_REQUIRE(pairs <= 65535 && S <= 65535, "prior_bank: more than 65535 query-class pairs or shots");
    PEMP_REQUIRE(ws_bytes >= pemp_prior_bank_workspace_bytes((int)pairs, S, HW), "prior_bank: workspace too small");
    float* sim = (float*)ws;
    hipLaunchKernelGGL(prior_bank_kernel, dim3(cdiv(HW, PT), S, (int)pairs), dim3(256), 0, (hipStream_t)stream, q, ldq, rows, norms,
                       count, index, sim, K, S, HW, C, cap);
    hipLaunchKernelGGL(prior_finish_kernel, dim3((int)pairs), dim3(1024), 0, (hipStream_t)stream, sim, out, S, HW);
    return launch_status("prior_bank");
}

extern "C" int pemp_bank_gather_rows_f32(const float* src, const int32_t* index, float* dst, int N, int K, int C, void* stream) {
    PEMP_REQUIRE(src && dst, "bank_gather_rows: null pointer");
    PEMP_REQUIRE(N > 0 && K > 0 && C > 0, "bank_gather_rows: bad sizes");
    const long long P = index ? N : (long long)N * K;
    PEMP_REQUIRE(P <= 0x7fffffff, "bank_gather_rows: too many rows");
    hipLaunchKernelGGL(bank_gather_rows_kernel, dim3(grid_of(P * C)), dim3(256), 0, (hipStream_t)stream, src, index, dst, (int)P, K,
                       C);
    return launch_status("bank_gather_rows");
}

extern "C" int pemp_adaptive_avgpool_nhwc_f32(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int Ho,
                                              int Wo, void* stream) {
    PEMP_REQUIRE(x && y, "adaptive_avgpool: null pointer");
    PEMP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0 && ldx >= C && ldy >= C, "adaptive_avgpool: bad sizes");
    const long long total = (long long)N * Ho * Wo * C;
    hipLaunchKernelGGL(adaptive_avgpool_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, N, H, W,
                       C, Ho, Wo);
    return launch_status("adaptive_avgpool");
}

extern "C" int pemp_resize_bilinear_ac_nhwc_f32(const float* x, long long xn, int ldx, int xc, float* y, long long yn, int ldy,
                                                int yc, int N, int C, int hi, int wi, int ho, int wo, int flags, void* stream) {
    PEMP_REQUIRE(x && y, "resize_bilinear_ac: null pointer");
    PEMP_REQUIRE(N > 0 && C > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0 && ldx > 0 && ldy > 0 && xc > 0 && yc > 0 && xn >= 0 &&
                     yn >= 0 && (flags & ~1) == 0, "resize_bilinear_ac: bad sizes or strides");
    const long long total = (long long)N * ho * wo * C;
    hipLaunchKernelGGL(resize_ac_kernel, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, x, xn, ldx, xc, y, yn, ldy, yc,
                       N, C, hi, wi, ho, wo, flags);
    return launch_status("resize_bilinear_ac");
}

extern "C" int pemp_weighted_gap_f32(const float* feat, int ldf, const float* mask, float* out, int B, int S, int h, int w, int C,
                                     void* stream) {
    PEMP_REQUIRE(feat && mask && out, "weighted_gap: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && C > 0 && ldf >= C && B <= 65535, "weighted_gap: bad sizes");
    hipLaunchKernelGGL(weighted_gap_kernel, dim3(cdiv(C, 64), B), dim3(64, 16), 0, (hipStream_t)stream, feat, ldf, mask, out, S, h,
                       w, C);
    return launch_status("weighted_gap");
}

extern "C" int pemp_scale_add_nhwc_f32(const float* x, int ldx, const float* m, const float* r, int ldr, float* y, int ldy,
                                       long long npix, int C, void* stream) {
    PEMP_REQUIRE(x && y && (m || r), "scale_add: null pointer");
    PEMP_REQUIRE(npix > 0 && C > 0 && ldx >= C && ldy >= C && (!r || ldr >= C), "scale_add: bad sizes");
    hipLaunchKernelGGL(scale_add_kernel, dim3(grid_of(npix * C)), dim3(256), 0, (hipStream_t)stream, x, ldx, m, r, ldr, y, ldy, npix,
                       C);
    return launch_status("scale_add");
}
