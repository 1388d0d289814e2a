// RPMMs inference kernels (reference: networks/rpmms.py): the EM of the prototype mixture models over the masked support
// features (PMMs.EM :65-86, generate_prototype :101-117), the probability map over the query (discriminative_model :119-141)
// and the sum over a mixture's prototypes of layer55(cat(query, prototype)) (:237-244) without the ten materialised convs.
// All fp32, fixed summation orders, no atomics and no grid-wide wait: results are bit-stable run to run and do not depend on
// the batch size (a block's work is a function of its image, its side and the feature size only).
#include "rpmms_common.h"

namespace pemp {
namespace {

typedef __attribute__((ext_vector_type(4))) float rv4f;

constexpr int RP_GMAX = 16;                  // pixel slices (blocks) per image and side
constexpr int RP_PART = RP_J * RP_C + 16;    // one block's partial: sums [10][256] | column sums [10] | padding
constexpr int RP_MLD = RP_C + 4;             // mu table row stride: the 16-B reads of 11 rows fall on different banks
constexpr int RP_SLD = 17;                   // assignment tile row stride
constexpr float RP_EPS = 1e-6f;
constexpr float RP_KAPPA = 20.f;

__device__ __forceinline__ rv4f ldv(const float* p) { return *(const rv4f*)p; }
// The current mu of one (image, side) from the G partials of the iteration before, every block for itself and every block in
// the same order: mu'_j = (sum_g part_g[j]) / (1e-6 + sum_g colsum_g[j]), mu_j = mu'_j / (1e-6 + |mu'_j|).  Thread = channel;
// returns the thread's ten values.  `red` is [RP_J][4], `cs` [RP_J].  The G <= 16 partials of a column are fetched as sixteen
// independent loads (slices past G re-read the last one and add 0) and added in slice order.
__device__ __forceinline__ void rebuild_mu(const float* __restrict__ part, int G, float (*red)[4], float* cs, float (&m)[RP_J]) {
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    if (c < RP_J) {
        float v[RP_GMAX], s = 0.f;
#pragma unroll
        for (int g = 0; g < RP_GMAX; ++g) v[g] = part[(size_t)min(g, G - 1) * RP_PART + RP_J * RP_C + c];
#pragma unroll
        for (int g = 0; g < RP_GMAX; ++g) s = __fadd_rn(s, g < G ? v[g] : 0.f);
        cs[c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RP_J; ++j) {
        float v[RP_GMAX], s = 0.f;
#pragma unroll
        for (int g = 0; g < RP_GMAX; ++g) v[g] = part[(size_t)min(g, G - 1) * RP_PART + j * RP_C + c];
#pragma unroll
        for (int g = 0; g < RP_GMAX; ++g) s = __fadd_rn(s, g < G ? v[g] : 0.f);
        m[j] = __fdiv_rn(s, __fadd_rn(RP_EPS, cs[j]));
        const float sq = wave_sum(__fmul_rn(m[j], m[j]));
        if (lane == 0) red[j][wave] = sq;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RP_J; ++j) {
        const float n2 = __fadd_rn(__fadd_rn(red[j][0], red[j][1]), __fadd_rn(red[j][2], red[j][3]));
        m[j] = __fdiv_rn(m[j], __fadd_rn(RP_EPS, __fsqrt_rn(n2)));
    }
    __syncthreads();
}

// One EM iteration of one pixel slice.  grid (G, 2, B), 256 threads.  Side 0 weighs pixel p with m_p, side 1 with 1 - m_p;
// x_p = wgt_p * f_p.  A wave owns 16 pixels at a time:
//   E: Z[16 px][16 cols] += X[16 px][4 ch] * MU[4 ch][16 cols] on v_mfma_f32_16x16x4_f32 -- lane (r = l & 15, q = l >> 4) reads
//      float4 #q of every 16-float chunk of pixel r's row and of column r's table row (columns >= 10: an all-zero row);
//   softmax of 20 * Z inside each mixture, max-subtracted (lanes 0..47: mixture l >> 4 of pixel l & 15); pixels past the
//      image get 0, pixels of weight 0 keep their 1 / K (as the reference);
//   M: ACC[16 cols][16 ch] += S^T[16 cols][4 px] * X[4 px][16 ch], sixteen tiles of channels {64 t + 4 n + e}: lane (n, q) reads
//      float4 #n of the 64-float chunk t of pixel 4 kk + q.
// The wave's sums, then the four waves' in the order (0 + 1) + (2 + 3), go to the block's partial.
__global__ __launch_bounds__(256) void em_iter_kernel(const float* __restrict__ feat, int ldf, const float* __restrict__ mask,
                                                      const float* __restrict__ mu0, const float* __restrict__ prev,
                                                      float* __restrict__ cur, int HW, int G) {
    __shared__ float mu_s[(RP_J + 1) * RP_MLD];
    __shared__ float s_tile[4][16 * RP_SLD];
    __shared__ float acc_red[4][RP_J][RP_C];
    __shared__ float cs_red[4][16][RP_J];
    __shared__ float red[RP_J][4];
    __shared__ float cs_s[RP_J];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, side = blockIdx.y, b = blockIdx.z;
    const size_t slot = ((size_t)b * 2 + side) * G;
    {
        float m[RP_J];
        if (prev) {
            rebuild_mu(prev + slot * RP_PART, G, red, cs_s, m);
        } else {
#pragma unroll
            for (int j = 0; j < RP_J; ++j) m[j] = mu0[j * RP_C + tid];
        }
#pragma unroll
        for (int j = 0; j < RP_J; ++j) mu_s[j * RP_MLD + tid] = m[j];
        mu_s[RP_J * RP_MLD + tid] = 0.f;
        for (int i = lane; i < 16 * RP_SLD; i += 64) s_tile[wave][i] = 0.f;      // columns 10..15 stay zero
    }
    __syncthreads();

    const float* fimg = feat + (size_t)b * HW * ldf;
    const float* mimg = mask + (size_t)b * HW;
    const int ntile = (HW + 15) / 16, tpb = (ntile + G - 1) / G;
    const int t_begin = g * tpb, t_end = min(t_begin + tpb, ntile);
    const int r = lane & 15, q = lane >> 4;
    const float* mrow = mu_s + (r < RP_J ? r : RP_J) * RP_MLD + 4 * q;
    float* st = s_tile[wave];
    rv4f macc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) macc[t][e] = rv4f{0.f, 0.f, 0.f, 0.f};
    float csum[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int i = 0; i < tpb; i += 4) {                      // the same trip count in every wave: the barriers below are uniform
        const int tile = t_begin + i + wave;
        const bool live = tile < t_end;
        const int p0 = tile * 16;
        if (live) {
            // E step
            const int pr = min(p0 + r, HW - 1);
            const float mv = mimg[pr];
            const float wr = side ? __fsub_rn(1.f, mv) : mv;
            const float* xr = fimg + (size_t)pr * ldf + 4 * q;
            rv4f z0 = rv4f{0.f, 0.f, 0.f, 0.f}, z1 = z0;
#pragma unroll
            for (int t = 0; t < RP_C / 16; t += 2) {
                rv4f xa = ldv(xr + 16 * t), xb = ldv(xr + 16 * t + 16);
                const rv4f pa = ldv(mrow + 16 * t), pb = ldv(mrow + 16 * t + 16);
                xa = rv4f{__fmul_rn(xa.x, wr), __fmul_rn(xa.y, wr), __fmul_rn(xa.z, wr), __fmul_rn(xa.w, wr)};
                xb = rv4f{__fmul_rn(xb.x, wr), __fmul_rn(xb.y, wr), __fmul_rn(xb.z, wr), __fmul_rn(xb.w, wr)};
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, pa.x, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb.x, pb.x, z1, 0, 0, 0);
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, pa.y, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb.y, pb.y, z1, 0, 0, 0);
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.z, pa.z, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb.z, pb.z, z1, 0, 0, 0);
                z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.w, pa.w, z0, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb.w, pb.w, z1, 0, 0, 0);
            }
            // Z[px = 4 q + e][col = r] lives in lane l, register e
            if (r < RP_J) {
#pragma unroll
                for (int e = 0; e < 4; ++e) st[(4 * q + e) * RP_SLD + r] = __fmul_rn(RP_KAPPA, __fadd_rn(z0[e], z1[e]));
            }
        }
        __syncthreads();
        if (live && lane < 48) {
            const int j0 = group_first(q), K = group_size(q);
            float* zp = st + r * RP_SLD + j0;
            if (p0 + r < HW) {
                float zv[6], mx = zp[0];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    zv[k] = k < K ? zp[k] : 0.f;
                    if (k < K) mx = fmaxf(mx, zv[k]);
                }
                float den = 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k < K) {
                        zv[k] = expf(__fsub_rn(zv[k], mx));
                        den = __fadd_rn(den, zv[k]);
                    }
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k < K) {
                        const float s = __fdiv_rn(zv[k], den);
                        zp[k] = s;
                        csum[k] = __fadd_rn(csum[k], s);
                    }
            } else {
                for (int k = 0; k < K; ++k) zp[k] = 0.f;
            }
        }
        __syncthreads();
        if (live) {
            // M step
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float av = st[(4 * kk + q) * RP_SLD + r];            // S[px = 4 kk + q][col = r]
                const int pq = min(p0 + 4 * kk + q, HW - 1);
                const float mq = mimg[pq];
                const float wq = side ? __fsub_rn(1.f, mq) : mq;
                const float* xq = fimg + (size_t)pq * ldf + 4 * r;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const rv4f xv = ldv(xq + 64 * t);
                    macc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __fmul_rn(xv.x, wq), macc[t][0], 0, 0, 0);
                    macc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __fmul_rn(xv.y, wq), macc[t][1], 0, 0, 0);
                    macc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __fmul_rn(xv.z, wq), macc[t][2], 0, 0, 0);
                    macc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __fmul_rn(xv.w, wq), macc[t][3], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ACC[col = 4 q + e2][ch = 64 t + 4 r + e] lives in lane l, macc[t][e][e2]
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
        const int j = 4 * q + e2;
        if (j < RP_J) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                *(float4*)&acc_red[wave][j][64 * t + 4 * r] = make_float4(macc[t][0][e2], macc[t][1][e2], macc[t][2][e2], macc[t][3][e2]);
        }
    }
    if (lane < 48) {
        const int j0 = group_first(q), K = group_size(q);
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < K) cs_red[wave][r][j0 + k] = csum[k];
    }
    __syncthreads();
    float* out = cur + (slot + g) * RP_PART;
#pragma unroll
    for (int j = 0; j < RP_J; ++j)
        out[j * RP_C + tid] = __fadd_rn(__fadd_rn(acc_red[0][j][tid], acc_red[1][j][tid]), __fadd_rn(acc_red[2][j][tid], acc_red[3][j][tid]));
    if (tid < RP_J) {
        float s = 0.f;
        for (int wv = 0; wv < 4; ++wv)
            for (int px = 0; px < 16; ++px) s = __fadd_rn(s, cs_red[wv][px][tid]);
        out[RP_J * RP_C + tid] = s;
    }
}

// mu_out[b][side][j][c] from the last iteration's partials.  grid (1, 2, B).
__global__ __launch_bounds__(256) void em_final_kernel(const float* __restrict__ prev, float* __restrict__ mu_out, int G) {
    __shared__ float red[RP_J][4];
    __shared__ float cs_s[RP_J];
    const size_t bs = (size_t)blockIdx.z * 2 + blockIdx.y;
    float m[RP_J];
    rebuild_mu(prev + bs * G * RP_PART, G, red, cs_s, m);
#pragma unroll
    for (int j = 0; j < RP_J; ++j) mu_out[(bs * RP_J + j) * RP_C + threadIdx.x] = m[j];
}

// Probability maps of the three mixtures (rpmms.py:119-139): per query pixel the softmax over the 2K dots <q, [mu_f | mu_b]>
// (no kappa), P_f = sum of the first K, P_b = sum of the last K -> channels C (P_b) and C + 1 (P_f) of mixture g's buffer.
// grid (pixel chunks, B); a wave owns one pixel at a time, lane l the channels 4 l .. 4 l + 3; the lane partials are summed by
// the fixed butterfly of wave_sum.
constexpr int PM_PIX = 32;
__global__ __launch_bounds__(256) void prob_map_kernel(const float* __restrict__ qry, int ldq, const float* __restrict__ mu,
                                                       float* __restrict__ out, int ldo, long long gstride, int HW) {
    __shared__ float4 mus[2 * RP_J][RP_C / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const float* mb = mu + (size_t)b * 2 * RP_J * RP_C;
    for (int i = tid; i < 2 * RP_J * RP_C / 4; i += 256) mus[i / (RP_C / 4)][i % (RP_C / 4)] = ld4(mb + 4 * i);
    __syncthreads();
    const int p_end = min((blockIdx.x + 1) * PM_PIX, HW);
    for (int p = blockIdx.x * PM_PIX + wave; p < p_end; p += 4) {
        const float4 v = ld4(qry + ((size_t)b * HW + p) * ldq + 4 * lane);
        float d[2 * RP_J];
#pragma unroll
        for (int n = 0; n < 2 * RP_J; ++n) {
            const float4 a = mus[n][lane];
            d[n] = wave_sum(__fmaf_rn(a.w, v.w, __fmaf_rn(a.z, v.z, __fmaf_rn(a.y, v.y, __fmul_rn(a.x, v.x)))));
        }
        if (lane < 3) {
            const int j0 = group_first(lane), K = group_size(lane);
            float mx = d[0];
#pragma unroll
            for (int n = 0; n < 2 * RP_J; ++n) {
                const int j = n < RP_J ? n : n - RP_J;
                if (j >= j0 && j < j0 + K) mx = (n == j0) ? d[n] : fmaxf(mx, d[n]);
            }
            float sf = 0.f, sb = 0.f;
#pragma unroll
            for (int n = 0; n < 2 * RP_J; ++n) {
                const int j = n < RP_J ? n : n - RP_J;
                if (j >= j0 && j < j0 + K) {
                    const float e = expf(__fsub_rn(d[n], mx));
                    if (n < RP_J) sf = __fadd_rn(sf, e);
                    else sb = __fadd_rn(sb, e);
                }
            }
            const float den = __fadd_rn(sf, sb);
            float* op = out + (size_t)lane * gstride + ((size_t)b * HW + p) * ldo + RP_C;
            op[0] = __fdiv_rn(sb, den);
            op[1] = __fdiv_rn(sf, den);
        }
    }
}

// out_g[b][p][c] = sum_{i in mixture g, ascending} relu(base[b][p][c] + bias[c] + R_i[p][c]), R_i = the sum, in tap order 0..8,
// of T[b][i][tap][c] over the taps of the 3x3 / dilation dil conv whose source pixel lies inside the image.  A thread owns four
// channels and walks the pixels of its chunk; the all-taps sums of its channels (every interior pixel's R_i) stay in registers,
// only the border ring recomputes.  grid (chunks of 16 pixels, B), 64 channel lanes x 4 pixel lanes.
constexpr int PS_PIX = 16;
__global__ __launch_bounds__(256) void proto_sum_kernel(const float* __restrict__ base, int ldb, const float* __restrict__ bias,
                                                        const float* __restrict__ T, float* __restrict__ out, int ldo,
                                                        long long gstride, int h, int w, int dil) {
    const int c = 4 * (threadIdx.x & 63), ty = threadIdx.x >> 6, b = blockIdx.y, HW = h * w;
    const float* Tb = T + (size_t)b * RP_J * 9 * RP_C + c;
    float4 full[RP_J];
#pragma unroll
    for (int i = 0; i < RP_J; ++i) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) s = add4(s, ld4(Tb + ((size_t)i * 9 + tap) * RP_C));
        full[i] = s;
    }
    const float4 bv = ld4(bias + c);
    const int p_end = min((blockIdx.x + 1) * PS_PIX, HW);
    for (int p = blockIdx.x * PS_PIX + ty; p < p_end; p += 4) {
        const int y = p / w, x = p - y * w;
        const bool interior = y >= dil && y + dil < h && x >= dil && x + dil < w;
        const size_t px = (size_t)b * HW + p;
        const float4 bb = add4(ld4(base + px * ldb + c), bv);
        float4 g0, g1, g2;
#pragma unroll
        for (int i = 0; i < RP_J; ++i) {
            float4 R = full[i];
            if (!interior) R = border_taps(Tb + (size_t)i * 9 * RP_C, y, x, h, w, dil);
            const float4 v = relu4(add4(bb, R));
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

// layer56's input of (query, class) pairs against a bank of K classes: prob_map_kernel and proto_sum_kernel in one walk.  Both
// give a pixel to a wave and the channels 4 l .. 4 l + 3 to lane l, so a wave makes all 258 channels of its pixel from one read
// of the query's layer5 row and one of its base row.  grid (chunks of BL_PIX pixels, N): a block keeps its chunk's rows in
// LDS (BL_PIX / 4 pixels per wave, 32 KB) and walks its query's classes -- all K of them (index == nullptr, pair n * K + k) or
// the one class index[n] (pair n); per class it reloads the 20 mu rows into LDS and the ten all-taps sums into registers.  Every
// arithmetic statement is the one of the two episode kernels, in their order: a pair's bits are theirs on (qry[n], base[n],
// mu[k], T[k]) and do not depend on N, K or the pair's place.
constexpr int BL_PIX = 16, BL_PER_WAVE = BL_PIX / 4;
__global__ __launch_bounds__(256) void bank_l56_kernel(const float* __restrict__ qry, int ldq, const float* __restrict__ base, int ldb,
                                                       const float* __restrict__ bias, const float* __restrict__ mu,
                                                       const float* __restrict__ T, const int* __restrict__ index,
                                                       float* __restrict__ out, int ldo, long long gstride, int K, int h, int w,
                                                       int dil) {
    __shared__ float4 mus[2 * RP_J][RP_C / 4];
    __shared__ float4 rows[4][BL_PER_WAVE][2][RP_C / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.y, HW = h * w, c = 4 * lane;
    const int p0 = blockIdx.x * BL_PIX + wave, p_end = min((blockIdx.x + 1) * BL_PIX, HW);
    // the chunk's rows, read once: lane l parks its float4s of the wave's pixels in LDS (its own slots: no barrier) and takes
    // them back per class; in registers they would cost the class loop its occupancy
    const float4 bv = ld4(bias + c);
    for (int s = 0; s < BL_PER_WAVE; ++s) {
        const size_t px = (size_t)n * HW + min(p0 + 4 * s, HW - 1);
        rows[wave][s][0][lane] = ld4(qry + px * ldq + c);
        rows[wave][s][1][lane] = add4(ld4(base + px * ldb + c), bv);
    }
    const int k_first = index ? index[n] : 0, k_last = index ? k_first + 1 : K;
    for (int k = k_first; k < k_last; ++k) {
        const float* mb = mu + (size_t)k * 2 * RP_J * RP_C;
        __syncthreads();                                     // the class before is read out
        for (int i = tid; i < 2 * RP_J * RP_C / 4; i += 256) mus[i / (RP_C / 4)][i % (RP_C / 4)] = ld4(mb + 4 * i);
        __syncthreads();
        const float* Tk = T + (size_t)k * RP_J * 9 * RP_C + c;
        float4 full[RP_J];
#pragma unroll
        for (int i = 0; i < RP_J; ++i) full[i] = full_taps(Tk + (size_t)i * 9 * RP_C);
        const size_t r = index ? (size_t)n : (size_t)n * K + k;
#pragma unroll 1
        for (int s = 0; s < BL_PER_WAVE; ++s) {
            const int p = p0 + 4 * s;
            if (p >= p_end) break;                           // wave-uniform
            float* op = out + (r * HW + p) * ldo;
            const float4 bb = rows[wave][s][1][lane];
            {   // proto_sum_kernel's pixel
                const int y = p / w, x = p - y * w;
                const bool interior = y >= dil && y + dil < h && x >= dil && x + dil < w;
                float4 g0, g1, g2;
#pragma unroll
                for (int i = 0; i < RP_J; ++i) {
                    float4 R = full[i];
                    if (!interior) R = border_taps(Tk + (size_t)i * 9 * RP_C, y, x, h, w, dil);
                    const float4 v = relu4(add4(bb, R));
                    if (i == 0) g0 = v;
                    else if (i == 1) g1 = v;
                    else if (i < 4) g1 = add4(g1, v);
                    else if (i == 4) g2 = v;
                    else g2 = add4(g2, v);
                }
                *(float4*)(op + c) = g0;
                *(float4*)(op + c + gstride) = g1;
                *(float4*)(op + c + 2 * gstride) = g2;
            }
            {   // prob_map_kernel's pixel
                const float4 v = rows[wave][s][0][lane];
                float d[2 * RP_J];
#pragma unroll
                for (int m = 0; m < 2 * RP_J; ++m) {
                    const float4 a = mus[m][lane];
                    d[m] = wave_sum(__fmaf_rn(a.w, v.w, __fmaf_rn(a.z, v.z, __fmaf_rn(a.y, v.y, __fmul_rn(a.x, v.x)))));
                }
                if (lane < 3) {
                    const int j0 = group_first(lane), Kg = group_size(lane);
                    float mx = d[0];
#pragma unroll
                    for (int m = 0; m < 2 * RP_J; ++m) {
                        const int j = m < RP_J ? m : m - RP_J;
                        if (j >= j0 && j < j0 + Kg) mx = (m == j0) ? d[m] : fmaxf(mx, d[m]);
                    }
                    float sf = 0.f, sb = 0.f;
#pragma unroll
                    for (int m = 0; m < 2 * RP_J; ++m) {
                        const int j = m < RP_J ? m : m - RP_J;
                        if (j >= j0 && j < j0 + Kg) {
                            const float e = expf(__fsub_rn(d[m], mx));
                            if (m < RP_J) sf = __fadd_rn(sf, e);
                            else sb = __fadd_rn(sb, e);
                        }
                    }
                    const float den = __fadd_rn(sf, sb);
                    float* pp = op + (size_t)lane * gstride + RP_C;
                    pp[0] = __fdiv_rn(sb, den);
                    pp[1] = __fdiv_rn(sf, den);
                }
            }
        }
    }
}

int em_blocks(int HW) { return std::min(RP_GMAX, cdiv(HW, 64)); }

}  // namespace
}  // namespace pemp

using namespace pemp;

extern "C" int pemp_rpmms_em_f32(const float* feat, int ldf, const float* mask, const float* mu0, float* work, float* mu_out, int B,
                                 int h, int w, int C, int iters, void* stream) {
    PEMP_REQUIRE(feat && mask && mu0 && work && mu_out, "rpmms_em: null pointer");
    PEMP_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && (long long)h * w < (1 << 24) && iters > 0, "rpmms_em: bad sizes");
    PEMP_REQUIRE(C == RP_C, "rpmms_em: the kernels are built for C = 256");
    PEMP_REQUIRE(ldf >= C && ldf % 4 == 0 && aligned16(feat) && aligned16(work), "rpmms_em: ldf must be a multiple of 4 and >= C, "
                 "feat / work 16-byte aligned");
    const int HW = h * w, G = em_blocks(HW);
    const size_t half = (size_t)B * 2 * G * RP_PART;
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < iters; ++it) {
        const float* prev = it == 0 ? nullptr : work + (size_t)((it - 1) & 1) * half;
        hipLaunchKernelGGL(em_iter_kernel, dim3(G, 2, B), dim3(256), 0, st, feat, ldf, mask, mu0, prev, work + (size_t)(it & 1) * half,
                           HW, G);
    }
    hipLaunchKernelGGL(em_final_kernel, dim3(1, 2, B), dim3(256), 0, st, (const float*)(work + (size_t)((iters - 1) & 1) * half), mu_out,
                       G);
    return launch_status("rpmms_em");
}

extern "C" int pemp_rpmms_prob_map_f32(const float* qry, int ldq, const float* mu, float* out, int ldo, long long gstride, int B,
                                       int HW, int C, void* stream) {
    PEMP_REQUIRE(qry && mu && out, "rpmms_prob_map: null pointer");
    PEMP_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW < (1 << 24), "rpmms_prob_map: bad sizes");
    PEMP_REQUIRE(C == RP_C, "rpmms_prob_map: the kernels are built for C = 256");
    PEMP_REQUIRE(ldq >= C && ldq % 4 == 0 && ldo >= C + 2 && gstride >= 0 && aligned16(qry) && aligned16(mu),
                 "rpmms_prob_map: ldq must be a multiple of 4 and >= C, ldo >= C + 2, qry / mu 16-byte aligned");
    hipLaunchKernelGGL(prob_map_kernel, dim3(cdiv(HW, PM_PIX), B), dim3(256), 0, (hipStream_t)stream, qry, ldq, mu, out, ldo, gstride,
                       HW);
    return launch_status("rpmms_prob_map");
}

extern "C" int pemp_rpmms_proto_sum_f32(const float* wz, const float* mu, const float* base, int ldb, const float* bias, float* T,
                                        float* out, int ldo, long long gstride, int B, int h, int w, int C, int dil, void* stream) {
    PEMP_REQUIRE(wz && mu && base && bias && T && out, "rpmms_proto_sum: null pointer");
    PEMP_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && (long long)h * w < (1 << 24) && dil > 0, "rpmms_proto_sum: bad sizes");
    PEMP_REQUIRE(C == RP_C, "rpmms_proto_sum: the kernels are built for C = 256");
    PEMP_REQUIRE(ldb >= C && ldb % 4 == 0 && ldo >= C && ldo % 4 == 0 && gstride >= 0 && gstride % 4 == 0 && aligned16(wz) &&
                     aligned16(mu) && aligned16(base) && aligned16(bias) && aligned16(T) && aligned16(out),
                 "rpmms_proto_sum: ldb, ldo and gstride must be multiples of 4, ldb / ldo >= C, operands 16-byte aligned");
    const int rows = 9 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tap_gemv_kernel, dim3(cdiv(rows, 4), B), dim3(256), 0, st, wz, mu, T, rows);
    hipLaunchKernelGGL(proto_sum_kernel, dim3(cdiv(h * w, PS_PIX), B), dim3(256), 0, st, base, ldb, bias, (const float*)T, out, ldo,
                       gstride, h, w, dil);
    return launch_status("rpmms_proto_sum");
}

extern "C" int pemp_rpmms_proto_taps_f32(const float* wz, const float* mu, float* T, int K, int C, void* stream) {
    PEMP_REQUIRE(wz && mu && T, "rpmms_proto_taps: null pointer");
    PEMP_REQUIRE(K > 0 && K <= 65535, "rpmms_proto_taps: bad sizes");
    PEMP_REQUIRE(C == RP_C, "rpmms_proto_taps: the kernels are built for C = 256");
    PEMP_REQUIRE(aligned16(wz) && aligned16(mu) && aligned16(T), "rpmms_proto_taps: operands 16-byte aligned");
    const int rows = 9 * C;
    hipLaunchKernelGGL(tap_gemv_kernel, dim3(cdiv(rows, 4), K), dim3(256), 0, (hipStream_t)stream, wz, mu, T, rows);
    return launch_status("rpmms_proto_taps");
}

extern "C" int pemp_rpmms_bank_l56_f32(const float* qry, int ldq, const float* base, int ldb, const float* bias, const float* mu,
                                       const float* T, const int* index, float* out, int ldo, long long gstride, int N, int K,
                                       int h, int w, int C, int dil, void* stream) {
    PEMP_REQUIRE(qry && base && bias && mu && T && out, "rpmms_bank_l56: null pointer");
    PEMP_REQUIRE(N > 0 && K > 0 && (long long)N * K <= 65535 && h > 0 && w > 0 && (long long)h * w < (1 << 24) && dil > 0,
                 "rpmms_bank_l56: bad sizes (N, K >= 1, N * K <= 65535)");
    PEMP_REQUIRE(C == RP_C, "rpmms_bank_l56: the kernels are built for C = 256");
    PEMP_REQUIRE(ldq >= C && ldq % 4 == 0 && ldb >= C && ldb % 4 == 0 && ldo >= C + 2 && ldo % 4 == 0 && gstride >= 0 &&
                     gstride % 4 == 0,
                 "rpmms_bank_l56: ldq, ldb, ldo and gstride must be multiples of 4, ldq / ldb >= C, ldo >= C + 2");
    PEMP_REQUIRE(aligned16(qry) && aligned16(base) && aligned16(bias) && aligned16(mu) && aligned16(T) && aligned16(out),
                 "rpmms_bank_l56: operands 16-byte aligned");
    hipLaunchKernelGGL(bank_l56_kernel, dim3(cdiv(h * w, BL_PIX), N), dim3(256), 0, (hipStream_t)stream, qry, ldq, base, ldb, bias, mu,
                       T, index, out, ldo, gstride, K, h, w, dil);
    return launch_status("rpmms_bank_l56");
}
