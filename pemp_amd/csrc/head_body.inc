// Body of head.hip: included once per MAXJ (PEMP_MAXJ, namespace PEMP_HEAD_NS); see head.hip.
namespace pemp {
namespace PEMP_HEAD_NS {
constexpr int MAXJ = PEMP_MAXJ;     // rows per pixel the kernels of this namespace keep in registers (2 * protos <= MAXJ)

// out[j] = wave-wide sum of v[j], in every lane (fixed order: wave_sum8 on each group of eight)
__device__ __forceinline__ void wave_totals(const float (&v)[MAXJ], float (&out)[MAXJ]) {
#if PEMP_MAXJ == 8
    const float tot = wave_sum8(v);          // lane l holds the total of v[l & 7]
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) out[j] = __shfl(tot, j, 64);
#else
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        lo[j] = v[j];
        hi[j] = v[8 + j];
    }
    const float t0 = wave_sum8(lo), t1 = wave_sum8(hi);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        out[j] = __shfl(t0, j, 64);
        out[8 + j] = __shfl(t1, j, 64);
    }
#endif
}


// -----------------------------------------------------------------------------------------------
// assign weights  A[bs][j][i]
//   MODE 0: meta-prototype soft assignment, networks/pemp_stage1.py:205-207
//   MODE 1: plain masks (fg, bg) at feature resolution, pemp_stage1.py:224-225
// one wave per pixel.
template <int MODE>
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ feat, int ldf,
                                                     const float* __restrict__ mask,
                                                     const float* __restrict__ ctr, const float* __restrict__ bias,
                                                     float* __restrict__ A,
                                                     int n, int h, int w, int H, int W, int c, int p) {
    const int bs = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int J = MODE == 0 ? 2 * p : 2;
    const int ncl = (c + 255) / 256;  // float4 chunks per lane

    float cw[MAXJ][MAXCL];            // this lane's slice of the centred centres (MODE 0; ctr = dc, bias: centre_kernel)
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < MAXCL / 4; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int ch = t * 256 + lane * 4 + e;
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) cw[j][t * 4 + e] = (t < ncl && ch < c && j < J) ? ctr[ch * J + j] : 0.f;
            }
    }
    const float* mk = mask + (size_t)bs * 2 * H * W;
    for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const int y = i / w, x = i - y * w;
        const int sy = nearest_src(y, H, h), sx = nearest_src(x, W, w);
        const float mfg = mk[(size_t)sy * W + sx];
        const float mbg = mk[(size_t)H * W + (size_t)sy * W + sx];
        float* out = A + ((size_t)bs * J) * n + i;
        if (MODE == 1) {
            if (lane == 0) {
                out[0] = mfg;
                out[n] = mbg;
            }
            continue;
        }
        const float* xp = feat + ((size_t)bs * n + i) * ldf;
        float d[MAXJ];
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) d[j] = 0.f;
#pragma unroll
        for (int t = 0; t < MAXCL / 4; ++t) {
            int ch = t * 256 + lane * 4;
            if (t < ncl && ch < c) {
                float4 v = *(const float4*)(xp + ch);
                float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j) d[j] += xv[e] * cw[j][t * 4 + e];
            }
        }
        {
            wave_totals(d, d);
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) d[j] = j < J ? 2.f * d[j] - bias[j] : 0.f;    // shift-invariant logits (head_common.h)
        }
        if (lane == 0) {
            for (int g = 0; g < 2; ++g) {
                float mx = -INFINITY;
                for (int j = 0; j < p; ++j) mx = fmaxf(mx, d[g * p + j]);
                float e[MAXJ / 2], s = 0.f;
                for (int j = 0; j < p; ++j) {
                    e[j] = expf(d[g * p + j] - mx);
                    s += e[j];
                }
                const float m = g == 0 ? mfg : mbg;
                for (int j = 0; j < p; ++j) out[(size_t)(g * p + j) * n] = (e[j] / s) * m;
            }
        }
    }
}

// MODE 2 (Baseline): A_g[p] = sum_P m_g[P] * W[P][p], W = bilinear align_corners weights of the
// h x w -> H x W upsampling (adjoint of networks/baseline.py:100), plus exact mask sums.
// one thread per low-res pixel and group.
__global__ void adjoint_mask_kernel(const float* __restrict__ mask, float* __restrict__ A, int n, int h, int w,
                                    int H, int W) {
    const int bs = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * n) return;
    const int g = idx / n, i = idx - g * n;
    const int y = i / w, x = i - y * w;
    const float* m = mask + ((size_t)bs * 2 + g) * H * W;
    const float sh = h > 1 && H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sw = w > 1 && W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    // rows Y whose source coordinate sh*Y lies in (y-1, y+1)
    int Y0 = sh > 0.f ? max(0, (int)floorf((float)(y - 1) / sh) - 1) : 0;
    int Y1 = sh > 0.f ? min(H - 1, (int)ceilf((float)(y + 1) / sh) + 1) : H - 1;
    int X0 = sw > 0.f ? max(0, (int)floorf((float)(x - 1) / sw) - 1) : 0;
    int X1 = sw > 0.f ? min(W - 1, (int)ceilf((float)(x + 1) / sw) + 1) : W - 1;
    float acc = 0.f;
    for (int Y = Y0; Y <= Y1; ++Y) {
        float fy = sh * (float)Y;
        int y0 = (int)fy;
        int y1 = y0 + (y0 < h - 1 ? 1 : 0);
        float ly = fy - (float)y0;
        float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y && y1 != y0 ? ly : 0.f);
        if (y1 == y0 && y0 == y) wy = 1.f;
        if (wy == 0.f) continue;
        float row = 0.f;
        for (int X = X0; X <= X1; ++X) {
            float fx = sw * (float)X;
            int x0 = (int)fx;
            int x1 = x0 + (x0 < w - 1 ? 1 : 0);
            float lx = fx - (float)x0;
            float wx = (x0 == x ? 1.f - lx : 0.f) + (x1 == x && x1 != x0 ? lx : 0.f);
            if (x1 == x0 && x0 == x) wx = 1.f;
            if (wx != 0.f) row += wx * m[(size_t)Y * W + X];
        }
        acc += wy * row;
    }
    A[((size_t)bs * 2 + g) * n + i] = acc;
}

// exact full-resolution mask sums (integers in fp32, so the order is immaterial), one 1024-thread block per (bs, g)
__global__ __launch_bounds__(1024) void mask_sum_kernel(const float* __restrict__ mask, float* __restrict__ out,
                                                        int HW) {
    __shared__ float red[16];
    const float* m = mask + (size_t)blockIdx.x * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = threadIdx.x;
    for (; i + 3072 < HW; i += 4096) {          // four independent loads in flight per thread
        s0 += m[i];
        s1 += m[i + 1024];
        s2 += m[i + 2048];
        s3 += m[i + 3072];
    }
    for (; i < HW; i += 1024) s0 += m[i];
    float s = wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += red[k];
        out[blockIdx.x] = t;
    }
}

// -----------------------------------------------------------------------------------------------
// pooling partial sums: part[bs][chunk][j][c] = sum_{i in chunk} x[i][c] * A[j][i]
//                       asum[bs][chunk][j]    = sum_{i in chunk} A[j][i]
// thread t owns channels t and t+256 (coalesced across the block), pixels in order.
__global__ __launch_bounds__(256) void pool_partial_kernel(const float* __restrict__ feat, int ldf,
                                                           const float* __restrict__ A, float* __restrict__ part,
                                                           float* __restrict__ asum, int n, int c, int J,
                                                           int nchunks) {
    __shared__ float As[MAXJ][PCHUNK];
    const int bs = blockIdx.y, ck = blockIdx.x;
    const int i0 = ck * PCHUNK;
    const int np = min(PCHUNK, n - i0);
    for (int t = threadIdx.x; t < J * PCHUNK; t += 256) {
        int j = t / PCHUNK, i = t - j * PCHUNK;
        As[j][i] = i < np ? A[((size_t)bs * J + j) * n + i0 + i] : 0.f;
    }
    __syncthreads();
    float acc[2][MAXJ];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) acc[k][j] = 0.f;
    const float* xb = feat + ((size_t)bs * n + i0) * ldf;
    for (int i = 0; i < np; ++i) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            int ch = threadIdx.x + 256 * k;
            if (ch < c) {
                float v = xb[(size_t)i * ldf + ch];
#pragma unroll
                for (int j = 0; j < MAXJ; ++j)
                    if (j < J) acc[k][j] += v * As[j][i];
            }
        }
    }
    float* pb = part + ((size_t)bs * nchunks + ck) * J * c;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int ch = threadIdx.x + 256 * k;
        if (ch < c)
#pragma unroll
            for (int j = 0; j < MAXJ; ++j)
                if (j < J) pb[(size_t)j * c + ch] = acc[k][j];
    }
    if (threadIdx.x < J) {
        float s = 0.f;
        for (int i = 0; i < np; ++i) s += As[threadIdx.x][i];
        asum[((size_t)bs * nchunks + ck) * J + threadIdx.x] = s;
    }
}

// protos[b][j][c] = mean_s ( sum_chunks part / (denominator + eps) ); block = 64 channels x 4 chunk lanes
__global__ __launch_bounds__(256) void pool_final_kernel(const float* __restrict__ part,
                                                         const float* __restrict__ asum,
                                                         const float* __restrict__ den_override,
                                                         float* __restrict__ protos, int S, int c, int J, int nchunks,
                                                         float eps) {
    __shared__ float red[4][64];
    const int b = blockIdx.y, j = blockIdx.x;
    const int ch = blockIdx.z * 64 + (threadIdx.x & 63), chl = min(ch, c - 1);
    float tot = 0.f;
    for (int s = 0; s < S; ++s) {
        const int bs = b * S + s;
        const float num = chunk_sum(part + ((size_t)bs * nchunks * J + j) * c + chl, (size_t)J * c, nchunks, red);
        float den = chunk_sum(asum + (size_t)bs * nchunks * J + j, (size_t)J, nchunks, red);
        if (den_override) den = den_override[bs * J + j];
        tot += num / (den + eps);
    }
    if (threadIdx.x < 64 && ch < c) protos[((size_t)b * J + j) * c + ch] = tot / (float)S;
}

// plain masks at feature resolution as pooling weights (MODE 1 of assign_kernel), one thread per pixel
__global__ void mask_assign_kernel(const float* __restrict__ mask, float* __restrict__ A, int n, int h, int w, int H,
                                   int W) {
    const int bs = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    const int sy = nearest_src(y, H, h), sx = nearest_src(x, W, w);
    const float* mk = mask + (size_t)bs * 2 * H * W;
    A[((size_t)bs * 2 + 0) * n + i] = mk[(size_t)sy * W + sx];
    A[((size_t)bs * 2 + 1) * n + i] = mk[(size_t)H * W + (size_t)sy * W + sx];
}

#if PEMP_MAXJ == 8      // the MFMA row-stream kernels are written for 2p <= 8 (16-column tiles, 8 rows extracted)
// -----------------------------------------------------------------------------------------------
// Pixel-row x small-matrix products on the matrix cores.  Both per-pixel passes of the prototype head
// have the same shape: every pixel's c-vector meets a fixed c x 2p matrix -- the L2-normalised
// prototypes for the cosine map (networks/pemp_stage1.py:214-222, 256-260), the MPM centres for the
// soft assignment (pemp_stage1.py:205-207) -- and the feature map is streamed from HBM exactly once.
// One wave owns 16 pixels: D[16 px][16 cols] += X[16 px][4 k] * T[4 k][16 cols] on
// v_mfma_f32_16x16x4_f32, columns 0..2p-1 real (rows of an LDS table, padded so the 16-B reads of the
// 2p+1 rows fall on different banks), the others read an all-zero row.  Lane (r = l&15, q = l>>4)
// reads float4 #q of every 16-float chunk of pixel r's row -- a wave-wide load is 16 rows x 64
// contiguous bytes -- and feeds it to four MFMAs (k = {16t + 4q + e}); |x|^2 comes from the same
// registers.  The kernel is latency-bound unless many loads are in flight: rows are fetched in groups
// of 8 chunks (8 KB per wave), two groups deep, and the first group is issued before the table is built.
typedef __attribute__((ext_vector_type(4))) float hv4f;
constexpr int SQ = 64;                 // channels per stage pass
constexpr int SLD = SQ + 4;            // stage row stride in floats: 16-B reads of 16 rows hit 64 different banks
#ifndef PEMP_HEAD_NB
#define PEMP_HEAD_NB 2
#endif
#ifndef PEMP_HEAD_OCC
#define PEMP_HEAD_OCC 5
#endif
constexpr int NB = PEMP_HEAD_NB;       // passes in flight (4 KB per wave each)
constexpr int TV = MAXJ * 64 * MAXCL / 256;   // table elements per thread

// 16 pixel rows x c channels through a wave-private LDS stage, SQ channels at a time.  HBM side: lane l reads
// float4 #(l & 15) of row 4u + (l >> 4), u = 0..3 -- a wave-wide load is 4 rows x 256 contiguous bytes, NB
// passes (16 KB per wave) in flight.  MFMA side: lane (r = l&15, q = l>>4) reads float4 #q of every 16-float
// chunk of row r from the stage and the matching table entries, and issues four MFMAs (k = {16t + 4q + e}).
// NQ = c / SQ is a template parameter: with every load and every pass known at compile time the s_waitcnt
// vmcnt bookkeeping is exact (a runtime trip count makes the compiler wait for ALL outstanding loads per pass).
template <int NQ>
struct RowTile {
    const float* base;                 // image base + 4 * (l & 15)
    int off[4];                        // element offset of row 4u + (l >> 4) (clamped to the last pixel)
    hv4f buf[NB][4];
    __device__ __forceinline__ void init(const float* img, int ldf, int i0, int n, int lane) {
        base = img + 4 * (lane & 15);
#pragma unroll
        for (int u = 0; u < 4; ++u) off[u] = min(i0 + 4 * u + (lane >> 4), n - 1) * ldf;
#pragma unroll
        for (int s = 0; s < NB; ++s)
            if (s < NQ) load(s, s);
    }
    __device__ __forceinline__ void load(int s, int qq) {
#pragma unroll
        for (int u = 0; u < 4; ++u) buf[s][u] = *(const hv4f*)(base + off[u] + qq * SQ);
    }
    template <bool NORM>
    __device__ __forceinline__ void pass(int s, int qq, float* stage, const float* bp, int lane, hv4f& acc, float& ss) {
#pragma unroll
        for (int u = 0; u < 4; ++u) *(hv4f*)(stage + (4 * u + (lane >> 4)) * SLD + 4 * (lane & 15)) = buf[s][u];
        if (qq + NB < NQ) load(s, qq + NB);
        __builtin_amdgcn_wave_barrier();
        const float* xr = stage + (lane & 15) * SLD + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < SQ / 16; ++t) {
            const hv4f xv = *(const hv4f*)(xr + 16 * t);
            const hv4f pv = *(const hv4f*)(bp + qq * SQ + 16 * t);
            if (NORM) ss += (xv.x * xv.x + xv.y * xv.y) + (xv.z * xv.z + xv.w * xv.w);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, pv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, pv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, pv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, pv.w, acc, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    template <bool NORM>
    __device__ __forceinline__ void run(float* stage, const float* bp, int lane, hv4f& acc, float& ss) {  // first NB passes loaded
#pragma unroll
        for (int qq = 0; qq < NQ; qq += NB) {
#pragma unroll
            for (int s = 0; s < NB; ++s)
                if (qq + s < NQ) pass<NORM>(s, qq + s, stage, bp, lane, acc, ss);
        }
    }
    // The same pass against T 16-column tables (prototype banks): the staged xv feeds one accumulator per tile.  Per tile
    // the MFMAs and their k order are those of pass(), so a column's sum is the same bits whichever tile holds it.
    template <bool NORM, int T>
    __device__ __forceinline__ void pass_tiles(int s, int qq, float* stage, const float* const (&bp)[T], int lane,
                                               hv4f (&acc)[T], float& ss) {
#pragma unroll
        for (int u = 0; u < 4; ++u) *(hv4f*)(stage + (4 * u + (lane >> 4)) * SLD + 4 * (lane & 15)) = buf[s][u];
        if (qq + NB < NQ) load(s, qq + NB);
        __builtin_amdgcn_wave_barrier();
        const float* xr = stage + (lane & 15) * SLD + 4 * (lane >> 4);
#pragma unroll
        for (int t = 0; t < SQ / 16; ++t) {
            const hv4f xv = *(const hv4f*)(xr + 16 * t);
            if (NORM) ss += (xv.x * xv.x + xv.y * xv.y) + (xv.z * xv.z + xv.w * xv.w);
#pragma unroll
            for (int tt = 0; tt < T; ++tt) {
                const hv4f pv = *(const hv4f*)(bp[tt] + qq * SQ + 16 * t);
                acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, pv.x, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, pv.y, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, pv.z, acc[tt], 0, 0, 0);
                acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, pv.w, acc[tt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    template <bool NORM, int T>
    __device__ __forceinline__ void run_tiles(float* stage, const float* const (&bp)[T], int lane, hv4f (&acc)[T], float& ss) {
#pragma unroll
        for (int qq = 0; qq < NQ; qq += NB) {
#pragma unroll
            for (int s = 0; s < NB; ++s)
                if (qq + s < NQ) pass_tiles<NORM, T>(s, qq + s, stage, bp, lane, acc, ss);
        }
    }
};
// D[i][j] of the 16x16 tile lives in lane 16*(i>>2) + j, register i&3: hand row (l & 15) to lane l.
__device__ __forceinline__ void rows_to_lanes(const hv4f& acc, int lane, float (&v)[MAXJ]) {
    const int row = lane & 15, src = 16 * (row >> 2), e = row & 3;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const float t0 = __shfl(acc[0], src + j, 64), t1 = __shfl(acc[1], src + j, 64);
        const float t2 = __shfl(acc[2], src + j, 64), t3 = __shfl(acc[3], src + j, 64);
        v[j] = e == 0 ? t0 : e == 1 ? t1 : e == 2 ? t2 : t3;
    }
}
// the same for columns C0 .. C0 + MAXJ - 1 of the tile (C0 = 8: the second class of a bank tile)
template <int C0>
__device__ __forceinline__ void cols_to_lanes(const hv4f& acc, int lane, float (&v)[MAXJ]) {
    const int row = lane & 15, src = 16 * (row >> 2) + C0, e = row & 3;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const float t0 = __shfl(acc[0], src + j, 64), t1 = __shfl(acc[1], src + j, 64);
        const float t2 = __shfl(acc[2], src + j, 64), t3 = __shfl(acc[3], src + j, 64);
        v[j] = e == 0 ? t0 : e == 1 ? t1 : e == 2 ? t2 : t3;
    }
}
static inline bool mfma_rows_ok(int c) { return c == 512 || c == 256 || c == 128 || c == 64; }   // instantiated NQ
static inline size_t proj_lds_bytes(int J, int c) { return ((size_t)(J + 1) * (c + 8) + 4 * 16 * SLD) * sizeof(float); }
// squared norms of the table rows, every wave for itself (lane l of the result holds row l & 7)
__device__ __forceinline__ float table_sqnorm(const float* tab, int ldt, int J, int c, int lane) {
    float s[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        s[j] = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCL / 4; ++k) {                        // branch-free: rows >= J are the zero row
            const int ch = 4 * lane + 256 * k;
            const hv4f v = *(const hv4f*)(tab + min(j, J) * ldt + (ch < c ? ch : 0));
            s[j] += ch < c ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
        }
    }
    return wave_sum8(s);
}

// table_sqnorm for the J rows that start at row0 of a table with several classes (rows >= J: the zero row zrow)
__device__ __forceinline__ float table_sqnorm_at(const float* tab, int ldt, int row0, int zrow, int J, int c, int lane) {
    float s[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        s[j] = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCL / 4; ++k) {
            const int ch = 4 * lane + 256 * k;
            const hv4f v = *(const hv4f*)(tab + (j < J ? row0 + j : zrow) * ldt + (ch < c ? ch : 0));
            s[j] += ch < c ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
        }
    }
    return wave_sum8(s);
}

// cosine map x dist_scalar, group maxima, response index: the MFMA outer product with fused L2 normalisation.
template <int NQ>
__global__ __launch_bounds__(256, PEMP_HEAD_OCC) void cosine_mfma_kernel(const float* __restrict__ qry, int ldf,
                                                          const float* __restrict__ protos, float* __restrict__ pred,
                                                          uint8_t* __restrict__ resp, int n, int c, int p,
                                                          float scalar) {
    extern __shared__ __attribute__((aligned(16))) float pnl[];      // [(2p + 1)][c + 8] prototypes, last row zeros | stages
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = 2 * p, ldt = c + 8;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    const int r = lane & 15, q = lane >> 4;
    float* stage = pnl + (J + 1) * ldt + wave * 16 * SLD;
    // the table's loads go first: waiting for them must not wait for the 16 KB of row data behind them
    const float* pb = protos + (size_t)b * J * c;
    float tv[TV];
#pragma unroll
    for (int k = 0; k < TV; ++k) tv[k] = pb[min((int)threadIdx.x + 256 * k, J * c - 1)];
    RowTile<NQ> rt;
    rt.init(qry + (size_t)b * n * ldf, ldf, i0, n, lane);
#pragma unroll
    for (int k = 0; k < TV; ++k) {
        const int t = threadIdx.x + 256 * k;
        if (t < J * c) pnl[(t / c) * ldt + t % c] = tv[k];
    }
    for (int ch = threadIdx.x; ch < c; ch += 256) pnl[J * ldt + ch] = 0.f;
    __syncthreads();
    // cos = x.p / (max(|x|, eps) max(|p|, eps)): the prototype norms are applied in the epilogue
    const float pn2 = table_sqnorm(pnl, ldt, J, c, lane);
    hv4f acc = {0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;
    rt.template run<true>(stage, pnl + (size_t)min(r, J) * ldt + 4 * q, lane, acc, ss);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);                                    // lane l: |x|^2 of pixel (l & 15)
    const float f = scalar / fmaxf(sqrtf(ss), 1e-8f);
    float v[MAXJ];
    rows_to_lanes(acc, lane, v);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) v[j] = v[j] / fmaxf(sqrtf(__shfl(pn2, j, 64)), 1e-8f) * f;
    const int i = i0 + r;
    if (q == 0 && i < n) {
        float best[2] = {0.f, 0.f};              // [0]: fg rows [0,p), [1]: bg rows [p,2p); first maximum wins
        int bi[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)            // static register indices: no scratch for v[]
            if (j < J) {
                const bool fg = j < p;
                const int first = fg ? 0 : p;
                if (fg) {
                    if (j == first || v[j] > best[0]) { best[0] = v[j]; bi[0] = j; }
                } else {
                    if (j == first || v[j] > best[1]) { best[1] = v[j]; bi[1] = j - p; }
                }
            }
        pred[((size_t)b * 2 + 0) * n + i] = best[1];
        pred[((size_t)b * 2 + 1) * n + i] = best[0];
        if (resp) resp[(size_t)b * n + i] = (uint8_t)(best[0] > best[1] ? bi[0] + 3 : bi[1]);
    }
}

// Prototype bank: the cosine map of cosine_mfma_kernel against SEVERAL classes' prototypes in one pass over the query
// rows.  bank is [K][2p][c].  Two classes share a 16-column tile (class 2t in columns 0..7, class 2t+1 in columns 8..15,
// columns past 2p and past the last class read the zero row) and a block keeps T tiles, i.e. up to 2T classes: the staged
// 16 x 64 slab of a pass feeds T accumulators, |x|^2 is taken once.  A column of a 16x16x4 MFMA depends on its own table
// column and on the k order alone, and the k order is that of cosine_mfma_kernel, so for every (query, class) the outputs
// are bit for bit what that kernel writes for protos = bank[class].  Classes beyond 2T go to blockIdx.z (those blocks
// read the rows again).  index != null: query b meets class index[b] only (clamped into the bank), one class per block.
// LDS: [ncap * 2p + 1][c + 8] table (compact: a class's rows follow the previous class's; last row used = zeros) | stages.
static inline int bank_ncap(bool indexed, int T, int K) { return indexed ? 1 : min(2 * T, K); }
static inline size_t bank_lds_bytes(int ncap, int J, int c) { return ((size_t)(ncap * J + 1) * (c + 8) + 4 * 16 * SLD) * sizeof(float); }
template <int NQ, int T>
__global__ __launch_bounds__(256) void cosine_bank_mfma_kernel(const float* __restrict__ qry, int ldf,
                                                               const float* __restrict__ bank,
                                                               const int32_t* __restrict__ index, float* __restrict__ pred,
                                                               uint8_t* __restrict__ resp, int n, int c, int p, int K,
                                                               float scalar) {
    extern __shared__ __attribute__((aligned(16))) float pnl[];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = 2 * p, ldt = c + 8;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    const int r = lane & 15, q = lane >> 4;
    const int ncap = index ? 1 : min(2 * T, K);                      // bank_ncap: the table the launch sized
    const int kbase = index ? min(max((int)index[b], 0), K - 1) : (int)blockIdx.z * 2 * T;
    const int ncls = index ? 1 : min(2 * T, K - kbase);              // classes of this block
    const size_t slot0 = index ? (size_t)b : (size_t)b * K + kbase;  // output image of the block's first class
    const int zrow = ncls * J;
    float* stage = pnl + (ncap * J + 1) * ldt + wave * 16 * SLD;
    RowTile<NQ> rt;
    rt.init(qry + (size_t)b * n * ldf, ldf, i0, n, lane);
    const float* pb = bank + (size_t)kbase * J * c;
    const int c4 = c / 4;
    for (int t = threadIdx.x; t < ncls * J * c4; t += 256) {
        const int row = t / c4, ch = (t - row * c4) * 4;
        *(hv4f*)(pnl + row * ldt + ch) = *(const hv4f*)(pb + (size_t)row * c + ch);
    }
    for (int ch = threadIdx.x; ch < c; ch += 256) pnl[zrow * ldt + ch] = 0.f;
    __syncthreads();
    const float* bp[T];
    hv4f acc[T];
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
        const int cl = 2 * tt + (r >> 3), j = r & 7;
        bp[tt] = pnl + (size_t)((j < J && cl < ncls) ? cl * J + j : zrow) * ldt + 4 * q;
        acc[tt] = (hv4f){0.f, 0.f, 0.f, 0.f};
    }
    float ss = 0.f;
    rt.template run_tiles<true, T>(stage, bp, lane, acc, ss);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);                                    // lane l: |x|^2 of pixel (l & 15)
    const float f = scalar / fmaxf(sqrtf(ss), 1e-8f);
    const int i = i0 + r;
#pragma unroll
    for (int tt = 0; tt < T; ++tt)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int cl = 2 * tt + half;
            if (cl < ncls) {                                         // block-uniform: the shuffles below are wave-wide
                const float pn2 = table_sqnorm_at(pnl, ldt, cl * J, zrow, J, c, lane);
                float v[MAXJ];
                if (half == 0) cols_to_lanes<0>(acc[tt], lane, v);
                else cols_to_lanes<8>(acc[tt], lane, v);
#pragma unroll
                for (int j = 0; j < MAXJ; ++j) v[j] = v[j] / fmaxf(sqrtf(__shfl(pn2, j, 64)), 1e-8f) * f;
                if (q == 0 && i < n) {
                    float best[2] = {0.f, 0.f};      // as cosine_mfma_kernel: first maximum wins
                    int bi[2] = {0, 0};
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j)
                        if (j < J) {
                            const bool fg = j < p;
                            const int first = fg ? 0 : p;
                            if (fg) {
                                if (j == first || v[j] > best[0]) { best[0] = v[j]; bi[0] = j; }
                            } else {
                                if (j == first || v[j] > best[1]) { best[1] = v[j]; bi[1] = j - p; }
                            }
                        }
                    const size_t slot = slot0 + cl;
                    pred[(slot * 2 + 0) * n + i] = best[1];
                    pred[(slot * 2 + 1) * n + i] = best[0];
                    if (resp) resp[slot * n + i] = (uint8_t)(best[0] > best[1] ? bi[0] + 3 : bi[1]);
                }
            }
        }
}

// MPM soft assignment on the same row stream (MODE 0 of assign_kernel): softmax_j(-|x - c_j|^2) within
// the fg and the bg group equals softmax_j(2 x.(c_j - m) - (|c_j|^2 - |m|^2)) for any m -- |x|^2 and m are common
// to a group and drop out -- so the MFMA accumulates x.dc_j (ctr = dc, bias: the centred centres and their bias left
// by centre_kernel, head_common.h) and the epilogue finishes 16 pixels on 16 lanes.
template <int NQ>
__global__ __launch_bounds__(256, PEMP_HEAD_OCC) void assign_mfma_kernel(const float* __restrict__ feat, int ldf,
                                                          const float* __restrict__ mask,
                                                          const float* __restrict__ ctr, const float* __restrict__ bias,
                                                          float* __restrict__ A,
                                                          int n, int h, int w, int H, int W, int c, int p) {
    extern __shared__ __attribute__((aligned(16))) float tab[];      // [(2p + 1)][c + 8]: centres, last row zeros | stages
    const int bs = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = 2 * p, ldt = c + 8;
    const int i0 = (blockIdx.x * 4 + wave) * 16;
    const int r = lane & 15, q = lane >> 4;
    float* stage = tab + (J + 1) * ldt + wave * 16 * SLD;
    float tv[TV];                                                    // table loads first (see cosine_mfma_kernel)
#pragma unroll
    for (int k = 0; k < TV; ++k) tv[k] = ctr[min((int)threadIdx.x + 256 * k, J * c - 1)];
    RowTile<NQ> rt;
    rt.init(feat + (size_t)bs * n * ldf, ldf, i0, n, lane);
#pragma unroll
    for (int k = 0; k < TV; ++k) {                                   // ctr is [c][2p]
        const int t = threadIdx.x + 256 * k;
        if (t < J * c) tab[(t % J) * ldt + t / J] = tv[k];
    }
    for (int ch = threadIdx.x; ch < c; ch += 256) tab[J * ldt + ch] = 0.f;
    __syncthreads();
    hv4f acc = {0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;
    rt.template run<false>(stage, tab + (size_t)min(r, J) * ldt + 4 * q, lane, acc, ss);
    float cn[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) cn[j] = bias[min(j, J - 1)];
    float v[MAXJ];
    rows_to_lanes(acc, lane, v);
    const int i = i0 + r;
    if (q == 0 && i < n) {
        const int y = i / w, x = i - y * w;
        const int sy = nearest_src(y, H, h), sx = nearest_src(x, W, w);
        const float* mk = mask + (size_t)bs * 2 * H * W;
        const float mg[2] = {mk[(size_t)sy * W + sx], mk[(size_t)H * W + (size_t)sy * W + sx]};
        float* out = A + ((size_t)bs * J) * n + i;
        float l[MAXJ], mx[2] = {-INFINITY, -INFINITY}, sm[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)            // static register indices throughout; group 0 = rows [0,p)
            if (j < J) {
                l[j] = 2.f * v[j] - cn[j];
                if (j < p) mx[0] = fmaxf(mx[0], l[j]);
                else mx[1] = fmaxf(mx[1], l[j]);
            }
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < J) {
                l[j] = expf(l[j] - (j < p ? mx[0] : mx[1]));
                if (j < p) sm[0] += l[j];
                else sm[1] += l[j];
            }
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < J) out[(size_t)j * n] = (l[j] / (j < p ? sm[0] : sm[1])) * (j < p ? mg[0] : mg[1]);
    }
}

// Masked pooling on the matrix cores: part[j][ch] = sum_i A[j][i] x[i][ch] over one chunk of PCHUNK pixels
// as D[16 rows j][16 ch] += A[j][4 px] * X[4 px][16 ch] (v_mfma_f32_16x16x4_f32, rows >= 2p read a zero row
// of the LDS weight table).  Lane (m = l&15, k = l>>4) reads float4 #m of pixel k's 64-channel slab -- a
// wave-wide load is 4 pixels x 256 contiguous bytes -- and feeds four MFMAs with four accumulators (channels
// 4m + e); wave v owns slabs v and v + 4, so a block covers c <= 512 channels and every row is read once.
// Four pixel-quads (8 KB per wave) are fetched per group, two groups in flight.
__global__ __launch_bounds__(256, PEMP_HEAD_OCC) void pool_mfma_kernel(const float* __restrict__ feat, int ldf,
                                                        const float* __restrict__ A, float* __restrict__ part,
                                                        float* __restrict__ asum, int n, int c, int J, int nchunks) {
    __shared__ float As[MAXJ + 1][PCHUNK];
    constexpr int QG = 2;                                            // pixel quads per prefetch group
    constexpr int NG = PCHUNK / (4 * QG);
    const int bs = blockIdx.y, ck = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    const int i0 = ck * PCHUNK;
    const int np = min(PCHUNK, n - i0);
    const int nslab = c / 64;
    const bool s0 = wave < nslab, s1 = wave + 4 < nslab;
    const float* xb = feat + (size_t)bs * n * ldf + 64 * wave + 4 * m;
    hv4f buf[2][QG][2];
    auto load = [&](int s, int g) {
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const float* xr = xb + (size_t)min(i0 + 4 * (g * QG + u) + k, n - 1) * ldf;
            if (s0) buf[s][u][0] = *(const hv4f*)xr;
            if (s1) buf[s][u][1] = *(const hv4f*)(xr + 256);
        }
    };
    load(0, 0);
    for (int t = threadIdx.x; t < (MAXJ + 1) * PCHUNK; t += 256) {
        const int j = t / PCHUNK, i = t - j * PCHUNK;
        As[j][i] = (j < J && i < np) ? A[((size_t)bs * J + j) * n + i0 + i] : 0.f;
    }
    __syncthreads();
    hv4f acc[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[s][e] = (hv4f){0.f, 0.f, 0.f, 0.f};
    const float* ap = &As[min(m, J)][k];
    auto mac = [&](int s, int g) {
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const float a = ap[4 * (g * QG + u)];
#pragma unroll
            for (int sl = 0; sl < 2; ++sl)
                if (sl == 0 ? s0 : s1) {
                    const hv4f xv = buf[s][u][sl];
                    acc[sl][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xv.x, acc[sl][0], 0, 0, 0);
                    acc[sl][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xv.y, acc[sl][1], 0, 0, 0);
                    acc[sl][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xv.z, acc[sl][2], 0, 0, 0);
                    acc[sl][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xv.w, acc[sl][3], 0, 0, 0);
                }
        }
    };
#pragma unroll
    for (int g = 0; g < NG; g += 2) {
        if (g + 1 < NG) load(1, g + 1);
        mac(0, g);
        if (g + 2 < NG) load(0, g + 2);
        if (g + 1 < NG) mac(1, g + 1);
    }
    // D[j][m]: lane (m, k) holds rows j = 4k + e' of channel 4m + e in acc[.][e][e']
    float* pb = part + ((size_t)bs * nchunks + ck) * J * c;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
        if (sl == 0 ? s0 : s1)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * k + e;
                if (j < J) {
                    const hv4f o = {acc[sl][0][e], acc[sl][1][e], acc[sl][2][e], acc[sl][3][e]};
                    *(hv4f*)(pb + (size_t)j * c + 64 * (wave + 4 * sl) + 4 * m) = o;
                }
            }
    if (threadIdx.x < J) {
        float s = 0.f;
        for (int i = 0; i < np; ++i) s += As[threadIdx.x][i];
        asum[((size_t)bs * nchunks + ck) * J + threadIdx.x] = s;
    }
}

#else
static inline bool mfma_rows_ok(int) { return false; }
static inline size_t proj_lds_bytes(int, int) { return 0; }
#endif
// -----------------------------------------------------------------------------------------------
// cosine map + group max, VALU variant (c not a multiple of 8, or PEMP_HEAD_VALU set): one wave per query pixel.
// torch>=2 F.cosine_similarity: each vector is divided by max(||.||, 1e-8), then dotted.
// qb: the query image's rows, pb: its [2p][c] prototypes, pred_b / resp_b: its output image (shared by the two kernels below)
__device__ __forceinline__ void cosine_pixels(const float* __restrict__ qb, int ldf, const float* __restrict__ pb,
                                              float* __restrict__ pred_b, uint8_t* __restrict__ resp_b, int n, int c, int p,
                                              float scalar) {
    __shared__ float pn[MAXJ][64 * MAXCL];
    __shared__ float nrm[MAXJ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = 2 * p;
    for (int j = wave; j < J; j += 4) {
        float s = 0.f;
        for (int ch = lane; ch < c; ch += 64) {
            float v = pb[(size_t)j * c + ch];
            s += v * v;
        }
        s = wave_sum(s);
        if (lane == 0) nrm[j] = fmaxf(sqrtf(s), 1e-8f);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < J * c; t += 256) {
        int j = t / c, ch = t - j * c;
        pn[j][ch] = pb[t] / nrm[j];
    }
    __syncthreads();
    const int ncl = (c + 255) / 256;
    for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const float* xp = qb + (size_t)i * ldf;
        float xv[MAXCL];
        float ss = 0.f;
#pragma unroll
        for (int t = 0; t < MAXCL / 4; ++t) {
            int ch = t * 256 + lane * 4;
            float4 v = (t < ncl && ch < c) ? *(const float4*)(xp + ch) : make_float4(0.f, 0.f, 0.f, 0.f);
            xv[t * 4 + 0] = v.x; xv[t * 4 + 1] = v.y; xv[t * 4 + 2] = v.z; xv[t * 4 + 3] = v.w;
            ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
        ss = wave_sum(ss);
        const float nx = fmaxf(sqrtf(ss), 1e-8f);
        float dot[MAXJ];
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) dot[j] = 0.f;
#pragma unroll
        for (int t = 0; t < MAXCL / 4; ++t) {
            int ch = t * 256 + lane * 4;
            if (t < ncl && ch < c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xn = xv[t * 4 + e] / nx;
#pragma unroll
                    for (int j = 0; j < MAXJ; ++j)
                        if (j < J) dot[j] += xn * pn[j][ch + e];
                }
            }
        }
        {
            wave_totals(dot, dot);
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) dot[j] = dot[j] * scalar;
        }
        if (lane == 0) {
            float best[2];
            int bi[2];
            for (int g = 0; g < 2; ++g) {  // g = 0: fg rows [0,p), g = 1: bg rows [p,2p)
                best[g] = dot[g * p];
                bi[g] = 0;
                for (int j = 1; j < p; ++j)
                    if (dot[g * p + j] > best[g]) {
                        best[g] = dot[g * p + j];
                        bi[g] = j;
                    }
            }
            pred_b[i] = best[1];                          // channel 0 = bg
            pred_b[(size_t)n + i] = best[0];              // channel 1 = fg
            if (resp_b) resp_b[i] = (uint8_t)(best[0] > best[1] ? bi[0] + 3 : bi[1]);
        }
    }
}
__global__ __launch_bounds__(256) void cosine_kernel(const float* __restrict__ qry, int ldf,
                                                     const float* __restrict__ protos, float* __restrict__ pred,
                                                     uint8_t* __restrict__ resp, int n, int c, int p, float scalar) {
    const int b = blockIdx.y;
    cosine_pixels(qry + (size_t)b * n * ldf, ldf, protos + (size_t)b * 2 * p * c, pred + (size_t)b * 2 * n,
                  resp ? resp + (size_t)b * n : nullptr, n, c, p, scalar);
}
// prototype bank, wave-per-pixel: block (x, b, k) is cosine_kernel's block (x, b) with protos = bank[k] (index: bank[index[b]])
__global__ __launch_bounds__(256) void cosine_bank_kernel(const float* __restrict__ qry, int ldf,
                                                          const float* __restrict__ bank, const int32_t* __restrict__ index,
                                                          float* __restrict__ pred, uint8_t* __restrict__ resp, int n, int c,
                                                          int p, int K, float scalar) {
    const int b = blockIdx.y;
    const int k = index ? min(max((int)index[b], 0), K - 1) : (int)blockIdx.z;
    const size_t slot = index ? (size_t)b : (size_t)b * K + k;
    cosine_pixels(qry + (size_t)b * n * ldf, ldf, bank + (size_t)k * 2 * p * c, pred + slot * 2 * n,
                  resp ? resp + slot * n : nullptr, n, c, p, scalar);
}

// masks[b][0][i] = [argmax_ch pred[b][.][i] == 1], masks[b][1][i] = [argmax == 0]  (channel 0 wins ties, as torch.argmax):
// the query masks of PANet's alignment branch (networks/panet.py:169-171)
__global__ void argmax_masks_kernel(const float* __restrict__ pred, float* __restrict__ masks, int B, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * n) return;
    const int b = t / n, i = t - b * n;
    const float fg = pred[((size_t)b * 2 + 1) * n + i] > pred[((size_t)b * 2 + 0) * n + i] ? 1.f : 0.f;
    masks[((size_t)b * 2 + 0) * n + i] = fg;
    masks[((size_t)b * 2 + 1) * n + i] = 1.f - fg;
}

// -----------------------------------------------------------------------------------------------
__global__ void upsample_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, int BC, int h, int w,
                                         int Ho, int Wo) {
    long long total = (long long)BC * Ho * Wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        int X = (int)(i % Wo);
        long long t = i / Wo;
        int Y = (int)(t % Ho);
        int bc = (int)(t / Ho);
        out[i] = bilerp(in + (size_t)bc * h * w, w, bilin_exact(Y, h, Ho), bilin_exact(X, w, Wo));
    }
}

__global__ void upsample_nearest_kernel(const uint8_t* __restrict__ in, int64_t* __restrict__ out, int B, int h,
                                        int w, int Ho, int Wo) {
    long long total = (long long)B * Ho * Wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        int X = (int)(i % Wo);
        long long t = i / Wo;
        int Y = (int)(t % Ho);
        int b = (int)(t / Ho);
        out[i] = in[((size_t)b * h + nearest_src(Y, h, Ho)) * w + nearest_src(X, w, Wo)];
    }
}

// The eight statistics of a 256-thread tail block, summed in a fixed order (butterfly per wave, then (w0 + w1) + (w2 + w3))
// -> out[8].  Every thread of the block must call.
__device__ __forceinline__ void tail_block_sums(const double (&v)[8], double* __restrict__ out) {
    __shared__ double red[4][8];
    for (int k = 0; k < 8; ++k) {
        double x = v[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        int k = threadIdx.x;
        out[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// What a tail thread adds up over its pixels: the CE sum, the weight sum, and valid, tp0, fp0, fn0, tp1, fp1, fn1.
struct TailAcc {
    double ce = 0.0, wsum = 0.0;
    int cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void count(int am, int t) {
        cnt[0]++;
        for (int j = 0; j < 2; ++j) {
            cnt[1 + 3 * j] += (am == j && t == j);
            cnt[2 + 3 * j] += (am == j && t != j);
            cnt[3 + 3 * j] += (am != j && t == j);
        }
    }
    __device__ __forceinline__ void rows(double (&v)[8]) const {
        v[0] = ce;
        for (int k = 0; k < 7; ++k) v[k + 1] = (double)cnt[k];
    }
};

// Pixel i of one image of the eval tail; the fixed-size and the ragged kernel both call it, so the arithmetic exists once.
// p0, p1: the image's two low-resolution planes; target, weight, pred_out, lg0, lg1: at the image's first pixel (or null).
__device__ __forceinline__ void eval_tail_pixel(const float* __restrict__ p0, const float* __restrict__ p1,
                                                const int64_t* __restrict__ target, const float* __restrict__ weight,
                                                uint8_t* __restrict__ pred_out, float* __restrict__ lg0, float* __restrict__ lg1,
                                                int i, int h, int w, int Ho, int Wo, TailAcc& a) {
    int Y = i / Wo, X = i - Y * Wo;
    Bilin by = bilin_exact(Y, h, Ho), bx = bilin_exact(X, w, Wo);
    float l0 = bilerp(p0, w, by, bx), l1 = bilerp(p1, w, by, bx);
    int am = l1 > l0 ? 1 : 0;
    pred_out[i] = (uint8_t)am;
    if (lg0) {
        lg0[i] = l0;
        lg1[i] = l1;
    }
    if (target) {
        int t = (int)target[i];
        // CELossDT (core/losses.py:33-43): per-pixel weights; the denominator sums the weight of EVERY
        // pixel, ignored ones included (their CE term is zero)
        const float wgt = weight ? weight[i] : 1.f;
        a.wsum += (double)wgt;
        if (t != 255) {
            a.ce += (double)(ce_pixel(l0, l1, t) * wgt);
            a.count(am, t);
        }
    }
}

// eval tail: upsample + argmax + CE partials + tp/fp/fn partials.  part[b][blk][8] doubles.
__global__ __launch_bounds__(256) void eval_tail_kernel(const float* __restrict__ pred,
                                                        const int64_t* __restrict__ target,
                                                        const float* __restrict__ weight,
                                                        uint8_t* __restrict__ pred_out, float* __restrict__ logits,
                                                        double* __restrict__ part, int h, int w, int Ho, int Wo) {
    const int b = blockIdx.y;
    const int npix = Ho * Wo;
    const size_t at = (size_t)b * npix;
    const float* p0 = pred + (size_t)b * 2 * h * w;
    TailAcc a;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        eval_tail_pixel(p0, p0 + h * w, target ? target + at : nullptr, weight ? weight + at : nullptr, pred_out + at,
                        logits ? logits + 2 * at : nullptr, logits ? logits + 2 * at + npix : nullptr, i, h, w, Ho, Wo, a);
    double v[8];
    a.rows(v);
    if (weight) v[1] = a.wsum;    // loss denominator: sum of weights instead of the valid-pixel count
    tail_block_sums(v, part + ((size_t)b * gridDim.x + blockIdx.x) * 8);
}

// Statistic k of one image: its nblk partial rows summed lane-strided, then a fixed butterfly -> deterministic
__device__ __forceinline__ double tail_final_sum(const double* __restrict__ rows, int nblk, int k, int lane) {
    double s = 0.0;
    for (int i = lane; i < nblk; i += 64) s += rows[(size_t)i * 8 + k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
// one wave per (episode, statistic)
__global__ void eval_tail_final_kernel(const double* __restrict__ part, double* __restrict__ stats, int nblk) {
    const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const double s = tail_final_sum(part + (size_t)b * nblk * 8, nblk, k, lane);
    if (lane == 0) stats[b * 8 + k] = s;
}

static inline int tail_blocks(int Ho, int Wo) {
    int nb = cdiv(Ho * Wo, 256 * 4);
    return nb < 1 ? 1 : (nb > 256 ? 256 : nb);
}

// The N-way decision of pixel i, the one place the rule exists (the label tails and the confusion tails call it): the
// upsample of the K plane pairs pn, the claim test l1 > l0, the margin __fsub_rn(l1, l0) and the strict > that lets the lowest k
// win equal margins.  -> the label (0: nobody claims, else 1 + k); bm: the winner's margin, top: the largest margin of all
// classes, w0 / w1: class wk's own logits (wk = -1: left at 0).  What a caller does not read costs nothing after inlining.
__device__ __forceinline__ int nway_decide(const float* __restrict__ pn, int wk, int i, int K, int h, int w, int Ho, int Wo,
                                           float& bm, float& top, float& w0, float& w1) {
    const int hw = h * w;
    int Y = i / Wo, X = i - Y * Wo;
    Bilin by = bilin_exact(Y, h, Ho), bx = bilin_exact(X, w, Wo);
    int best = 0;                               // the label so far
    bm = 0.f, top = -INFINITY;                  // its margin; the largest margin of all classes
    w0 = 0.f, w1 = 0.f;                         // the wanted class's own logits
    const float* p = pn;
    for (int k = 0; k < K; ++k, p += 2 * hw) {
        float l0 = bilerp(p, w, by, bx), l1 = bilerp(p + hw, w, by, bx);
        float m = __fsub_rn(l1, l0);
        if (l1 > l0 && (best == 0 || m > bm)) {
            best = k + 1;
            bm = m;
        }
        if (m > top) top = m;
        if (k == wk) {
            w0 = l0;
            w1 = l1;
        }
    }
    return best;
}

// Pixel i of one image of the N-way tail, shared like eval_tail_pixel.  pn: the image's K plane pairs; wk: the wanted class
// (-1 without a target); target, labels, margin: at the image's first pixel (or null).
__device__ __forceinline__ void nway_tail_pixel(const float* __restrict__ pn, const int64_t* __restrict__ target, int wk,
                                                uint8_t* __restrict__ labels, float* __restrict__ margin, int i, int K, int h,
                                                int w, int Ho, int Wo, TailAcc& a) {
    float bm, top, w0, w1;
    const int best = nway_decide(pn, wk, i, K, h, w, Ho, Wo, bm, top, w0, w1);
    labels[i] = (uint8_t)best;
    if (margin) margin[i] = best ? bm : top;
    if (target) {
        int t = (int)target[i];
        if (t != 255) {
            a.ce += (double)ce_pixel(w0, w1, t);
            a.count(best == wk + 1 ? 1 : 0, t);
        }
    }
}

// N-way tail: the K binary maps of an all-classes bank call pred[n][k][2][h][w] fused into one label map.  Per output pixel the
// interpolation indices and weights are formed once and serve all 2K planes (~10 KB each, L2-resident); k walks upward.
// Class k claims the pixel iff U1 > U0 (eval_tail's comparison), the claiming class with the largest margin
// __fsub_rn(U1, U0) owns it (strict >: the lowest k wins equal margins), label = 1 + k or 0 when nobody claims;
// margin = the winner's, or the largest (<= 0) margin where nobody claims.  With a target: part[n][blk][8] doubles in
// eval_tail's layout -- the CE of class want[n]'s own logits, tp/fp/fn of the image (label == want[n] + 1).
__global__ __launch_bounds__(256) void nway_tail_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                        const int32_t* __restrict__ want, uint8_t* __restrict__ labels,
                                                        float* __restrict__ margin, double* __restrict__ part, int K, int h,
                                                        int w, int Ho, int Wo) {
    const int n = blockIdx.y;
    const int npix = Ho * Wo;
    const size_t at = (size_t)n * npix;
    const float* pn = pred + (size_t)n * K * 2 * h * w;
    const int wk = target ? want[n] : -1;
    TailAcc a;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256)
        nway_tail_pixel(pn, target ? target + at : nullptr, wk, labels + at, margin ? margin + at : nullptr, i, K, h, w, Ho, Wo,
                        a);
    if (!target) return;                            // uniform over the grid: no statistics asked for
    double v[8];
    a.rows(v);
    tail_block_sums(v, part + ((size_t)n * gridDim.x + blockIdx.x) * 8);
}

// Ragged tails: image b has its own output size, items[b] (pemp_tail_item, planned by pemp_tail_ragged_workspace_bytes).  Grid
// (max nblk, B): image b is walked by its first nblk_b blocks exactly as the fixed-size kernel walks it alone -- pixel
// blk * 256 + tid, stride nblk_b * 256, the same pixel body, tail_block_sums, the same final sum -- so its results are the
// fixed-size tail's bit for bit; the other blocks of the row leave at once.  The descriptor read is uniform per block and the
// kernels only read it.  target, labels and margin are packed end to end: image b starts at element pix_off.
__global__ __launch_bounds__(256) void eval_tail_ragged_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                               const pemp_tail_item* __restrict__ items,
                                                               uint8_t* __restrict__ pred_out, double* __restrict__ part, int h,
                                                               int w) {
    const int b = blockIdx.y;
    const pemp_tail_item it = items[b];
    if ((int)blockIdx.x >= it.nblk) return;
    const int npix = it.Ho * it.Wo;
    const float* p0 = pred + (size_t)b * 2 * h * w;
    TailAcc a;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += it.nblk * 256)
        eval_tail_pixel(p0, p0 + h * w, target ? target + it.pix_off : nullptr, nullptr, pred_out + it.pix_off, nullptr, nullptr,
                        i, h, w, it.Ho, it.Wo, a);
    if (!target) return;
    double v[8];
    a.rows(v);
    tail_block_sums(v, part + ((size_t)it.part_off + blockIdx.x) * 8);
}

// (8 waves per SIMD asked for: left alone the descriptor's fields took the kernel to 70 VGPRs and 7 waves, 7 % slower than
// nway_tail_kernel's 8 on equal sizes; both are at 58 VGPRs since the decision moved into nway_decide)
__global__ __launch_bounds__(256, 8) void nway_tail_ragged_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                               const int32_t* __restrict__ want,
                                                               const pemp_tail_item* __restrict__ items,
                                                               uint8_t* __restrict__ labels, float* __restrict__ margin,
                                                               double* __restrict__ part, int K, int h, int w) {
    const int n = blockIdx.y;
    const pemp_tail_item it = items[n];
    if ((int)blockIdx.x >= it.nblk) return;
    const int npix = it.Ho * it.Wo;
    const float* pn = pred + (size_t)n * K * 2 * h * w;
    const int wk = target ? want[n] : -1;
    TailAcc a;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += it.nblk * 256)
        nway_tail_pixel(pn, target ? target + it.pix_off : nullptr, wk, labels + it.pix_off,
                        margin ? margin + it.pix_off : nullptr, i, K, h, w, it.Ho, it.Wo, a);
    if (!target) return;
    double v[8];
    a.rows(v);
    tail_block_sums(v, part + ((size_t)it.part_off + blockIdx.x) * 8);
}

// one wave per (image, statistic), over the image's own nblk partial rows
__global__ void tail_final_ragged_kernel(const double* __restrict__ part, const pemp_tail_item* __restrict__ items,
                                         double* __restrict__ stats) {
    const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const pemp_tail_item it = items[b];
    const double s = tail_final_sum(part + (size_t)it.part_off * 8, it.nblk, k, lane);
    if (lane == 0) stats[b * 8 + k] = s;
}

// N-way confusion tail: the label of nway_decide counted against a target, conf[t][p] of one image ([K+1][K+1] int64, zeroed
// by the entry) += the block's pixels.  Block blk of nblk walks the image as the label tails do.  hist: (K+1)^2 uint32 in LDS
// (at most 4096 bins = 16 KB).  On real data most pixels are background predicted as background, and 64 lanes adding to one LDS
// address serialise: bin (0,0) is counted in a register per thread and folded in by a wave butterfly, only the other bins go
// through LDS integer atomics.  The block's non-zero bins then go to conf with 64-bit integer atomic adds: integer sums are
// exact in any order, so the table does not depend on the grid, the batch or the run.  lifted: target is the binary mask
// 0 / 1 / 255 of class slot `want` (1 -> want + 1); otherwise it holds slot labels 0..K.  Every other value is ignored before it
// can index the table.
constexpr int CONF_MAX_K = 63;

__device__ __forceinline__ void nway_confusion_image(const float* __restrict__ pn, const int64_t* __restrict__ target,
                                                     bool lifted, int want, uint8_t* __restrict__ labels,
                                                     unsigned long long* __restrict__ conf, uint32_t* hist, int blk, int nblk,
                                                     int K, int h, int w, int Ho, int Wo) {
    const int C = K + 1, bins = C * C, tid = threadIdx.x, npix = Ho * Wo;
    for (int b = tid; b < bins; b += 256) hist[b] = 0;
    __syncthreads();
    uint32_t c00 = 0;
    for (int i = blk * 256 + tid; i < npix; i += nblk * 256) {
        float bm, top, w0, w1;
        const int best = nway_decide(pn, -1, i, K, h, w, Ho, Wo, bm, top, w0, w1);
        if (labels) labels[i] = (uint8_t)best;
        int64_t t = target[i];
        if (lifted) t = t == 1 ? (int64_t)want + 1 : (t == 0 ? 0 : -1);
        if (t >= 0 && t <= K) {
            const int bin = (int)t * C + best;
            if (bin == 0)
                ++c00;
            else
                atomicAdd(&hist[bin], 1u);
        }
    }
    for (int o = 32; o > 0; o >>= 1) c00 += __shfl_xor(c00, o, 64);
    if ((tid & 63) == 0 && c00) atomicAdd(&hist[0], c00);
    __syncthreads();
    for (int b = tid; b < bins; b += 256) {
        const uint32_t v = hist[b];
        if (v) atomicAdd(conf + b, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256, 8) void nway_confusion_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                                const int32_t* __restrict__ want, uint8_t* __restrict__ labels,
                                                                unsigned long long* __restrict__ conf, int K, int h, int w,
                                                                int Ho, int Wo) {
    extern __shared__ uint32_t conf_hist[];
    const int n = blockIdx.y;
    const size_t at = (size_t)n * Ho * Wo;
    nway_confusion_image(pred + (size_t)n * K * 2 * h * w, target + at, want != nullptr, want ? want[n] : 0,
                         labels ? labels + at : nullptr, conf + (size_t)n * (K + 1) * (K + 1), conf_hist, blockIdx.x, gridDim.x,
                         K, h, w, Ho, Wo);
}

// the ragged walk of nway_tail_ragged_kernel: image n's first nblk blocks, target and labels packed
__global__ __launch_bounds__(256, 8) void nway_confusion_ragged_kernel(const float* __restrict__ pred,
                                                                       const int64_t* __restrict__ target,
                                                                       const int32_t* __restrict__ want,
                                                                       const pemp_tail_item* __restrict__ items,
                                                                       uint8_t* __restrict__ labels,
                                                                       unsigned long long* __restrict__ conf, int K, int h,
                                                                       int w) {
    extern __shared__ uint32_t conf_hist[];
    const int n = blockIdx.y;
    const pemp_tail_item it = items[n];
    if ((int)blockIdx.x >= it.nblk) return;
    nway_confusion_image(pred + (size_t)n * K * 2 * h * w, target + it.pix_off, want != nullptr, want ? want[n] : 0,
                         labels ? labels + it.pix_off : nullptr, conf + (size_t)n * (K + 1) * (K + 1), conf_hist, blockIdx.x,
                         it.nblk, K, h, w, it.Ho, it.Wo);
}

}  // namespace PEMP_HEAD_NS
}  // namespace pemp

namespace pemp {
namespace PEMP_HEAD_NS {

// workspace layout for pooling: A[BS][J][n] | part[BS][nchunks][J][c] | asum[BS][nchunks][J] | msum[BS][2]
static size_t pool_ws_bytes(int BS, int n, int c, int J) { return pool_ws_floats(BS, n, c, J) * sizeof(float); }

static size_t pemp_mpm_workspace_bytes(int B, int S, int n, int c, int p) {
    return pool_ws_bytes(B * S, n, c, 2 * p);
}
static size_t pemp_map_workspace_bytes(int B, int S, int n, int c) { return pool_ws_bytes(B * S, n, c, 2); }

static int pooled_protos(int mode, const float* feat, int ldf, const float* mask, const float* ctr, float* protos,
                         void* ws, size_t ws_bytes, int B, int S, int h, int w, int H, int W, int c, int p,
                         hipStream_t st) {
    const int BS = B * S, n = h * w;
    const int J = mode == 0 ? 2 * p : 2;
    PEMP_REQUIRE(feat && mask && protos && ws, "protos: null pointer");
    PEMP_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && H > 0 && W > 0, "protos: bad dims");
    PEMP_REQUIRE(c > 0 && c % 4 == 0 && c <= 64 * MAXCL && ldf >= c && ldf % 4 == 0, "protos: c=%d must be a multiple of 4 and <= %d", c, 64 * MAXCL);
    PEMP_REQUIRE(J >= 2 && J <= MAXJ, "protos: 2p=%d not in 2..%d", J, MAXJ);
    PEMP_REQUIRE(ws_bytes >= pool_ws_bytes(BS, n, c, J), "protos: workspace too small");
    PEMP_REQUIRE(((uintptr_t)feat & 15) == 0, "protos: feat must be 16-byte aligned");
    const int nck = nchunks_of(n);
    const PoolWs L = pool_ws_layout(ws, BS, n, c, J);
    static const bool force_valu = getenv("PEMP_HEAD_VALU") != nullptr;       // A/B switch for measurements
    float *A = L.A, *part = L.part, *asum = L.asum, *msum = L.msum;
    // few, long-lived blocks: every block first loads its lanes' slice of ctr (48 values per lane)
    const int ablk = min(cdiv(n, 4), max(1, 512 / BS));
    if (mode == 0) {
        PEMP_REQUIRE(ctr, "protos: ctr is null");
        hipLaunchKernelGGL(centre_kernel<MAXJ>, dim3(1), dim3(256), 0, st, ctr, L.dc, L.cm, L.bias, c, p);
#if PEMP_MAXJ == 8
        if (mfma_rows_ok(c) && !force_valu) {
            const dim3 grid(cdiv(cdiv(n, 16), 4), BS);
#define PEMP_ASG(NQ)                                                                                                  \
    hipLaunchKernelGGL(assign_mfma_kernel<NQ>, grid, dim3(256), proj_lds_bytes(J, c), st, feat, ldf, mask, (const float*)L.dc, \
                       (const float*)L.bias, A, n, h, w, H, W, c, p)
            if (c == 512) PEMP_ASG(8);
            else if (c == 256) PEMP_ASG(4);
            else if (c == 128) PEMP_ASG(2);
            else PEMP_ASG(1);
#undef PEMP_ASG
        }
        else
#endif
            hipLaunchKernelGGL(assign_kernel<0>, dim3(ablk, BS), dim3(256), 0, st, feat, ldf, mask, (const float*)L.dc,
                               (const float*)L.bias, A, n, h, w, H, W, c, p);
    } else if (mode == 1) {
        hipLaunchKernelGGL(mask_assign_kernel, dim3(cdiv(n, 256), BS), dim3(256), 0, st, mask, A, n, h, w, H, W);
    } else {
        hipLaunchKernelGGL(adjoint_mask_kernel, dim3(cdiv(2 * n, 256), BS), dim3(256), 0, st, mask, A, n, h, w, H, W);
        hipLaunchKernelGGL(mask_sum_kernel, dim3(BS * 2), dim3(1024), 0, st, mask, msum, H * W);
    }
    int e = launch_status("protos/assign");
    if (e) return e;
#if PEMP_MAXJ == 8
    if (c % 64 == 0 && !force_valu)
        hipLaunchKernelGGL(pool_mfma_kernel, dim3(nck, BS), dim3(256), 0, st, feat, ldf, A, part, asum, n, c, J, nck);
    else
#endif
        hipLaunchKernelGGL(pool_partial_kernel, dim3(nck, BS), dim3(256), 0, st, feat, ldf, A, part, asum, n, c, J, nck);
    hipLaunchKernelGGL(pool_final_kernel, dim3(J, B, cdiv(c, 64)), dim3(256), 0, st, part, asum, mode == 2 ? msum : (const float*)nullptr,
                       protos, S, c, J, nck, mode == 0 ? 1e-6f : 1e-5f);
    return launch_status("protos/pool");
}

static int pemp_mpm_protos_f32(const float* feat, int ldf, const float* mask, const float* ctr, float* protos,
                                   void* ws, size_t ws_bytes, int B, int S, int h, int w, int H, int W, int c, int p,
                                   void* stream) {
    PEMP_REQUIRE(p >= 1 && p <= MAXJ / 2, "mpm_protos: p=%d not in 1..%d", p, MAXJ / 2);
    return pooled_protos(0, feat, ldf, mask, ctr, protos, ws, ws_bytes, B, S, h, w, H, W, c, p, (hipStream_t)stream);
}

static int pemp_masked_avg_pool_f32(const float* feat, int ldf, const float* mask, float* protos, void* ws,
                                        size_t ws_bytes, int B, int S, int h, int w, int H, int W, int c, int full_res,
                                        void* stream) {
    return pooled_protos(full_res ? 2 : 1, feat, ldf, mask, nullptr, protos, ws, ws_bytes, B, S, h, w, H, W, c, 1,
                         (hipStream_t)stream);
}

static int pemp_cosine_proto_max_f32(const float* qry, int ldf, const float* protos, float* pred, uint8_t* resp,
                                         int B, int n, int c, int p, float dist_scalar, void* stream) {
    PEMP_REQUIRE(qry && protos && pred, "cosine: null pointer");
    PEMP_REQUIRE(B > 0 && n > 0 && p >= 1 && 2 * p <= MAXJ, "cosine: bad dims");
    PEMP_REQUIRE(c > 0 && c % 4 == 0 && c <= 64 * MAXCL && ldf >= c && ldf % 4 == 0, "cosine: c=%d must be a multiple of 4 and <= %d", c, 64 * MAXCL);
    PEMP_REQUIRE(((uintptr_t)qry & 15) == 0, "cosine: qry must be 16-byte aligned");
    static const bool force_valu = getenv("PEMP_HEAD_VALU") != nullptr;     // A/B switch for measurements
#if PEMP_MAXJ == 8
    if (mfma_rows_ok(c) && !force_valu) {
        // MFMA outer product: 16 query pixels x (2p prototypes padded to 16 columns) per wave
        const size_t lds = proj_lds_bytes(2 * p, c);
        const dim3 grid(cdiv(cdiv(n, 16), 4), B);
#define PEMP_COS(NQ)                                                                                                  \
    hipLaunchKernelGGL(cosine_mfma_kernel<NQ>, grid, dim3(256), lds, (hipStream_t)stream, qry, ldf, protos, pred, resp, n, c, \
                       p, dist_scalar)
        if (c == 512) PEMP_COS(8);
        else if (c == 256) PEMP_COS(4);
        else if (c == 128) PEMP_COS(2);
        else PEMP_COS(1);
#undef PEMP_COS
        return launch_status("cosine_mfma");
    }
#endif
    hipLaunchKernelGGL(cosine_kernel, dim3(min(cdiv(n, 4), max(1, 4096 / B)), B), dim3(256), 0, (hipStream_t)stream, qry, ldf, protos,
                       pred, resp, n, c, p, dist_scalar);
    return launch_status("cosine");
}

static int pemp_cosine_bank_max_f32(const float* qry, int ldf, const float* bank, const int32_t* index, float* pred,
                                    uint8_t* resp, int N, int K, int n, int c, int p, float dist_scalar, void* stream) {
    PEMP_REQUIRE(qry && bank && pred, "cosine_bank: null pointer");
    PEMP_REQUIRE(N > 0 && K > 0 && n > 0 && p >= 1 && 2 * p <= MAXJ, "cosine_bank: bad dims");
    PEMP_REQUIRE(N <= 65535 && K <= 65535, "cosine_bank: N=%d, K=%d must be <= 65535", N, K);
    PEMP_REQUIRE(c > 0 && c % 4 == 0 && c <= 64 * MAXCL && ldf >= c && ldf % 4 == 0, "cosine_bank: c=%d must be a multiple of 4 and <= %d", c, 64 * MAXCL);
    PEMP_REQUIRE(((uintptr_t)qry & 15) == 0 && ((uintptr_t)bank & 15) == 0, "cosine_bank: qry and bank must be 16-byte aligned");
    static const bool force_valu = getenv("PEMP_HEAD_VALU") != nullptr;     // A/B switch for measurements
    const hipStream_t st = (hipStream_t)stream;
#if PEMP_MAXJ == 8
    if (mfma_rows_ok(c) && !force_valu) {
        // tiles per block: all K classes in one pass over the query rows up to 8 classes (4 tiles, <= 153 KB of LDS);
        // PEMP_BANK_TILES=1..4 caps it (A/B switch for measurements)
        static const int cap_t = getenv("PEMP_BANK_TILES") ? atoi(getenv("PEMP_BANK_TILES")) : 4;
        const int T = index ? 1 : min(cdiv(K, 2), max(1, min(cap_t, 4)));
        const size_t lds = bank_lds_bytes(bank_ncap(index != nullptr, T, K), 2 * p, c);
        const dim3 grid(cdiv(cdiv(n, 16), 4), N, index ? 1 : cdiv(K, 2 * T));
#define PEMP_BANK(NQ, TT)                                                                                             \
    do {                                                                                                              \
        if (lds > 64 * 1024) {                                                                                        \
            hipError_t e = hipFuncSetAttribute((const void*)cosine_bank_mfma_kernel<NQ, TT>,                          \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                 \
            if (e != hipSuccess) {                                                                                    \
                set_error("cosine_bank: hipFuncSetAttribute(lds=%zu): %s", lds, hipGetErrorString(e));                \
                return (int)e;                                                                                        \
            }                                                                                                         \
        }                                                                                                             \
        hipLaunchKernelGGL((cosine_bank_mfma_kernel<NQ, TT>), grid, dim3(256), lds, st, qry, ldf, bank, index, pred, resp, n, \
                           c, p, K, dist_scalar);                                                                     \
    } while (0)
#define PEMP_BANK_T(NQ)                                                                                               \
    do {                                                                                                              \
        if (T == 1) PEMP_BANK(NQ, 1);                                                                                 \
        else if (T == 2) PEMP_BANK(NQ, 2);                                                                            \
        else if (T == 3) PEMP_BANK(NQ, 3);                                                                            \
        else PEMP_BANK(NQ, 4);                                                                                        \
    } while (0)
        if (c == 512) PEMP_BANK_T(8);
        else if (c == 256) PEMP_BANK_T(4);
        else if (c == 128) PEMP_BANK_T(2);
        else PEMP_BANK_T(1);
#undef PEMP_BANK_T
#undef PEMP_BANK
        return launch_status("cosine_bank_mfma");
    }
#endif
    hipLaunchKernelGGL(cosine_bank_kernel, dim3(min(cdiv(n, 4), max(1, 4096 / N)), N, index ? 1 : K), dim3(256), 0, st, qry, ldf,
                       bank, index, pred, resp, n, c, p, K, dist_scalar);
    return launch_status("cosine_bank");
}

static int pemp_argmax_masks_f32(const float* pred, float* masks, int B, int n, void* stream) {
    PEMP_REQUIRE(pred && masks && B > 0 && n > 0, "argmax_masks: bad arguments");
    hipLaunchKernelGGL(argmax_masks_kernel, dim3(cdiv(B * n, 256)), dim3(256), 0, (hipStream_t)stream, pred, masks, B, n);
    return launch_status("argmax_masks");
}

static int pemp_upsample_bilinear_ac_f32(const float* pred, float* out, int B, int C, int h, int w, int Ho, int Wo,
                                             void* stream) {
    PEMP_REQUIRE(pred && out && B > 0 && C > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0, "upsample: bad arguments");
    long long total = (long long)B * C * Ho * Wo;
    int grid = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(upsample_bilinear_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, out, B * C, h, w, Ho, Wo);
    return launch_status("upsample_bilinear");
}

static int pemp_upsample_nearest_u8_i64(const uint8_t* resp, int64_t* out, int B, int h, int w, int Ho, int Wo,
                                            void* stream) {
    PEMP_REQUIRE(resp && out && B > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0, "upsample_nearest: bad arguments");
    long long total = (long long)B * Ho * Wo;
    int grid = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(upsample_nearest_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, resp, out, B, h, w, Ho, Wo);
    return launch_status("upsample_nearest");
}

static size_t pemp_eval_tail_workspace_bytes(int B, int Ho, int Wo) {
    return (size_t)B * tail_blocks(Ho, Wo) * 8 * sizeof(double);
}

static int pemp_eval_tail_weighted_f32(const float* pred, const int64_t* target, const float* weight,
                                           uint8_t* pred_out, float* logits_out, double* stats, void* ws,
                                           size_t ws_bytes, int B, int h, int w, int Ho, int Wo, void* stream);

static int pemp_eval_tail_f32(const float* pred, const int64_t* target, uint8_t* pred_out, float* logits_out,
                                  double* stats, void* ws, size_t ws_bytes, int B, int h, int w, int Ho, int Wo,
                                  void* stream) {
    return pemp_eval_tail_weighted_f32(pred, target, nullptr, pred_out, logits_out, stats, ws, ws_bytes, B, h, w, Ho, Wo,
                                       stream);
}

static int pemp_eval_tail_weighted_f32(const float* pred, const int64_t* target, const float* weight,
                                           uint8_t* pred_out, float* logits_out, double* stats, void* ws,
                                           size_t ws_bytes, int B, int h, int w, int Ho, int Wo, void* stream) {
    PEMP_REQUIRE(pred && pred_out && stats && ws, "eval_tail: null pointer");
    PEMP_REQUIRE(!weight || target, "eval_tail: weight without target");
    PEMP_REQUIRE(B > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0, "eval_tail: bad dims");
    PEMP_REQUIRE(ws_bytes >= pemp_eval_tail_workspace_bytes(B, Ho, Wo), "eval_tail: workspace too small");
    const int nb = tail_blocks(Ho, Wo);
    hipLaunchKernelGGL(eval_tail_kernel, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, pred, target, weight, pred_out,
                       logits_out, (double*)ws, h, w, Ho, Wo);
    hipLaunchKernelGGL(eval_tail_final_kernel, dim3(B, 8), dim3(64), 0, (hipStream_t)stream, (const double*)ws, stats, nb);
    return launch_status("eval_tail");
}

static size_t pemp_nway_tail_workspace_bytes(int N, int Ho, int Wo) { return pemp_eval_tail_workspace_bytes(N, Ho, Wo); }

static int pemp_nway_tail_f32(const float* pred, const int64_t* target, const int32_t* want, uint8_t* labels, float* margin,
                              double* stats, void* ws, size_t ws_bytes, int N, int K, int h, int w, int Ho, int Wo,
                              void* stream) {
    PEMP_REQUIRE(pred && labels && ws, "nway_tail: null pointer");
    PEMP_REQUIRE((target != nullptr) == (want != nullptr) && (target != nullptr) == (stats != nullptr),
                 "nway_tail: target, want and stats come together");
    PEMP_REQUIRE(N > 0 && N <= 65535 && K > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0 && (long long)Ho * Wo < (1LL << 31) &&
                     (long long)h * w < (1LL << 29),
                 "nway_tail: bad dims");
    PEMP_REQUIRE(K <= 255, "nway_tail: K <= 255 (the labels are uint8, 0 = no class)");
    PEMP_REQUIRE(ws_bytes >= pemp_nway_tail_workspace_bytes(N, Ho, Wo), "nway_tail: workspace too small");
    const int nb = tail_blocks(Ho, Wo);
    hipLaunchKernelGGL(nway_tail_kernel, dim3(nb, N), dim3(256), 0, (hipStream_t)stream, pred, target, want, labels, margin,
                       (double*)ws, K, h, w, Ho, Wo);
    if (stats)
        hipLaunchKernelGGL(eval_tail_final_kernel, dim3(N, 8), dim3(64), 0, (hipStream_t)stream, (const double*)ws, stats, nb);
    return launch_status("nway_tail");
}

// Ragged tails: the planner (host only) and the two launches.  A pixel count stays below 2^31 - 2^16, so that the walk's
// index cannot wrap when the last stride (at most 256 * 256) is added.
static inline bool tail_item_ok(const pemp_tail_item& it) {
    return it.Ho >= 1 && it.Wo >= 1 && (long long)it.Ho * it.Wo < (1LL << 31) - (1LL << 16);
}

static size_t pemp_tail_ragged_workspace_bytes(pemp_tail_item* items, int n) {
    if (!items || n < 1 || n > 65535) {
        set_error("tail_ragged: bad arguments (items %p, n = %d; 1 <= n <= 65535)", (void*)items, n);
        return 0;
    }
    long long pix = 0, blk = 0;
    for (int i = 0; i < n; ++i) {
        pemp_tail_item& it = items[i];
        if (!tail_item_ok(it)) {
            set_error("tail_ragged: item %d has the size %d x %d", i, it.Ho, it.Wo);
            return 0;
        }
        it.nblk = tail_blocks(it.Ho, it.Wo);
        it.part_off = (int32_t)blk;
        it.pix_off = pix;
        blk += it.nblk;
        pix += (long long)it.Ho * it.Wo;
    }
    return (size_t)blk * 8 * sizeof(double);
}

// The host copy of the descriptors checked against the plan -> the widest image's block count (the grid's x), or -1.
static int tail_ragged_check(const char* what, const pemp_tail_item* items, int n, size_t ws_bytes) {
    long long pix = 0, blk = 0;
    int widest = 0;
    for (int i = 0; i < n; ++i)
        PEMP_REQUIRE(tail_item_ok(items[i]), "%s: item %d has the size %d x %d", what, i, items[i].Ho, items[i].Wo);
    for (int i = 0; i < n; ++i) {
        const pemp_tail_item& it = items[i];
        PEMP_REQUIRE(it.nblk == tail_blocks(it.Ho, it.Wo) && it.part_off == blk && it.pix_off == pix,
                     "%s: item %d was not planned (pemp_tail_ragged_workspace_bytes)", what, i);
        blk += it.nblk;
        pix += (long long)it.Ho * it.Wo;
        widest = widest > it.nblk ? widest : it.nblk;
    }
    PEMP_REQUIRE(ws_bytes >= (size_t)blk * 8 * sizeof(double), "%s: workspace too small", what);
    return widest;
}

static int pemp_eval_tail_ragged_f32(const float* pred, const int64_t* target, const pemp_tail_item* items_host,
                                     const pemp_tail_item* items_dev, int B, int h, int w, uint8_t* pred_out, double* stats,
                                     void* ws, size_t ws_bytes, void* stream) {
    PEMP_REQUIRE(pred && items_host && items_dev && pred_out && ws, "eval_tail_ragged: null pointer");
    PEMP_REQUIRE((target != nullptr) == (stats != nullptr), "eval_tail_ragged: target and stats come together");
    PEMP_REQUIRE(B >= 1 && B <= 65535 && h > 0 && w > 0 && (long long)h * w < (1LL << 29), "eval_tail_ragged: bad dims");
    const int nb = tail_ragged_check("eval_tail_ragged", items_host, B, ws_bytes);
    if (nb < 0) return -1;
    hipLaunchKernelGGL(eval_tail_ragged_kernel, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, pred, target, items_dev,
                       pred_out, (double*)ws, h, w);
    if (stats)
        hipLaunchKernelGGL(tail_final_ragged_kernel, dim3(B, 8), dim3(64), 0, (hipStream_t)stream, (const double*)ws, items_dev,
                           stats);
    return launch_status("eval_tail_ragged");
}

static int pemp_nway_tail_ragged_f32(const float* pred, const int64_t* target, const int32_t* want,
                                     const pemp_tail_item* items_host, const pemp_tail_item* items_dev, int N, int K, int h,
                                     int w, uint8_t* labels, float* margin, double* stats, void* ws, size_t ws_bytes,
                                     void* stream) {
    PEMP_REQUIRE(pred && items_host && items_dev && labels && ws, "nway_tail_ragged: null pointer");
    PEMP_REQUIRE((target != nullptr) == (want != nullptr) && (target != nullptr) == (stats != nullptr),
                 "nway_tail_ragged: target, want and stats come together");
    PEMP_REQUIRE(N >= 1 && N <= 65535 && K > 0 && h > 0 && w > 0 && (long long)h * w < (1LL << 29),
                 "nway_tail_ragged: bad dims");
    PEMP_REQUIRE(K <= 255, "nway_tail_ragged: K <= 255 (the labels are uint8, 0 = no class)");
    const int nb = tail_ragged_check("nway_tail_ragged", items_host, N, ws_bytes);
    if (nb < 0) return -1;
    hipLaunchKernelGGL(nway_tail_ragged_kernel, dim3(nb, N), dim3(256), 0, (hipStream_t)stream, pred, target, want, items_dev,
                       labels, margin, (double*)ws, K, h, w);
    if (stats)
        hipLaunchKernelGGL(tail_final_ragged_kernel, dim3(N, 8), dim3(64), 0, (hipStream_t)stream, (const double*)ws, items_dev,
                           stats);
    return launch_status("nway_tail_ragged");
}

// N-way confusion tails.  The blocks flush into conf with global integer atomics after a memset (no partial tables: at K = 63
// those would be 4096 bins x 256 blocks x 8 B = 8 MB per image), so neither form needs a workspace: the planner returns 0 and
// ws / ws_bytes are accepted and left alone.
static size_t pemp_nway_confusion_workspace_bytes(int N, int K, int Ho, int Wo) {
    (void)N, (void)K, (void)Ho, (void)Wo;
    return 0;
}

static int nway_confusion_clear(int64_t* conf, int N, int K, hipStream_t st, const char* what) {
    const hipError_t e = hipMemsetAsync(conf, 0, (size_t)N * (K + 1) * (K + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) {
        set_error("%s: clearing conf: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

static int pemp_nway_confusion_f32(const float* pred, const int64_t* target, const int32_t* want, uint8_t* labels, int64_t* conf,
                                   void* ws, size_t ws_bytes, int N, int K, int h, int w, int Ho, int Wo, void* stream) {
    (void)ws, (void)ws_bytes;
    PEMP_REQUIRE(pred && target && conf, "nway_confusion: null pointer");
    PEMP_REQUIRE(N > 0 && N <= 65535 && K > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0 &&
                     (long long)Ho * Wo < (1LL << 31) - (1LL << 16) && (long long)h * w < (1LL << 29),
                 "nway_confusion: bad dims");
    PEMP_REQUIRE(K <= CONF_MAX_K, "nway_confusion: K <= 63 (the block's table of (K + 1)^2 counters is 16 KB of LDS at most)");
    if (int rc = nway_confusion_clear(conf, N, K, (hipStream_t)stream, "nway_confusion")) return rc;
    hipLaunchKernelGGL(nway_confusion_kernel, dim3(tail_blocks(Ho, Wo), N), dim3(256), (size_t)(K + 1) * (K + 1) * sizeof(uint32_t),
                       (hipStream_t)stream, pred, target, want, labels, (unsigned long long*)conf, K, h, w, Ho, Wo);
    return launch_status("nway_confusion");
}

static int pemp_nway_confusion_ragged_f32(const float* pred, const int64_t* target, const int32_t* want,
                                          const pemp_tail_item* items_host, const pemp_tail_item* items_dev, int N, int K, int h,
                                          int w, uint8_t* labels, int64_t* conf, void* ws, size_t ws_bytes, void* stream) {
    (void)ws, (void)ws_bytes;
    PEMP_REQUIRE(pred && target && items_host && items_dev && conf, "nway_confusion_ragged: null pointer");
    PEMP_REQUIRE(N >= 1 && N <= 65535 && K > 0 && h > 0 && w > 0 && (long long)h * w < (1LL << 29),
                 "nway_confusion_ragged: bad dims");
    PEMP_REQUIRE(K <= CONF_MAX_K,
                 "nway_confusion_ragged: K <= 63 (the block's table of (K + 1)^2 counters is 16 KB of LDS at most)");
    const int nb = tail_ragged_check("nway_confusion_ragged", items_host, N, ~(size_t)0);      // the plan alone: no workspace
    if (nb < 0) return -1;
    if (int rc = nway_confusion_clear(conf, N, K, (hipStream_t)stream, "nway_confusion_ragged")) return rc;
    hipLaunchKernelGGL(nway_confusion_ragged_kernel, dim3(nb, N), dim3(256), (size_t)(K + 1) * (K + 1) * sizeof(uint32_t),
                       (hipStream_t)stream, pred, target, want, items_dev, labels, (unsigned long long*)conf, K, h, w);
    return launch_status("nway_confusion_ragged");
}

}  // namespace PEMP_HEAD_NS
}  // namespace pemp
