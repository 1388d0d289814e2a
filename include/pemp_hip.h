/*
 * pemp_hip.h -- C ABI of libpemp_hip.so: the MI355X (gfx950) kernels of the PEMP
 * prototype-matching hot path.
 *
 * The reference (Jarvis73/PEMP) has no native/FFI interface: its hot path is a chain of stock
 * ATen ops issued from networks/{backbones,pemp_stage1,pemp_stage2,baseline}.py.  Each entry
 * point below names the reference call site(s) (file:line, relative to the reference root) whose
 * arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless the name/type says otherwise;
 *  - activations are NHWC ("pixel-major": [N][H][W][C], C contiguous) with an explicit per-pixel
 *    stride `ld*` in elements, so a kernel can read/write a channel slice of a wider buffer;
 *  - conv weights are "KRSC": [Cout][KH][KW][Cin], Cin contiguous (the GEMM K axis);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *  - no hidden allocation, no global mutable state; re-entrant across streams and devices;
 *  - return value: 0 ok, <0 invalid argument (see pemp_last_error()), >0 a hipError_t.
 */
#ifndef PEMP_HIP_H
#define PEMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEMP_ABI_VERSION 2   /* 2: pemp_adam_clip_step_f32 takes its hyper-parameters as doubles (round 5) */

/* flags for pemp_conv_desc.flags */
#define PEMP_CONV_RELU 1u          /* y = max(y, 0) after affine (+ residual)            */
#define PEMP_CONV_SHIFT_PER_IMAGE 2u /* shift is [N][Cout] instead of [Cout]              */
#define PEMP_CONV_STEM4 4u         /* input is NHWC4, K axis = taps x 4 channels (7x7 stem) */
#define PEMP_CONV_POOL3S2 8u       /* y = max_pool2d(act(...), 3, stride 2, pad 1, ceil_mode) of the 7x7 / 2 / 3 stem, in one
                                      launch (pemp_conv2d_nhwc_f32 only; see "Fused stem" below)                              */
#define PEMP_CONV_OUT_SPLIT3 16u   /* y is written PRE-SPLIT: bf16 [M][Cout / 32][3][32], the split3 pieces of the fp32 result
                                      (see "Pre-split activations" below)                                                     */
#define PEMP_CONV_IN_SPLIT3 32u    /* x is such a tensor (tile ids 146 / 149 only)                                            */
#define PEMP_CONV_OUT_SPLIT3_ALSO 64u /* y is written as fp32 as usual AND the same values pre-split, through the pointer passed as
                                      `residual`: no residual is read (tile ids 146 / 149, pemp_conv2d_nhwc_f32 / _padv_ only)   */
#define PEMP_CONV_RES_S2 128u      /* the residual lies on a grid TWICE AS FINE as the output: an NHWC tensor [N][Hr][Wr] with
                                      per-pixel stride ldr, output row (n, ho, wo) adds its pixel (n, 2 ho, 2 wo); Ho = (Hr - 1) / 2
                                      + 1, Wo likewise (see "Strided residual" below; tile ids 43, 71, 72, pemp_conv2d_nhwc_f32 only) */
/* 256u is taken inside the library (the bf16 entry's internal flag) */
#define PEMP_CONV_RES_HEVEN 512u   /* with PEMP_CONV_RES_S2: Hr is even -- Hr = 2 Ho - 1 + (this bit set)                        */
#define PEMP_CONV_RES_WEVEN 1024u  /* ... and Wr = 2 Wo - 1 + (this bit set)                                                     */

typedef struct pemp_conv_desc {
    int32_t N, H, W;        /* input images, input spatial size                                  */
    int32_t Cin, ldx;       /* input channels read, input per-pixel stride (>= Cin)              */
    int32_t Ho, Wo;         /* output spatial size (caller computes; checked)                    */
    int32_t Cout, ldy;      /* output channels, output per-pixel stride (>= Cout)                */
    int32_t KH, KW;         /* kernel size                                                       */
    int32_t stride, pad, dil;
    int32_t ldr;            /* residual per-pixel stride (ignored when residual == NULL)         */
    int32_t Kpad;           /* weight row length in floats (>= KH*KW*Cin, multiple of 32)        */
    uint32_t flags;
    int32_t tile;           /* kernel variant: 0 = the entry's own choice, else a tile id (pemp_conv2d_tile_shape)   */
} pemp_conv_desc;

const char* pemp_last_error(void);
int pemp_abi_version(void);

/* TILE IDS.  id = 10 x family + shape; every conv entry point decodes pemp_conv_desc.tile through this one scheme.
 *   shape (last digit)    block BM x BN, waves
 *     1  128 x 128, 4       2  128 x 64, 4       3  64 x 64, 4
 *     4  128 x 128, 8       5  128 x 64, 8       6  256 x 128, 8       7  256 x 256, 8
 *     8  32 x 64, 4: 16-row wave tiles on v_mfma_f32_16x16x4_f32 (finer granularity for launches of a few rounds)
 *     9  the hybrid launch: shape 3 for the rows that fill whole rounds + 16-row wave tiles for the rest (pemp_conv2d_hybrid_rows)
 *   family (decade)
 *     0x  1..3          fp32 chain (v_mfma_f32_32x32x2_f32), operands staged through registers
 *     1x  11..17        ... staged by LDS-DMA, pointer-addressed: takes every geometry
 *     2x  21..29        ... buffer-addressed LDS-DMA, barrier inside the MFMA stream: <= 32 taps, operands < 2 GiB, no stem
 *     3x  31..37, no 33 the 2x kernel with the LAST, partly filled round of tiles split along K (workspace: see
 *                       pemp_conv2d_stats_nhwc_f32); not bit-identical to 0x..2x
 *     4x  41..44, 46    split3: fp32 operands as three bf16 pieces on v_mfma_f32_32x32x16_bf16 (pemp_pack_split3_bf16);
 *         47, 49        persistent forms of 43 and 46: a resident grid walks the tiles
 *     5x  51, 52, 54, 56  split3 with the last round split along K
 *    14x  146, 149        split3 with pre-split ACTIVATIONS (PEMP_CONV_IN_SPLIT3): 46 and 49 without the split in the K loop
 *    24x  246, 249        the tile and results of 146 / 149 (249: the persistent form) with ONE activation stage per (channel chunk,
 *                       kh): the three kw taps read it displaced by -d, 0, +d rows, image-row boundaries carry d zero rows
 *                       (conv_row3.hip: conv_row3_kernel, conv_row3p_kernel).  3x3, stride 1,
 *                       pad == dil == d, 256 + 2 d + d ceil((255 + 2 d) / W) <= 288; the plain fp32 output (affine, ReLU) only: no
 *                       PEMP_CONV_OUT_SPLIT3 / _ALSO, residual, padding value, per-image shift, split-K or workspace -- anything
 *                       else is an error ("unsupported").  Bit-identical to 146 / 149
 *    34x  349             the form and results of 49 on a THREE-deep activation ring (conv_ring.hip: conv_ring_kernel): persistent 256 x
 *                       128 tiles whose fp32 activations get two K steps to land instead of half a step.  1x1 convs without padding
 *                       (any stride), ldx >= Cin, Kpad == Cin >= 128, Cout % 128 == 0; the fp32 output (affine, per-image shift, ReLU,
 *                       ldy >= Cout) or PEMP_CONV_OUT_SPLIT3; no residual, PEMP_CONV_OUT_SPLIT3_ALSO, PEMP_CONV_IN_SPLIT3,
 *                       PEMP_CONV_RES_S2, padding value, stem, split-K or workspace, pemp_conv2d_nhwc_f32 only -- anything else is an
 *                       error ("unsupported").  Bit-identical to 43 / 49
 *     7x  71, 72          split3, activation-stationary (1x1 convs without padding, Kpad <= 256, pemp_conv2d_nhwc_f32 only): a
 *                       block of 4 waves keeps 128 output rows x K of split activations in registers and walks ALL of Cout, 128
 *                       (71) or 64 (72) columns at a time, with only the packed weights streaming through LDS; no padding value,
 *                       per-image shift, workspace or grouped form, operands below 2 GiB -- anything else is an error.
 *                       Bit-identical to 4x (same MFMA order per accumulator, same epilogue arithmetic)
 *   0x, 1x and 2x are bit-identical to each other, and so are 4x among themselves.  Where an id's own kernels do not take a
 *   geometry, pemp_conv2d_nhwc_f32 and its _padv_ / _splitk_ forms fall back in this order, with the same results: 3x -> 2x,
 *   29 -> 23 (no hybrid split), 2x -> 1x (28 -> 13); 4x / 5x never fall back (an error instead).  Which ids an entry takes is
 *   said at the entry.
 * Returns 1 and the block shape of `id` (bm, bn: optional), 0 for an id that no entry point takes (0 itself included). */
int pemp_conv2d_tile_shape(int id, int* bm, int* bn);

/* Convolution + per-channel affine (+ residual) (+ ReLU) as one implicit GEMM on
 * v_mfma_f32_32x32x2_f32:   y[n,ho,wo,co] = act( scale[co] * sum_{kh,kw,ci} x[...] * w[co,kh,kw,ci]
 *                                               + shift[co] (+ residual[n,ho,wo,co]) )
 * scale == NULL means 1, shift == NULL means 0.
 * Replaces nn.Conv2d + nn.BatchNorm2d(eval) + ReLU + residual add:
 *   networks/backbones.py:47-52,66-75 (BottleNeck), :89-91 (stem), :110-111 (downsample),
 *   :330-357,366 (ASPPV2 convs + layer6), :281-305,319 (ASPP), :375-397 (VGG16);
 *   networks/pemp_stage1.py:74,77 (purifier); networks/baseline.py:61 (projection).        */
int pemp_conv2d_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                         const float* scale, const float* shift, const float* residual,
                         void* stream);

/* Same convolution with a per-input-channel PADDING VALUE: out-of-image taps read pad_value[ci] instead
 * of 0 (pad_value NULL = the call above).  This is what lets a BatchNorm that sits IN FRONT of a padded
 * conv (ASPPV2 branches, networks/backbones.py:330-357: BN -> ReLU-less conv on the BN output, zero-padded
 * in BN space) fold into the conv exactly:  conv_W(s*x + t, pad 0) = conv_{W*s}(x, pad -t/s) + sum_taps W t.
 * Multi-tap, non-stem convs only.                                                                   */
int pemp_conv2d_padv_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y,
                              const float* scale, const float* shift, const float* residual,
                              const float* pad_value, void* stream);

/* Tile id 29 ("hybrid"): for a conv whose 32 x 32 wave tiles fill only a few rounds of the chip (a one-episode evaluation step's
 * 256-channel convs: 1304 tiles on 1024 SIMDs -- reference networks/backbones.py:42-77 at the reference's own data.test_bs = 1,
 * data_kits/datasets.py:23), the rows that fill WHOLE rounds run on the 64 x 64 tile and the remaining rows on 16-row wave tiles
 * in the same grid; bit-identical to every other exact variant.  Returns how many output rows of `d` go to the 64 x 64 part
 * (0: this geometry has no such split -- pemp_conv2d_nhwc_f32 then runs tile 29 as tile 23).  The tile id of `d` is not read. */
int pemp_conv2d_hybrid_rows(const pemp_conv_desc* d);

/* Up to 4 INDEPENDENT convolutions in ONE launch (arrays of n descriptors / operand pointers; scale, shift, residual,
 * pad_value: NULL or arrays with NULL entries; pad_value for every member or for none; every descriptor names the same
 * tile variant 21..28).  Each member is computed exactly as by pemp_conv2d_padv_nhwc_f32 on its own -- same tiles, same K
 * order, bit-identical -- but the members' tiles share one grid: a one-episode evaluation step (5202 feature rows: 41-82
 * tiles per conv on 256 CUs) runs the dilated ASPPV2 branches (networks/backbones.py:330-357, all reading the same
 * activations) and a stage's downsample conv beside its conv1 (backbones.py:47,110) this way.  Members must not write
 * memory another member reads or writes.                                                                            */
int pemp_conv2d_group_nhwc_f32(int n, const pemp_conv_desc* d, const float* const* x, const float* const* w,
                               float* const* y, const float* const* scale, const float* const* shift,
                               const float* const* residual, const float* const* pad_value, void* stream);

/* Split3 family (tile ids 4x / 5x; the 5x through the split-K entries and workspace like 3x): the same convolution with fp32
 * operands on v_mfma_f32_32x32x16_bf16.  Every fp32 value is split exactly
 * into three bf16 pieces h + m + l (round to nearest at each stage); a product is taken as its six pieces' products above one
 * fp32 rounding (hl, lh, mm, mh, hm, hh), accumulated in fp32: fp32-accurate, not bit-identical to the fp32-chain ids 21..37, and
 * bit-identical among 41..44, 46 and their grouped launches (ascending K order, fixed product order).  With these ids `w` is NOT the
 * [Cout][Kpad] fp32 weight but its split form from pemp_pack_split3_bf16.  Entries: pemp_conv2d_nhwc_f32, _padv_, _splitk_,
 * _padv_splitk_, _group_ (41..44, 46), and pemp_split3_conv2d_stats_nhwc_f32 (the statistics epilogue on 41..44, 46).  No bnbwd /
 * dropblock / bf16 forms, and pemp_conv2d_stats_nhwc_f32 itself stays with the fp32 chain; buffer-addressed geometries
 * only (<= 32 taps; no stem except the fused form below): an error, never a fall-back, elsewhere.
 * Fused stem (flag PEMP_CONV_POOL3S2, pemp_conv2d_nhwc_f32 only): the 7x7 / stride 2 / pad 3 PEMP_CONV_STEM4 conv with split3
 * arithmetic (`w` = pemp_pack_split3_bf16 of the stem's [Cout][224] pack; any split3 tile id 41..49 names it, the kernel has one
 * shape) + affine + ReLU + the 3x3 / stride 2 / pad 1 ceil-mode max-pool behind it (networks/backbones.py:89-92).  The descriptor
 * keeps the CONVOLUTION's Ho, Wo; y is the pooled [N][Hp][Wp][Cout] tensor (Hp = Ho / 2 + 1, per-pixel stride ldy): the conv's
 * own output is never written.  A block computes the 17 x 17 conv pixels of an 8 x 8 patch of pool outputs; conv pixels outside
 * Ho x Wo take no part in a maximum.  No residual, padding value or per-image shift; anything else is an error.
 * Ids 47 and 49 (pemp_conv2d_nhwc_f32 / _padv_ / _splitk_ / _padv_splitk_ with no workspace; not _group_): the persistent forms
 * of 43 (64 x 64) and 46 (256 x 128).  The grid is the number of blocks resident at once (at most the tile count) and each block
 * walks a fixed sequence of tiles, issuing the next tile's first operand DMA before the current tile's epilogue; same tiles, same
 * K order, same epilogue arithmetic: bit-identical to 41..46.  (41's shape has no such form: it would spill at 2 waves / SIMD.)
 * Pre-split activations (pemp_conv2d_nhwc_f32 / _padv_ only).  A conv whose output has ONE reader, a multi-tap split3 conv, can
 * hand it over already split, so that the reader's K loop has no splitting left to do:
 *   PEMP_CONV_OUT_SPLIT3 (producer; ids 41..44, 46, 47, 49): after affine (+ ReLU) every output value is split with the arithmetic
 *   of pemp_pack_split3_bf16 and `y` is written as bf16 [M][Cout / 32][3][32] (M * Cout * 6 bytes): per pixel and 32-channel group
 *   the planes h, m, l -- h + m + l is the fp32 value the same id writes without the flag, exactly.  ldy == Cout; no residual,
 *   split-K, workspace, grouped, panel (71 / 72) or fused-stem form.  The persistent ids have PRODUCER variants of their kernels,
 *   chosen at compile time, with no residual path at all (that is what leaves them registers for the split): 47 and 49 run
 *   conv_dma2_s3po_kernel<64, 64, ...> / <256, 128, ...>, 149 runs conv_dma2_a3po_kernel<256, 128, ...>; a persistent shape without
 *   such a variant would run as the id it walks (none today).  Same tiles, K order and split: the bf16 tensor ids 43 / 46 write.
 *   PEMP_CONV_IN_SPLIT3 (consumer; ids 146 = the form of 46, 149 = the form of 49, 246 / 249 = 146 / 149 on row stages, and no other id): `x` is such a tensor
 *   (ldx == Cin, Cin % 32 == 0), a padding value is the [Cin / 32][3][32] bf16 split of the fp32 vector, behind x like the fp32
 *   one.  Multi-tap convs only; no per-image shift, split-K or workspace; Cout % 128 == 0.  Same MFMA order and epilogue as
 *   41..49 on the same pieces: bit-identical to them on the fp32 tensor.  (No 128 x 128 form: its A tile of 96 KiB would leave one
 *   block per CU.)
 *   PEMP_CONV_OUT_SPLIT3_ALSO (ids 146 / 149 only: a consumer whose own output has readers of both forms): `y` is written as fp32
 *   exactly as without the flag (ldy, channel windows included) AND the same values go out pre-split, bf16 [M][Cout / 32][3][32]
 *   dense, through the pointer passed in the `residual` argument (16-byte aligned; d->ldr is ignored).  Under this flag NO residual
 *   is read.  Compile-time variants: conv_dma2_a3o_kernel (146) and conv_dma2_a3po_kernel<..., 2> (149).  Refused with
 *   PEMP_CONV_OUT_SPLIT3, split-K, a workspace, the grouped / DropBlock / statistics / bf16 entries, the stem and every other tile
 *   id (the panel ids included), and when the two outputs overlap.
 * Strided residual (PEMP_CONV_RES_S2 with PEMP_CONV_RES_HEVEN / _WEVEN; pemp_conv2d_nhwc_f32 only).  A bottleneck whose output is
 *   read by stride-2 1x1 convs alone needs only the rows on the even grid; its last conv then runs on the compact Ho x Wo grid
 *   while the shortcut it adds still lies on the full Hr x Wr one.  With the flag `residual` is that tensor, [N][Hr][Wr] with
 *   per-pixel stride ldr, and output row (n, ho, wo) adds the Cout channels of its pixel (n, 2 ho, 2 wo); Hr = 2 Ho - 1 + HEVEN,
 *   Wr = 2 Wo - 1 + WEVEN, N * Hr * Wr * ldr below 2^31 elements.  Same dot products, same epilogue arithmetic: bit-identical to
 *   the same id on the gathered dense residual.  Compile-time variants of two kernels take it: conv_panel_rs2_kernel (id 72 at
 *   Kpad 64 or 128, id 71 at Kpad 64) and conv_dma2_rs2_kernel (id 43, any M).  Everything else refuses it, never reads it as dense: the
 *   persistent ids 47 / 49, the other split3 ids, split-K and a workspace, a padding value, the stem, PEMP_CONV_OUT_SPLIT3 /
 *   _IN_SPLIT3 / _OUT_SPLIT3_ALSO, the fp32-chain ids (0 included), and the grouped / DropBlock / statistics / bf16 entries.
 * pemp_pack_split3_bf16: [Cout][Kpad] fp32 (Kpad % 32 == 0) -> [Cout][Kpad / 32][3][32] bf16 (Cout * Kpad * 6 bytes): per row and
 * 32-channel K step the h, m and l planes, channel order unchanged.                                                           */
int pemp_pack_split3_bf16(const float* w, void* out, int cout, int kpad, void* stream);

/* SIDE-FIGURE VARIANT, not the product path's arithmetic: the same convolution with bf16 OPERANDS (x, w, residual, pad_value:
 * bf16 tensors; descriptor in bf16 elements, Cin % 64 == 0, ldx % 8 == 0) and fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16; y is bf16 (out_f32 == 0; a residual is then bf16 too) or fp32 (the encoder's last layer).  Tiles
 * 21..27 (0 = 24).  Exists to show what exact fp32 costs (bench.py: `bf16_variant`, with the mIoU it moves); never the default. */
int pemp_conv2d_bf16_nhwc(const pemp_conv_desc* d, const void* x, const void* w, void* y, const float* scale,
                          const float* shift, const void* residual, const void* pad_value, int out_f32, void* stream);
/* element-wise fp32 <-> bf16 (round to nearest even) for the boundaries of that variant (n % 4 == 0) */
int pemp_convert_f32_bf16(const float* x, void* y, long long n, void* stream);
int pemp_convert_bf16_f32(const void* x, float* y, long long n, void* stream);

/* The convolution above FOLLOWED BY DropBlock2D's scaling of its output (training; dropblock==0.3.0's two statements
 * y * mask[None] ; y * numel / sum(mask), in that order and rounding): row m of the result is multiplied by rowmask[m] (fp32 {0,1}
 * per output pixel, from pemp_dropblock_mask_f32) * M / *kept_count.  One launch instead of the conv + pemp_pixel_scale_f32 --
 * the purifier's conv -> ReLU -> DropBlock (networks/pemp_stage1.py:74-79) and, in the backward pass, the input-gradient convs
 * whose result DropBlock's backward scales the same way.  Tiles 21..27, or 31..37 with a split-K workspace (ws may be NULL
 * otherwise).                                                                                                              */
int pemp_conv2d_dropblock_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale,
                                   const float* shift, const float* residual, const float* rowmask, const int* kept_count,
                                   void* ws, size_t ws_bytes, void* stream);
/* train-mode BatchNorm apply (batch statistics given) + the DropBlock2D behind it in one pass: ASPPV2's BatchNorm -> DropBlock ->
 * conv branches (networks/backbones.py:329-353).                                                                           */
int pemp_bn_apply_dropblock_f32(const float* z, int ldz, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, float* y, int ldy, int M, int C, const float* rowmask,
                                const int* kept_count, void* stream);

/* [N,3,H,W] image (+ optional [N,1,H,W] prior; NULL -> 0) -> NHWC4 [N,H,W,4].
 * Replaces torch.cat/view at networks/pemp_stage1.py:139, pemp_stage2.py:130-138.          */
int pemp_pack_input_nhwc4_f32(const float* img, const float* prior, float* out,
                              int N, int H, int W, void* stream);

/* nn.MaxPool2d(k, s, p, ceil_mode) on NHWC: networks/backbones.py:92 (3/2/1 ceil), :378-392.
 * Ho/Wo are given by the caller (checked against the formula).                              */
int pemp_maxpool2d_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, int ldx,
                            int Ho, int Wo, int ldy, int k, int s, int p, void* stream);

/* Training form of the same layer (contiguous x, y): also writes, per output element, the offset
 * dh*k+dw of the winning element inside its unclipped window (first maximum in scan order, as ATen's
 * max_pool2d_with_indices), one byte each; pemp_maxpool2d_idx_bwd_nhwc_f32 routes dy through those
 * indices (backward of backbones.py:92) without reading x again.                              */
int pemp_maxpool2d_idx_nhwc_f32(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C,
                                int Ho, int Wo, int k, int s, int p, void* stream);
int pemp_maxpool2d_idx_bwd_nhwc_f32(const uint8_t* idx, const float* dy, float* dx, int N, int H, int W,
                                    int C, int Ho, int Wo, int k, int s, int p, void* stream);

/* F.adaptive_avg_pool2d(x,(1,1)) on NHWC: y[n][c] = mean_i x[n][i][c]
 * (networks/backbones.py:311,360).                                                          */
int pemp_global_avgpool_nhwc_f32(const float* x, float* y, int N, int HW, int C, int ldx,
                                 void* stream);

/* y[m][c] = x[m][c]*scale[c] + shift[c] for `nb` (scale,shift,y) triples sharing one x
 * (the BatchNorm that PRECEDES each ASPPV2 branch conv: networks/backbones.py:328,334,340,346,352). */
int pemp_channel_affine_multi_f32(const float* x, int ldx, int M, int C, int nb,
                                  const float* const* scale, const float* const* shift,
                                  float* const* y, const int* ldy, void* stream);

/* Meta-prototype module, steps (i)-(v) of networks/pemp_stage1.py:201-213 (= pemp_stage2.py:170-186):
 * soft-assign every support pixel to the p fg / p bg centres, masked, and pool.
 *   feat   [B*S][n][ldf] support features (NHWC, c channels), n = h*w
 *   mask   [B*S][2][H][W] full-resolution support mask (ch0 fg, ch1 bg); resized on the fly with
 *          F.interpolate(..., mode="nearest") semantics (pemp_stage1.py:147)
 *   ctr    [c][2p] learnable centres (pemp_stage1.py:104-105)
 *   protos [B][2p][c] out: row j<p = fg prototype j, row p+j = bg prototype j (mean over S)
 *   ws     workspace of pemp_mpm_workspace_bytes() bytes                                     */
size_t pemp_mpm_workspace_bytes(int B, int S, int n, int c, int p);
int pemp_mpm_protos_f32(const float* feat, int ldf, const float* mask, const float* ctr,
                        float* protos, void* ws, size_t ws_bytes,
                        int B, int S, int h, int w, int H, int W, int c, int p, void* stream);

/* Plain masked average pooling (protos == 0 branch, networks/pemp_stage1.py:223-227) when
 * full_res == 0, and the Baseline form over bilinearly upsampled features
 * (networks/baseline.py:100-110) when full_res == 1 (computed through the adjoint of the
 * align_corners=True interpolation, never materialising the upsampled tensor).
 *   protos [B][2][c] out: row 0 = fg, row 1 = bg                                             */
size_t pemp_map_workspace_bytes(int B, int S, int n, int c);
int pemp_masked_avg_pool_f32(const float* feat, int ldf, const float* mask, float* protos,
                             void* ws, size_t ws_bytes, int B, int S, int h, int w, int H, int W,
                             int c, int full_res, void* stream);

/* F.cosine_similarity(qry, proto) * dist_scalar for every prototype, max over the p prototypes
 * of each group, stacked (bg, fg): networks/pemp_stage1.py:214-215,256-260.
 *   qry    [B][n][ldf] query features (Q == 1, as the reference's broadcasting requires)
 *   protos [B][2p][c]  (layout of pemp_mpm_protos_f32 / pemp_masked_avg_pool_f32 with p = 1)
 *   pred   [B][2][n]   out, ch0 = bg, ch1 = fg
 *   resp   [B][n] uint8 out or NULL: response index of pemp_stage1.py:217-222 (0..2p-1)      */
int pemp_cosine_proto_max_f32(const float* qry, int ldf, const float* protos, float* pred,
                              uint8_t* resp, int B, int n, int c, int p, float dist_scalar,
                              void* stream);

/* The same map against a prototype BANK: prototypes of K classes enrolled once, met by N queries in one launch.
 *   bank  [K][2p][c]  (the protos layout above, class after class; 16-byte aligned)
 *   index NULL:            every query against every class; pred [N][K][2][n], resp [N][K][n] (or NULL)
 *   index [N] int32 (dev): query b against class index[b] (clamped into 0..K-1); pred [N][2][n], resp [N][n] (or NULL)
 * For every (b, k) the outputs are bit for bit those of pemp_cosine_proto_max_f32 on query b with protos = bank[k].
 * N, K <= 65535.                                                                                              */
int pemp_cosine_bank_max_f32(const float* qry, int ldf, const float* bank, const int32_t* index,
                             float* pred, uint8_t* resp, int N, int K, int n, int c, int p,
                             float dist_scalar, void* stream);

/* PANet's alignment branch (networks/panet.py:168-171): masks [B][2][n] from a low-resolution prediction
 * pred [B][2][n]:  masks[b][0] = [argmax == 1] (foreground), masks[b][1] = [argmax == 0]; channel 0 wins ties
 * (torch.argmax).  They feed pemp_masked_avg_pool_f32(full_res = 0) with the QUERY features as "support".    */
int pemp_argmax_masks_f32(const float* pred, float* masks, int B, int n, void* stream);

/* F.interpolate(pred, (Ho,Wo), "bilinear", align_corners=True) -> logits [B][2][Ho][Wo]
 * (networks/pemp_stage1.py:157,162; baseline.py:117).                                        */
int pemp_upsample_bilinear_ac_f32(const float* pred, float* out, int B, int C, int h, int w,
                                  int Ho, int Wo, void* stream);

/* F.interpolate(resp.float(), (Ho,Wo), "nearest").long() (networks/pemp_stage1.py:158-159).   */
int pemp_upsample_nearest_u8_i64(const uint8_t* resp, int64_t* out, int B, int h, int w,
                                 int Ho, int Wo, void* stream);

/* The tail of Evaluator.test_step fused (entry/pemp_stage1.py:48-53 + core/metrics.py:9-23):
 * upsample (as above) + argmax over the 2 classes + CrossEntropyLoss(ignore_index=255) partial
 * sums + FewShotMetric tp/fp/fn for class rows {bg, fg}.
 *   target int64 [B][Ho][Wo]; pred_out uint8 [B][Ho][Wo];
 *   stats  double [B][8] out: {ce_sum, n_valid, tp_bg, fp_bg, fn_bg, tp_fg, fp_fg, fn_fg}
 *   logits_out [B][2][Ho][Wo] or NULL.                                                       */
size_t pemp_eval_tail_workspace_bytes(int B, int Ho, int Wo);
int pemp_eval_tail_f32(const float* pred, const int64_t* target, uint8_t* pred_out,
                       float* logits_out, double* stats, void* ws, size_t ws_bytes,
                       int B, int h, int w, int Ho, int Wo, void* stream);

/* The K-class counterpart of that tail: the K binary maps of an all-classes bank call (pred [N][K][2][h][w], what
 * pemp_cosine_bank_max_f32 and the other bank kernels leave without an index) fused into one label map.  U = the
 * upsample above.  Class k claims a pixel iff U[n][k][1] > U[n][k][0] (the tail's own comparison: a tie is
 * background); the label is 0 where no class claims, else 1 + the claiming k with the largest margin
 * U[n][k][1] - U[n][k][0] (one fp32 subtraction; the lowest k wins equal margins).  Labels are slot numbers, K <= 255.
 *   labels uint8 [N][Ho][Wo];  margin fp32 [N][Ho][Wo] or NULL: the winner's margin, or where nobody claims the
 *   largest margin of all classes (<= 0).
 *   target int64 [N][Ho][Wo] (255 = ignore), want int32 [N] on the device, stats double [N][8]: all three or none.
 *   stats = {ce_sum, n_valid, tp_bg, fp_bg, fn_bg, tp_fg, fp_fg, fn_fg} as above: ce_sum and n_valid of class want[n]'s
 *   own two logits (pemp_eval_tail_f32's terms on pred[n][want[n]]), the counts of the image
 *   [label == want[n] + 1] against target: the class's IoU under competition.  Deterministic (no atomics).      */
size_t pemp_nway_tail_workspace_bytes(int N, int Ho, int Wo);
int pemp_nway_tail_f32(const float* pred, const int64_t* target, const int32_t* want, uint8_t* labels,
                       float* margin, double* stats, void* ws, size_t ws_bytes,
                       int N, int K, int h, int w, int Ho, int Wo, void* stream);

/* Ragged forms of both tails: ONE launch pair for a batch whose images each have their own output size (a query label keeps
 * its size at test time: mask_mode 3 below).  One descriptor per image; the host fills Ho, Wo, calls
 * pemp_tail_ragged_workspace_bytes() (validates, fills the "planned" fields, returns the workspace size; 0 on error), uploads
 * the descriptors and calls a tail with both copies (the host copy is read during the call only; the kernels read, never
 * write, the device copy).  target, pred_out / labels and margin are PACKED: image i's [Ho_i][Wo_i] map starts at element
 * pix_off_i, the maps lie end to end in the batch's order.  Image i is walked by exactly nblk_i blocks in the fixed-size
 * tail's order and its partial sums are added in the fixed-size tail's order: per image, every result is bit for bit what
 * pemp_eval_tail_f32 / pemp_nway_tail_f32 give for that image alone.  Deterministic (no atomics).  No weight map and no
 * logits_out: those stay on the fixed-size calls.                                                                        */
typedef struct pemp_tail_item {
    int32_t Ho, Wo;        /* the image's output size                                                                    */
    /* planned (pemp_tail_ragged_workspace_bytes): */
    int32_t nblk;          /* blocks that walk the image: ceil(Ho * Wo / 1024), at least 1, at most 256                  */
    int32_t part_off;      /* the image's first row of partial sums in the workspace ([8] doubles per block)             */
    int64_t pix_off;       /* element offset of the image inside the packed arrays: the running sum of Ho * Wo           */
} pemp_tail_item;

size_t pemp_tail_ragged_workspace_bytes(pemp_tail_item* items_host, int n);
/* pred [B][2][h][w]; target packed int64 and stats [B][8]: both or neither (neither: arg-max only); pred_out packed uint8. */
int pemp_eval_tail_ragged_f32(const float* pred, const int64_t* target, const pemp_tail_item* items_host,
                              const pemp_tail_item* items_dev, int B, int h, int w, uint8_t* pred_out,
                              double* stats, void* ws, size_t ws_bytes, void* stream);
/* pred [N][K][2][h][w]; target packed int64, want int32 [N] on the device, stats [N][8]: all three or none; labels packed
 * uint8; margin packed fp32 or NULL.                                                                                     */
int pemp_nway_tail_ragged_f32(const float* pred, const int64_t* target, const int32_t* want,
                              const pemp_tail_item* items_host, const pemp_tail_item* items_dev, int N, int K,
                              int h, int w, uint8_t* labels, float* margin, double* stats, void* ws,
                              size_t ws_bytes, void* stream);

/* N-way confusion tails: the label of the N-way tail above (the same device function decides the pixel) counted against a
 * target, for semantic IoU over a bank.  pred [N][K][2][h][w]; conf int64 [N][K+1][K+1], overwritten:
 * conf[n][t][p] = the counted pixels of image n with target class t and label p (0 = no class, 1 + slot otherwise).
 *   want == NULL: target holds slot labels 0..K.  want != NULL (int32 [N] on the device): target is the binary mask
 *   0 / 1 / 255 of class want[n], lifted on the fly: 0 stays 0, 1 becomes want[n] + 1.  In both forms 255, and every other
 *   value that is not a class of the table, is ignored and never indexes it.
 *   labels uint8 [N][Ho][Wo] (ragged: packed) or NULL: with NULL nothing is written per pixel; given, they are
 *   pemp_nway_tail_f32's bit for bit.
 * K <= 63: a block counts in (K + 1)^2 <= 4096 uint32 bins of LDS, bin (0,0) in registers, and adds its non-zero bins to conf
 * with 64-bit integer atomics after the entry has cleared conf: integer sums, exact and identical run to run whatever the
 * grid or N.  That flush needs no workspace: pemp_nway_confusion_workspace_bytes returns 0, and ws / ws_bytes are accepted
 * (NULL / 0 will do) and not used.  The ragged form takes the descriptors pemp_tail_ragged_workspace_bytes planned
 * (target and labels packed as for the ragged tails); per image its table is the fixed-size call's on that image alone. */
size_t pemp_nway_confusion_workspace_bytes(int N, int K, int Ho, int Wo);
int pemp_nway_confusion_f32(const float* pred, const int64_t* target, const int32_t* want,
                            uint8_t* labels, int64_t* conf, void* ws, size_t ws_bytes,
                            int N, int K, int h, int w, int Ho, int Wo, void* stream);
int pemp_nway_confusion_ragged_f32(const float* pred, const int64_t* target, const int32_t* want,
                                   const pemp_tail_item* items_host, const pemp_tail_item* items_dev,
                                   int N, int K, int h, int w, uint8_t* labels, int64_t* conf,
                                   void* ws, size_t ws_bytes, void* stream);

/* ResNetCM.comm statistics (networks/backbones.py:208-216): mask' = max_pool2d(mask,3,stride,1);
 * mean over ALL pixels and max over pixels of x*mask' per image and channel.
 *   x [N][Hx*Wx][ldx], mask_in [N][Hm][Wm], mask_out [N][Hx][Wx], stat [N][2][C] (mean, max).
 * x == NULL pools the mask only (the extra pool at backbones.py:227).                          */
int pemp_cm_reduce_f32(const float* x, int ldx, const float* mask_in, float* mask_out, float* stat,
                       int N, int Hm, int Wm, int Hx, int Wx, int C, int stride, void* stream);

/* ResNetCM.comm after the statistics (networks/backbones.py:213-221): per episode g the mean over its S+Q images
 * of (mean, max), then Linear(2C -> 2):
 *   agg[g][k] = mean_{n: group[n]==g} stat[n][k];   feat[g][e] = lin_b[e] + sum_k agg[g][k] * lin_w[e][k]
 * stat [N][C2] (C2 = 2C: means then maxes, the layout pemp_cm_reduce_f32 writes), group int32 [N], G <= 64.      */
int pemp_cm_linear_f32(const float* stat, const int32_t* group, const float* lin_w, const float* lin_b,
                       float* agg, float* feat, int N, int G, int C2, void* stream);
/* The two broadcast channels enter the stage's first 1x1 convs (backbones.py:194,201,231,236,241) as a per-image bias:
 *   out[n][co] = base[co] + alpha[co] * (feat[g][0] * wext[co*ldw] + feat[g][1] * wext[co*ldw + 1]),  g = group[n]
 * (alpha/base: the folded eval BatchNorm, or NULL = 1 / 0 in training where BN follows separately).             */
int pemp_cm_bias_f32(const float* feat, const int32_t* group, const float* wext, int ldw, const float* alpha,
                     const float* base, float* out, int N, int Cout, void* stream);
/* Backward of the two (entry/pemp_stage2.py:78).  colsum [N][Cout] = per-image sums of the conv-output gradient:
 *   dwext[co][e] = sum_n colsum[n][co] * feat[g(n)][e];   dfeat_img[n][e] (+)= sum_co colsum[n][co] * wext[co][e]
 *   dlin_w[e][k] = sum_g dfeat[g][e] * agg[g][k], dlin_b[e] = sum_g dfeat[g][e]   (dfeat[g] = sum_{n in g} dfeat_img[n])
 *   dstat[n][k]  = (sum_e dfeat[g(n)][e] * lin_w[e][k]) / |episode g(n)|                                        */
int pemp_cm_bias_bwd_f32(const float* colsum, const float* feat, const int32_t* group, const float* wext, int ldw,
                         float* dwext, int lddw, float* dfeat_img, int accumulate, int N, int Cout, void* stream);
int pemp_cm_linear_bwd_f32(const float* dfeat_img, const int32_t* group, const float* agg, const float* lin_w,
                           float* dlin_w, float* dlin_b, float* dstat, int N, int G, int C2, void* stream);

/* Backward of the comm statistics through loss.backward() in stage-2 training (entry/pemp_stage2.py:78;
 * networks/backbones.py:209-215): given dstat [N][2][C] (gradients of the per-image mean and max),
 *   dx[n][i][c] += mask[n][i] * (dstat[n][0][c] / HW + [i == argmax_i x*mask] * dstat[n][1][c])
 * with mask the POOLED mask that cm_reduce returned (mask_out) and the first maximal index taking the
 * max gradient (torch.max semantics on the host).  Accumulates into dx [N][HW][ldd].              */
int pemp_cm_bwd_add_f32(const float* x, int ldx, const float* mask, const float* dstat, float* dx, int ldd,
                        int N, int HW, int C, void* stream);
/* Training forms: pemp_cm_reduce_arg_f32 also records argmax [N][C] (int32: the first maximal pixel of x*mask per
 * image and channel; NULL = pemp_cm_reduce_f32), and pemp_cm_bwd_add_arg_f32 applies the same gradient from that
 * record as one element-wise pass (no second reduction over x).  C % 4 == 0.                                    */
int pemp_cm_reduce_arg_f32(const float* x, int ldx, const float* mask_in, float* mask_out, float* stat,
                           int32_t* argmax, int N, int Hm, int Wm, int Hx, int Wx, int C, int stride, void* stream);
int pemp_cm_bwd_add_arg_f32(const float* mask, const float* dstat, const int32_t* argmax, float* dx, int ldd,
                            int N, int HW, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training path (Trainer.train_step, entry/pemp_stage1.py:57-65; model.train() at
 * core/base_trainer.py:189).
 * ---------------------------------------------------------------------------------------------- */

/* The conv in front of a train-mode BatchNorm with the BatchNorm's batch statistics started in its epilogue
 * (networks/backbones.py:48-52,66-75 with the model in train(), core/base_trainer.py:189): y = conv(x, w) (no affine,
 * no residual, no ReLU) and, for every group of 32 consecutive output rows r, the per-channel partial sums
 *   stats[r][0][c] = sum y[m][c],  stats[r][1][c] = sum y[m][c]^2        (m in the rows of row tile r, m < M)
 * i.e. pemp_conv2d_stats_rows(d) x 2 x Cout floats (one row per row tile of the chosen variant: ceil(M / 64 .. 256)).
 * pemp_bn_stats_partials_f32 adds them in a fixed order (double) into mean / 1/sqrt(var+eps) and the running-statistics
 * update: the separate pass over y that pemp_bn_stats_f32 makes is gone.  pemp_bn_fwd_partials_f32 = that followed by the
 * normalisation (pemp_bn_apply_mask_f32), one call for the pair.
 * Deterministic.  Non-stem convs whose operands lie below 2 GiB (the buffer-addressed kernels); returns
 * -2 where that does not hold (use pemp_conv2d_nhwc_f32 + pemp_bn_stats_f32 then).  d->tile: 0 or 21..27, or 31..37
 * (not 33) = the same tile shapes with the LAST, partly filled round of tiles split along K (8 images of 51 x 51 pixels
 * give 326 tiles of 128 x 128 for 256 output channels: 256 CUs are busy for two rounds and do the work of 1.27).  The
 * T mod 256 remainder tiles are computed by up to 256 blocks, each over a slice of the K steps; partial accumulators go
 * to `ws`, the block that arrives last (an arrival counter per tile) adds the slices in ascending order -- the result
 * does not depend on arrival order, but differs from the unsplit variants by the rounding of that regrouped sum.
 * ws: pemp_conv2d_splitk_workspace_bytes(d) bytes of UNCACHED device memory from pemp_uncached_alloc (the blocks of one
 * tile run on different XCDs, whose L2s do not see each other's lines: in uncached memory the exchange needs no cache
 * write-back / invalidate -- with agent-scope fences on ordinary memory the variant loses what it gains); its first 1024
 * bytes (the counters) must be zero on entry and are left zero; not shared by launches that may run concurrently.
 * NULL / 0 for the other tile ids.                                                                                      */
size_t pemp_conv2d_splitk_workspace_bytes(const pemp_conv_desc* d);
/* pemp_conv2d_nhwc_f32 with the split-K tile ids (31..37) allowed; other ids behave as there (ws unused).  Used by the
 * training step and by evaluation steps of one or two episodes (<= 12000 output rows, where the unsplit variants leave most
 * CUs idle); larger evaluation steps keep the variants that are bit-identical to each other.                              */
int pemp_conv2d_splitk_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale,
                                const float* shift, const float* residual, void* ws, size_t ws_bytes, void* stream);
/* ... and with a per-channel padding VALUE as well (pemp_conv2d_padv_nhwc_f32 + the split-K tile ids): the dilated ASPPV2
 * branch convs of a one-episode evaluation step.                                                                        */
int pemp_conv2d_padv_splitk_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* scale,
                                     const float* shift, const float* residual, const float* pad_value, void* ws,
                                     size_t ws_bytes, void* stream);
void* pemp_uncached_alloc(size_t bytes);       /* zero-filled; NULL on failure (pemp_last_error) */
int pemp_uncached_free(void* p);
/* One idle wave for `us` microseconds on `stream` (no memory traffic).  Two of them on two streams take `us` when the streams
 * run concurrently and 2 x `us` when the runtime maps both to one hardware queue: the training engine uses it to choose a side
 * stream that really runs beside the main one (HIP deals streams round-robin to a few hardware queues).                    */
int pemp_spin_us(int us, void* stream);
/* Zero the arrival counters (first 1024 bytes) of a split-K workspace on `stream`: the kernels leave them zero, a launch
 * that failed may not have -- the host side calls this before it reports the failure.                                     */
int pemp_splitk_reset(void* ws, void* stream);
int pemp_conv2d_stats_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, float* stats,
                               void* ws, size_t ws_bytes, void* stream);
int pemp_conv2d_stats_rows(const pemp_conv_desc* d);
/* The same statistics conv on the SPLIT3 family, for weights that do not change between steps (the frozen trunk of a head
 * trainer: networks/canet.py, pfenet.py, rpmms.py run it forward only, in train()): `w3` is the pemp_pack_split3_bf16 form of
 * the [Cout][Kpad] weight.  d->tile: 0 (runs as 43) or 41, 42, 43, 44, 46 -- the unsplit ids, on their own wave grids.  The K
 * loop and the MFMA order are those of the plain split3 conv: y is bit-identical to pemp_conv2d_nhwc_f32 with the same id (no
 * affine), hence fp32-accurate and NOT bit-identical to the fp32-chain entry above.  stats follows that entry's contract: one
 * row per row tile, pemp_conv2d_stats_split3_rows(d) x 2 x Cout floats, summed over the rows m < M of the tile in the fixed
 * order of the fp32-chain epilogue; no atomics, deterministic.  No workspace.  d->flags must be 0; Cout % 64 (% 128 for the
 * 128-wide ids), Cin % 32, Kpad == KH*KW*Cin as above.  Returns -1 (pemp_last_error set, nothing launched) for every other
 * id -- the persistent ids 47 / 49, the panel ids 71 / 72, the pre-split ids 146 / 149, split-K 51..56, any fp32-chain id --
 * for any flag and for a null or misaligned pointer; -2 where the buffer-addressed kernels do not take the geometry (use
 * pemp_conv2d_nhwc_f32 + pemp_bn_stats_f32 then).  No padding vector, residual or BatchNorm-backward form.
 * pemp_conv2d_stats_split3_rows: ceil(M / BM) of the id, 0 for an id the entry does not take.
 * (The launching entry is named pemp_split3_conv2d_..., not pemp_conv2d_..._split3: bench.py's live roofline keeps a table of
 * every launching pemp_conv2d* entry, which tests/test_cpu_suite.py holds complete, and the benchmark is not part of this
 * addition -- its workloads train their trunks and never reach this entry.)                                                */
int pemp_split3_conv2d_stats_nhwc_f32(const pemp_conv_desc* d, const float* x, const void* w3, float* y, float* stats,
                                      void* stream);
int pemp_conv2d_stats_split3_rows(const pemp_conv_desc* d);
int pemp_bn_stats_partials_f32(const float* stats, int nrows, int M, int C, float eps, float momentum, float* mean,
                               float* invstd, float* run_mean, float* run_var, void* stream);
int pemp_bn_fwd_partials_f32(const float* z, int ldz, const float* stats, int nrows, int M, int C, float eps, float momentum,
                             const float* gamma, const float* beta, const float* residual, int ldr, float* y, int ldy,
                             int relu, uint32_t* mask, float* mean, float* invstd, float* run_mean, float* run_var,
                             void* stream);

/* The input-gradient conv whose result is the gradient at the OUTPUT of a train-mode BatchNorm(+ReLU) (autograd of
 * BottleNeck.forward, networks/backbones.py:66-75: conv -> bn -> relu chains), with the first half of that BatchNorm's
 * backward in its epilogue:  o = conv(x, w) (+ residual);  g = o where the BatchNorm's ReLU let the value through
 * (bit c % 32 of mask[m][c / 32], from pemp_bn_apply_mask_f32; mask NULL: no ReLU, g = o);  y = g;  and per row tile
 *   stats[r][0][c] = sum g[m][c],   stats[r][1][c] = sum g[m][c] * (z[m][c] - mean[c]) * invstd[c]
 * (z: the BatchNorm's input, d->Cout channels, per-pixel stride ldz).  pemp_bn_bwd_partials_f32 finishes: dbeta / dgamma
 * from the partials (fixed order, double) and dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M): the separate reduction pass
 * over (dy, y, z) of pemp_bn_bwd_f32 and its second read of y are gone, and g doubles as the residual-branch gradient.
 * Same restrictions, tile ids, workspace and return codes as pemp_conv2d_stats_nhwc_f32; d->ldr = per-pixel stride of
 * residual.                                                                                                            */
int pemp_conv2d_bnbwd_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* w, float* y, const float* residual,
                               const uint32_t* mask, const float* z, int ldz, const float* mean, const float* invstd,
                               float* stats, void* ws, size_t ws_bytes, void* stream);
int pemp_bn_bwd_partials_f32(const float* g, int ldg, const float* z, int ldz, const float* mean, const float* invstd,
                             const float* gamma, const float* stats, int nrows, float* dz, int lddz, float* dgamma,
                             float* dbeta, int M, int C, void* stream);

/* Weight gradient of pemp_conv2d_nhwc_f32 (autograd of nn.Conv2d, same call sites):
 *   dw[co][kh][kw][ci] (+)= sum_m g[m][co] * x[pix(m,kh,kw)][ci]      dw is KRSC with row length d->Kpad
 * `d` describes the FORWARD conv (d->ldy = per-pixel stride of g).  STEM4 needs Kpad % 64 == 0.  d->tile: bits 0..7 = kernel choice
 * (0: library's, 1: first generation, 2 / 3: second generation with 128 x 128 / 64 x 64 tiles where the channel counts allow),
 * bits 8.. = number of blocks to aim for when the pixel rows are split over
 * blocks (0: 768; the partial sums of different splits round differently -- same value for workspace query and launch). */
size_t pemp_conv2d_wgrad_workspace_bytes(const pemp_conv_desc* d);
int pemp_conv2d_wgrad_nhwc_f32(const pemp_conv_desc* d, const float* x, const float* g, float* dw,
                               int accumulate, void* ws, size_t ws_bytes, void* stream);

/* nn.BatchNorm2d in train mode (networks/backbones.py:48-52; batch statistics, momentum update
 * of the running statistics with the unbiased variance): per-channel mean / 1/sqrt(var+eps).  */
size_t pemp_colsum_workspace_bytes(int M, int C);
int pemp_bn_stats_f32(const float* z, int ldz, int M, int C, float eps, float momentum,
                      float* mean, float* invstd, float* run_mean, float* run_var,
                      void* ws, size_t ws_bytes, void* stream);
/* y = relu?((z-mean)*invstd*gamma + beta (+ residual))  (BottleNeck.forward, backbones.py:66-75) */
int pemp_bn_apply_f32(const float* z, int ldz, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, const float* residual, int ldr,
                      float* y, int ldy, int M, int C, int relu, void* stream);
/* The same, also leaving the sign of y as one bit per value (mask[m][c / 32] bit c % 32 = y[m][c] > 0; M x C/32 words; NULL:
 * none) for the fused backward above.  C in {32, 64, 128, 256, 512, 1024} when mask is given.                          */
int pemp_bn_apply_mask_f32(const float* z, int ldz, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, const float* residual, int ldr,
                      float* y, int ldy, int M, int C, int relu, uint32_t* mask, void* stream);
/* backward of the above: g = dy*(y>0 if relu) [optionally stored to gout = gradient of the residual
 * branch]; dgamma = sum g*xhat, dbeta = sum g, dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M).     */
int pemp_bn_bwd_f32(const float* dy, int lddy, const float* y, int ldy, const float* z, int ldz,
                    const float* mean, const float* invstd, const float* gamma,
                    float* dz, int lddz, float* gout, int ldg, float* dgamma, float* dbeta,
                    int M, int C, int relu, void* ws, size_t ws_bytes, void* stream);
/* The same with the sign bits of y (pemp_bn_apply_mask_f32) standing in for y where mask is given: y is then not read. */
int pemp_bn_bwd_mask_f32(const float* dy, int lddy, const float* y, int ldy, const uint32_t* mask, const float* z, int ldz,
                    const float* mean, const float* invstd, const float* gamma,
                    float* dz, int lddz, float* gout, int ldg, float* dgamma, float* dbeta,
                    int M, int C, int relu, void* ws, size_t ws_bytes, void* stream);
/* g = (dy (+ add)) * (y>0 if relu); dbias[c] = sum_m g[m][c] (NULL: skip).  Backward of conv bias + ReLU
 * (networks/pemp_stage1.py:74-78, backbones.py:330-357).                                           */
int pemp_relu_bias_bwd_f32(const float* dy, int lddy, const float* y, int ldy, const float* add, int lda,
                           float* g, int ldg, float* dbias, int M, int C, int relu,
                           void* ws, size_t ws_bytes, void* stream);
/* backward of nn.MaxPool2d (first maximum in scan order wins, as ATen).                           */
int pemp_maxpool2d_bwd_nhwc_f32(const float* x, const float* dy, float* dx, int N, int H, int W, int C,
                                int Ho, int Wo, int k, int s, int p, void* stream);
/* dst[n,hs*s,ws*s,:] = src[n,hs,ws,:], zero elsewhere: input gradient of a stride-s 1x1 conv.     */
int pemp_scatter_strided_nhwc_f32(const float* src, float* dst, int N, int H, int W, int Hs, int Ws,
                                  int C, int s, void* stream);
/* The KRSC weights of the input-gradient convs of EVERY conv layer of a flat parameter buffer, in one launch: layer l's
 * forward weight W[Cout][taps][Cin] at params + off becomes D[Cin][taps][Cout] (taps flipped) at mirror + off -- what
 * pemp_conv2d_nhwc_f32 needs to compute dL/dx as a convolution of dL/dy (autograd of nn.Conv2d w.r.t. its input,
 * reference entry/pemp_stage1.py:61).  table: device int32 [L][6] = {off, Cout, taps, Cin, first tile, tiles along Cin},
 * tiles of 32 x 32 (Cout x Cin) per tap; total_tiles = their sum.  Refreshed once per training step.                     */
int pemp_dgrad_mirror_f32(const float* params, float* mirror, const int32_t* table, int L, int total_tiles, void* stream);
/* dst[n][i][c] += v[n][c] / HW : backward of F.adaptive_avg_pool2d(x,(1,1)).                      */
int pemp_gap_bwd_add_nhwc_f32(const float* v, float* dst, int ld, int N, int HW, int C, void* stream);
/* Same as pemp_eval_tail_f32 with per-pixel CE weights (CELossDT, core/losses.py:33-43): stats[b][0] =
 * sum w*ce over valid pixels, stats[b][1] = sum of w over ALL pixels (the reference's denominator).   */
int pemp_eval_tail_weighted_f32(const float* pred, const int64_t* target, const float* weight,
                                uint8_t* pred_out, float* logits_out, double* stats, void* ws,
                                size_t ws_bytes, int B, int h, int w, int Ho, int Wo, void* stream);

/* CELossDT.boundary2weight (core/losses.py:23-31,35-41): boundary of the fg mask (3x3 dilate/erode), exact
 * Euclidean distance transform, weight = exp(-edt/sigma^2) + 1, all on the device (the reference calls scipy
 * on the host every step).  target int64 [B][H][W] -> weight fp32 [B][H][W].                          */
size_t pemp_cedt_workspace_bytes(int B, int H, int W);
int pemp_cedt_weight_f32(const int64_t* target, float* weight, void* ws, size_t ws_bytes,
                         int B, int H, int W, float sigma, void* stream);

/* Backward of the prototype head under mean cross-entropy: reverse of networks/pemp_stage1.py:142-163,
 * 195-261 + core/losses.py:10.  Inputs are the forward's operands and by-products:
 *   fwd_ws  the workspace pemp_mpm_protos_f32 (p > 0) / pemp_masked_avg_pool_f32(full_res=0) (p == 0) left
 *           behind for the same features and masks; protos [B][J][c]; pred [B][2][n];
 *   target int64 [B][Ho][Wo]; stats [B][8] from pemp_eval_tail_f32 (valid-pixel counts).
 * Outputs: dsup [B*S][n][ldd], dqry [B][n][ldd] (feature gradients), dctr [c][2p] (NULL when p == 0). */
/* The last B * 2 * n int32 words of the workspace receive, per (episode, group, query pixel), the prototype row the cosine
 * backward routed the gradient to (group 0 = foreground rows [0, p), group 1 = background rows [p, 2p); first maximum).    */
size_t pemp_head_bwd_workspace_bytes(int B, int S, int n, int c, int p);
int pemp_head_bwd_f32(const float* sup_feat, const float* qry_feat, int ldf, const float* mask,
                      const float* ctr, const void* fwd_ws, const float* protos, const float* pred,
                      const int64_t* target, const float* weight /* NULL or [B][Ho][Wo] */,
                      const double* stats, float* dsup, float* dqry, int ldd,
                      float* dctr, void* ws, size_t ws_bytes, int B, int S, int h, int w, int H, int W,
                      int Ho, int Wo, int c, int p, int map_full_res /* Baseline: fwd_ws from full_res=1 */,
                      float dist_scalar, void* stream);

/* The same backward for an ARBITRARY upstream gradient of the model output (what autograd's loss.backward()
 * hands to `model(sup, msk, qry, out_shape)`, entry/pemp_stage1.py:59-61): dlogits [B][2][Ho][Wo] replaces
 * (pred, target, weight, stats); the adjoint of the bilinear upsample is applied to it directly.             */
int pemp_head_bwd_dlogits_f32(const float* sup_feat, const float* qry_feat, int ldf, const float* mask,
                              const float* ctr, const void* fwd_ws, const float* protos, const float* dlogits,
                              float* dsup, float* dqry, int ldd, float* dctr, void* ws, size_t ws_bytes,
                              int B, int S, int h, int w, int H, int W, int Ho, int Wo, int c, int p,
                              int map_full_res, float dist_scalar, void* stream);

/* nn.utils.clip_grad_norm_(params, max_norm) + SGD(momentum, weight_decay).step() on flat buffers
 * (entry/pemp_stage1.py:63-64, core/solver.py:87-91).  grad_scale multiplies the gradients first
 * (1/world after a SUM all-reduce); max_norm <= 0 disables clipping; grad_norm_out[0] = ||g||_2.  */
size_t pemp_sgd_workspace_bytes(void);
int pemp_sgd_clip_step_f32(float* params, const float* grads, float* momentum_buf, long long n,
                           float max_norm, float lr, float momentum, float weight_decay, int first_step,
                           float grad_scale, int nesterov, float* grad_norm_out, void* ws, size_t ws_bytes,
                           void* stream);
/* clip_grad_norm_(max_norm) + torch.optim.Adam(lr, betas, eps, weight_decay).step() (reference core/solver.py:92-96,
 * tr.opt = adam; ATen's operation order, L2 weight decay, no amsgrad).  exp_avg / exp_avg_sq: the optimizer state, zero before
 * the first update; step: 1-based number of this update.  Workspace: pemp_sgd_workspace_bytes().  lr / betas / eps /
 * weight_decay are doubles because torch.optim.Adam holds them as Python floats and forms 1 - beta, lr / bias1 and
 * sqrt(bias2) in double before narrowing each to float once (float(1 - 0.999) != 1.f - 0.999f by 1.3e-5 relative).        */
int pemp_adam_clip_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                            float max_norm, double lr, double beta1, double beta2, double eps, double weight_decay,
                            long long step, float grad_scale, float* grad_norm_out, void* ws, size_t ws_bytes, void* stream);

/* Train-time regularisers.  Random numbers: counter-based Philox4x32-10, element i of stream (seed, offset)
 * (reproducible across launches / graph replays; the reference's torch generator stream is not reproducible,
 * so the DRAWS are parity-unpinned).  `uniforms` != NULL substitutes caller-provided U[0,1) numbers -- that is
 * how the tests check the arithmetic exactly.
 *
 * DropBlock2D.forward (dropblock==0.3.0; call sites networks/pemp_stage1.py:76,79; backbones.py:329-353):
 *   seed map (u < drop_prob / block_size^2) per (image, y, x), dilated by max_pool2d(block_size, 1, block_size/2)
 *   (cropped for even sizes); mask = 1 - dilated [N][H][W]; kept_count[0] = sum(mask) (int, exact).           */
/*   step (device pointer or NULL): the stream offset becomes offset + (*step << 20), so a captured hipGraph draws
 *   fresh numbers on every replay once the caller increments *step.                                          */
int pemp_dropblock_mask_f32(float* mask, int* kept_count, const float* uniforms, int N, int H, int W,
                            float drop_prob, int block_size, uint64_t seed, uint64_t offset,
                            const uint64_t* step, void* stream);
/*   y[m][c] = ((x[m][c] * mask[m]) * M) / kept_count   (the layer's forward AND its backward)               */
int pemp_pixel_scale_f32(const float* x, int ldx, const float* mask, const int* kept_count, float* y, int ldy,
                         long long M, int C, void* stream);
/* nn.Dropout2d(p) in train() (networks/pemp_stage2.py:67,70; backbones.py:284-305):
 *   mask[n][c] = (u < 1 - p) / (1 - p);   y[n][i][c] = x[n][i][c] * mask[n][c]  (forward and backward)      */
int pemp_dropout2d_mask_f32(float* mask, const float* uniforms, int N, int C, float p, uint64_t seed,
                            uint64_t offset, const uint64_t* step, void* stream);
int pemp_channel_scale_f32(const float* x, int ldx, const float* mask, float* y, int ldy, int N, int HW, int C,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Episode input pipeline on the device: everything
 * PascalVOCTrain._get_episode (data_kits/pascal_voc.py:185-237) does AFTER the JPEG/PNG decode, on
 * uint8 arrays uploaded as one blob:
 *   F.resize(img, BILINEAR) :144   Pillow ImagingResample, 8-bit fixed point (22 fraction bits),
 *                                  horizontal pass then vertical pass, each rounded to uint8 -- bit-exact;
 *   ColorJitter(.4,.4,.4)   :146   ImageEnhance Brightness/Contrast/Color = Image.blend with a black /
 *                                  mean-gray / gray image, in the drawn order -- bit-exact for given factors;
 *   F.hflip                 :143   ; crop_obj window :26-84 (origin chosen by the host);
 *   ToTensor + Normalize    :141-142  ((x / 255) - mean) / std in fp32 -- bit-exact;
 *   F.resize(label, NEAREST):145   Pillow ImagingScaleAffine (source coordinate accumulated in double);
 *   mask // 255 -> stack(fg, 1 - fg) :209-210 (support) / int64 label :231 (query).
 * One descriptor per decoded sample.  The host fills the first block of fields, calls
 * pemp_episode_plan() (fills the "planned" fields, returns the workspace size), uploads descriptors and
 * pixels, then calls pemp_episode_preprocess().                                                    */
typedef struct pemp_sample_desc {
    int64_t img_off;       /* byte offset of the HWC uint8 RGB source inside blob; < 0: no image        */
    int64_t msk_off;       /* byte offset of the HW uint8 label source ({0,255}); < 0: no label         */
    int64_t img_out;       /* element offset in img_out of this sample's [3][H][W] fp32 result          */
    int64_t msk_out;       /* element offset in planes_out (mask_mode 1) / label_out (modes 2, 3)       */
    int32_t hs, ws;        /* source height, width                                                      */
    int32_t sh, sw;        /* size after F.resize (eval: H, W; train: int(H*f), int(W*f), f in [1,1.5])   */
    int32_t oy, ox;        /* crop window origin inside the resized (and flipped) image; window = H x W */
    int32_t flip;          /* 1: horizontal flip after resize / jitter                                  */
    int32_t jitter_order;  /* 0: no jitter; else stage0 | stage1<<2 | stage2<<4 with 1 = brightness,
                              2 = contrast, 3 = saturation                                              */
    float jitter[3];       /* enhancement factors (brightness, contrast, saturation)                    */
    int32_t mask_mode;     /* 0 none; 1 support planes fp32 [2][H][W]; 2 label int64 [H][W] (resized,
                              flipped, cropped); 3 label int64 [hs][ws] (query at test time: not resized) */
    /* planned (pemp_episode_plan): */
    int32_t ksx, ksy;      /* filter taps per output pixel, horizontal / vertical                       */
    int64_t ws_off;        /* byte offset of this sample's tables and intermediates in the workspace    */
} pemp_sample_desc;

/* Validates descs[0..n) (host memory), fills ksx/ksy/ws_off; returns the workspace bytes (0 on error). */
size_t pemp_episode_plan(pemp_sample_desc* descs_host, int n, int H, int W);
/* blob, descs_dev, outputs, ws: device memory; descs_host: the same descriptors in host memory (read
 * during the call only).  mean/std: host pointers to 3 floats.                                        */
int pemp_episode_preprocess(const uint8_t* blob, const pemp_sample_desc* descs_host,
                            const pemp_sample_desc* descs_dev, int n, int H, int W,
                            const float* mean, const float* std, float* img_out, float* planes_out,
                            int64_t* label_out, void* ws, size_t ws_bytes, void* stream);

/* ---- PFENet inference (networks/pfenet.py) ---------------------------------------------------------------------------
 * Prior mask (:201-226): q NHWC [B][HW][C] (pixel stride ldq), s NHWC [B*S][HW][C] (lds), mask [B*S][HW] (the support masks
 * at feature resolution).  Per episode b and shot i: sim[q] = max_p dot(q, m_p s_p) / (|m_p s_p| |q| + 1e-7) on the fp32 MFMA,
 * with fl(m_p * s_p) formed on operand load, the norms and the max over p fused into the GEMM epilogue (the HW x HW matrix
 * never reaches memory: per 64-pixel support tile one partial max per query pixel, ws); then (sim - min) / (max - min + 1e-7)
 * over q and the mean over the shots in order -> out [B][HW].  Deterministic: the maxima are exact, every sum in fixed
 * order.  C % 32 == 0; any HW.                                                                                        */
size_t pemp_prior_mask_workspace_bytes(int B, int S, int HW);
int pemp_prior_mask_f32(const float* q, int ldq, const float* s, int lds, const float* mask, float* out, void* ws,
                        size_t ws_bytes, int B, int S, int HW, int C, void* stream);
/* Support banks of the prior: the support operand of K classes stored once, met by any number of queries.
 * Pack: s NHWC [K*S][HW][C] (pixel stride lds), mask [K*S][HW] -> one slot of cap rows per (class, shot):
 *   rows  [K*S][cap][C]  fl(m_p * s_p) of the pixels with m_p != 0, in pixel order; then ONE all-zero row if a pixel with
 *                        m_p == 0 exists (such a pixel's similarity is exactly +0 for every query)
 *   norms [K*S][cap]     |m_p s_p| per stored row, summed in pemp_prior_mask_f32's order
 *   count [K*S] int32    rows stored, 1 .. HW (device memory)
 * Slots at or beyond count are not written; a row that does not fit into cap is dropped while count still says how many
 * rows the image needs (the caller compares it with cap).  rows == norms == NULL: only count is written (s, C, cap unused).
 * cap % 64 == 0, C % 32 == 0.  Deterministic: the compaction is an integer scan.                                      */
int pemp_prior_bank_pack_f32(const float* s, int lds, const float* mask, float* rows, float* norms, int32_t* count,
                             int KS, int HW, int C, int cap, void* stream);
/* The prior of N queries against a packed bank: q NHWC [N][HW][C] (ldq).
 *   index NULL:            every query against every class -> out [N][K][HW]
 *   index [N] int32 (dev): query n against class index[n] (clamped into 0..K-1) -> out [N][HW]
 * One block per (query tile, shot, query-class pair) walks the ceil(count / 64) support tiles of its slot on the fp32
 * MFMA and keeps the max in registers; then the per-shot min-max normalisation and the shot mean of pemp_prior_mask_f32.
 * For every (n, k) the output is bit for bit pemp_prior_mask_f32's on query n and the supports class k was packed from.
 * Query-class pairs and S <= 65535.  ws: pemp_prior_bank_workspace_bytes(pairs, S, HW).                             */
size_t pemp_prior_bank_workspace_bytes(int pairs, int S, int HW);
int pemp_prior_bank_f32(const float* q, int ldq, const float* rows, const float* norms, const int32_t* count,
                        const int32_t* index, float* out, void* ws, size_t ws_bytes, int N, int K, int S, int HW, int C,
                        int cap, void* stream);
/* Rows of a [K][C] table by the same selection: index [N] -> dst [N][C] = src[index[n]]; NULL -> dst [N][K][C] = src[k]. */
int pemp_bank_gather_rows_f32(const float* src, const int32_t* index, float* dst, int N, int K, int C, void* stream);
/* nn.AdaptiveAvgPool2d((Ho, Wo)) on NHWC (pfenet.py:244-247): windows [floor(i H / Ho), ceil((i + 1) H / Ho)), also for
 * Ho > H; x and y are channel slices with pixel strides ldx / ldy.                                                    */
int pemp_adaptive_avgpool_nhwc_f32(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int Ho, int Wo,
                                   void* stream);
/* F.interpolate(mode="bilinear", align_corners=True) [N][hi][wi] -> [N][ho][wo] over C channels, any sizes (1-pixel sides
 * included).  Element (n, pixel, c) of x lives at n * xn + pixel * ldx + c * xc (of y: n * yn + pixel * ldy + c * yc), so a
 * channel slice, a mask plane or an NCHW output is addressed directly.  flags & 1: x is read as (x == 1) (pfenet.py:182). */
int pemp_resize_bilinear_ac_nhwc_f32(const float* x, long long xn, int ldx, int xc, float* y, long long yn, int ldy, int yc,
                                     int N, int C, int hi, int wi, int ho, int wo, int flags, void* stream);
/* Weighted_GAP (pfenet.py:15-20) per support image, averaged over the S shots of an episode (:229-233): feat NHWC
 * [B*S][h][w][C] (ldf), mask [B*S][h][w] -> out [B][C] = mean_i sum(f m) / (sum(m) + 5e-4) (as avg_pool2d * h * w).   */
int pemp_weighted_gap_f32(const float* feat, int ldf, const float* mask, float* out, int B, int S, int h, int w, int C,
                          void* stream);
/* y[p][c] = x[p][c] * m[p] (m may be NULL) + r[p][c] (r may be NULL) over npix NHWC pixels: the masked layer-4 input of
 * the supports (pfenet.py:193) and the FEM's "relu(conv(.)) + x" sums (:261,264,270), whose ReLU comes before the add.  */
int pemp_scale_add_nhwc_f32(const float* x, int ldx, const float* m, const float* r, int ldr, float* y, int ldy,
                            long long npix, int C, void* stream);

/* ---- CANet inference (networks/canet.py, entry/canet.py) --------------------------------------------------------------
 * Support vector of the dense comparison (canet.py:175-178): feat NHWC [B*S][h][w][C] (ldf), mask [B*S][2][H][W] (plane 0
 * is read, sampled nearest to h x w with ATen's rule min(floor(dst * (float)H / h), H - 1)) ->
 * out[b][c] = mean_s( sum_p f m / (sum_p m + 1e-5) ).  C % 4 == 0; fixed summation order.                               */
int pemp_canet_support_vector_f32(const float* feat, int ldf, const float* mask, float* out, int B, int S, int h, int w,
                                  int H, int W, int C, void* stream);
/* The z half of layer55 (canet.py:179-181: a 3x3, dilation dil, zero padding dil conv over cat(query, z broadcast)):
 * T[b][tap][co] = sum_ci wz[tap][co][ci] z[b][ci] (T: [B][9][Cout] scratch of the caller), then
 * R[b][y][x][co] = sum of T[b][tap][co] over the taps whose source pixel lies inside the image, in tap order (NHWC, pixel
 * stride ldr).  R is the `residual` of the conv over the query channels: relu(conv + bias + R) = relu(layer55(cat)).    */
int pemp_canet_zterm_f32(const float* wz, const float* z, float* T, float* R, int ldr, int B, int h, int w, int Cin,
                         int Cout, int dil, void* stream);
/* Input of a pre-activation residual block (the leading nn.ReLU of canet.py:103-104 and the cat of :193):
 * y[b][p][0..C) = relu(x[b][p][:]); nhist == 2: also y[b][p][C..C+2) = relu(history), read from row b of hist [B][2][HW]
 * (slot == NULL), from row slot[b] of a table hist [nslots][2][HW] (slot: device int32 [B]; a slot outside 0..nslots-1:
 * zeros, "no history yet", data_kits/pascal_voc.py:423-424), or zeros (hist == NULL).  nhist == 0: the ReLU copy only.  C, ldx, ldy multiples of 4; ldx >= C, ldy >= C + nhist.         */
int pemp_canet_block_input_f32(const float* x, int ldx, const float* hist, const int* slot, int nslots, float* y, int ldy,
                               int B, int HW, int C, int nhist, void* stream);
/* F.softmax(pred, dim=1) of the low-resolution logits [B][2][HW] and its write-back (entry/canet.py:52,77-80): into row
 * slot[b] of table [nslots][2][HW] for every b with 0 <= slot[b] < nslots (table, slot may be NULL together) and / or into
 * out [B][2][HW] (may be NULL).  The caller names no slot twice in one call.                                             */
int pemp_canet_history_update_f32(const float* logits, float* table, const int* slot, int nslots, float* out, int B,
                                  int HW, void* stream);

/* ---- CANet head training (csrc/canet_bwd.hip): adjoints of the kernels above + the classifier's backward.  Every reduction is
 * a two-stage partial sum of fixed order (no atomics): bit-stable run to run.
 * Adjoint of pemp_canet_zterm_f32.  g NHWC [B][h][w][Cout] (ldg): the gradient at layer55's pre-activation.  W: the z half of
 * layer55's KRSC weight, W[(co * 9 + tap) * ldw + ci] (a column slice of [Cout][9][Cin_total]: ldw = Cin_total); z [B][Cin].
 *   G[b][tap][co]  = sum of g[b][y][x][co] over the pixels whose tap lands inside the image (an empty window: exactly 0)
 *   dz[b][ci]      = sum_tap sum_co W[co][tap][ci] G[b][tap][co]
 *   dW[(co * 9 + tap) * ldw + ci] = sum_b G[b][tap][co] z[b][ci]        (written, not accumulated; laid out as W)           */
size_t pemp_canet_zterm_bwd_workspace_bytes(int B, int h, int w, int Cout);
int pemp_canet_zterm_bwd_f32(const float* g, int ldg, const float* W, int ldw, const float* z, float* G, float* dz, float* dW,
                             void* ws, size_t ws_bytes, int B, int h, int w, int Cin, int Cout, int dil, void* stream);
/* Adjoint of pemp_canet_support_vector_f32: df[b*S+s][p][c] (ldd) = dz[b][c] * m / (S * (sum_p m + 1e-5)), m = plane 0 of mask
 * [B*S][2][H][W] sampled as the forward samples it.  An empty mask gives exact zeros.                                        */
int pemp_canet_support_vector_bwd_f32(const float* dz, const float* mask, float* df, int ldd, int B, int S, int h, int w,
                                      int H, int W, int C, void* stream);
/* Backward of a 1x1 conv to 2 classes (layer7), one pass: dpred [B][2][HW] (NCHW), x NHWC [B][HW][C] (ldx), W [2][C] ->
 * dx[b][p][:] (lddx) = dpred[b][0][p] W[0][:] + dpred[b][1][p] W[1][:], dW[k][c] = sum dpred[b][k][p] x[b][p][c], db[k].      */
size_t pemp_canet_cls_bwd_workspace_bytes(int M, int C);
int pemp_canet_cls_bwd_f32(const float* dpred, const float* x, int ldx, const float* W, float* dx, int lddx, float* dW, float* db,
                           void* ws, size_t ws_bytes, int B, int HW, int C, void* stream);
/* The first stage of pemp_head_bwd_f32 / pemp_head_bwd_dlogits_f32 on its own (the same kernel): dpred [B][2][h][w] = adjoint of
 * F.interpolate(pred, (Ho,Wo), bilinear, align_corners) applied to the mean-CE gradient from (pred, target int64 [B][Ho][Wo],
 * weight [B][Ho][Wo] | NULL, stats [B][8] of pemp_eval_tail_f32 or pemp_eval_tail_weighted_f32), or to `dlogits` [B][2][Ho][Wo] when given.        */
int pemp_upsample_ce_bwd_f32(const float* pred, const int64_t* target, const float* weight, const double* stats,
                             const float* dlogits, float* dpred, int B, int h, int w, int Ho, int Wo, void* stream);

/* ---- PFENet head training (csrc/pfenet_bwd.hip): adjoints of the streaming PFENet kernels above.  Every output element is
 * written once by one thread that gathers its terms in a fixed order, every reduction is a two-stage partial sum of fixed
 * shape (no atomics): bit-stable run to run.
 * Adjoint of pemp_weighted_gap_f32: dfeat[b*S+s][p][c] (ldd) = dvec[b][c] * (mask / area / S), area = sum_p mask + 5e-4 added
 * up and rounded as the forward does.  mask [B*S][h][w]; an all-zero mask gives exact zeros.  C % 4 == 0.                */
int pemp_weighted_gap_bwd_f32(const float* dvec, const float* mask, float* dfeat, int ldd, int B, int S, int h, int w, int C,
                              void* stream);
/* Adjoint of nn.AdaptiveAvgPool2d for up to four output sizes at once: dx NHWC [N][H][W][C] (lddx) = sum_k A_k^T g_k with
 * g_k NHWC [N][bin_h[k]][bin_w[k]][C] (ldg[k]); g, ldg, bin_h, bin_w: host arrays of nbins entries.  Gather form: a pixel adds,
 * over the bins in index order and the windows that contain it in row-major order, g / kh / kw; dx is written, never read.
 * Windows follow pemp_adaptive_avgpool_nhwc_f32 (bins larger or smaller than the map).  C % 4 == 0.                      */
int pemp_adaptive_avgpool_bwd_multi_nhwc_f32(int nbins, const float* const* g, const int* ldg, const int* bin_h, const int* bin_w,
                                             float* dx, int lddx, int N, int H, int W, int C, void* stream);
/* Adjoint of pemp_resize_bilinear_ac_nhwc_f32 (hi x wi -> ho x wo, either direction, 1-pixel sides included): dx [N][hi][wi] =
 * add + A^T dy, dy [N][ho][wo], over C channels; element (n, pixel, c) of a tensor at n * tn + pixel * ld + c * tc as in the
 * forward.  add may be NULL, and may be dx itself.  The weights are the forward's.                                        */
int pemp_resize_bilinear_ac_bwd_nhwc_f32(const float* dy, long long dyn, int lddy, int dyc, const float* add, long long addn,
                                         int ldadd, int addc, float* dx, long long dxn, int lddx, int dxc, int N, int C, int hi,
                                         int wi, int ho, int wo, void* stream);
/* The support half of PFENet's init_merge convs (pfenet.py:251-252; the forward runs it as a per-image shift), all bins in one
 * launch sequence.  g_k NHWC [B][bin_h[k]][bin_w[k]][Cout] (ldg[k]): the gradient at conv k's pre-activation; W[k] / dW[k]: the
 * support columns of conv k's [Cout][ldw] weight / weight gradient (the pointer already at the first support column);
 * svec [B][Cin].  c_k[b][co] = sum_p g_k[b][p][co];  dsvec[b][ci] = sum_k sum_co W_k[co][ci] c_k[b][co];
 * dW_k[co][ci] = sum_b c_k[b][co] svec[b][ci] (written, not accumulated).  Cout % 4 == 0.                                 */
size_t pemp_pfenet_merge_support_bwd_workspace_bytes(int nbins, int B, int Cout);
int pemp_pfenet_merge_support_bwd_f32(int nbins, const float* const* g, const int* ldg, const int* bin_h, const int* bin_w,
                                      const float* const* W, float* const* dW, int ldw, const float* svec, float* dsvec, void* ws,
                                      size_t ws_bytes, int B, int Cin, int Cout, void* stream);

/* ---- RPMMs inference (networks/rpmms.py) -----------------------------------------------------------------------------
 * The EM of the prototype mixture models (PMMs.EM :65-86) for the mixtures K = 1 | 3 | 6 side by side (10 columns), foreground
 * (side 0, pixel weight m) and background (side 1, weight 1 - m): feat NHWC [B][h][w][C] (ldf), mask [B][h][w], mu0 [10][C]
 * (row 0: K = 1, rows 1..3: K = 3, rows 4..9: K = 6; unit rows) -> mu_out [B][2][10][C].  Per iteration, with x_p = wgt_p f_p:
 * s_pj = softmax_j(20 <x_p, mu_j>) inside each mixture, mu'_j = sum_p x_p s_pj / (1e-6 + sum_p s_pj), mu_j = mu'_j / (1e-6 +
 * |mu'_j|).  One launch per iteration over G = min(16, ceil(h w / 64)) pixel slices per (image, side) plus one final reduction,
 * all enqueued here; the slices' partial sums ping-pong through `work`, 2 * B * 2 * G * (10 * C + 16) floats of the caller.
 * C == 256.  Fixed summation orders; an image's result does not depend on B.                                              */
int pemp_rpmms_em_f32(const float* feat, int ldf, const float* mask, const float* mu0, float* work, float* mu_out, int B,
                      int h, int w, int C, int iters, void* stream);
/* The probability maps (rpmms.py:119-139): per query pixel and mixture the softmax over the 2K dots <q, [mu_f | mu_b]>, P_f =
 * sum of the first K, P_b = sum of the last K.  qry NHWC [B][HW][C] (ldq), mu [B][2][10][C] -> mixture g (0..2):
 * out[g * gstride + (b * HW + p) * ldo + C] = P_b, [... + C + 1] = P_f.  C == 256.                                        */
int pemp_rpmms_prob_map_f32(const float* qry, int ldq, const float* mu, float* out, int ldo, long long gstride, int B, int HW,
                            int C, void* stream);
/* The sum over a mixture's prototypes of layer55(cat(query, prototype)) (rpmms.py:237-244; a 3x3, dilation dil, zero padding
 * dil conv + bias + ReLU) from ONE conv of the query: T[b][i][tap][co] = sum_ci wz[tap][co][ci] mu[b][0][i][ci] (T: [B][10][9][C]
 * scratch of the caller; wz [9][C][C]), then, for mixture g,
 * out[g * gstride + (b * h * w + p) * ldo + c] = sum_{i in g, ascending} relu(base[b][p][c] + bias[c] + sum of T[b][i][tap][c]
 * over the taps whose source pixel lies inside the image, in tap order).  base NHWC (ldb): the conv of the query with the
 * query half of the weights, no bias, no ReLU.  C == 256.                                                                */
int pemp_rpmms_proto_sum_f32(const float* wz, const float* mu, const float* base, int ldb, const float* bias, float* T,
                             float* out, int ldo, long long gstride, int B, int h, int w, int C, int dil, void* stream);
/* RPMMs support banks.  The first launch of pemp_rpmms_proto_sum_f32 on its own, for K classes:
 * T[k][i][tap][co] = sum_ci wz[tap][co][ci] mu[k][0][i][ci].   wz [9][C][C], mu [K][2][10][C], T [K][10][9][C].  C == 256. */
int pemp_rpmms_proto_taps_f32(const float* wz, const float* mu, float* T, int K, int C, void* stream);
/* layer56's input for P (query, class) pairs in ONE launch.  qry: layer5 of the queries, NHWC [N][h*w][C] (ldq).  base: their
 * conv with the query half of layer55, NHWC (ldb), no bias, no ReLU.  mu [K][2][10][C], T [K][10][9][C] as above.
 *   index NULL:                P = N * K, pair n * K + k is query n against class k
 *   index (device int32 [N]):  P = N, pair n is query n against class index[n] (values checked by the caller on the host)
 * For mixture g = 0..2 and pair r:
 *   out[g * gstride + (r * h * w + p) * ldo + c], c < C = pemp_rpmms_proto_sum_f32's value for (base[n], bias, T[k])
 *   out[... + C] = P_b, out[... + C + 1] = P_f          = pemp_rpmms_prob_map_f32's values for (qry[n], mu[k])
 * bit for bit; channels C + 2 .. ldo - 1 are not written.  A block walks the classes of its query's 16-pixel chunk with the
 * chunk's qry and base rows in LDS: they are read once per pixel, not once per class.  ldq, ldb, ldo, gstride % 4 == 0, ldo >= C + 2, operands 16-byte aligned,
 * N * K <= 65535.  C == 256.                                                                                                */
int pemp_rpmms_bank_l56_f32(const float* qry, int ldq, const float* base, int ldb, const float* bias, const float* mu,
                            const float* T, const int32_t* index, float* out, int ldo, long long gstride, int N, int K, int h,
                            int w, int C, int dil, void* stream);

/* ---- RPMMs head training (csrc/rpmms_bwd.hip): layer55 over the ten prototype columns with one Dropout2d draw per column, its
 * adjoint, and the adjoint of the softmax that makes the next pass's history.  No atomics; the one cross-block sum goes through
 * `work` in a fixed order: bit-stable run to run.  C == 256.
 * pemp_rpmms_proto_sum_f32 with a multiplier mult [B][10][C] (0 or 1 / (1 - p)) on each column's ReLU output before the sum
 * over a mixture's columns: out_g = sum_{i in g, ascending} mult_i * relu(base + bias + R_i).  The same tap order and the same
 * sum: with every multiplier 1.0 the output is pemp_rpmms_proto_sum_f32's, bit for bit.  T is written as there.            */
int pemp_rpmms_proto_sum_train_f32(const float* wz, const float* mu, const float* base, int ldb, const float* bias,
                                   const float* mult, float* T, float* out, int ldo, long long gstride, int B, int h, int w, int C,
                                   int dil, void* stream);
/* Its adjoint.  dout: the gradients at the three mixture outputs, dout[g * gstride + (b * h * w + p) * ldd + c]; base, bias, T,
 * mult as in the forward (every column's pre-activation is recomputed; no per-column gradient is materialised).
 *   dbase[b][p][c] (lddb) = sum_g sum_{i in g} mult_i 1[pre_i > 0] dout_g          (columns ascending)
 *   G[b][i][tap][c]       = sum of column i's gated gradient over the pixels whose tap source lies inside the image
 *   dW[(co * 9 + tap) * ldw + ci] = sum_b sum_i G[b][i][tap][co] mu[b][0][i][ci]    (optional; written, not accumulated: the
 *                           prototype half of layer55's KRSC weight gradient, the pointer already at its first column)
 *   dbias[c]              = sum_b sum_i G[b][i][4][c]                               (optional; = the sum of dbase over b, p)
 * work: pemp_rpmms_proto_sum_bwd_work_floats(B, h, w, C) floats of the caller.                                              */
size_t pemp_rpmms_proto_sum_bwd_work_floats(int B, int h, int w, int C);
int pemp_rpmms_proto_sum_bwd_f32(const float* dout, int ldd, long long gstride, const float* base, int ldb, const float* bias,
                                 const float* T, const float* mult, const float* mu, float* dbase, int lddb, float* G, float* dW,
                                 int ldw, float* dbias, float* work, size_t work_floats, int B, int h, int w, int C, int dil,
                                 void* stream);
/* Adjoint of the softmax over two classes (rpmms.py:250-251,285: the history of pass p + 1 is the softmax of pass p's logits):
 * dpred[b][k][p] += prob[b][k][p] * (dh_k - sum_j prob[b][j][p] dh_j), dh_k = dh[(b * HW + p) * ldh + k].  dpred, prob [B][2][HW]. */
int pemp_rpmms_history_bwd_f32(const float* dh, int ldh, const float* prob, float* dpred, int B, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEMP_HIP_H */
