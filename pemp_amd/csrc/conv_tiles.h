// Host side of the conv engine's dispatch: the ONE table of tile shapes, the decoder of tile ids (the id scheme itself is
// documented once, next to pemp_conv2d_tile_shape in pemp_hip.h), the compile-time dispatcher every launch entry goes through,
// and the two launch helpers they share.  No device code here.
#pragma once
#include <initializer_list>
#include "conv_common.h"

namespace pemp {

// ---- the table: shape index = last digit of a tile id -------------------------------------------------------------------
// BM x BN block, NW waves in a WGM x (NW / WGM) grid.  wgm3: the split3 family's wave grid on the same block (full-width wave
// strips where the block has as many 32-row strips as waves -- see launch_conv_dma2_split3; 0: the family has no such shape).
// 8: 16-row wave tiles (32 x 64 block).  9: the hybrid launch, whose main member is shape 3 (its rest runs on 16-row tiles).
struct TileShape { int bm, bn, wgm, nw, wgm3; };
inline constexpr TileShape kTileShapes[10] = {
    {0, 0, 0, 0, 0},
    {128, 128, 2, 4, 4},   // 1
    {128, 64, 2, 4, 4},    // 2
    {64, 64, 2, 4, 2},     // 3
    {128, 128, 4, 8, 4},   // 4
    {128, 64, 4, 8, 0},    // 5
    {256, 128, 4, 8, 8},   // 6
    {256, 256, 4, 8, 0},   // 7
    {32, 64, 2, 4, 0},     // 8
    {64, 64, 2, 4, 0},     // 9
};

// a table row as template constants; S3: with the split3 family's wave grid
template <int S, bool S3 = false>
struct Tile {
    static constexpr int BM = kTileShapes[S].bm, BN = kTileShapes[S].bn, NW = kTileShapes[S].nw;
    static constexpr int WGM = S3 ? kTileShapes[S].wgm3 : kTileShapes[S].wgm;
};

// ---- kernel families: the shapes each one instantiates (bit s = shape s) ---------------------------------------------------
constexpr unsigned shape_bits(std::initializer_list<int> l) {
    unsigned m = 0;
    for (int s : l) m |= 1u << s;
    return m;
}
struct FamIgemm { static constexpr unsigned shapes = shape_bits({1, 2, 3}); static constexpr bool s3 = false; };      // conv_igemm.hip
struct FamFp32 { static constexpr unsigned shapes = shape_bits({1, 2, 3, 4, 5, 6, 7}); static constexpr bool s3 = false; };    // also bf16, dropblock, conv_dma.hip
struct FamGroup { static constexpr unsigned shapes = shape_bits({1, 2, 3, 4, 5, 6, 7, 8}); static constexpr bool s3 = false; };
struct FamSplitK { static constexpr unsigned shapes = shape_bits({1, 2, 4, 5, 6, 7}); static constexpr bool s3 = false; };
struct FamSplit3 { static constexpr unsigned shapes = shape_bits({1, 2, 3, 4, 6}); static constexpr bool s3 = true; };
struct FamSplit3Stats { static constexpr unsigned shapes = shape_bits({1, 2, 3, 4, 6}); static constexpr bool s3 = true; };   // statistics epilogue
struct FamPersist { static constexpr unsigned shapes = shape_bits({3, 6}); static constexpr bool s3 = true; };
struct FamPanel { static constexpr unsigned shapes = shape_bits({1, 2}); static constexpr bool s3 = true; };     // conv_panel.hip: 128 rows x all of Cout, BN columns at a time

template <class Fam> inline bool in_family(int shape) { return shape >= 1 && shape <= 9 && ((Fam::shapes >> shape) & 1u); }

// f(Tile<shape, Fam::s3>{}) for a shape of the family; any other shape is an error (and instantiates nothing)
template <class Fam, int S = 1, class F>
int with_tile(int shape, F&& f) {
    if constexpr (S > 9) {
        set_error("conv: tile shape %d outside the kernel family", shape);
        return -1;
    } else {
        if constexpr ((Fam::shapes >> S) & 1u) {
            if (shape == S) return f(Tile<S, Fam::s3>{});
        }
        return with_tile<Fam, S + 1>(shape, f);
    }
}

// ---- tile ids ---------------------------------------------------------------------------------------------------------------
enum TileFamily { TILE_NONE = 0, TILE_IGEMM, TILE_DMA, TILE_DMA2, TILE_SPLIT3 };
struct TileId {
    int family;        // TILE_NONE: the id belongs to no decade of the scheme
    int shape;         // 1..9: row of kTileShapes (a persistent id: the shape it walks)
    bool splitk;       // 3x / 5x: the last round of tiles split along K
    bool persistent;   // 47, 49
    bool exists;       // some entry point takes the id
    bool panel;        // 71, 72: the activation-stationary 1x1 form (conv_panel.hip)
    bool presplit;     // 146, 149, 246, 249: the activations come pre-split (PEMP_CONV_IN_SPLIT3); the forms of 46 / 49
    bool row3;         // 246, 249: the tile of 146 / 149 with one A stage for the three taps of a kernel row (conv_row3.hip)
    bool ring;         // 349: the form of 49 on a three-deep activation ring, 1x1 convs without padding only (conv_ring.hip)
};

inline TileId decode_tile(int id) {
    TileId t = {TILE_NONE, 0, false, false, false, false, false, false, false};
    const int decade = id / 10, s = id % 10;
    if (id == 349) {
        t.family = TILE_SPLIT3, t.shape = 6, t.exists = t.persistent = t.ring = true;
        return t;
    }
    if (id == 146 || id == 149 || id == 246 || id == 249) {
        t.family = TILE_SPLIT3, t.shape = 6, t.exists = t.presplit = true, t.persistent = id % 10 == 9, t.row3 = id > 200;
        return t;
    }
    if (decade == 7 && in_family<FamPanel>(s)) {
        t.family = TILE_SPLIT3, t.shape = s, t.exists = t.panel = true;
        return t;
    }
    if (id < 1 || id > 56 || s == 0) return t;
    t.shape = s;
    if (decade == 0) t.family = TILE_IGEMM, t.exists = in_family<FamIgemm>(s);
    else if (decade == 1) t.family = TILE_DMA, t.exists = in_family<FamFp32>(s);
    else if (decade == 2) t.family = TILE_DMA2, t.exists = true;
    else if (decade == 3) t.family = TILE_DMA2, t.splitk = true, t.exists = in_family<FamSplitK>(s);
    else if (decade == 4 && (s == 7 || s == 9)) t.family = TILE_SPLIT3, t.persistent = t.exists = true, t.shape = s == 7 ? 3 : 6;
    else if (decade == 4) t.family = TILE_SPLIT3, t.exists = in_family<FamSplit3>(s);
    else t.family = TILE_SPLIT3, t.splitk = true, t.exists = in_family<FamSplit3>(s) && in_family<FamSplitK>(s);
    return t;
}

// Cout is a whole number of the shape's BN-wide tile columns
inline bool tile_cout_ok(int shape, int Cout) { return Cout % kTileShapes[shape].bn == 0; }
// ... as the entry points report it (`who`: the entry's name)
#define PEMP_REQUIRE_COUT(who, shape, Cout)                                                                              \
    do {                                                                                                                 \
        PEMP_REQUIRE(kTileShapes[shape].bn != 128 || tile_cout_ok(shape, Cout), "%s: tile N=128 needs Cout %% 128 == 0", who);   \
        PEMP_REQUIRE(kTileShapes[shape].bn != 256 || tile_cout_ok(shape, Cout), "%s: tile 256x256 needs Cout %% 256 == 0", who); \
    } while (0)

// ---- launches ---------------------------------------------------------------------------------------------------------------
// one launch with `lds` bytes of dynamic LDS (above 64 KiB the kernel has to be told first)
template <class Kern>
int allow_lds(Kern kern, size_t lds) {
    if (lds <= 64 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) set_error("hipFuncSetAttribute(lds=%zu): %s", lds, hipGetErrorString(e));
    return (int)e;
}

template <class Kern, class Args>
int launch_with_lds(Kern kern, int grid, int threads, size_t lds, hipStream_t st, const Args& args, const char* what) {
    const int rc = allow_lds(kern, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, args);
    return launch_status(what);
}

// operand staging of the fp32-chain / bf16 kernels (8 quads per row of A and B, double buffered) and of the split3 ones (B rows
// carry their three bf16 planes: 12 quads)
template <class T> constexpr size_t tile_lds() { return (size_t)2 * 8 * (T::BM + T::BN) * sizeof(v4f); }
template <class T> constexpr size_t tile_lds_s3() { return (size_t)2 * (8 * T::BM + 12 * T::BN) * sizeof(v4f); }
// ... with pre-split activations (ids 146 / 149): A rows carry their three planes too
template <class T> constexpr size_t tile_lds_a3() { return (size_t)2 * 12 * (T::BM + T::BN) * sizeof(v4f); }
template <class T> int tile_grid(const ConvArgs& a) { return cdiv(a.M, T::BM) * (a.Cout / T::BN); }

// points `a` at the split-K workspace of `plan` (counters first, then the partial tiles); -> the grid, or -1 (error set)
inline int bind_splitk(ConvArgs& a, const SplitKPlan& p, void* ws, size_t ws_bytes) {
    if (!ws || ws_bytes < p.ws_bytes || ((uintptr_t)ws & 15)) {
        set_error("conv split-K: workspace of %zu bytes needed (16-byte aligned), got %zu", p.ws_bytes, ws_bytes);
        return -1;
    }
    a.sk_cnt = (int*)ws;
    a.sk_ws = (float*)((char*)ws + 1024);
    a.sk_full = p.full;
    a.sk_S = p.pieces;
    return p.full + p.split * p.pieces;
}

}  // namespace pemp
