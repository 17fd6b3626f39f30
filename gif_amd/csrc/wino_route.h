// Which kernels a Winograd F(2x2, 3x3) forward / data-gradient call gets, and every size that follows from its shape: host-only, plain
// C++17, no HIP and no common.h, so that a host compiler builds it alone (tests/host/wino_route_dump.cpp prints it over a grid of shapes;
// tests/test_wino_route.py compares that with a recorded table).
//
// conv_winograd.hip asks wino_route once per call and launches what the returned value names; the transform launchers ask
// input_transform_route / gy_transform_route; the size queries and conv_wgrad.hip (the transforms of the Winograd weight gradient) ask the
// padding functions.  Nothing else in the library decides a Winograd transform kernel, GEMM tile, ring depth, twin, padded dimension or
// profiling family of this path.  (The 16 plane GEMMs of the weight gradient are wgrad_route.h's.)
// The epilogue fields, the fused column-sum / dot workspace (common.h FusedSums) and the dynamic-LDS launch helper are shared with
// conv_igemm.hip through conv_common.h.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

namespace gif_wino {

// GEMM tile of wino_gemm_mfma<2>: 256 threads = 4 waves as 2 (M) x 2 (N); wave tile 64 tiles x 32 couts; block tile 128 x 64; BK = 32;
// WNSTAGE: ring depth of wino_gemm_mfma and wino_gemm_x3.
constexpr int WBM = 128, WBN = 64, WBK = 32, WNSTAGE = 3;
constexpr int WPAD = 256;  // row padding of the V / Mg planes: the bf16x3 GEMM walks them in 256-row blocks
constexpr int XFORM_THREADS = 256;        // lanes per workgroup of the input / gradient transforms
constexpr long XFORM_CAP_WG = 256 * 32;   // their grid cap: beyond it the grid-stride loop takes another trip
constexpr long WIDE_MIN_WG = 512;         // wino_gemm_mfma<4> from this many 128 x 128 workgroups

// The GIF_* variables the Winograd fwd / dgrad host code reads (all gated by GIF_EXPERIMENTAL: common.h gif::knob).  The defaults are the
// behaviour with nothing set; each comment gives the parsing rule that fills the field.
struct WinoKnobs {
    int xform_rows = 8;       // GIF_WINO_XFORM: "rowsN" -> atoi(N), any other string -> 0.  4, 8, 16 select wino_input_transform_rows<N>;
                              // every other value ("tile", "rows7", "rows") the one-patch-per-lane wino_input_transform
    int wn = 0;               // GIF_WINO_WN: atoi.  4: wino_gemm_mfma<4> iff RP % 128 == 0; 2: never; else the measured rule (gemm_wide)
    bool x3_tile256 = false;  // GIF_WINO_X3_TILE: atoi == 256 -> a bf16x3 GEMM that is no f16x2 launch's twin runs 256 x 64 tiles
    int h2_stages = 3;        // GIF_WINO_H2_STAGES: atoi; 3 -> 3, 5 -> 5, anything else -> 4 (ring depth of wino_gemm_h2)
};

// the four raw environment strings, each NULL when the variable is not set
inline WinoKnobs parse_knobs(const char* xform, const char* wn, const char* x3_tile, const char* h2_stages) {
    WinoKnobs k;
    if (xform) k.xform_rows = !strncmp(xform, "rows", 4) ? atoi(xform + 4) : 0;
    if (wn) k.wn = atoi(wn);
    if (x3_tile) k.x3_tile256 = atoi(x3_tile) == 256;
    if (h2_stages) {
        const int n = atoi(h2_stages);
        k.h2_stages = n == 3 ? 3 : n == 5 ? 5 : 4;
    }
    return k;
}

// ---- padded dimensions and sizes -----------------------------------------------------------------------------------------------
inline long wino_tiles(int B, int H, int W) { return (long)B * (H / 2) * (W / 2); }
// a transformed operand V / Mg is [16][padded_tiles][padded_channels]
inline long padded_tiles(long ntiles) { return (ntiles + WPAD - 1) / WPAD * WPAD; }
inline int padded_channels(int C) { return (C + WBK - 1) / WBK * WBK; }
// the transformed weight U is [16][RP][CP] fp32 for the native GEMM (rows to its 64-wide N tile) and [16][3][RP][CP] bf16 / the f16x2
// planes for the split GEMMs (rows to their 128-wide N tile)
inline void pack_dims(int cout, int cin, bool split, int* RP, int* CP) {
    const int bn = split ? 128 : WBN;
    *RP = (cout + bn - 1) / bn * bn;
    *CP = padded_channels(cin);
}
inline long v_floats(int B, int H, int W, int C) { return 16 * padded_tiles(wino_tiles(B, H, W)) * padded_channels(C); }
// f16x2 operands start with a header of [RP] row exponents and [RP] row flags (common.h gif::h2_header_bytes, held equal in the .hip)
constexpr size_t h2_header_bytes(int RP) { return (size_t)2 * RP * sizeof(int); }
inline long h2_weight_bytes(int RP, int CP) { return (long)h2_header_bytes(RP) + 16L * 2 * RP * CP * 2; }
inline bool fits_i32(long n) { return n < (1L << 31); }  // the kernels' element offsets are 32-bit

// ---- transforms ----------------------------------------------------------------------------------------------------------------
enum XformKernel {
    XFORM_TILE = 0,  // wino_input_transform: one lane = one 4x4 patch x 4 channels
    XFORM_ROWS = 1,  // wino_input_transform_rows<rows>: one lane walks up to `rows` tiles down a tile column
    XFORM_GY = 2,    // wino_gy_transform
};
struct XformRoute {
    int kernel;       // XformKernel
    int rows;         // XFORM_ROWS: 4, 8 or 16
    long ntiles, ntiles_pad;
    int CP;
    long lanes;       // work items of the grid-stride loop
    unsigned blocks;  // workgroups of XFORM_THREADS lanes
    int family;       // profiling family (common.h)
};
inline unsigned transform_blocks(long lanes) {
    const long blocks = (lanes + XFORM_THREADS - 1) / XFORM_THREADS;
    return (unsigned)(blocks > XFORM_CAP_WG ? XFORM_CAP_WG : blocks);
}
// The vertical-reuse variant with 8 tiles per lane is the default (profiles/r4_wino_transform_rows.txt: 23.8 -> 23.0 ms/step, HBM bytes
// of the transform family 1.10x -> 1.065x the algorithmic count); the other depths and the one-patch-per-lane kernel are A/B.
inline XformRoute input_transform_route(int B, int H, int W, int C, const WinoKnobs& k) {
    XformRoute t{};
    t.ntiles = wino_tiles(B, H, W);
    t.ntiles_pad = padded_tiles(t.ntiles);
    t.CP = padded_channels(C);
    t.family = 4;
    const int rows = k.xform_rows;
    if (rows == 4 || rows == 8 || rows == 16) {
        t.kernel = XFORM_ROWS;
        t.rows = rows;
        t.lanes = (long)B * ((H / 2 + rows - 1) / rows) * (W / 2) * (t.CP / 4);
    } else {
        t.kernel = XFORM_TILE;
        t.lanes = t.ntiles * (t.CP / 4);
    }
    t.blocks = transform_blocks(t.lanes);
    return t;
}
inline XformRoute gy_transform_route(int B, int H, int W, int C) {
    XformRoute t{};
    t.kernel = XFORM_GY;
    t.ntiles = wino_tiles(B, H, W);
    t.ntiles_pad = padded_tiles(t.ntiles);
    t.CP = padded_channels(C);
    t.family = 4;
    t.lanes = t.ntiles * (t.CP / 4);
    t.blocks = transform_blocks(t.lanes);
    return t;
}

// ---- the GEMM route ------------------------------------------------------------------------------------------------------------
enum WinoMode { MODE_NATIVE = 0, MODE_BF16X3 = 1, MODE_F16X2 = 2 };  // by the entry point: _f32, _f32x3, _f32h2
enum WinoGemm {
    GEMM_MFMA = 0,  // wino_gemm_mfma<WN>: 128 x (32 * WN) tiles on 2 x WN waves
    GEMM_X3 = 1,    // wino_gemm_x3<BM, BN> (bf16x3, 512 threads)
    GEMM_H2 = 2,    // wino_gemm_h2<BM, BN, NST> (f16x2, 512 threads)
};
enum WinoError {  // the 32-bit-offset limits, in the order they are checked
    WINO_OK = 0,
    WINO_V_TOO_LARGE = 1,  // ntiles_pad * CP
    WINO_Y_TOO_LARGE = 2,  // B * H * W * Co
    WINO_X_TOO_LARGE = 3,  // B * H * W * C
    WINO_U_TOO_LARGE = 4,  // 3 * RP * CP (the split forms)
};

// one GEMM launch: the kernel's template arguments, its grid, block size and dynamic LDS bytes
struct WinoLaunch {
    int kernel;  // WinoGemm
    int WN;      // GEMM_MFMA
    int BM, BN;  // GEMM_X3, GEMM_H2
    int NST;     // GEMM_H2
    int bm, bn;  // block tile in Winograd tiles x output channels
    int tiles_m, tiles_n;
    unsigned grid;
    int threads;
    size_t lds;
};

struct WinoRoute {
    int error;  // WinoError; != WINO_OK: only ntiles .. CP below are filled
    long ntiles, ntiles_pad;
    int RP, CP;
    XformRoute xform;
    WinoLaunch primary;
    bool has_twin;   // guarded f16x2: the bf16x3 twin follows (a no-op unless the primary raised the gate)
    WinoLaunch twin;
    int sum_rows;    // fused column sums / dot products: partial-sum rows (= row tiles) ...
    int sum_tile;    // ... of this many Winograd tiles each
    int family;      // profiling family of the GEMM (common.h)
};

// 128-wide N tile (8 waves) whenever the output channels fill it.  Measured: +1-2 % on the >= 32^2 layers, slower when the launch has
// fewer than ~512 workgroups of 512 threads.  GIF_WINO_WN=2 / 4 forces a variant (benchmarking).
inline bool gemm_wide(int Co, int RP, int tiles_m, const WinoKnobs& k) {
    if (k.wn == 4) return RP % 128 == 0;
    if (k.wn == 2) return false;
    return Co % 128 == 0 && (long)tiles_m * (RP / 128) >= WIDE_MIN_WG;
}

inline WinoLaunch gemm_launch(int kernel, int bm, int bn, long ntiles_pad, int RP) {
    WinoLaunch l{};
    l.kernel = kernel;
    l.bm = bm; l.bn = bn;
    l.tiles_m = (int)(ntiles_pad / bm);
    l.tiles_n = RP / bn;
    l.grid = (unsigned)(l.tiles_m * l.tiles_n);
    return l;
}
inline WinoLaunch x3_launch(int bm, int bn, long ntiles_pad, int RP) {
    WinoLaunch l = gemm_launch(GEMM_X3, bm, bn, ntiles_pad, RP);
    l.BM = bm; l.BN = bn;
    l.threads = 512;
    l.lds = (size_t)WNSTAGE * ((size_t)bm * WBK * sizeof(float) + 3 * (size_t)bn * 64);
    return l;
}

// guarded: an f16x2 call that also got the bf16x3 transform of its weights (else no twin is launched)
inline WinoRoute wino_route(int B, int H, int W, int C, int Co, int mode, bool guarded, const WinoKnobs& k) {
    WinoRoute r{};
    const bool split = mode != MODE_NATIVE;
    r.ntiles = wino_tiles(B, H, W);
    r.ntiles_pad = padded_tiles(r.ntiles);
    pack_dims(Co, C, split, &r.RP, &r.CP);
    r.error = !fits_i32(r.ntiles_pad * r.CP)         ? WINO_V_TOO_LARGE
              : !fits_i32((long)B * H * W * Co)      ? WINO_Y_TOO_LARGE
              : !fits_i32((long)B * H * W * C)       ? WINO_X_TOO_LARGE
              : split && !fits_i32(3L * r.RP * r.CP) ? WINO_U_TOO_LARGE
                                                     : WINO_OK;
    if (r.error) return r;
    r.xform = input_transform_route(B, H, W, C, k);
    if (!split) {
        const bool wide = gemm_wide(Co, r.RP, (int)(r.ntiles_pad / WBM), k);
        const int bn = wide ? 128 : WBN;
        r.primary = gemm_launch(GEMM_MFMA, WBM, bn, r.ntiles_pad, r.RP);
        r.primary.WN = wide ? 4 : 2;
        r.primary.threads = 128 * r.primary.WN;
        r.primary.lds = (size_t)WNSTAGE * (WBM + bn) * WBK * sizeof(float);
        r.family = 2;
    } else if (mode == MODE_BF16X3) {
        // 128 x 128 blocks (4 x 2 waves) by default; GIF_WINO_X3_TILE=256 selects 256 x 64 (8 x 1 waves: every V fragment split once
        // instead of twice) — measured equal (2.998 / 2.141 / 1.790 ms vs 2.993 / 2.133 / 1.757 ms on the three big layers)
        r.primary = k.x3_tile256 ? x3_launch(256, 64, r.ntiles_pad, r.RP) : x3_launch(128, 128, r.ntiles_pad, r.RP);
        r.family = 10;
    } else {
        // ring depth 3 / 4 / 5 (96 / 128 / 160 KB): measured equal — 2.648 / 2.638 / 2.686 ms on 128 -> 128 at 256^2, batch 32: the GEMM
        // does not wait for its DMA; GIF_WINO_H2_STAGES keeps the A/B
        r.primary = gemm_launch(GEMM_H2, 128, 128, r.ntiles_pad, r.RP);
        r.primary.BM = 128; r.primary.BN = 128; r.primary.NST = k.h2_stages;
        r.primary.threads = 512;
        r.primary.lds = (size_t)k.h2_stages * ((size_t)128 * WBK * sizeof(float) + 2 * (size_t)128 * 64);
        r.has_twin = guarded;
        r.twin = x3_launch(128, 128, r.ntiles_pad, r.RP);  // (same grid)
        r.family = 14;
    }
    r.sum_rows = r.primary.tiles_m;
    r.sum_tile = r.primary.bm;
    return r;
}

}  // namespace gif_wino
