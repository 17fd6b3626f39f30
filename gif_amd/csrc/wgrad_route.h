// Which weight-gradient kernel a layer gets: host-only, plain C++17, no HIP and no common.h, so that a host compiler builds it alone
// (tests/host/wgrad_route_dump.cpp prints it over a grid of shapes; tests/test_wgrad_route.py compares that with a recorded table).
//
// conv_wgrad.hip asks ONE of the three route functions per call — wgrad_route (the direct fp32 entry points in the three contraction
// modes, and with shape.planes the 16 plane GEMMs of the Winograd weight gradient), wgrad_route_f16 (f16 operands) — and launches what
// the returned value names; the splits queries ask wgrad_splits / wgrad_splits_f16.  Nothing else in the library decides a weight-
// gradient tile, stage depth, twin or profiling family.  NOT modelled here, because they depend on the filled kernel parameters or on
// run-time state and sit next to the launch: the buffer-addressed form of conv_wgrad_h2v2 (h2v2_buf_ok: GIF_H2_WGRAD_BUF) and
// GIF_H2_GUARD=0 (no gate: the guarded twin is not launched).
// What the launches share with the other conv sources (the dynamic-LDS launch helper, the knob reader) is conv_common.h; the weight
// PACKING entry points are weight_pack.hip's, except the f16x2 ones, which stay in conv_wgrad.hip (see there).
#pragma once
#include <stddef.h>

namespace gif_wgrad {

constexpr int BKP_MAX = 32;  // host-side rounding unit of the pixel chunks (any BKP of the kernels divides it)

// The GIF_* variables the weight-gradient host code reads (all gated by GIF_EXPERIMENTAL: common.h gif::knob).  The defaults are the
// behaviour with nothing set; each comment gives the parsing rule that fills the field.
struct WgradKnobs {
    int x3_wgrad_thin = 1;        // GIF_X3_WGRAD_THIN: atoi; 0 = no 128x32 bf16x3 / f16x2 tiles, 4 = the four-wave 128x32 bf16x3 kernel
    bool x3_wgrad_simple = false;  // GIF_X3_WGRAD_SIMPLE: atoi != 0 = 16-pixel stages, no software pipeline, no f16x2
    bool h2_wgrad_plain_tab = true;  // GIF_H2_WGRAD_PLAIN_TAB: atoi != 0 = un-modulated f16x2 launches run the scale-table instantiation
    bool h2_wgrad_v2 = true;      // GIF_H2_WGRAD_V2: atoi != 0 = conv_wgrad_h2v2 (0: the per-wave-split conv_wgrad_mfma<..., 2>)
    bool h2_wgrad_taps = true;    // GIF_H2_WGRAD_TAPS: atoi != 0 = thin big sides group several taps per 128-column tile
    bool wgrad_big = true;        // GIF_WGRAD_BIG: off iff atoi == 0 (256x128 native tiles)
    bool small_wgrad = true;      // GIF_SMALL_WGRAD: off iff atoi == 0 (conv_wgrad_small_mfma)
    bool f16_wgrad256 = true;     // GIF_F16_WGRAD256: off iff atoi == 0 (256x256 f16 tiles)
    bool f16_halo_wgrad = true;   // GIF_F16_HALO_WGRAD: off iff atoi == 0 (conv_wgrad_halo_f16)
    bool f16_halo_wgrad_tr = true;  // GIF_F16_HALO_WGRAD_TR: off iff atoi == 0 (transposing LDS reads in conv_wgrad_halo_f16)
    bool conv_variant_set = false;  // GIF_CONV_VARIANT: its presence alone disables the 256x128 tile ...
    int conv_variant = 0;         // ... and its atoi selects: 1 = register-staged operands, 7 = 32-pixel stages on the 128x128 tile
};

// One weight-gradient call: gif_conv_geom plus what the entry point knows.  planes: the Winograd plane GEMMs (16 "taps" without a
// spatial shift over B = 1, Hs = 1, Ws = tiles, KH = KW = 1, channels already padded by the transforms).
struct WgradShape {
    int B, Hb, Wb, Cb, Hs, Ws, Cs, KH, KW, stride, pad;
    bool scaled;  // per-sample scales on either side (modulated layer)
    bool planes;
};

inline int wgrad_taps(const WgradShape& g) { return g.planes ? 16 : g.KH * g.KW; }
inline long wgrad_ntot(const WgradShape& g) { return (long)g.B * g.Hs * g.Ws; }
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- shape helpers -------------------------------------------------------------------------------------------------------------
// wgrad tiles follow the SAME row/col padding as the forward packing (gif_conv2d_pack_dims(Cs, Cb)):
// rows RP multiple of 32 or 128, cols CP multiple of 8 or 32 — so pad further to the tile here.
inline int tile_of(int c) { return c <= 32 ? 32 : 128; }

// wgrad workspace dims: rows/cols padded to the wgrad tile (32 or 128)
inline void wgrad_dims(int Cs, int Cb, int* RP, int* CP) {
    int bp = tile_of(Cs), bq = tile_of(Cb);
    *RP = (Cs + bp - 1) / bp * bp;
    *CP = (Cb + bq - 1) / bq * bq;
}

// taps per 128-column tile and the number of column tiles for a thin big side of Cb (<= 32) channels
inline void thin_tap_tiles(int Cb, int T, int* tpt, int* tgroups) {
    int n = 128 / Cb;
    if (n > T) n = T;
    *tpt = n;
    *tgroups = (T + n - 1) / n;
}

// 256x128 tiles (wave tile 128x64: 6 LDS operand reads per 8 MFMAs instead of 4 per 4 — the operand reads, one ds_read_b32 per
// MFMA operand in this [pixel][channel] layout, are what caps the 128x128 kernel) whenever the row count allows it and the
// operands go through the plain LDS-DMA path.  GIF_WGRAD_BIG=0 disables it.
inline bool wgrad_big_tile(int Cs, int Cb, bool scaled, long Ntot, bool knob_big) {
    // (below ~16K reduction rows the halved workgroup count costs more than the operand reuse gains: measured)
    return knob_big && !scaled && Ntot >= 16384 && tile_of(Cs) == 128 && tile_of(Cb) == 128 && ((Cs + 127) / 128 * 128) % 256 == 0;
}
inline int tile_rows(int Cs, int Cb, bool scaled, long Ntot, bool knob_big) {
    return wgrad_big_tile(Cs, Cb, scaled, Ntot, knob_big) ? 256 : tile_of(Cs);
}

// conv_wgrad_small_mfma: the condition-noise convs (3x3, stride 1, pad 1, Cs <= 32, Cb <= 16) from 65536 pixels.  GIF_SMALL_WGRAD=0: off
inline bool small_wgrad_ok(const WgradShape& g, bool knob_small) {
    return knob_small && !g.planes && !g.scaled && g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && g.Hs == g.Hb && g.Ws == g.Wb &&
           g.Cs <= 32 && g.Cb <= 16 && wgrad_ntot(g) >= 65536;
}

// square tile of the f16 weight-gradient kernel: 32 / 64 for the thin layers of the 512^2 / 1024^2 blocks, else 128
inline int wgrad_tile_f16(int Cs, int Cb) {
    const int m = Cs > Cb ? Cs : Cb;
    return m <= 32 ? 32 : (m <= 64 ? 64 : 128);
}
inline void wgrad_dims_f16(int Cs, int Cb, int* RP, int* CP) {
    const int t = wgrad_tile_f16(Cs, Cb);
    *RP = (Cs + t - 1) / t * t;
    *CP = (Cb + t - 1) / t * t;
}

// 256 x 256 tiles on 8 waves (wave tile 128 x 64) for the f16 weight gradients with multiples of 256 channels on both sides: half
// the LDS-DMA pieces and 6 instead of 8 operand gathers per MFMA (the 128 x 128 loop is bound by both: DESIGN 3b).  GIF_F16_WGRAD256=0: A/B.
// Modulated launches too (the per-sample scale table of a 32-pixel stage is 2 KB per sample).
inline bool wgrad_tile256_f16(const WgradShape& g, bool knob_256) {
    return knob_256 && g.Cs % 256 == 0 && g.Cb % 256 == 0 && wgrad_ntot(g) >= 16384 && ((long)g.Hs * g.Ws) % 32 == 0;
}

// conv_wgrad_halo_f16 (thin high-resolution f16 layers).  GIF_F16_HALO_WGRAD=0: A/B knob (the per-tap kernel).  Workgroups (= splits):
// two per CU, never more than patches.
inline bool halo_wgrad_ok(const WgradShape& g, bool knob_halo) {
    return knob_halo && g.stride == 1 && g.Cs <= 32 && g.Cb <= 32 && g.KH <= 3 && g.KW <= 3 && g.Hs == g.Hb && g.Ws == g.Wb &&
           g.KH == 2 * g.pad + 1 && g.KW == 2 * g.pad + 1 && g.Hs >= 16 && g.Ws >= 16 &&
           (long)g.B * cdiv(g.Hs, 16) * cdiv(g.Ws, 16) >= 512;
}
inline int halo_wgrad_splits(const WgradShape& g) {
    const long patches = (long)g.B * cdiv(g.Hs, 16) * cdiv(g.Ws, 16);
    return (int)(patches < 512 ? patches : 512);
}

// pixels per split, rounded to the stage unit; samples a pixel chunk can touch (rows of the LDS scale table)
inline long wgrad_chunk(long Ntot, int nsplit) {
    long chunk = (Ntot + nsplit - 1) / nsplit;
    chunk = (chunk + BKP_MAX - 1) / BKP_MAX * BKP_MAX;
    return chunk < BKP_MAX ? BKP_MAX : chunk;
}
inline int wgrad_stab_nb(long chunk, long HWs, int B) {
    const int nb = (int)((chunk + HWs - 1) / HWs + 1);
    return nb > B ? B : nb;
}

// The f16x2 kernel that groups several taps of a thin big side (Cb <= 32) into one 128-column tile, conv_wgrad_h2v2<false, true>, can
// take this layer in this contraction mode.  The splits query stops here (it knows neither whether the call will be modulated nor the
// GIF_X3_WGRAD_THIN / _SIMPLE knobs); wgrad_route adds those.
inline bool thin_taps_shape(const WgradShape& g, int mode, const WgradKnobs& k) {
    return !g.planes && tile_of(g.Cs) == 128 && tile_of(g.Cb) == 32 && wgrad_taps(g) > 1 && k.h2_wgrad_taps && k.h2_wgrad_v2 && mode == 2;
}

// ---- the route -----------------------------------------------------------------------------------------------------------------
enum WgradKernel {
    WGRAD_MFMA = 0,   // conv_wgrad_mfma<T, BP, BQ, WP, WQ, GLDS, BKP, TAB, X3>
    WGRAD_H2V2 = 1,   // conv_wgrad_h2v2<TAB, TAPS> (f16x2, 128x128 tiles, 256 threads)
    WGRAD_SMALL = 2,  // conv_wgrad_small_mfma
    WGRAD_HALO = 3,   // conv_wgrad_halo_f16<TR>
};

// one launch: the kernel's template arguments, its block size and its workgroups per split (grid = wgs_per_split * nsplit)
struct WgradLaunch {
    int kernel;                   // WgradKernel
    bool f16;                     // T: gif::f16 instead of float
    int BP, BQ, WP, WQ;
    bool GLDS;
    int BKP;
    bool TAB;                     // conv_wgrad_mfma / conv_wgrad_h2v2: the scale-table instantiation
    int X3;                       // 0 the operands' own MFMA, 1 bf16x3, 2 f16x2
    bool TAPS;                    // conv_wgrad_h2v2: grouped taps; tpt taps per column tile, tgroups column tiles
    int tpt, tgroups;
    bool TR;                      // conv_wgrad_halo_f16
    bool unit_tab;                // TAB over a one-row table of ones (the launch gets stab_nb = 1)
    int threads;
    long wgs_per_split;
};

struct WgradRoute {
    WgradLaunch primary;
    bool has_twin;                // f16x2: the guarded bf16x3 twin follows (same grid rule, its own kernel)
    WgradLaunch twin;
    int RP, CP;                   // workspace rows / columns
    int tile_f16;                 // f16: the square tile before the 256 upgrade (its scale table bounds the modulated launches)
    int tiles_q, tiles_pq;        // column tiles, row x column tiles of the primary launch (kernel parameters)
    int stab_nb;                  // samples a pixel chunk can touch
    long chunk;                   // pixels per split
    int family;                   // profiling family (common.h)
};

inline WgradLaunch mfma_launch(bool f16, int BP, int BQ, int WP, int WQ, bool GLDS, int BKP, bool TAB, int X3, long wgs) {
    WgradLaunch l{};
    l.kernel = WGRAD_MFMA; l.f16 = f16; l.BP = BP; l.BQ = BQ; l.WP = WP; l.WQ = WQ; l.GLDS = GLDS; l.BKP = BKP; l.TAB = TAB; l.X3 = X3;
    l.threads = 64 * WP * WQ; l.wgs_per_split = wgs;
    return l;
}
inline WgradLaunch h2v2_launch(bool TAB, bool unit_tab, long wgs) {
    WgradLaunch l{};
    l.kernel = WGRAD_H2V2; l.BP = 128; l.BQ = 128; l.TAB = TAB; l.X3 = 2; l.unit_tab = unit_tab; l.threads = 256; l.wgs_per_split = wgs;
    return l;
}

// Direct fp32 weight gradient (mode: 0 native fp32 MFMA, 1 bf16x3, 2 f16x2 with the guarded bf16x3 twin; launch shapes the split modes
// are not built for run the native kernels) and, with g.planes, the Winograd plane GEMMs.
inline WgradRoute wgrad_route(const WgradShape& g, int mode, int nsplit, const WgradKnobs& k) {
    WgradRoute r{};
    const bool scaled = g.scaled && !g.planes;  // (the Winograd transforms have applied the scales)
    const int T = wgrad_taps(g);
    const long Ntot = wgrad_ntot(g), HWs = (long)g.Hs * g.Ws;
    wgrad_dims(g.Cs, g.Cb, &r.RP, &r.CP);
    const int bp = tile_of(g.Cs), bq = tile_of(g.Cb);
    if (small_wgrad_ok(g, k.small_wgrad)) {
        // one 16-wave workgroup per split; 64-pixel chunks
        r.primary.kernel = WGRAD_SMALL; r.primary.threads = 1024; r.primary.wgs_per_split = 1;
        r.chunk = ((Ntot + nsplit - 1) / nsplit + 63) / 64 * 64;
        r.family = 1;
        return r;
    }
    r.chunk = wgrad_chunk(Ntot, nsplit);
    r.stab_nb = g.planes ? 0 : wgrad_stab_nb(r.chunk, HWs, g.B);
    const bool tab_fits = HWs % 16 == 0 && (size_t)r.stab_nb * 256 * sizeof(float) <= 64 * 1024;
    // bf16x3 / f16x2 tiles: 128x128, and 128x32 for the un-modulated layers with a thin big side (the 24-channel condition-noise maps);
    // the 256x128 tile's 128 accumulator registers leave no room for the split operands, and layers with a <= 32-channel small side stay
    // on the native kernels (same operands, same workspace)
    bool x3 = mode != 0;
    const bool x3_thin = x3 && !g.planes && k.x3_wgrad_thin != 0 && bp == 128 && bq == 32 && !scaled;
    x3 = x3 && bp == 128 && (bq == 128 || x3_thin) && (!scaled || tab_fits);
    const bool variant_set = k.conv_variant_set && !g.planes;  // (the plane GEMMs never read GIF_CONV_VARIANT)
    const int variant = variant_set ? k.conv_variant : 0;
    const bool big_tile = !x3 && wgrad_big_tile(g.Cs, g.Cb, scaled, Ntot, k.wgrad_big) && !variant_set;
    r.tiles_q = r.CP / bq;
    r.tiles_pq = (r.RP / (big_tile ? 256 : bp)) * r.tiles_q;
    const long wgs = (long)r.tiles_pq * T;
    const bool glds = !scaled && variant != 1;
    // Un-modulated f16x2 launches run the scale-table instantiation with unit scales (x 1.0f: bit-identical results) wherever it
    // applies: that instantiation's instruction stream is 3-5 % faster than the plain one on every 128 x 128-tile shape — 3.02 -> 2.91 ms
    // at 128@256^2, 2.92 -> 2.77 at 512@64^2, the modulated launches themselves 2.82 / 2.79 — for no reason visible in the source (the
    // extra multiply moves hipcc's interleave of the conversion); -0.6 ms per step, three alternating pairs.  GIF_H2_WGRAD_PLAIN_TAB=0: A/B
    const bool tab = !g.planes && (scaled || (k.h2_wgrad_plain_tab && x3 && mode == 2 && HWs % 32 == 0)) && (variant != 1 || x3) && tab_fits;
    // f16x2: the software-pipelined 32-pixel-stage instantiations; the launch is followed by its guarded bf16x3 twin
    const bool h2 = x3 && mode == 2 && !k.x3_wgrad_simple && (x3_thin || !tab || HWs % 32 == 0);
    r.family = g.planes ? (h2 ? 16 : x3 ? 11 : 3) : (h2 ? 15 : x3 ? 9 : 1);

    WgradLaunch l;  // the bf16x3 / native launch: the guarded twin of an f16x2 launch, else the call's only one
    if (x3_thin) {
        // two waves of 64x32: 3 fragment splits per 12 MFMAs (four waves of 32x32: 2 per 6 — GIF_X3_WGRAD_THIN=4 for the A/B:
        // 128x24 at 256^2 76 -> 80 TFLOP/s, 256x24 at 128^2 70 -> 78, 512x24 at 64^2 80 -> 82)
        l = k.x3_wgrad_thin == 4 ? mfma_launch(false, 128, 32, 4, 1, true, 32, false, 1, wgs) : mfma_launch(false, 128, 32, 2, 1, true, 32, false, 1, wgs);
    } else if (x3 && tab && HWs % 32 == 0 && !k.x3_wgrad_simple) {
        l = mfma_launch(false, 128, 128, 2, 2, true, 32, true, 1, wgs);
    } else if (x3 && tab) {
        l = mfma_launch(false, 128, 128, 2, 2, true, 16, true, 1, wgs);
    } else if (x3 && !k.x3_wgrad_simple) {
        l = mfma_launch(false, 128, 128, 2, 2, true, 32, false, 1, wgs);
    } else if (x3) {
        l = mfma_launch(false, 128, 128, 2, 2, true, 16, false, 1, wgs);
    } else if (big_tile) {
        l = mfma_launch(false, 256, 128, 2, 2, true, 16, false, 0, wgs);
    } else if (bp == 128 && bq == 128 && tab) {
        // modulated wgrad (x*s, dy*d): LDS-DMA operands + scale table
        l = mfma_launch(false, 128, 128, 2, 2, true, 16, true, 0, wgs);
    } else if (bp == 128 && bq == 128 && glds && variant != 7) {
        // 16-pixel stages: 32 KB of LDS per workgroup => 4 workgroups (16 waves) per CU; +6 % over 32-pixel stages
        l = mfma_launch(false, 128, 128, 2, 2, true, 16, false, 0, wgs);
    } else if (bp == 128 && bq == 128) {
        l = mfma_launch(false, 128, 128, 2, 2, glds, 32, false, 0, wgs);
    } else if (bp == 128 && bq == 32) {
        l = mfma_launch(false, 128, 32, 4, 1, glds, 32, false, 0, wgs);
    } else if (bp == 32 && bq == 128) {
        l = mfma_launch(false, 32, 128, 1, 4, glds, 32, false, 0, wgs);
    } else {
        l = mfma_launch(false, 32, 32, 1, 1, glds, 32, false, 0, wgs);
    }
    if (!h2) {
        r.primary = l;
        return r;
    }
    r.has_twin = true;
    r.twin = l;
    if (x3_thin && thin_taps_shape(g, mode, k)) {
        // several taps per 128-column tile; the guarded twin keeps its per-tap grid
        r.primary = h2v2_launch(false, false, 0);
        r.primary.TAPS = true;
        thin_tap_tiles(g.Cb, T, &r.primary.tpt, &r.primary.tgroups);
        r.primary.wgs_per_split = (long)r.tiles_pq * r.primary.tgroups;
    } else if (x3_thin) {
        r.primary = mfma_launch(false, 128, 32, 2, 1, true, 32, false, 2, wgs);
    } else if (k.h2_wgrad_v2) {
        // (the plane GEMMs too run the scale-table instantiation, with a one-row table of ones)
        r.primary = g.planes ? h2v2_launch(k.h2_wgrad_plain_tab, k.h2_wgrad_plain_tab, wgs) : h2v2_launch(tab, false, wgs);
    } else {
        r.primary = mfma_launch(false, 128, 128, 2, 2, true, 32, tab, 2, wgs);
    }
    return r;
}

// f16 operands (BASELINE config 5): square tiles on the LDS-DMA kernel (MFMA work on padded channels is cheap at the f16 rate), fp32
// partial sums; the persistent halo kernel for the thin high-resolution layers when the caller passes that kernel's split count.
inline WgradRoute wgrad_route_f16(const WgradShape& g, int nsplit, const WgradKnobs& k) {
    WgradRoute r{};
    const int T = wgrad_taps(g);
    const long Ntot = wgrad_ntot(g), HWs = (long)g.Hs * g.Ws;
    wgrad_dims_f16(g.Cs, g.Cb, &r.RP, &r.CP);
    r.family = 7;
    const int t = wgrad_tile_f16(g.Cs, g.Cb);
    if (halo_wgrad_ok(g, k.f16_halo_wgrad) && nsplit == halo_wgrad_splits(g) && r.RP == 32 && r.CP == 32) {
        r.primary.kernel = WGRAD_HALO; r.primary.f16 = true; r.primary.TR = k.f16_halo_wgrad_tr; r.primary.threads = 256;
        r.primary.wgs_per_split = 1;
        return r;
    }
    r.chunk = wgrad_chunk(Ntot, nsplit);
    r.stab_nb = wgrad_stab_nb(r.chunk, HWs, g.B);
    const bool st16 = g.scaled && HWs % 32 != 0;  // modulated layer on 4x4 maps: 16-pixel stages
    // the 64-wide tile has no 16-pixel-stage variant (one DMA pass covers 32 pixel rows): such a launch runs 32x32 tiles over
    // the same 64-padded workspace
    int tl = (t == 64 && st16) ? 32 : t;
    r.tile_f16 = tl;
    int bkp = st16 ? 16 : 32, wp = 2, wq = 2;
    if (tl == 128 && wgrad_tile256_f16(g, k.f16_wgrad256) && (!g.scaled || (size_t)r.stab_nb * 512 * sizeof(float) <= 32 * 1024)) {
        tl = 256; wq = 4; bkp = 32;  // (Hs*Ws % 32 == 0 here: never 16-pixel stages)
    } else if (tl == 32) {
        wp = wq = 1;
    }
    r.tiles_q = r.CP / tl;
    r.tiles_pq = (r.RP / tl) * r.tiles_q;
    r.primary = mfma_launch(true, tl, tl, wp, wq, true, bkp, g.scaled, 0, (long)r.tiles_pq * T);
    return r;
}

// ---- split counts --------------------------------------------------------------------------------------------------------------
// Fill k full rounds of `slots` resident workgroups and never spill a few blocks into an extra, almost empty round (floor, not ceil);
// at least 4 stages of pixels per split; at most 128 MB of partial sums.
inline int wgrad_clamp_splits(long tiles, long slots, long Ntot, long bytes_per_split) {
    long n = tiles >= slots ? 1 : slots / tiles;
    const long max_by_work = (Ntot + 4 * BKP_MAX - 1) / (4 * BKP_MAX);
    const long max_by_mem = (128L << 20) / bytes_per_split;
    if (n > max_by_work) n = max_by_work;
    if (n > max_by_mem) n = max_by_mem;
    if (n < 1) n = 1;
    return (int)n;
}

// Workgroups per split of the fp32 launch a LATER call in `mode` is expected to make.  The query does not know whether that call will
// be modulated: it counts the un-modulated launch (scaled launches of the same geometry use 128-row tiles: they simply get half the
// splits they could use), and it counts 256-row tiles wherever wgrad_big_tile allows them, in every mode.
inline long wgrad_tiles_per_split(const WgradShape& g, int mode, const WgradKnobs& k) {
    int RP, CP;
    wgrad_dims(g.Cs, g.Cb, &RP, &CP);
    if (thin_taps_shape(g, mode, k)) {
        // fewer, larger workgroups per split.  The native / bf16x3 kernels run one workgroup per tap and keep their own count (they
        // got ~4.5 x the splits, i.e. workspace and unpack traffic, for nothing)
        int tpt, tg;
        thin_tap_tiles(g.Cb, wgrad_taps(g), &tpt, &tg);
        return (long)(RP / 128) * tg;
    }
    return (long)(RP / tile_rows(g.Cs, g.Cb, false, wgrad_ntot(g), k.wgrad_big)) * (CP / tile_of(g.Cb)) * wgrad_taps(g);
}

// 2 workgroups fit per CU (64 KB LDS each) => 512 concurrent slots on 256 CUs: fill k full rounds of 512 (1024 slots)
inline int wgrad_splits(const WgradShape& g, int mode, const WgradKnobs& k) {
    WgradShape u = g;
    u.scaled = false;
    if (small_wgrad_ok(u, k.small_wgrad)) return 256;  // one 16-wave workgroup per CU (conv_wgrad_small_mfma); scaled calls never
                                                       // reach that kernel and simply use 256 splits of the generic one
    int RP, CP;
    wgrad_dims(g.Cs, g.Cb, &RP, &CP);
    return wgrad_clamp_splits(wgrad_tiles_per_split(u, mode, k), 1024, wgrad_ntot(g), (long)wgrad_taps(g) * RP * CP * 4);
}

inline int wgrad_splits_f16(const WgradShape& g, const WgradKnobs& k) {
    if (halo_wgrad_ok(g, k.f16_halo_wgrad)) return halo_wgrad_splits(g);  // conv_wgrad_halo_f16: one split per persistent workgroup
    int RP, CP;
    wgrad_dims_f16(g.Cs, g.Cb, &RP, &CP);
    const int t = wgrad_tile256_f16(g, k.f16_wgrad256) ? 256 : wgrad_tile_f16(g.Cs, g.Cb);
    const long tiles = (long)(RP / t) * (CP / t) * wgrad_taps(g);
    const long slots = t == 256 ? 512 : t == 128 ? 1024 : 2048;  // resident workgroups: 4 per CU at 32 KB of LDS, more for the small tiles
    return wgrad_clamp_splits(tiles, slots, wgrad_ntot(g), (long)wgrad_taps(g) * RP * CP * 4);
}

}  // namespace gif_wgrad
