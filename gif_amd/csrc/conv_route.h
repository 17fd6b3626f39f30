// Which forward / data-gradient kernel a convolution gets: host-only, plain C++17, no HIP and no common.h, so that a host compiler builds
// it alone (tests/host/conv_route_dump.cpp prints it over a grid of shapes; tests/test_conv_route.py compares that with a recorded table).
//
// conv_igemm.hip builds the phases of an op (conv_phases_fwd: one; conv_phases_bwd_data: the output-parity phases of a transposed
// convolution), asks conv_route ONCE for them — and once more with x3 = 1 for the guarded bf16x3 twin of an f16x2 op — and hands every
// ConvLaunch of the returned value to its conv_dispatch.  Nothing else in the library decides a tile, a wave layout, a stage depth, a
// bulk + remainder split, a merge of phases, the partial-sum rows or the profiling family of these ops.  NOT modelled here, because they
// are run-time state and sit next to the launch: the zero page, the gate of the guarded twin (GIF_H2_GUARD), the operand pointers and
// the epilogue.
// The epilogue fields, the fused column-sum / dot workspace (common.h FusedSums) and the dynamic-LDS launch helper are shared with
// conv_winograd.hip through conv_common.h; the packed weight operand comes from weight_pack.hip (f16x2: conv_wgrad.hip).
#pragma once
#include <stddef.h>

namespace gif_conv {

// The GIF_* variables the forward / data-gradient host code reads (all gated by GIF_EXPERIMENTAL: common.h gif::knob).  The defaults are
// the behaviour with nothing set; each comment gives the parsing rule that fills the field.
struct ConvKnobs {
    bool h2_ring3 = true;      // GIF_H2_RING: three operand stages in the 8-wave f16x2 kernels unless atoi == 2
    bool h2_rows_thin = true;  // GIF_H2_ROWS_THIN: off iff atoi == 0 (conv3x3_rows_thin_h2)
    int x3_waves = 81;         // GIF_X3_WAVES: atoi; 42 selects the 4 x 2 (256x128) / 2 x 2 (128x128) wave layouts for bf16x3
    bool f16_tile256 = true;   // GIF_F16_TILE256: off iff atoi == 0 (256x256 f16 tiles)
    bool x3_big = true;        // GIF_X3_BIG: off iff atoi == 0 (256x128 bf16x3 / f16x2 tiles)
    bool dense128 = true;      // GIF_DENSE_TILE: 128x128 tiles for the tap-dense layers unless atoi == 256
    bool x3_multi_big = true;  // GIF_X3_MULTI_BIG: off iff atoi == 0 (merged 256x128 phases of the big transposed convs)
    int conv_variant = 0;      // GIF_CONV_VARIANT: atoi; 1 = register-staged operands, 3 = no 128x128 remainder split, != 0 = no merged phases
    bool f16_halo = true;      // GIF_F16_HALO: atoi != 0; the INITIAL value of the run-time switch gif_conv2d_f16_halo_enable (conv_route's halo_on)
};

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- shape helpers -------------------------------------------------------------------------------------------------------------
struct TileCfg {
    int BM, BN, BK;
};

// fp32: BK = 32 floats (LDS-DMA kernel) or 8 (register-staged kernel of the Cin < 32 layers).
// f16 : BK = 64 halfs, LDS-DMA kernel only (channel counts are multiples of 8 there: every 16-byte DMA chunk is 8 halfs).
// x3  : the bf16x3 / f16x2 kernels only have 32-float K chunks: 24..31 input channels are zero-padded to one chunk
inline TileCfg pick_cfg(bool f16, int cout, int cin, bool x3 = false) {
    TileCfg c;
    // f16 also has a 128x64 tile: the 64-channel layers of the 512^2 / 1024^2 blocks would waste half of a 128-wide N tile
    c.BN = cout <= 32 ? 32 : ((f16 && cout <= 64) ? 64 : 128);
    c.BK = f16 ? 64 : ((cin < 32 && !x3) ? 8 : 32);
    c.BM = c.BN == 32 ? 256 : 128;
    return c;
}

// packed weight rows (>= cout, multiple of BN) / cols (>= cin, multiple of BK)
inline void pack_dims(bool f16, int cout, int cin, bool x3, int* RP, int* CP) {
    const TileCfg c = pick_cfg(f16, cout, cin, x3);
    *RP = (cout + c.BN - 1) / c.BN * c.BN;
    *CP = (cin + c.BK - 1) / c.BK * c.BK;
    if (f16 && cin <= 32) *CP = 32;  // "pair" mode of the f16 kernel: two taps per 64-half K chunk (ConvPhase::pair)
}

// >= 24 input channels: a 24-channel layer wastes a quarter of its one 32-float K chunk and still beats the native kernel
inline bool x3_eligible(int cout, int cin) { return cout > 0 && cin >= 24 && cin % 4 == 0; }

constexpr size_t LDS_MAX = 160 * 1024;  // dynamic LDS a workgroup can get
constexpr int ROWS_THIN_A = 288;        // conv3x3_rows_thin_h2: staged rows per stage
constexpr int halo_lds_floats(int cp) { return cp == 32 ? 5376 : 10496; }  // conv_halo_f16: (18 * 18 * CPP chunks rounded up to 64) * 4 floats

// LDS bytes of the double-buffered operand tiles: 128-byte rows; X3: the weight tile is three 64-byte-row bf16 tiles
constexpr size_t stage_bytes(int BM, int BN, int X3, int NST) {
    return X3 ? (size_t)NST * BM * 128 + (size_t)NST * (X3 == 2 ? 2 : 3) * BN * 64 : (size_t)2 * (BM + BN) * 128;
}
// LDS bytes of the register-staged kernel's tiles (+4-float row pad)
constexpr size_t simple_bytes(int BM, int BN, int BK) { return (size_t)2 * (BM + BN) * (BK + 4) * sizeof(float); }

// the per-sample scale table of the LDS-DMA kernels: samples a BM-row tile can touch, and its row stride in elements (+ one 16-byte
// chunk: consecutive samples start 4 banks apart)
inline int stab_nb(int BM, int HWp, int B) {
    const int nb = (BM - 1) / HWp + 2;
    return nb > B ? B : nb;
}
inline int stab_stride(int CP, bool f16) { return CP + (f16 ? 8 : 4); }

// One convolution op: gif_conv_geom plus what the entry point knows.
struct ConvShape {
    int B, Hb, Wb, Cb, Hs, Ws, Cs, KH, KW, stride, pad;
    bool f16;     // f16 activations (else fp32)
    int x3;       // fp32 only: 0 native MFMA, 1 bf16x3, 2 f16x2
    bool dense;   // tap-dense K order of the bf16x3 / f16x2 kernels
    bool scaled;  // per-sample input scales (modulated layer)
    bool dot;     // the modulation-gradient dot fusion is on (one tile size for the whole op, whole tiles per sample)
};

// One launch's view of the op: the integer fields of the kernel parameters (conv_igemm.hip GatherParams, same names) the decisions read.
struct ConvPhase {
    int B, Hi, Wi, Ci;  // input tensor
    int Ho, Wo, Co;     // output tensor
    int Hp, Wp;         // output sub-grid of this phase
    int os, ooy, oox;   // output pixel = (oy'*os + ooy, ox'*os + oox)
    int is;             // input  pixel = (oy'*is + dy[t], ox'*is + dx[t])
    int ntaps, nky, nkx, dy0, ddy, dx0, ddx, ky0, kx0, kstep, KW;  // the tap grid
    int RP, CP;
    int M;  // B*Hp*Wp
    int x3, dense, pair;
    bool scaled, dot;
    int no_split;
};

struct ConvPhases {
    ConvPhase ph[4];  // (the tensor, packing and mode fields are filled in all four, the sub-grid and taps in the first nph)
    int nph;
    bool need_zero;   // some output-parity phase has no tap: the output is zero-filled first
};

inline ConvPhase phase_base(const ConvShape& s, bool transposed) {
    ConvPhase p{};
    p.B = s.B;
    if (transposed) { p.Hi = s.Hs; p.Wi = s.Ws; p.Ci = s.Cs; p.Ho = s.Hb; p.Wo = s.Wb; p.Co = s.Cb; }
    else { p.Hi = s.Hb; p.Wi = s.Wb; p.Ci = s.Cb; p.Ho = s.Hs; p.Wo = s.Ws; p.Co = s.Cs; }
    pack_dims(s.f16, p.Co, p.Ci, s.x3 != 0, &p.RP, &p.CP);
    p.pair = (s.f16 && p.CP == 32) ? 1 : 0;
    p.x3 = s.x3;
    p.dense = s.dense ? p.Ci / 4 : 0;  // 16-byte chunks per tap
    p.scaled = s.scaled;
    p.dot = s.dot;
    p.no_split = s.dot ? 1 : 0;
    p.KW = s.KW;
    return p;
}

inline ConvPhases conv_phases_fwd(const ConvShape& s) {
    ConvPhases r{};
    ConvPhase p = phase_base(s, false);
    p.Hp = s.Hs; p.Wp = s.Ws; p.os = 1; p.ooy = 0; p.oox = 0; p.is = s.stride;
    p.nky = s.KH; p.nkx = s.KW; p.ntaps = s.KH * s.KW;
    p.dy0 = -s.pad; p.ddy = 1; p.dx0 = -s.pad; p.ddx = 1;
    p.ky0 = 0; p.kx0 = 0; p.kstep = 1;
    p.M = p.B * p.Hp * p.Wp;
    for (ConvPhase& q : r.ph) q = p;
    r.nph = 1;
    return r;
}

// The (up to 4) output-parity phases of a data gradient; phases with no tap (e.g. 1x1 stride 2) are zero-filled.
inline ConvPhases conv_phases_bwd_data(const ConvShape& s) {
    ConvPhases r{};
    const ConvPhase base = phase_base(s, true);
    for (ConvPhase& q : r.ph) q = base;
    const int st = s.stride;
    const auto pmod = [st](int a) { return ((a % st) + st) % st; };
    for (int py = 0; py < st; ++py)
        for (int px = 0; px < st; ++px) {
            ConvPhase p = base;
            p.Hp = (s.Hb - py + st - 1) / st;
            p.Wp = (s.Wb - px + st - 1) / st;
            if (p.Hp <= 0 || p.Wp <= 0) continue;
            p.os = st; p.ooy = py; p.oox = px; p.is = 1;
            // taps with ky == (py+pad) mod st (and likewise kx): small pixel = big' + (py+pad-ky)/st
            p.ky0 = pmod(py + s.pad); p.kx0 = pmod(px + s.pad); p.kstep = st;
            p.nky = p.ky0 < s.KH ? (s.KH - p.ky0 + st - 1) / st : 0;
            p.nkx = p.kx0 < s.KW ? (s.KW - p.kx0 + st - 1) / st : 0;
            p.ntaps = p.nky * p.nkx;
            p.dy0 = (py + s.pad - p.ky0) / st; p.ddy = -1;
            p.dx0 = (px + s.pad - p.kx0) / st; p.ddx = -1;
            if (p.ntaps == 0) { r.need_zero = true; continue; }
            p.M = p.B * p.Hp * p.Wp;
            r.ph[r.nph++] = p;
        }
    return r;
}

// conv3x3_rows_thin_h2: f16x2 launches of stride-1 3x3 layers with <= 32 output channels whose 256-row tiles are whole image rows or
// 256-pixel pieces of one (always the whole phase: the route never splits a 32-channel launch).  GIF_H2_ROWS_THIN=0: the gather kernel, A/B
inline bool rows_thin_ok(const ConvPhase& p, const ConvKnobs& k) {
    const bool unit = (p.ddy == 1 || p.ddy == -1) && (p.ddx == 1 || p.ddx == -1) && p.dy0 + p.ddy == 0 && p.dx0 + p.ddx == 0;
    return k.h2_rows_thin && p.x3 == 2 && !p.dense && !p.scaled && p.nky == 3 && p.nkx == 3 && unit && p.is == 1 && p.os == 1 && p.ooy == 0 &&
           p.oox == 0 && p.RP == 32 && p.CP % 32 == 0 && p.M % 256 == 0 && p.Hp == p.Hi && p.Wp == p.Wi &&
           p.Ho == p.Hp && p.Wo == p.Wp && (p.Wp % 256 == 0 || (p.Wp >= 32 && 256 % p.Wp == 0)) &&
           ((long)p.B * p.Hi * p.Wi + p.Wi) * p.Ci * 4 < (1L << 32);
}

// bytes of the weight slices a halo launch stages in LDS: [ntaps][BN][CP] halfs
inline long halo_weight_bytes(const ConvPhase& p) {
    const int bn = p.RP <= 32 ? 32 : 64, cp = p.CP <= 32 ? 32 : 64;
    return (long)p.ntaps * bn * cp * 2;
}

// Which f16 launches take the halo kernel: unit-stride gathers (forward stride 1, every data gradient incl. the output-parity
// phases of a transposed convolution) over a tap grid of <= 3 x 3 with <= 64 contraction and <= 64 output channels, on a
// sub-grid that fills at least one patch.  The modulation-gradient dot fusion needs whole patches (one partial row per patch,
// Hp * Wp / 256 of them per sample).  halo_on: GIF_F16_HALO / gif_conv2d_f16_halo_enable (0: the gather kernel, A/B).
inline bool halo_eligible(const ConvPhase& p, bool halo_on) {
    if (!halo_on || p.is != 1 || p.RP > 64 || p.CP > 64) return false;
    if (p.nky < 1 || p.nky > 3 || p.nkx < 1 || p.nkx > 3 || (p.ddy != 1 && p.ddy != -1) || (p.ddx != 1 && p.ddx != -1)) return false;
    if (p.Hp < 16 || p.Wp < 16 || (long)p.B * cdiv(p.Hp, 16) * cdiv(p.Wp, 16) >= (1L << 23)) return false;
    if (p.dot && (p.Hp % 16 || p.Wp % 16)) return false;
    if (halo_weight_bytes(p) > 36864) return false;  // 9 taps of 64 x 64 channels (72 KB) stay on the gather kernel
    return true;
}
// would a FORWARD f16 convolution of this shape (activation channel counts, output grid Hs x Ws) run the halo kernel?
inline bool halo_eligible_fwd(int cin, int cout, int KH, int KW, int stride, int Hs, int Ws, bool halo_on) {
    if (cin <= 0 || cout <= 0 || KH < 1 || KW < 1 || stride < 1 || Hs <= 0 || Ws <= 0) return false;
    ConvPhase p{};
    pack_dims(true, cout, cin, false, &p.RP, &p.CP);
    p.is = stride; p.nky = KH; p.nkx = KW; p.ntaps = KH * KW; p.ddy = 1; p.ddx = 1; p.Hp = Hs; p.Wp = Ws; p.B = 1;
    return halo_eligible(p, halo_on);
}

// the kernels index both tensors with 32-bit offsets
inline bool fits_32bit(const ConvPhase& p) {
    return (long)p.B * p.Hi * p.Wi * p.Ci < (1L << 31) && (long)p.B * p.Ho * p.Wo * p.Co < (1L << 31);
}
// Tile counts of a phase on 128x128 / 256x128 tiles, and the two size classes every rule below shares.
// small: low-resolution layers (4x4 .. 16x16 at batch 32) — a 128x128 grid would leave most CUs idle behind a 144-step K loop; 64x64
// tiles give 4x the workgroups (and 32 KB of LDS: 4 per CU) at a quarter of the latency.  big: at least two rounds of 256x128 tiles.
inline long tiles128(const ConvPhase& p) { return (long)cdiv(p.M, 128) * (p.RP / 128); }
inline long tiles256(const ConvPhase& p) { return (long)cdiv(p.M, 256) * (p.RP / 128); }
inline bool small_tiles(const ConvPhase& p) { return tiles128(p) < 384; }
inline bool big_tiles(const ConvPhase& p) { return tiles256(p) >= 512; }

// ---- the route -----------------------------------------------------------------------------------------------------------------
enum ConvKernel {
    CONV_SIMPLE = 0,     // conv_gather_mfma<BM, BN, BK, WM, WN> (register-staged, fp32)
    CONV_GLDS = 1,       // conv_gather_mfma_glds<T, BM, BN, WM, WN, SCALE, BK, X3, NST>
    CONV_GLDS_MULTI = 2, // conv_gather_mfma_glds_multi<same>: all phases in one grid
    CONV_ROWS_THIN = 3,  // conv3x3_rows_thin_h2
    CONV_HALO = 4,       // conv_halo_f16<BN, HCP>
};

// one kernel launch; the per-phase arrays are indexed from phase0
struct ConvLaunch {
    int kernel;  // ConvKernel
    bool f16;    // T: gif::f16 instead of float
    int BM, BN, BK, WM, WN;
    bool SCALE;
    int X3, NST;
    int HCP;             // conv_halo_f16: channel tile
    int m_begin, M;      // GEMM rows [m_begin, M) (a merged launch: every phase's own [0, M))
    int phase0, nph;     // the phases it covers
    int tiles_m[4], tiles_n;
    long grid;
    int threads;
    size_t lds_bytes;
    int stab_nb[4], stab_stride;
    int t2_tx, t2_ty;    // halo kernel: 16 x 16-pixel patches per row / column of the sub-grid
    int part_row0[4];    // first partial-sum row of each phase's tiles
};

enum ConvError {
    CONV_OK = 0,
    CONV_ERR_2G = 1,      // a tensor of >= 2^31 elements
    CONV_ERR_DMA = 2,     // bf16x3 / f16x2 / f16: >= 4 GiB of input or > 32 taps (err_elems, err_taps)
    CONV_ERR_X3_CIN = 3,  // bf16x3 / f16x2 with < 24 input channels outside the tap-dense order
    CONV_ERR_NOFIT = 4,   // no LDS-DMA configuration fits the LDS and the operand format has no other kernel (err_rc)
};

struct ConvRoute {
    ConvLaunch launch[8];  // in launch order: four phases times bulk + remainder
    int nlaunch;
    int part_rows;   // partial-sum rows the op's tiles write (bulk + remainder launches, phases)
    int tile_rows;   // rows per tile of the last launch
    bool merged;     // all phases in one launch
    bool f16;
    int family;      // profiling family (common.h)
    int error;       // ConvError; every one is "not supported"
    long err_elems;
    int err_taps, err_rc;
};

// 0 / 5 native on the LDS-DMA / register-staged kernel, 6 f16, 8 bf16x3, 13 f16x2, 12 / 17 their tap-dense order
inline int conv_family(const ConvPhase& p, bool f16) {
    return f16 ? 6 : p.dense ? (p.x3 == 2 ? 17 : 12) : p.x3 == 2 ? 13 : p.x3 ? 8 : (p.Ci >= 32 ? 0 : 5);
}

inline void push(ConvRoute& r, ConvLaunch l) {
    for (int i = 0; i < l.nph; ++i) {
        l.part_row0[i] = r.part_rows;
        r.part_rows += l.tiles_m[i];
    }
    r.tile_rows = l.BM;
    r.launch[r.nlaunch++] = l;
}

// an LDS-DMA launch of nph phases on BM x BN tiles, WM x WN waves, with the phases' operand format
inline ConvLaunch glds_launch(const ConvPhase* ph, int phase0, int nph, bool f16, int BM, int BN, int WM, int WN, int NST, int m_begin, int M) {
    ConvLaunch l{};
    const ConvPhase& p0 = ph[phase0];
    l.kernel = nph > 1 ? CONV_GLDS_MULTI : CONV_GLDS;
    l.f16 = f16;
    l.BM = BM; l.BN = BN; l.BK = f16 ? 64 : 32; l.WM = WM; l.WN = WN;  // 128-byte LDS rows
    l.SCALE = p0.scaled;
    l.X3 = f16 ? 0 : p0.x3;
    l.NST = NST;
    l.m_begin = m_begin; l.M = M;
    l.phase0 = phase0; l.nph = nph;
    l.tiles_n = p0.RP / BN;
    l.threads = 64 * WM * WN;
    l.stab_stride = l.SCALE ? stab_stride(p0.CP, f16) : 0;
    for (int i = 0; i < nph; ++i) {
        const ConvPhase& p = ph[phase0 + i];
        l.tiles_m[i] = cdiv((nph > 1 ? p.M : M) - m_begin, BM);
        l.grid += (long)l.tiles_m[i] * l.tiles_n;
        size_t lds = stage_bytes(BM, BN, l.X3, NST);
        if (l.SCALE) {
            l.stab_nb[i] = stab_nb(BM, p.Hp * p.Wp, p.B);
            lds += (size_t)l.stab_nb[i] * l.stab_stride * (f16 ? 2 : 4);
        }
        if (lds > l.lds_bytes) l.lds_bytes = lds;
    }
    return l;
}

// One phase, rows [m_begin, M), on this tile if its stages and scale table fit the LDS.  The 8-wave f16x2 tiles run three stages when the
// table fits beside them, else two.
inline bool try_glds(ConvRoute& r, const ConvPhase* ph, int i, bool f16, const ConvKnobs& k, int BM, int BN, int WM, int WN, int m_begin, int M) {
    for (int nst = (!f16 && ph[i].x3 == 2 && WM * WN == 8 && k.h2_ring3) ? 3 : 2; nst >= 2; --nst) {
        const ConvLaunch l = glds_launch(ph, i, 1, f16, BM, BN, WM, WN, nst, m_begin, M);
        if (l.lds_bytes > LDS_MAX) continue;
        push(r, l);
        return true;
    }
    return false;
}

// All phases in one launch (64x64 tiles for the low-resolution layers, 256x128 / 8 waves for the big bf16x3 / f16x2 ones: one grid instead
// of up to eight launches with a partly filled last round each), if the configuration fits.
inline bool try_multi(ConvRoute& r, const ConvPhase* ph, int nph, bool f16, int BM, int BN, int WM, int WN, int NST) {
    const ConvLaunch l = glds_launch(ph, 0, nph, f16, BM, BN, WM, WN, NST, 0, 0);
    if (l.lds_bytes > LDS_MAX) return false;
    push(r, l);
    r.merged = true;
    return true;
}

inline void push_simple(ConvRoute& r, const ConvPhase& p, int i, int BM, int BN, int BK, int WM, int WN) {
    ConvLaunch l{};
    l.kernel = CONV_SIMPLE;
    l.BM = BM; l.BN = BN; l.BK = BK; l.WM = WM; l.WN = WN; l.NST = 2;
    l.M = p.M;
    l.phase0 = i; l.nph = 1;
    l.tiles_m[0] = cdiv(p.M, BM);
    l.tiles_n = p.RP / BN;
    l.grid = (long)l.tiles_m[0] * l.tiles_n;
    l.threads = 256;
    l.lds_bytes = simple_bytes(BM, BN, BK);
    push(r, l);
}

// whole-image-row tiles of 256 pixels (rows_thin) / 16 x 16-pixel patches (halo): one N tile
inline void push_rows_thin(ConvRoute& r, const ConvPhase& p, int i) {
    ConvLaunch l{};
    l.kernel = CONV_ROWS_THIN;
    l.BM = 256; l.BN = 32; l.BK = 32; l.WM = 4; l.WN = 1; l.X3 = 2; l.NST = 2;
    l.M = p.M;
    l.phase0 = i; l.nph = 1;
    l.tiles_m[0] = p.M / 256;
    l.tiles_n = 1;
    l.grid = l.tiles_m[0];
    l.threads = 256;
    l.lds_bytes = (size_t)2 * ROWS_THIN_A * 32 * sizeof(float);
    push(r, l);
}
inline void push_halo(ConvRoute& r, const ConvPhase& p, int i) {
    ConvLaunch l{};
    l.kernel = CONV_HALO;
    l.f16 = true;
    l.BM = 256; l.BN = p.RP <= 32 ? 32 : 64; l.HCP = p.CP <= 32 ? 32 : 64; l.BK = 64; l.WM = 4; l.WN = 1; l.NST = 1;
    l.M = p.M;
    l.phase0 = i; l.nph = 1;
    l.t2_tx = cdiv(p.Wp, 16);
    l.t2_ty = cdiv(p.Hp, 16);
    l.tiles_m[0] = p.B * l.t2_tx * l.t2_ty;
    l.tiles_n = 1;  // RP <= 64 is one N tile
    l.grid = l.tiles_m[0];
    l.threads = 256;
    l.lds_bytes = (size_t)halo_lds_floats(l.HCP) * sizeof(float) + (size_t)p.ntaps * l.BN * l.HCP * 2;
    push(r, l);
}

// Tile quantisation: `slots` workgroups of a kernel are resident (512 of the 128x128 kernels, 2 per CU; 256 of the 8-wave 256x128 ones),
// so T tiles cost ceil(T / slots) rounds.  The odd-sized phase grids of the transposed convolutions (129^2, 65^2, 33^2 pixels) give e.g.
// 4161 or 1092 tiles = 8.13 / 2.13 rounds: the nearly empty last round costs 10-30 %.  Such launches are split: the full rounds on BM x
// 128 tiles, the remaining rows on 64x64 tiles (4x the workgroups, a quarter of the latency each).  False: the BM x 128 tile does not fit.
inline bool try_bulk_rem(ConvRoute& r, const ConvPhase* ph, int i, bool f16, const ConvKnobs& k, int BM, int WM, int WN, long slots, bool may_split) {
    const ConvPhase& p = ph[i];
    const long tn = p.RP / 128, tiles = (long)cdiv(p.M, BM) * tn, full = tiles / slots, rem = tiles % slots;
    const bool split = may_split && !p.no_split && full >= 1 && rem > 0 && rem * 2 <= slots && slots % tn == 0;
    const int m_bulk = split ? (int)(full * slots / tn) * BM : p.M;
    if (!try_glds(r, ph, i, f16, k, BM, 128, WM, WN, 0, m_bulk)) return false;
    // The 64x64 launch fits whenever the bulk did (smaller stages, no more table rows), so the error below is unreachable; the
    // try-in-order code this replaced would have returned its bare "does not fit" code there without a message.
    if (split && !try_glds(r, ph, i, f16, k, 64, 64, 2, 2, m_bulk, p.M)) { r.error = CONV_ERR_NOFIT; r.err_rc = -100; }
    return true;
}

inline void route_phase(ConvRoute& r, const ConvPhase* ph, int i, bool f16, const ConvKnobs& k, bool halo_on) {
    const ConvPhase& p = ph[i];
    if (p.M <= 0 || p.ntaps <= 0) return;
    if (!fits_32bit(p)) { r.error = CONV_ERR_2G; return; }
    const long in_elems = (long)p.B * p.Hi * p.Wi * p.Ci;
    if ((p.x3 || f16) && (in_elems * (f16 ? 2 : 4) > (1L << 32) - (1L << 26) || p.nky * p.nkx > 32)) {
        r.error = CONV_ERR_DMA; r.err_elems = in_elems; r.err_taps = p.nky * p.nkx;
        return;
    }
    const TileCfg c = pick_cfg(f16, p.Co, p.Ci, p.x3 != 0);
    // LDS-DMA path: every layer whose K chunk is a 128-byte row (rows are 16-byte aligned in HBM: Ci % 4 == 0 for fp32,
    // Ci % 8 == 0 for f16)
    const bool only_glds = f16 || p.x3;  // no register-staged fallback for these operand formats
    const bool glds = only_glds || (c.BK == 32 && k.conv_variant != 1);
    if (p.x3 && p.Ci < 24 && !p.dense) { r.error = CONV_ERR_X3_CIN; return; }
    const auto whole = [&](int BM, int BN, int WM, int WN) { return try_glds(r, ph, i, f16, k, BM, BN, WM, WN, 0, p.M); };
    const auto nofit = [&] { r.error = CONV_ERR_NOFIT; r.err_rc = -100; };  // (the code the message has always shown for "LDS")
    if (f16) {
        if (halo_eligible(p, halo_on)) return push_halo(r, p, i);
        if (c.BN == 64) {
            if (!whole(128, 64, 2, 2)) nofit();
            return;
        }
        // f16 MFMAs are 8x shorter than fp32 ones while an LDS-DMA piece costs the same to issue: on 128x128 tiles a wave issues
        // one 1-KiB piece per two MFMAs and the loop is bound by DMA issue + LDS traffic, not by the matrix pipe.  Layers with
        // >= 256 output channels and enough rows run 256x256 tiles on 8 waves (2 x 4, wave tile 128x64: one piece per four
        // MFMAs, 0.75 instead of 1 operand read per MFMA; 128 KB of LDS, one workgroup per CU): 512->512 at 64^2 780 -> 886
        // TFLOP/s, 256->256 at 128^2 710 -> 752.  GIF_F16_TILE256=0: A/B knob.
        if (k.f16_tile256 && c.BN == 128 && p.RP % 256 == 0 && (long)cdiv(p.M, 256) * (p.RP / 256) >= 512 && whole(256, 256, 2, 4)) return;
    }
    if (c.BN == 128 && (f16 || c.BK == 32)) {
        // low-resolution bf16x3 / f16x2 layers with at least one workgroup per CU: 128x64 tiles, 4 waves stacked along M (wave tile
        // 32x64: one activation fragment split per 12 MFMAs instead of per 6 on the 64x64 tile's 32x32 wave tiles) — 512->512 at
        // 16^2 143 -> 165 TFLOP/s, modulated 127 -> 157, stride-2 512->512 at 33^2 142 -> 170
        if (p.x3 && small_tiles(p) && (long)cdiv(p.M, 128) * (p.RP / 64) >= 256 && whole(128, 64, 4, 1)) return;
        if (glds && small_tiles(p) && whole(64, 64, 2, 2)) return;
        // bf16x3: the pre-split weight tile (48 KB) + the fp32 activation tile (32 KB) fill half a CU's LDS exactly, and a
        // modulated conv's scale table no longer fits beside them.  Big layers run 256x128 tiles on 8 waves instead: one
        // workgroup per CU (112 KB + table), still two waves per SIMD, a quarter less operand traffic per MFMA — 8 (M) x 1 (N)
        // waves, wave tile 32 x 128: ONE activation fragment to split per 24 MFMAs (the 4 x 2 layout splits two).
        // Not the tap-dense layers (K = 9 taps x 8..28 channels: 3..7 stages): one 8-wave workgroup per CU spends most of a tile in its
        // prologue and epilogue with nothing else resident; two 4-wave workgroups per CU on 128x128 tiles: 24 -> 256 at 128^2 129 ->
        // 133 TFLOP/s, 24 -> 512 at 64^2 130 -> 134, the family in the step 8.57 -> 8.19 ms (GIF_DENSE_TILE=256: A/B)
        if (p.x3 && k.x3_big && big_tiles(p) && !(p.dense && k.dense128)) {
            const bool w42 = k.x3_waves == 42 && p.x3 == 1;
            if (try_bulk_rem(r, ph, i, f16, k, 256, w42 ? 4 : 8, w42 ? 2 : 1, 256, true)) return;
        }
        if (glds) {
            // 128x128 tile: 2 x 2 waves of 64 x 64; bf16x3 / f16x2: 4 x 1 waves of 32 x 128
            const bool w41 = p.x3 == 2 || (p.x3 && k.x3_waves != 42);
            if (try_bulk_rem(r, ph, i, f16, k, 128, w41 ? 4 : 2, w41 ? 1 : 2, 512, k.conv_variant != 3)) return;
            if (only_glds) return nofit();
        }
        return push_simple(r, p, i, 128, 128, 32, 2, 2);
    }
    if (rows_thin_ok(p, k)) return push_rows_thin(r, p, i);  // f16x2, stride-1 3x3, <= 32 output channels: rows + halo staged once per kernel row
    if (only_glds) {
        if (!whole(256, 32, 4, 1)) nofit();
        return;
    }
    if (c.BN == 128) return push_simple(r, p, i, 128, 128, 8, 2, 2);
    if (c.BK == 32) {
        if (glds && whole(256, 32, 4, 1)) return;
        return push_simple(r, p, i, 256, 32, 32, 4, 1);
    }
    push_simple(r, p, i, 256, 32, 8, 4, 1);
}

// The route of one op over its nph phases (ph[0]'s mode fields are read even when nph == 0).  halo_on: the run-time halo switch.
inline ConvRoute conv_route(const ConvPhase* ph, int nph, bool f16, const ConvKnobs& k, bool halo_on) {
    ConvRoute r{};
    r.f16 = f16;
    r.family = conv_family(ph[0], f16);
    // small transposed convs: every phase alone would sit on the 64x64-tile path with a partly filled chip; big bf16x3 / f16x2
    // ones: every phase would run 256x128 tiles on its own (bulk + remainder launch each)
    if (nph > 1 && k.conv_variant == 0) {
        const TileCfg c = pick_cfg(f16, ph[0].Co, ph[0].Ci, ph[0].x3 != 0);
        const bool wide = c.BN == 128 && (f16 || c.BK == 32);
        bool small_all = wide, big_all = wide && ph[0].x3 && k.x3_multi_big;
        for (int i = 0; i < nph; ++i) {
            small_all = small_all && small_tiles(ph[i]) && fits_32bit(ph[i]);
            big_all = big_all && big_tiles(ph[i]) && fits_32bit(ph[i]);
        }
        if (small_all) try_multi(r, ph, nph, f16, 64, 64, 2, 2, 2);
        else if (big_all) try_multi(r, ph, nph, f16, 256, 128, 8, 1, (ph[0].x3 == 2 && k.h2_ring3) ? 3 : 2);
    }
    if (!r.merged)
        for (int i = 0; i < nph && !r.error; ++i) route_phase(r, ph, i, f16, k, halo_on);
    return r;
}

}  // namespace gif_conv
