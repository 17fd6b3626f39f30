// Prints the forward / data-gradient route table of gif_amd/csrc/conv_route.h (host only: this program includes nothing else of the library).
// One line per case:
//   name | op | mode | flags | the forward conv's geometry -> packing, family, phases, zero fill, merged, partial rows x tile rows [, halo] : launches
// (f16x2 cases: the route of the guarded bf16x3 twin after " + twin").  Cases: first the lines of the file given as the first argument
// (tests/golden/conv_route_cases.txt: the library calls ops.conv_plan decides on for the rows of tests/test_gpu_conv_routes.py), then a grid of
// its own that puts every predicate of the header on both sides of its threshold, all with the default knobs; then once per non-default
// knob value over that grid, where only the cases are printed whose line differs from the default one (and how many of how many did).
// tests/test_conv_route.py builds this with AddressSanitizer and UBSan (host code only), runs it and compares the output with
// tests/golden/conv_route_table.txt line by line.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "conv_route.h"

using namespace gif_conv;

namespace {

const char* const kModeName[] = {"native", "bf16x3", "f16x2", "f16"};
const char* const kKernelName[] = {"simple", "glds", "multi", "rows_thin", "halo"};

// a case: the FORWARD convolution (big side H x W, channel counts as the activations carry them) and the op run on it
struct Case {
    std::string name;
    bool dgrad;
    int mode;  // 0 native, 1 bf16x3, 2 f16x2, 3 f16 activations
    bool dense, scaled, dot;
    int B, Cin, Cout, K, stride, pad, H, W;
};

std::string launch_text(const ConvLaunch& l) {
    char b[400];
    int n = snprintf(b, sizeof b, "%s", kKernelName[l.kernel]);
    if (l.kernel == CONV_HALO) n += snprintf(b + n, sizeof b - n, " bn%d cp%d t2 %dx%d", l.BN, l.HCP, l.t2_tx, l.t2_ty);
    else if (l.kernel == CONV_SIMPLE) n += snprintf(b + n, sizeof b - n, " %dx%dx%d w%dx%d", l.BM, l.BN, l.BK, l.WM, l.WN);
    else if (l.kernel != CONV_ROWS_THIN)
        n += snprintf(b + n, sizeof b - n, " %s %dx%dx%d w%dx%d sc%d x3=%d nst%d", l.f16 ? "f16" : "f32", l.BM, l.BN, l.BK, l.WM, l.WN, (int)l.SCALE,
                      l.X3, l.NST);
    if (l.kernel == CONV_GLDS_MULTI) n += snprintf(b + n, sizeof b - n, " ph0-%d", l.nph - 1);
    else n += snprintf(b + n, sizeof b - n, " ph%d m[%d,%d)", l.phase0, l.m_begin, l.M);
    n += snprintf(b + n, sizeof b - n, " grid%ld thr%d lds%zu tn%d stride%d", l.grid, l.threads, l.lds_bytes, l.tiles_n, l.stab_stride);
    for (int i = 0; i < l.nph; ++i) n += snprintf(b + n, sizeof b - n, " (tm%d nb%d row%d)", l.tiles_m[i], l.stab_nb[i], l.part_row0[i]);
    return b;
}

std::string route_text(const ConvRoute& r) {
    char b[200];
    if (r.error) {
        snprintf(b, sizeof b, "error %d elems %ld taps %d rc %d", r.error, r.err_elems, r.err_taps, r.err_rc);
        return b;
    }
    snprintf(b, sizeof b, "merged%d rows %d x %d :", (int)r.merged, r.part_rows, r.tile_rows);
    std::string s = b;
    for (int i = 0; i < r.nlaunch; ++i) s += (i ? " ; " : " ") + launch_text(r.launch[i]);
    return s;
}

std::string line(const Case& c, const ConvKnobs& k, bool halo_on) {
    const bool f16 = c.mode == 3;
    const int Hs = (c.H + 2 * c.pad - c.K) / c.stride + 1, Ws = (c.W + 2 * c.pad - c.K) / c.stride + 1;
    const ConvShape shape{c.B, c.H, c.W, c.Cin, Hs, Ws, c.Cout, c.K, c.K, c.stride, c.pad, f16, f16 ? 0 : c.mode, c.dense, c.scaled, c.dot};
    ConvPhases ph = c.dgrad ? conv_phases_bwd_data(shape) : conv_phases_fwd(shape);
    const ConvRoute r = conv_route(ph.ph, ph.nph, f16, k, halo_on);
    char head[300];
    int n = snprintf(head, sizeof head, "%s | %s | %s | d%d s%d t%d | B%d Ci%d Co%d k%d s%d p%d %dx%d -> RP%d CP%d pair%d fam%d nph%d zero%d", c.name.c_str(),
                     c.dgrad ? "dgrad" : "fwd", kModeName[c.mode], (int)c.dense, (int)c.scaled, (int)c.dot, c.B, c.Cin, c.Cout, c.K, c.stride, c.pad, c.H,
                     c.W, ph.ph[0].RP, ph.ph[0].CP, ph.ph[0].pair, r.family, ph.nph, (int)ph.need_zero);
    if (f16 && !c.dgrad) snprintf(head + n, sizeof head - n, " halo%d", (int)(r.nlaunch > 0 && r.launch[0].kernel == CONV_HALO));
    std::string s = std::string(head) + " " + route_text(r);
    if (c.mode == 2) {  // the guarded twin: the same phases with x3 = 1
        for (ConvPhase& q : ph.ph) q.x3 = 1;
        s += " + twin " + route_text(conv_route(ph.ph, ph.nph, false, k, halo_on));
    }
    return s;
}

std::vector<Case> file_cases(const char* path) {
    std::vector<Case> v;
    FILE* f = fopen(path, "r");
    if (!f) return v;
    char name[64], op[16], mode[16];
    int d, s, t, B, Cin, Cout, K, st, pad, H, W;
    while (fscanf(f, "%63s %15s %15s %d %d %d %d %d %d %d %d %d %d %d", name, op, mode, &d, &s, &t, &B, &Cin, &Cout, &K, &st, &pad, &H, &W) == 14) {
        int m = 0;
        while (m < 3 && strcmp(mode, kModeName[m])) ++m;
        v.push_back(Case{name, !strcmp(op, "dgrad"), m, d != 0, s != 0, t != 0, B, Cin, Cout, K, st, pad, H, W});
    }
    fclose(f);
    return v;
}

const int kNative = 1, kX3 = 2, kH2 = 4, kF16 = 8, kFp32 = 7, kSplit = 6;
enum { DENSE = 1, SCALED = 2, DOT = 4, DGRAD = 8 };

// modes: bit m set = add the case in mode m
void add(std::vector<Case>& v, const char* name, int modes, int flags, int B, int Cin, int Cout, int K, int stride, int pad, int H, int W) {
    for (int m = 0; m < 4; ++m)
        if (modes >> m & 1)
            v.push_back(Case{name, (flags & DGRAD) != 0, m, (flags & DENSE) != 0, (flags & SCALED) != 0, (flags & DOT) != 0, B, Cin, Cout, K, stride, pad, H, W});
}

// Every predicate of the header on both sides of its threshold.
std::vector<Case> grid() {
    std::vector<Case> v;
    // tiles128 = cdiv(M, 128) * RP / 128: 383 | 384 (64x64 / 128x64 tiles below)
    add(v, "g_t128_383", kFp32, 0, 1, 36, 48, 3, 1, 1, 127, 386);
    add(v, "g_t128_384", kFp32, 0, 1, 36, 48, 3, 1, 1, 127, 387);
    add(v, "g_t128_383", kF16, 0, 1, 40, 72, 3, 1, 1, 127, 386);
    add(v, "g_t128_384", kF16, 0, 1, 40, 72, 3, 1, 1, 127, 387);
    // bf16x3 / f16x2: 128x64 tiles from cdiv(M, 128) * RP / 64 >= 256: 254 | 256
    add(v, "g_t64_254", kSplit, SCALED, 2, 36, 48, 3, 1, 1, 63, 129);
    add(v, "g_t64_256", kSplit, SCALED, 2, 36, 48, 3, 1, 1, 63, 130);
    // tiles256 = cdiv(M, 256) * RP / 128: 511 | 512 (256x128 on 8 waves; f16: 256x256 with RP / 256)
    add(v, "g_t256_511", kFp32, 0, 1, 36, 48, 3, 1, 1, 255, 513);
    add(v, "g_t256_512", kFp32, 0, 1, 36, 48, 3, 1, 1, 255, 514);
    add(v, "g_t256_511", kF16, 0, 1, 72, 256, 1, 1, 0, 255, 513);
    add(v, "g_t256_512", kF16, 0, 1, 72, 256, 1, 1, 0, 255, 514);
    add(v, "g_t256_rp384", kF16, 0, 1, 72, 384, 1, 1, 0, 511, 514);  // RP % 256 != 0
    // bulk + remainder: rem * 2 <= slots (split modes: 256 slots of 256-row tiles, rem 128 | 129; native and f16: 512 slots of 128-row
    // tiles, rem 255 | 257), slots % tn (tn 2 | 3), full >= 1 (g_t128_384: 384 tiles, no full round), no_split (the dot fusion)
    add(v, "g_rem128", kFp32, 0, 1, 36, 48, 3, 1, 1, 255, 642);
    add(v, "g_rem129", kFp32, 0, 1, 36, 48, 3, 1, 1, 255, 643);
    add(v, "g_rem128", kF16, 0, 1, 40, 72, 3, 1, 1, 255, 642);
    add(v, "g_rem129", kF16, 0, 1, 40, 72, 3, 1, 1, 255, 643);
    add(v, "g_rem128_dot", kFp32 | kF16, DOT, 1, 40, 72, 3, 1, 1, 255, 642);
    add(v, "g_rem_tn2", kFp32 | kF16, SCALED, 1, 40, 136, 3, 1, 1, 129, 509);
    add(v, "g_rem_tn3", kFp32 | kF16, 0, 1, 40, 384, 3, 1, 1, 171, 255);
    add(v, "g_rem128_dgrad", kFp32, DGRAD, 1, 48, 36, 3, 1, 1, 255, 642);
    // tap-dense layers: 128x128 instead of 256x128 tiles
    add(v, "g_dense_big", kSplit, DENSE, 1, 24, 256, 3, 1, 1, 256, 256);
    add(v, "g_dense_c20", kSplit, DENSE, 2, 20, 48, 3, 1, 1, 33, 40);
    add(v, "g_c20_plain", kFp32, 0, 2, 20, 48, 3, 1, 1, 33, 40);  // bf16x3 / f16x2 without the dense order: error
    // rows_thin_ok, clause by clause (f16x2; the bf16x3 line shows the same shape without the kernel)
    add(v, "g_thin", kSplit, 0, 2, 36, 32, 3, 1, 1, 24, 32);
    add(v, "g_thin_dgrad", kH2, DGRAD, 2, 20, 40, 3, 1, 1, 16, 64);
    add(v, "g_thin_scaled", kH2, SCALED, 2, 36, 32, 3, 1, 1, 24, 32);
    add(v, "g_thin_dense", kH2, DENSE, 2, 24, 32, 3, 1, 1, 24, 32);
    add(v, "g_thin_1x1", kH2, 0, 2, 36, 32, 1, 1, 0, 24, 32);
    add(v, "g_thin_pad0", kH2, 0, 2, 36, 32, 3, 1, 0, 26, 34);
    add(v, "g_thin_s2", kH2, 0, 2, 36, 32, 3, 2, 1, 47, 63);
    add(v, "g_thin_s2_dgrad", kH2, DGRAD, 2, 32, 36, 3, 2, 1, 47, 63);
    add(v, "g_thin_o36", kH2, 0, 2, 36, 36, 3, 1, 1, 24, 32);
    add(v, "g_thin_w256", kH2, 0, 1, 40, 32, 3, 1, 1, 3, 256);
    add(v, "g_thin_w48", kH2, 0, 1, 36, 32, 3, 1, 1, 16, 48);
    add(v, "g_thin_w16", kH2, 0, 1, 36, 32, 3, 1, 1, 32, 16);
    add(v, "g_thin_m320", kH2, 0, 1, 36, 32, 3, 1, 1, 5, 64);
    add(v, "g_thin_4g_62", kH2, 0, 1, 64, 32, 3, 1, 1, 62, 262144);  // (B*Hi*Wi + Wi) * Ci * 4: 2^32 - 2^26 | 2^32
    add(v, "g_thin_4g_63", kH2, 0, 1, 64, 32, 3, 1, 1, 63, 262144);
    // halo_eligible, clause by clause (f16)
    add(v, "g_halo_16", kF16, 0, 2, 32, 64, 3, 1, 1, 16, 16);
    add(v, "g_halo_15", kF16, 0, 2, 32, 64, 3, 1, 1, 15, 17);
    add(v, "g_halo_w15", kF16, 0, 2, 32, 64, 3, 1, 1, 17, 15);
    add(v, "g_halo_c40_o32", kF16, 0, 1, 40, 32, 3, 1, 1, 17, 20);
    add(v, "g_halo_c40_o40", kF16, 0, 1, 40, 40, 3, 1, 1, 17, 20);
    add(v, "g_halo_c72", kF16, 0, 1, 72, 32, 1, 1, 0, 17, 20);
    add(v, "g_halo_o72", kF16, 0, 1, 32, 72, 3, 1, 1, 17, 20);
    add(v, "g_halo_s2", kF16, 0, 2, 32, 32, 3, 2, 0, 33, 35);
    add(v, "g_halo_s2_dgrad", kF16, DGRAD, 2, 32, 32, 3, 2, 0, 33, 35);
    add(v, "g_halo_k4", kF16, 0, 2, 8, 8, 4, 1, 1, 32, 32);
    add(v, "g_halo_dot_h24", kF16, DOT, 2, 16, 24, 3, 1, 1, 24, 32);
    add(v, "g_halo_dot_h32", kF16, DOT, 2, 16, 24, 3, 1, 1, 32, 32);
    // (the patch-count clause, B * patches >= 2^23, lies behind the 2^31-element limit: 2^23 patches of 256 pixels x >= 8 channels)
    // LDS: a modulated 256x128 f16x2 launch whose scale table fits (8x8 maps: 5 rows) | does not fit (4x4: 17 rows) beside three stages
    add(v, "g_ring3_fits", kSplit, SCALED, 512, 512, 512, 3, 1, 1, 8, 8);
    add(v, "g_ring3_nofit", kSplit, SCALED, 2048, 512, 512, 3, 1, 1, 4, 4);
    // a modulated 256x256 f16 launch that fits 160 KB (512 channels) | does not (1024)
    add(v, "g_f16_256_fits", kF16, SCALED, 2048, 512, 1024, 3, 1, 1, 4, 4);
    add(v, "g_f16_256_nofit", kF16, SCALED, 2048, 1024, 1024, 3, 1, 1, 4, 4);
    // native: the scale table of 129 one-pixel samples fits no LDS-DMA tile -> the register-staged kernel; bf16x3 / f16x2 / f16: error
    add(v, "g_lds_o128", kFp32 | kF16, SCALED, 129, 512, 128, 1, 1, 0, 1, 1);
    add(v, "g_lds_o32", kFp32 | kF16, SCALED, 257, 512, 32, 1, 1, 0, 1, 1);
    add(v, "g_lds_o128_plain", kNative, 0, 129, 512, 128, 1, 1, 0, 1, 1);
    // the register-staged kernels of the native mode, and the 256x32 LDS-DMA tile
    add(v, "g_c8_o48", kNative, 0, 1, 8, 48, 3, 1, 1, 33, 40);
    add(v, "g_c8_o32", kNative, 0, 1, 8, 32, 3, 1, 1, 33, 40);
    add(v, "g_c36_o32", kFp32, 0, 1, 36, 32, 3, 1, 1, 33, 40);
    add(v, "g_c40_o32", kF16, SCALED, 1, 40, 32, 3, 2, 0, 33, 41);
    add(v, "g_c40_o64", kF16, SCALED, 1, 72, 64, 3, 1, 1, 33, 40);
    // transposed convs: small_all (phase 0: 383 | 384 tiles of 128) and big_all (smallest phase: 512 | 511 tiles of 256) with one phase on
    // the wrong side; the 1x1 stride-2 data gradient with three empty phases
    add(v, "g_tconv_small_all", kFp32, DGRAD | SCALED, 1, 48, 36, 3, 2, 0, 311, 627);
    add(v, "g_tconv_not_small", kFp32, DGRAD | SCALED, 1, 48, 36, 3, 2, 0, 311, 629);
    add(v, "g_tconv_small_all", kF16, DGRAD, 1, 72, 40, 3, 2, 0, 311, 627);
    add(v, "g_tconv_not_small", kF16, DGRAD, 1, 72, 40, 3, 2, 0, 311, 629);
    add(v, "g_tconv_big_all", kFp32, DGRAD | SCALED, 1, 48, 36, 3, 2, 0, 725, 725);
    add(v, "g_tconv_not_big", kFp32, DGRAD, 1, 48, 36, 3, 2, 0, 723, 725);
    add(v, "g_tconv_o32", kFp32 | kF16, DGRAD, 2, 32, 40, 3, 2, 0, 33, 35);
    add(v, "g_dgrad_1x1_s2", kFp32 | kF16, DGRAD, 2, 16, 40, 1, 2, 0, 31, 19);
    add(v, "g_dgrad_1x1_s2_p1_h1", kNative, DGRAD, 2, 16, 40, 1, 2, 1, 1, 1);  // no phase has a tap
    // every error kind: >= 2^31 elements; >= 4 GiB of input or > 32 taps on the buffer-addressed DMA; < 24 channels (g_c20_plain); LDS (g_lds_*)
    add(v, "g_err_2g", kFp32, 0, 64, 36, 4, 3, 1, 1, 1024, 1024);
    add(v, "g_err_4gib", kFp32, 0, 32, 36, 4, 3, 1, 1, 1024, 1024);
    add(v, "g_err_taps", kSplit | kF16, 0, 1, 40, 40, 6, 1, 1, 33, 40);
    add(v, "g_err_2g_tconv", kX3, DGRAD, 64, 4, 36, 3, 2, 0, 2047, 2047);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    const ConvKnobs def;
    if (argc > 1)
        for (const Case& c : file_cases(argv[1])) puts(line(c, def, true).c_str());
    const std::vector<Case> g = grid();
    for (const Case& c : g) puts(line(c, def, true).c_str());

    struct Setting {
        const char* name;
        ConvKnobs k;
        bool halo_on;
    };
    std::vector<Setting> settings;
    const auto with = [&](const char* name, auto set, bool halo_on = true) {
        ConvKnobs k;
        set(k);
        settings.push_back(Setting{name, k, halo_on});
    };
    with("GIF_H2_RING=2", [](ConvKnobs& k) { k.h2_ring3 = false; });
    with("GIF_H2_ROWS_THIN=0", [](ConvKnobs& k) { k.h2_rows_thin = false; });
    with("GIF_X3_WAVES=42", [](ConvKnobs& k) { k.x3_waves = 42; });
    with("GIF_F16_TILE256=0", [](ConvKnobs& k) { k.f16_tile256 = false; });
    with("GIF_X3_BIG=0", [](ConvKnobs& k) { k.x3_big = false; });
    with("GIF_DENSE_TILE=256", [](ConvKnobs& k) { k.dense128 = false; });
    with("GIF_X3_MULTI_BIG=0", [](ConvKnobs& k) { k.x3_multi_big = false; });
    with("GIF_CONV_VARIANT=1", [](ConvKnobs& k) { k.conv_variant = 1; });
    with("GIF_CONV_VARIANT=2", [](ConvKnobs& k) { k.conv_variant = 2; });
    with("GIF_CONV_VARIANT=3", [](ConvKnobs& k) { k.conv_variant = 3; });
    with("GIF_F16_HALO=0", [](ConvKnobs& k) { k.f16_halo = false; }, false);  // (the switch's initial value: conv_route's halo_on)
    for (const Setting& st : settings) {
        int differ = 0;
        for (const Case& c : g) {
            const std::string a = line(c, def, true), b = line(c, st.k, st.halo_on);
            if (a == b) continue;
            ++differ;
            printf("%s: %s\n", st.name, b.c_str());
        }
        printf("%s: %d of %zu cases differ from the default\n", st.name, differ, g.size());
    }
    return 0;
}
