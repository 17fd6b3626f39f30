// Prints the weight-gradient route table of gif_amd/csrc/wgrad_route.h (host only: this program includes nothing else of the library).
// One line per case:
//   geometry | mode | u(nscaled) / s(caled) | nsplit -> primary launch [+ twin] ; route fields | tiles per split, splits of the query
// first over a fixed grid with the default knobs, then once per non-default knob value over a smaller grid, where only the cases are
// printed whose line differs from the default one (and how many of how many did).  With arguments: the lines of the plane GEMMs and
// convolutions asked for (see main).  tests/test_wgrad_route.py builds this with
// AddressSanitizer and UBSan (host code only), runs it and compares the output with tests/golden/wgrad_route_table.txt line by line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "wgrad_route.h"

using namespace gif_wgrad;

namespace {

const int kMode16 = 3;  // f16 operands (the fp32 contraction modes are 0 native, 1 bf16x3, 2 f16x2)
const char* const kModeName[] = {"native", "bf16x3", "f16x2", "f16"};

// a convolution by the shape of its small side (the output gradient): the big side follows from kernel, stride and pad
WgradShape conv(int B, int Hs, int Ws, int Cs, int Cb, int K, int stride, bool scaled) {
    const int pad = stride == 1 ? (K - 1) / 2 : 0;
    const int Hb = (Hs - 1) * stride + K - 2 * pad, Wb = (Ws - 1) * stride + K - 2 * pad;
    return WgradShape{B, Hb, Wb, Cb, Hs, Ws, Cs, K, K, stride, pad, scaled, false};
}
WgradShape planes(long ntiles, int CsP, int CbP) { return WgradShape{1, 1, (int)ntiles, CbP, 1, (int)ntiles, CsP, 1, 1, 1, 0, false, true}; }

std::string launch_text(const WgradLaunch& l) {
    char b[256];
    int n = 0;
    switch (l.kernel) {
    case WGRAD_SMALL: snprintf(b, sizeof b, "small thr%d wgs%ld", l.threads, l.wgs_per_split); break;
    case WGRAD_HALO: snprintf(b, sizeof b, "halo tr%d thr%d wgs%ld", (int)l.TR, l.threads, l.wgs_per_split); break;
    case WGRAD_H2V2:
        n = snprintf(b, sizeof b, "h2v2 tab%d thr%d wgs%ld", (int)l.TAB, l.threads, l.wgs_per_split);
        if (l.TAPS) n += snprintf(b + n, sizeof b - n, " taps tpt%d tg%d", l.tpt, l.tgroups);
        if (l.unit_tab) snprintf(b + n, sizeof b - n, " unit");
        break;
    default:
        snprintf(b, sizeof b, "mfma %s %dx%d w%dx%d glds%d bkp%d tab%d x3=%d thr%d wgs%ld", l.f16 ? "f16" : "f32", l.BP, l.BQ, l.WP, l.WQ, (int)l.GLDS,
                 l.BKP, (int)l.TAB, l.X3, l.threads, l.wgs_per_split);
    }
    return b;
}

// nsplit <= 0: the count the splits query returns (what the Python side passes)
std::string line(const WgradShape& g, int mode, int nsplit, const WgradKnobs& k) {
    const bool f16 = mode == kMode16;
    WgradShape u = g;
    u.scaled = false;
    const int splits = f16 ? wgrad_splits_f16(u, k) : wgrad_splits(u, mode, k);
    const long tiles = f16 ? -1 : wgrad_tiles_per_split(u, mode, k);
    if (nsplit <= 0) nsplit = splits;
    const WgradRoute r = f16 ? wgrad_route_f16(g, nsplit, k) : wgrad_route(g, mode, nsplit, k);
    char head[200], tail[200];
    if (g.planes) snprintf(head, sizeof head, "planes tiles%d Cs%d Cb%d", g.Ws, g.Cs, g.Cb);
    else if (g.KH != g.KW) snprintf(head, sizeof head, "B%d Hs%d Ws%d Cs%d Cb%d k%dx%d s%d p%d", g.B, g.Hs, g.Ws, g.Cs, g.Cb, g.KH, g.KW, g.stride, g.pad);
    else snprintf(head, sizeof head, "B%d Hs%d Ws%d Cs%d Cb%d k%d s%d p%d", g.B, g.Hs, g.Ws, g.Cs, g.Cb, g.KH, g.stride, g.pad);
    snprintf(tail, sizeof tail, " ; RP%d CP%d t%d tq%d tpq%d stab%d chunk%ld fam%d | tiles %ld splits %d", r.RP, r.CP, r.tile_f16, r.tiles_q, r.tiles_pq,
             r.stab_nb, r.chunk, r.family, tiles, splits);
    std::string s = std::string(head) + " | " + kModeName[mode] + " | " + (g.scaled ? "s" : "u") + " | n" + std::to_string(nsplit) + " -> " +
                    launch_text(r.primary);
    if (r.has_twin) s += " + twin " + launch_text(r.twin);
    return s + tail;
}

struct Case {
    WgradShape g;
    int mode, nsplit;
};

// modes: bit m set = print contraction mode m (bit 3: f16 operands, dropped where the channels are no multiples of 8)
const int kAll = 15, kF16 = 8;
void add(std::vector<Case>& v, const WgradShape& g, int modes = kAll, int nsplit = 0) {
    for (int mode = 0; mode <= kMode16; ++mode) {
        if (!(modes >> mode & 1) || (mode == kMode16 && (g.planes || g.Cs % 8 || g.Cb % 8))) continue;
        v.push_back(Case{g, mode, nsplit});
    }
}

// Every predicate of the header on both sides of its threshold (the rows of tests/test_gpu_conv_routes.py and their neighbours).
std::vector<Case> full_grid() {
    std::vector<Case> v;
    // channel classes at 16384 pixels, 3x3: tile_of (32 | 36), Cs % 256 rows (128 | 132 -> 256 | 384 | 512), thin big side, f16 tiles
    const int pairs[][2] = {{4, 4},     {16, 16},   {20, 20},   {24, 24},   {32, 32},   {36, 36},   {64, 64},   {128, 128}, {132, 132}, {256, 256},
                            {384, 384}, {512, 512}, {32, 16},   {32, 20},   {36, 16},   {48, 24},   {40, 36},   {132, 36},  {24, 128},  {64, 32},
                            {72, 24},   {256, 128}, {128, 256}, {384, 256}};
    for (const auto& c : pairs) add(v, conv(1, 128, 128, c[0], c[1], 3, 1, false));
    const int mod[][2] = {{32, 32}, {48, 24}, {36, 128}, {128, 128}, {256, 256}, {64, 64}};
    for (const auto& c : mod) add(v, conv(1, 128, 128, c[0], c[1], 3, 1, true));
    // 16383 | 16384 pixels: 256-row native tiles, 256x256 f16 tiles
    add(v, conv(1, 127, 129, 256, 256, 3, 1, false));
    add(v, conv(1, 127, 129, 132, 36, 3, 1, false), 1);
    // 65280 | 65536 pixels: conv_wgrad_small_mfma (un-modulated, Cb <= 16, 3x3 stride 1 only)
    for (int w : {255, 256})
        for (bool scaled : {false, true}) add(v, conv(1, 256, w, 32, 16, 3, 1, scaled), scaled ? 1 : kAll);
    add(v, conv(1, 256, 256, 32, 20, 3, 1, false), 1);
    add(v, conv(1, 256, 256, 36, 16, 3, 1, false), 1);
    add(v, conv(1, 256, 256, 32, 16, 1, 1, false), 1);
    // Hs*Ws modulo 16 and 32: 16 (4x4), 272, 64, 35 pixels per sample; scale-table kernels, 16-pixel stages, the f16 64 -> 32 tile
    const int maps[][2] = {{4, 4}, {16, 17}, {8, 8}, {5, 7}};
    for (const auto& m : maps) {
        add(v, conv(2, m[0], m[1], 128, 128, 3, 1, false), 4 | kF16);
        add(v, conv(2, m[0], m[1], 128, 128, 3, 1, true));
        add(v, conv(2, m[0], m[1], 64, 64, 3, 1, true), kF16);
    }
    // 1x1, stride 2, odd sizes
    const int odd[][2] = {{48, 24}, {40, 36}, {32, 16}};
    for (const auto& c : odd) {
        add(v, conv(2, 33, 35, c[0], c[1], 1, 1, false));
        add(v, conv(2, 16, 17, c[0], c[1], 3, 2, false));
    }
    // scale-table limits: the fp32 and the 128-wide f16 table hold 64 samples (64 KB), the 256-wide f16 table 16 (32 KB); the samples
    // a chunk touches follow from the split count: 65 | 45 of 16 pixels, 17 | 9 of 256 pixels
    for (int nsplit : {2, 3}) {
        add(v, conv(128, 4, 4, 128, 128, 3, 1, true), kAll, nsplit);
        add(v, conv(128, 4, 4, 128, 128, 3, 1, false), 4, nsplit);
    }
    for (int nsplit : {4, 8}) add(v, conv(64, 16, 16, 256, 256, 3, 1, true), kF16, nsplit);
    // conv_wgrad_halo_f16: 512 | 480 patches, 15 rows, 40 channels, and only with its own split count
    add(v, conv(2, 256, 256, 32, 32, 3, 1, false), kF16);
    add(v, conv(2, 256, 256, 32, 32, 1, 1, true), kF16);
    add(v, conv(2, 255, 240, 32, 32, 3, 1, false), kF16);
    add(v, conv(512, 15, 16, 32, 32, 3, 1, false), kF16);
    add(v, conv(2, 256, 256, 40, 32, 3, 1, false), kF16);
    for (int nsplit : {511, 513}) add(v, conv(2, 256, 256, 32, 32, 3, 1, false), kF16, nsplit);
    // Winograd plane GEMMs (channels as the transforms pad them)
    const int pl[][2] = {{32, 32}, {128, 32}, {32, 128}, {128, 128}, {256, 128}, {256, 256}};
    for (const auto& c : pl)
        for (long ntiles : {16380L, 16384L}) add(v, planes(ntiles, c[0], c[1]));
    for (long ntiles : {2046L, 2048L}) add(v, planes(ntiles, 128, 128));
    return v;
}

std::vector<Case> knob_grid() {
    std::vector<Case> v;
    const int pairs[][2] = {{48, 24}, {256, 256}, {32, 16}, {32, 32}};
    for (const auto& c : pairs)
        for (bool scaled : {false, true}) {
            add(v, conv(1, 128, 128, c[0], c[1], 3, 1, scaled));
            add(v, conv(2, 256, 256, c[0], c[1], 3, 1, scaled));
        }
    add(v, planes(16384, 256, 256));
    return v;
}

}  // namespace

// Argument groups, any number of them, one line per group instead of the table:
//   planes <ntiles> <CsP> <CbP> <mode> <nsplit>: the plane GEMMs of that Winograd weight gradient (tests/test_cpu_wiring.py asks for the
//     rows of tests/test_gpu_winograd_edges.py this way)
//   conv <B> <Hs> <Ws> <Cs> <Cb> <KH> <KW> <stride> <pad> <scaled> <mode> <nsplit>: a direct weight gradient by the shape of its small
//     side (mode 3: f16 operands; nsplit 0: the query's count) — the rows of tests/test_gpu_wgrad_edges.py
int main(int argc, char** argv) {
    const WgradKnobs def;
    if (argc > 1) {
        for (int i = 1; i < argc;) {
            if (strcmp(argv[i], "planes") == 0 && i + 6 <= argc) {
                const int mode = atoi(argv[i + 4]);
                if (mode < 0 || mode > 2) return 2;
                puts(line(planes(atol(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3])), mode, atoi(argv[i + 5]), def).c_str());
                i += 6;
            } else if (strcmp(argv[i], "conv") == 0 && i + 13 <= argc) {
                int a[12];
                for (int j = 0; j < 12; ++j) a[j] = atoi(argv[i + 1 + j]);
                const int KH = a[5], KW = a[6], stride = a[7], pad = a[8], mode = a[10];
                const int Hb = (a[1] - 1) * stride + KH - 2 * pad, Wb = (a[2] - 1) * stride + KW - 2 * pad;
                if (mode < 0 || mode > kMode16 || a[0] < 1 || Hb < 1 || Wb < 1 || a[3] < 1 || a[4] < 1 || KH < 1 || KW < 1 || stride < 1) return 2;
                puts(line(WgradShape{a[0], Hb, Wb, a[4], a[1], a[2], a[3], KH, KW, stride, pad, a[9] != 0, false}, mode, a[11], def).c_str());
                i += 13;
            } else {
                return 2;
            }
        }
        return 0;
    }
    for (const Case& c : full_grid()) puts(line(c.g, c.mode, c.nsplit, def).c_str());

    struct Setting {
        const char* name;
        WgradKnobs k;
    };
    std::vector<Setting> settings;
    const auto with = [&](const char* name, auto set) {
        WgradKnobs k;
        set(k);
        settings.push_back(Setting{name, k});
    };
    with("GIF_X3_WGRAD_THIN=0", [](WgradKnobs& k) { k.x3_wgrad_thin = 0; });
    with("GIF_X3_WGRAD_THIN=4", [](WgradKnobs& k) { k.x3_wgrad_thin = 4; });
    with("GIF_X3_WGRAD_SIMPLE=1", [](WgradKnobs& k) { k.x3_wgrad_simple = true; });
    with("GIF_H2_WGRAD_PLAIN_TAB=0", [](WgradKnobs& k) { k.h2_wgrad_plain_tab = false; });
    with("GIF_H2_WGRAD_V2=0", [](WgradKnobs& k) { k.h2_wgrad_v2 = false; });
    with("GIF_H2_WGRAD_TAPS=0", [](WgradKnobs& k) { k.h2_wgrad_taps = false; });
    with("GIF_WGRAD_BIG=0", [](WgradKnobs& k) { k.wgrad_big = false; });
    with("GIF_SMALL_WGRAD=0", [](WgradKnobs& k) { k.small_wgrad = false; });
    with("GIF_F16_WGRAD256=0", [](WgradKnobs& k) { k.f16_wgrad256 = false; });
    with("GIF_F16_HALO_WGRAD=0", [](WgradKnobs& k) { k.f16_halo_wgrad = false; });
    with("GIF_F16_HALO_WGRAD_TR=0", [](WgradKnobs& k) { k.f16_halo_wgrad_tr = false; });
    with("GIF_CONV_VARIANT=0", [](WgradKnobs& k) { k.conv_variant_set = true; k.conv_variant = 0; });
    with("GIF_CONV_VARIANT=1", [](WgradKnobs& k) { k.conv_variant_set = true; k.conv_variant = 1; });
    with("GIF_CONV_VARIANT=7", [](WgradKnobs& k) { k.conv_variant_set = true; k.conv_variant = 7; });
    const std::vector<Case> grid = knob_grid();
    for (const Setting& st : settings) {
        int differ = 0;
        for (const Case& c : grid) {
            const std::string a = line(c.g, c.mode, c.nsplit, def), b = line(c.g, c.mode, c.nsplit, st.k);
            if (a == b) continue;
            ++differ;
            printf("%s: %s\n", st.name, b.c_str());
        }
        printf("%s: %d of %zu cases differ from the default\n", st.name, differ, grid.size());
    }
    return 0;
}
