// Prints the Winograd forward / data-gradient route table of gif_amd/csrc/wino_route.h (host only: this program includes nothing else of
// the library).  One line per case:
//   geometry | mode | g(uarded) / u(nguarded) -> input transform ; GEMM launch [+ twin] ; padded dims, sizes, partial sums, family
// or "-> error <which 32-bit limit>" with the dims alone; "gy ..." lines for the gradient transform of the weight gradient.  First over
// a fixed grid with the default knobs, then once per knob value (the raw string, through the header's parser) over a smaller grid, where
// only the cases are printed whose line differs from the default one (and how many of how many did).  With arguments: the lines of the
// calls asked for (see main).  tests/test_wino_route.py builds this with AddressSanitizer and UBSan (host code only), runs it and compares
// the output with tests/golden/wino_route_table.txt line by line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "wino_route.h"

using namespace gif_wino;

namespace {

const char* const kModeName[] = {"native", "bf16x3", "f16x2"};

std::string xform_text(const XformRoute& t) {
    char b[160], name[32];
    if (t.kernel == XFORM_ROWS) snprintf(name, sizeof name, "rows<%d>", t.rows);
    else snprintf(name, sizeof name, "%s", t.kernel == XFORM_GY ? "gy" : "tile");
    const long per_trip = (long)t.blocks * XFORM_THREADS;
    snprintf(b, sizeof b, "%s lanes%ld blocks%u thr%d trips%ld fam%d", name, t.lanes, t.blocks, XFORM_THREADS, (t.lanes + per_trip - 1) / per_trip,
             t.family);
    return b;
}

std::string launch_text(const WinoLaunch& l) {
    char b[200], name[32];
    if (l.kernel == GEMM_MFMA) snprintf(name, sizeof name, "mfma<%d>", l.WN);
    else if (l.kernel == GEMM_X3) snprintf(name, sizeof name, "x3<%d,%d>", l.BM, l.BN);
    else snprintf(name, sizeof name, "h2<%d,%d,%d>", l.BM, l.BN, l.NST);
    snprintf(b, sizeof b, "%s bm%d bn%d tm%d tn%d grid%u thr%d lds%zu", name, l.bm, l.bn, l.tiles_m, l.tiles_n, l.grid, l.threads, l.lds);
    return b;
}

struct Case {
    int B, H, W, C, Co;
};

std::string line(const Case& c, int mode, bool guarded, const WinoKnobs& k) {
    const WinoRoute r = wino_route(c.B, c.H, c.W, c.C, c.Co, mode, guarded, k);
    char head[160], dims[200];
    snprintf(head, sizeof head, "B%d H%d W%d C%d Co%d | %s | %s -> ", c.B, c.H, c.W, c.C, c.Co, kModeName[mode], guarded ? "g" : "u");
    snprintf(dims, sizeof dims, " ; ntiles%ld pad%ld RP%d CP%d vfloats%ld u2bytes%ld", r.ntiles, r.ntiles_pad, r.RP, r.CP,
             v_floats(c.B, c.H, c.W, c.C), mode == MODE_NATIVE ? 0L : h2_weight_bytes(r.RP, r.CP));
    if (r.error) {
        const char* const which[] = {"", "V", "y", "x", "U"};
        return std::string(head) + "error " + which[r.error] + dims;
    }
    char tail[80];
    snprintf(tail, sizeof tail, " sums%dx%d fam%d", r.sum_rows, r.sum_tile, r.family);
    std::string s = head + xform_text(r.xform) + " ; " + launch_text(r.primary);
    if (r.has_twin) s += " + twin " + launch_text(r.twin);
    return s + dims + tail;
}

std::string gy_line(int B, int H, int W, int C) {
    const XformRoute t = gy_transform_route(B, H, W, C);
    char b[200];
    snprintf(b, sizeof b, "gy B%d H%d W%d C%d -> %s ; ntiles%ld pad%ld CP%d", B, H, W, C, xform_text(t).c_str(), t.ntiles, t.ntiles_pad, t.CP);
    return b;
}

// Every predicate of the header on both sides of its threshold.
std::vector<Case> full_grid() {
    std::vector<Case> v;
    // Co % 128 at 512 row tiles: the wide native GEMM, the row padding of U in both forms
    for (int Co : {127, 128, 132, 256}) v.push_back({1, 512, 512, 32, Co});
    // tiles_m * (RP / 128) at 510 | 512 | 514 (Co 128) and 508 | 512 | 516 (Co 256): tiles_m is even
    for (int tm : {510, 512, 514}) v.push_back({1, 2, 2 * tm * 128, 32, 128});
    for (int tm : {254, 256, 258}) v.push_back({1, 2, 2 * tm * 128, 32, 256});
    // ntiles at 255 | 256 | 257: the row padding of V
    for (int nt : {255, 256, 257}) v.push_back({1, 2, 2 * nt, 32, 64});
    // C at 28 | 32 | 36: CP
    for (int C : {28, 32, 36}) v.push_back({1, 2, 512, C, 64});
    // TH at 7 | 8 | 9 and 15 | 16 | 17: tile rows per lane of the input transform
    for (int TH : {7, 8, 9, 15, 16, 17}) v.push_back({2, 2 * TH, 6, 32, 64});
    // lanes of the input transform under the grid cap, at it, one tile over it
    v.push_back({16, 2, 510, 2048, 4});
    v.push_back({16, 2, 512, 2048, 4});
    v.push_back({17, 2, 482, 2048, 4});
    // the 32-bit limits, just under and just over: V (ntiles_pad * CP), y (B H W Co), x (B H W C), U (3 RP CP, the split forms)
    v.push_back({1, 16382, 16384, 4, 4});
    v.push_back({1, 16384, 16384, 4, 4});
    v.push_back({1, 8192, 16384, 4, 12});
    v.push_back({1, 8192, 16384, 4, 16});
    v.push_back({1, 8192, 16384, 12, 4});
    v.push_back({1, 8192, 16384, 16, 4});
    v.push_back({1, 2, 2, 26624, 26880});
    v.push_back({1, 2, 2, 26880, 26880});
    // the benchmark's three big layers (batch 32)
    v.push_back({32, 256, 256, 128, 128});
    v.push_back({32, 128, 128, 256, 256});
    v.push_back({32, 64, 64, 512, 512});
    return v;
}

std::vector<Case> knob_grid() {
    return {{2, 14, 6, 32, 64}, {2, 34, 6, 36, 64}, {17, 2, 482, 2048, 4}, {1, 512, 512, 32, 128}, {1, 510, 512, 32, 128}, {1, 512, 512, 32, 132},
            {1, 2, 172, 32, 64}, {1, 2, 514, 32, 256}, {32, 256, 256, 128, 128}};
}

std::vector<std::string> lines_of(const std::vector<Case>& grid, const WinoKnobs& k) {
    std::vector<std::string> out;
    for (const Case& c : grid) {
        for (int mode = 0; mode < 3; ++mode) out.push_back(line(c, mode, false, k));
        out.push_back(line(c, MODE_F16X2, true, k));  // (only an f16x2 call can be guarded)
    }
    return out;
}

}  // namespace

// Argument groups, any number of them, one line per group instead of the table:
//   fwd <B> <H> <W> <C> <Co> <mode> <guarded>: that forward / data-gradient call with the default knobs (mode 0 native, 1 bf16x3, 2 f16x2)
//     — tests/test_cpu_wiring.py asks for the rows of tests/test_gpu_winograd_edges.py this way
//   K: the header's constants
int main(int argc, char** argv) {
    const WinoKnobs def;
    if (argc > 1) {
        for (int i = 1; i < argc;) {
            if (strcmp(argv[i], "K") == 0) {
                printf("WBM=%d WBN=%d WBK=%d WNSTAGE=%d WPAD=%d TYB=%d CAP_WG=%ld WIDE_MIN=%ld\n", WBM, WBN, WBK, WNSTAGE, WPAD, def.xform_rows,
                       XFORM_CAP_WG, WIDE_MIN_WG);
                i += 1;
            } else if (strcmp(argv[i], "fwd") == 0 && i + 8 <= argc) {
                int a[7];
                for (int j = 0; j < 7; ++j) a[j] = atoi(argv[i + 1 + j]);
                if (a[0] < 1 || a[1] < 2 || a[2] < 2 || a[3] < 1 || a[4] < 1 || a[5] < 0 || a[5] > 2) return 2;
                puts(line(Case{a[0], a[1], a[2], a[3], a[4]}, a[5], a[6] != 0, def).c_str());
                i += 8;
            } else {
                return 2;
            }
        }
        return 0;
    }
    for (const std::string& l : lines_of(full_grid(), def)) puts(l.c_str());
    puts(gy_line(2, 14, 6, 28).c_str());
    puts(gy_line(2, 14, 6, 36).c_str());
    puts(gy_line(1, 2, 514, 32).c_str());
    puts(gy_line(16, 2, 512, 2048).c_str());
    puts(gy_line(17, 2, 482, 2048).c_str());

    // per knob: the raw strings of the environment, through the header's parser (NULL: not set)
    struct Setting {
        const char* name;
        const char *xform, *wn, *x3_tile, *h2_stages;
    };
    const Setting settings[] = {
        {"GIF_WINO_XFORM=rows4", "rows4", nullptr, nullptr, nullptr},   {"GIF_WINO_XFORM=rows8", "rows8", nullptr, nullptr, nullptr},
        {"GIF_WINO_XFORM=rows16", "rows16", nullptr, nullptr, nullptr}, {"GIF_WINO_XFORM=rows7", "rows7", nullptr, nullptr, nullptr},
        {"GIF_WINO_XFORM=rows", "rows", nullptr, nullptr, nullptr},     {"GIF_WINO_XFORM=tile", "tile", nullptr, nullptr, nullptr},
        {"GIF_WINO_WN=2", nullptr, "2", nullptr, nullptr},              {"GIF_WINO_WN=4", nullptr, "4", nullptr, nullptr},
        {"GIF_WINO_WN=3", nullptr, "3", nullptr, nullptr},              {"GIF_WINO_X3_TILE=256", nullptr, nullptr, "256", nullptr},
        {"GIF_WINO_X3_TILE=128", nullptr, nullptr, "128", nullptr},     {"GIF_WINO_H2_STAGES=3", nullptr, nullptr, nullptr, "3"},
        {"GIF_WINO_H2_STAGES=4", nullptr, nullptr, nullptr, "4"},       {"GIF_WINO_H2_STAGES=5", nullptr, nullptr, nullptr, "5"},
        {"GIF_WINO_H2_STAGES=6", nullptr, nullptr, nullptr, "6"},
    };
    const std::vector<Case> grid = knob_grid();
    const std::vector<std::string> base = lines_of(grid, def);
    for (const Setting& st : settings) {
        const WinoKnobs k = parse_knobs(st.xform, st.wn, st.x3_tile, st.h2_stages);
        const std::vector<std::string> with = lines_of(grid, k);
        int differ = 0;
        for (size_t i = 0; i < with.size(); ++i) {
            if (with[i] == base[i]) continue;
            ++differ;
            printf("%s: %s\n", st.name, with[i].c_str());
        }
        printf("%s: rows%d wn%d tile256=%d stages%d: %d of %zu cases differ from the default\n", st.name, k.xform_rows, k.wn, (int)k.x3_tile256,
               k.h2_stages, differ, with.size());
    }
    return 0;
}
