// Prints the FIR / reduction / pointwise-grid table of gif_amd/csrc/ew_route.h (host only: this program includes nothing else of the
// library).  Line kinds:
//   fir <name> | <shape> | cs<0|1> -> <kernel> grid<X>x<Y> thr<N> items<N> [; partial<N> ; <plan> ; ws_rows<N>]
//       an upfirdn2d call without / with the fused column sum; ws_rows = epilogue_ws_rows of the call's B * Ho * Wo output rows
//   plan Y<Y> nblk<N> -> <plan> ; bounds single<N> samples<N> epilogue<N>
//       <plan> = "<n> stages: <src>+<row> per<rows per group> x<groups> > <dst>+<row> | ... ; tmp<rows written>", p = partial, t = tmp,
//       o = out; the bounds are reduce_tmp_rows_single(), reduce_tmp_rows(Y) and epilogue_tmp_rows()
//   grid ew | colsum | mul_reduce | tex_pair | stage2 ...: the block counts
//   tmp_rows Y<Y> -> <N>, epilogue rows<N> -> cap<N> ws_rows<N>: the scratch sizes callers allocate by
//   GIF_FIR_BLOCK=<string>: how many of the fir lines the value changes, for "0" the changed lines themselves first
// The fir rows named like a row of tests/test_gpu_conv_routes.py FIR_ROWS are that row's shape.  tests/test_ew_route.py builds this with
// AddressSanitizer and UBSan (host code only), runs it and compares the output with tests/golden/ew_route_table.txt line by line.
#include <stdio.h>

#include <string>
#include <vector>

#include "ew_route.h"

using namespace gif_ew;

namespace {

std::string plan_text(const ReducePlan& p) {
    std::string s = std::to_string(p.nstages) + " stages:";
    for (int i = 0; i < p.nstages; ++i) {
        const ReduceStage& st = p.stage[i];
        char b[120];
        snprintf(b, sizeof b, "%s %c+%ld per%d x%d > %c+%ld", i ? " |" : "", st.from_tmp ? 't' : 'p', st.in_row, st.per, st.groups,
                 st.to_tmp ? 't' : 'o', st.out_row);
        s += b;
    }
    return s + " ; tmp" + std::to_string(p.tmp_rows);
}

struct FirCase {
    const char* name;
    int B, C, Ho, Wo, up, down, padx0, pady0, KH, KW;
};

std::string fir_line(const FirCase& c, bool cs, const FirKnobs& k) {
    const FirRoute r = fir_route(FirShape{c.B, c.C, c.Ho, c.Wo, c.up, c.down, c.padx0, c.pady0, c.KH, c.KW}, cs, k);
    char name[48];
    switch (r.kernel) {
    case FIR_BLUR_ROWS: snprintf(name, sizeof name, "blur_rows<16,4>"); break;
    case FIR_BLUR_TILED: snprintf(name, sizeof name, "blur_tiled<2,4>"); break;
    case FIR_UP2_BLOCK: snprintf(name, sizeof name, "up2_block"); break;
    case FIR_RESAMPLE: snprintf(name, sizeof name, "resample<%d,%d>", r.UP, r.DOWN); break;
    default: snprintf(name, sizeof name, "generic");
    }
    char b[400];
    snprintf(b, sizeof b, "fir %s | B%d C%d Ho%d Wo%d up%d down%d px%d py%d k%dx%d | cs%d -> %s grid%ux%u thr%d items%ld", c.name, c.B, c.C, c.Ho,
             c.Wo, c.up, c.down, c.padx0, c.pady0, c.KH, c.KW, (int)cs, name, r.grid_x, r.grid_y, r.threads, r.items);
    std::string s = b;
    if (r.partial_rows)
        s += " ; partial" + std::to_string(r.partial_rows) + " ; " + plan_text(r.plan) + " ; ws_rows" +
             std::to_string(epilogue_ws_rows((long)c.B * c.Ho * c.Wo));
    return s;
}

// name, B, C, Ho, Wo, up, down, pad0 of every row of FIR_ROWS (the input size does not enter the route)
std::vector<FirCase> test_rows() {
    return {
        {"up2_even", 3, 8, 74, 58, 2, 1, 2, 2, 4, 4},
        {"up2_odd", 3, 8, 73, 57, 2, 1, 1, 1, 4, 4},
        {"up2_even_bra", 3, 8, 75, 59, 2, 1, 2, 2, 4, 4},
        {"up2_odd_bra", 2, 16, 65, 67, 2, 1, 1, 1, 4, 4},
        {"up2_bho_65535", 3, 8, 21845, 6, 2, 1, 2, 2, 4, 4},
        {"up2_bho_65536", 4, 8, 16384, 6, 2, 1, 2, 2, 4, 4},
        {"up2_bho_65532_bra", 4, 8, 16383, 5, 2, 1, 1, 1, 4, 4},
        {"down2", 2, 8, 18, 20, 1, 2, 1, 1, 4, 4},
        {"down2_pad2", 3, 16, 17, 16, 1, 2, 2, 2, 4, 4},
        {"down2_generic", 2, 8, 32770, 2, 1, 2, 1, 1, 4, 4},
        {"blur_tiled_small", 2, 8, 37, 41, 1, 1, 1, 1, 4, 4},
        {"blur_tiled_tail", 1, 4, 260, 4096, 1, 1, 1, 1, 4, 4},
        {"blur_tiled_131008", 1, 4, 1024, 8188, 1, 1, 1, 1, 4, 4},
        {"blur_rows_131072", 1, 4, 1024, 8189, 1, 1, 1, 1, 4, 4},
        {"blur_rows_513", 1, 4, 1024, 8193, 1, 1, 1, 1, 4, 4},
        {"blur_rows_tail", 1, 4, 1040, 8189, 1, 1, 1, 1, 4, 4},
        {"blur_plain_c24", 2, 24, 21, 20, 1, 1, 2, 2, 4, 4},
    };
}

// Every FIR predicate of the header on both sides of its threshold.
std::vector<FirCase> edge_grid() {
    return {
        // blur: 131071 | 131072 column strips (B * cdiv(Ho, 16) * cdiv(Wo, 4) * C / 4), in one row band and spread over all four factors
        {"strips_131071", 1, 4, 16, 524284, 1, 1, 1, 1, 4, 4},
        {"strips_131072", 1, 4, 16, 524288, 1, 1, 1, 1, 4, 4},
        {"strips_131040", 2, 16, 33, 21837, 1, 1, 2, 2, 4, 4},  // 2 * 3 * 5460 * 4
        {"strips_131088", 2, 16, 33, 21845, 1, 1, 2, 2, 4, 4},  // 2 * 3 * 5462 * 4
        // not the 4 x 4 blur: other taps, or a resample factor, go to the by-rows kernels or the generic one
        {"blur_3x3", 2, 8, 37, 41, 1, 1, 1, 1, 3, 3},
        {"blur_4x3", 2, 8, 37, 41, 1, 1, 1, 1, 4, 3},
        {"up2_3x3", 2, 8, 37, 41, 2, 1, 1, 1, 3, 3},
        {"up4", 2, 8, 37, 41, 4, 1, 1, 1, 4, 4},
        {"up2_down2", 2, 8, 37, 41, 2, 2, 1, 1, 4, 4},
        {"down4", 2, 8, 37, 41, 1, 4, 1, 1, 4, 4},
        // B * Ho at 65535 | 65536, up and down
        {"up2_edge_65535", 1, 4, 65535, 3, 2, 1, 2, 2, 4, 4},
        {"up2_edge_65536", 1, 4, 65536, 3, 2, 1, 2, 2, 4, 4},
        {"down2_edge_65535", 5, 4, 13107, 3, 1, 2, 1, 1, 4, 4},
        {"down2_edge_65536", 2, 4, 32768, 3, 1, 2, 1, 1, 4, 4},
        // the four pad parities of the block kernel on even and odd output sizes
        {"up2_pad_ee_even", 2, 8, 10, 12, 2, 1, 2, 2, 4, 4},
        {"up2_pad_oo_even", 2, 8, 10, 12, 2, 1, 1, 1, 4, 4},
        {"up2_pad_eo_even", 2, 8, 10, 12, 2, 1, 2, 1, 4, 4},
        {"up2_pad_oe_even", 2, 8, 10, 12, 2, 1, 1, 2, 4, 4},
        {"up2_pad_ee_odd", 2, 8, 11, 13, 2, 1, 2, 2, 4, 4},
        {"up2_pad_oo_odd", 2, 8, 11, 13, 2, 1, 1, 1, 4, 4},
        {"up2_pad_eo_odd", 2, 8, 11, 13, 2, 1, 2, 1, 4, 4},
        {"up2_pad_oe_odd", 2, 8, 11, 13, 2, 1, 1, 2, 4, 4},
        // the 64-block cap of a row: 63 | 64 | 64 (last one not full) | 65 wanted; resample (Wo * C / 4 items), block (nbx * C / 4)
        {"down2_row_16128", 1, 4, 4, 16128, 1, 2, 1, 1, 4, 4},
        {"down2_row_16129", 1, 4, 4, 16129, 1, 2, 1, 1, 4, 4},
        {"down2_row_16384", 1, 4, 4, 16384, 1, 2, 1, 1, 4, 4},
        {"down2_row_16385", 1, 4, 4, 16385, 1, 2, 1, 1, 4, 4},
        {"up2_row_16384", 1, 8, 4, 16382, 2, 1, 2, 2, 4, 4},  // nbx 8192, two float4 each
        {"up2_row_16386", 1, 8, 4, 16384, 2, 1, 2, 2, 4, 4},  // nbx 8193
        // ew_grid's cap under the generic kernel (4095 | 4096 | 4097 wanted) and under the rows blur (4095 | 4096 | 4097 wanted, with the column sum)
        {"generic_grid_4095", 1, 4, 4095, 256, 4, 1, 1, 1, 4, 4},
        {"generic_grid_4096", 1, 4, 4096, 256, 4, 1, 1, 1, 4, 4},
        {"generic_grid_4097", 1, 4, 4096, 257, 4, 1, 1, 1, 4, 4},
        {"generic_grid_1", 1, 4, 1, 1, 4, 1, 1, 1, 4, 4},
        {"blur_grid_4095", 1, 4, 2, 4193280, 1, 1, 1, 1, 4, 4},
        {"blur_grid_4096", 1, 4, 2, 4194304, 1, 1, 1, 1, 4, 4},
        {"blur_grid_4097", 1, 4, 2, 4194308, 1, 1, 1, 1, 4, 4},
        // the benchmark's blur and upsample at 1024^2, batch 8
        {"bench_blur_1024", 8, 32, 1024, 1024, 1, 1, 2, 2, 4, 4},
        {"bench_up2_1024", 8, 32, 1024, 1024, 2, 1, 2, 2, 4, 4},
    };
}

std::vector<std::string> fir_lines(const std::vector<FirCase>& grid, const FirKnobs& k) {
    std::vector<std::string> out;
    for (const FirCase& c : grid)
        for (int cs = 0; cs < 2; ++cs) out.push_back(fir_line(c, cs != 0, k));
    return out;
}

void plan_line(int Y, int nblk) {
    printf("plan Y%d nblk%d -> %s ; bounds single%ld samples%ld epilogue%ld\n", Y, nblk, plan_text(reduce_plan(Y, nblk)).c_str(),
           reduce_tmp_rows_single(), reduce_tmp_rows(Y), epilogue_tmp_rows());
}

}  // namespace

int main() {
    const FirKnobs def;
    printf("K threads%d grid_cap%ld row_blocks%d grid_y%ld rows_min%ld colsum%d chunks%d tex%d long_min%d groups%d sample_min%d per_sample%d sample_cap%ld\n",
           EW_THREADS, EW_GRID_CAP, FIR_ROW_BLOCKS_CAP, FIR_GRID_Y_MAX, BLUR_ROWS_MIN_STRIPS, COLSUM_BLOCKS_CAP, MUL_REDUCE_CHUNKS_CAP,
           TEX_PAIR_BLOCKS_CAP, RED_LONG_MIN, RED_GROUPS, RED_SAMPLE_MIN, RED_PER_SAMPLE, RED_SAMPLE_TMP_CAP);
    std::vector<FirCase> all = test_rows();
    for (const std::string& l : fir_lines(all, def)) puts(l.c_str());
    const std::vector<FirCase> edges = edge_grid();
    for (const std::string& l : fir_lines(edges, def)) puts(l.c_str());

    // reduce_plan: nothing to sum; one long reduction at 512 | 513, with and without a tail, at ew_grid's cap and past every grid; per-sample
    // sums at 1024 rows, multiples of 16 and not, at 256 | 257 samples
    for (int nblk : {0, 1, 2, 511, 512, 513, 520, 576, 4095, 4096, 4097, 65536, 1000000}) plan_line(1, nblk);
    plan_line(0, 8);
    for (int Y : {2, 3, 8, 32, 255, 256, 257, 300})
        for (int nblk : {1, 513, 1008, 1023, 1024, 1025, 1032, 1040, 4096, 65536}) plan_line(Y, nblk);

    // block counts: under the floor, at it, at every cap and one past it
    for (long n : {0L, 1L, 256L, 257L, 4095L * 256, 4095L * 256 + 1, 4096L * 256, 4096L * 256 + 1, 1L << 33}) printf("grid ew n%ld -> %d\n", n, ew_grid(n));
    struct CS {
        long nrows;
        int C4;
    };
    for (const CS& c : {CS{0, 16}, CS{1, 16}, CS{256, 16}, CS{257, 16}, CS{511 * 256, 16}, CS{512 * 256, 16}, CS{512 * 256 + 1, 16}, CS{513 * 256, 16},
                        CS{512 * 16, 256}, CS{512 * 16 + 1, 256}, CS{512 * 4096, 1}, CS{512 * 4096 + 1, 1}, CS{33 * 85 * 16, 3}, CS{33 * 85 * 16 + 1, 3},
                        CS{1L << 33, 8}}) {
        const int nblk = colsum_blocks(c.nrows, c.C4);
        printf("grid colsum nrows%ld C%d -> blocks%d rpb%ld\n", c.nrows, c.C4 * 4, nblk, colsum_rows_per_block(c.nrows, nblk));
    }
    for (long HW : {1L, 128L, 129L, 63L * 128, 63L * 128 + 1, 8192L, 8193L, 1L << 20}) {
        const int n = mul_reduce_chunks(HW);
        printf("grid mul_reduce HW%ld -> chunks%d rpb%ld\n", HW, n, colsum_rows_per_block(HW, n));
    }
    for (long n : {0L, 1L, 256L, 257L, 1023L * 256 + 1, 1024L * 256, 1024L * 256 + 1, 1L << 33}) printf("grid tex_pair n%ld -> %d\n", n, tex_pair_blocks(n));

    for (int C : {1, 27, 63, 64, 65, 1024}) printf("grid stage2 C%d -> %d\n", C, reduce_channel_blocks(C));

    // what callers allocate
    for (long Y : {1L, 2L, 3L, 8L, 32L, 255L, 256L, 257L, 300L, 100000L}) printf("tmp_rows Y%ld -> %ld\n", Y, reduce_tmp_rows(Y));
    for (long rows : {1L, 63L, 64L, 1024L, 8L * 1024 * 1024, 1L << 33}) printf("epilogue rows%ld -> cap%ld ws_rows%ld\n", rows, epilogue_ws_cap(rows), epilogue_ws_rows(rows));

    // GIF_FIR_BLOCK: the raw strings of the environment, through the header's parser
    all.insert(all.end(), edges.begin(), edges.end());
    const std::vector<std::string> base = fir_lines(all, def);
    for (const char* v : {"0", "1", "2", "-1", "00", "", "off", "0x1"}) {
        const FirKnobs k = parse_fir_knobs(v);
        const std::vector<std::string> with = fir_lines(all, k);
        int differ = 0;
        for (size_t i = 0; i < with.size(); ++i) {
            if (with[i] == base[i]) continue;
            ++differ;
            if (v[0] == '0' && !v[1]) printf("GIF_FIR_BLOCK=%s: %s\n", v, with[i].c_str());  // (every other value: the count alone)
        }
        printf("GIF_FIR_BLOCK=%s: block%d: %d of %zu cases differ from the default\n", v, (int)k.block, differ, with.size());
    }
    const FirKnobs unset = parse_fir_knobs(nullptr);
    printf("GIF_FIR_BLOCK unset: block%d\n", (int)unset.block);
    return 0;
}
