// Which kernel an upfirdn2d call gets, the grid of every pointwise and column-sum launch, the stages of the fixed-order reduction of
// partial sums and the scratch rows those stages write: host-only, plain C++17, no HIP and no common.h, so that a host compiler builds it
// alone (tests/host/ew_route_dump.cpp prints it over a grid of shapes; tests/test_ew_route.py compares that with a recorded table).
//
// elementwise.hip asks fir_route once per upfirdn2d call and launches what the returned value names; gif::reduce_partials launches the
// stages of reduce_plan; the column-sum, per-sample-product and texture-loss launchers and their size queries ask the block-count
// functions; common.h (FusedSums), shade.hip and flame.hip size the scratch of their reductions by the reduce_tmp_rows functions.  Nothing
// else in the library decides one of these numbers.
#pragma once
#include <stdlib.h>

namespace gif_ew {

constexpr int EW_THREADS = 256;         // lanes per workgroup of every kernel routed here
constexpr long EW_GRID_CAP = 256 * 16;  // ew_grid: beyond it the grid-stride loop takes another trip
constexpr int FIR_ROW_BLOCKS_CAP = 64;  // gridDim.x of the by-rows FIR kernels (gridDim.y = B * rows)
constexpr long FIR_GRID_Y_MAX = 65535;  // ... which need B * Ho within gridDim.y
constexpr long BLUR_ROWS_MIN_STRIPS = 256L * 256 * 2;  // blur: the 16-row sliding window from this many column strips (fills the chip)
constexpr int COLSUM_BLOCKS_CAP = 512, MUL_REDUCE_CHUNKS_CAP = 64, TEX_PAIR_BLOCKS_CAP = 1024;
// reduce_plan.  One long reduction (Y == 1, more than RED_LONG_MIN rows) first sums RED_GROUPS groups; per-sample sums (Y > 1) over at
// least RED_SAMPLE_MIN rows first sum RED_PER_SAMPLE groups per sample, while those fit RED_SAMPLE_TMP_CAP rows of scratch.
constexpr int RED_LONG_MIN = 512, RED_GROUPS = 64;
constexpr int RED_SAMPLE_MIN = 1024, RED_PER_SAMPLE = 16;
constexpr long RED_SAMPLE_TMP_CAP = EW_GRID_CAP;

inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// ---- grids -----------------------------------------------------------------------------------------------------------------------
// workgroups of a grid-stride kernel over n work items
inline int ew_grid(long n) {
    long b = cdivl(n, EW_THREADS);
    if (b > EW_GRID_CAP) b = EW_GRID_CAP;
    if (b < 1) b = 1;
    return (int)b;
}
// colsum_stage1 over nrows rows of C4 float4 columns (C4 <= 256): a workgroup is 256 / C4 row lanes of >= 16 rows each
inline int colsum_blocks(long nrows, int C4) {
    const long R = EW_THREADS / C4;
    long want = cdivl(nrows, R * 16);
    if (want > COLSUM_BLOCKS_CAP) want = COLSUM_BLOCKS_CAP;
    if (want < 1) want = 1;
    return (int)want;
}
inline long colsum_rows_per_block(long nrows, int nblk) { return cdivl(nrows, nblk); }
// chunks per sample of the per-sample products (mul_reduce, act_inv_mul_reduce) over HW pixels
inline int mul_reduce_chunks(long HW) {
    const int n = colsum_blocks(HW, 32);
    return n > MUL_REDUCE_CHUNKS_CAP ? MUL_REDUCE_CHUNKS_CAP : n;
}
// stage-1 workgroups (= partial sums) of the texture pair loss over n elements
inline int tex_pair_blocks(long n) {
    const long b = cdivl(n, EW_THREADS);
    return (int)(b > TEX_PAIR_BLOCKS_CAP ? TEX_PAIR_BLOCKS_CAP : (b < 1 ? 1 : b));
}

// ---- fixed-order reduction of partial rows: out[y] = sum_k partial[y][k], y < Y, k < nblk ---------------------------------------------
constexpr int RED_CHANNELS = 64;  // colsum_stage2: a workgroup sums 64 channels (gridDim.x), on 4 row lanes
inline int reduce_channel_blocks(int C) { return (int)cdivl(C, RED_CHANNELS); }
// One colsum_stage2 launch (gridDim.y = groups): group g sums rows [in_row + g * per, in_row + (g + 1) * per) of its source into row
// out_row + g of its destination.  The source is `partial`, or the scratch `tmp` when from_tmp; the destination `out`, or `tmp` when to_tmp.
struct ReduceStage {
    long in_row;
    int per, groups;
    long out_row;
    bool from_tmp, to_tmp;
};
struct ReducePlan {
    int nstages;  // 0: nothing to sum (Y or nblk <= 0)
    ReduceStage stage[3];
    long tmp_rows;  // rows of tmp the stages write
};
inline ReducePlan reduce_plan(int Y, int nblk) {
    ReducePlan p{};
    if (Y <= 0 || nblk <= 0) return p;
    if (Y == 1 && nblk > RED_LONG_MIN) {
        // two blocks of 64 channels alone would crawl through one long reduction.  Groups of `per` rows; stage 2 takes one row count per
        // launch, so the full groups and the short last one (the tail) are separate launches
        const int per = (int)cdivl(nblk, RED_GROUPS), full = nblk / per, tail = nblk - full * per;
        p.stage[p.nstages++] = {0, per, full, 0, false, true};
        if (tail) p.stage[p.nstages++] = {(long)full * per, tail, 1, full, false, true};
        p.tmp_rows = full + (tail ? 1 : 0);
        p.stage[p.nstages++] = {0, (int)p.tmp_rows, 1, 0, true, false};
    } else if (Y > 1 && nblk >= RED_SAMPLE_MIN && nblk % RED_PER_SAMPLE == 0 && (long)Y * RED_PER_SAMPLE <= RED_SAMPLE_TMP_CAP) {
        // per-sample sums over thousands of rows (the halo kernels' one row per 16 x 16 patch at 1024^2): Y blocks alone would crawl.  The
        // groups of one sample are consecutive rows of tmp
        p.stage[p.nstages++] = {0, nblk / RED_PER_SAMPLE, Y * RED_PER_SAMPLE, 0, false, true};
        p.tmp_rows = (long)Y * RED_PER_SAMPLE;
        p.stage[p.nstages++] = {0, RED_PER_SAMPLE, Y, 0, true, false};
    } else {
        p.stage[p.nstages++] = {0, nblk, Y, 0, false, false};
    }
    return p;
}

// What a caller of reduce_partials sizes tmp by: the most rows any plan writes ...
constexpr long reduce_tmp_rows_single() { return RED_GROUPS; }  // ... for Y == 1, whatever nblk (cdiv(nblk, cdiv(nblk, 64)) <= 64)
inline long reduce_tmp_rows(long Y) {                            // ... for up to Y samples (covers both staged plans)
    const long cap = RED_SAMPLE_TMP_CAP / RED_PER_SAMPLE;
    return reduce_tmp_rows_single() + RED_PER_SAMPLE * (Y < cap ? Y : cap);
}
// The red_ws workspace of an epilogue reduction over `rows` output rows, in rows of Co floats: `cap` partial rows of column sums, `cap`
// of dot products (conv tiles of >= 64 rows), then epilogue_tmp_rows of scratch.  The scratch holds a FIR launch's partial rows (one per
// workgroup, <= EW_GRID_CAP) with the rows of their Y == 1 plan behind them, or a convolution's plan of either kind.
constexpr long epilogue_tmp_rows() { return EW_GRID_CAP + reduce_tmp_rows_single(); }
static_assert(RED_SAMPLE_TMP_CAP <= epilogue_tmp_rows(), "the per-sample plan of a convolution's dot products must fit the scratch");
inline long epilogue_ws_cap(long rows) { return rows / 64 + 16; }
inline long epilogue_ws_rows(long rows) { return 2 * epilogue_ws_cap(rows) + epilogue_tmp_rows(); }

// ---- upfirdn2d ---------------------------------------------------------------------------------------------------------------------
// The GIF_* variable the FIR host code reads (gated by GIF_EXPERIMENTAL: common.h gif::knob).
struct FirKnobs {
    bool block = true;  // GIF_FIR_BLOCK: atoi == 0 -> the one-pixel-per-lane kernel for up = 2 as well (A/B; the block kernel gives the same bits)
};
// the raw environment string, NULL when the variable is not set
inline FirKnobs parse_fir_knobs(const char* fir_block) {
    FirKnobs k;
    if (fir_block) k.block = atoi(fir_block) != 0;
    return k;
}

enum FirKernel {
    FIR_BLUR_ROWS = 0,   // blur4x4_rows_kernel<T, 16, 4>: a lane slides a 16-row window down a strip of 4 columns x 4 channels
    FIR_BLUR_TILED = 1,  // blur4x4_tiled_kernel<T, 2, 4>
    FIR_UP2_BLOCK = 2,   // fir4x4_up2_block_kernel<T>: 2 x 2 output blocks, opening on the parity of the pad
    FIR_RESAMPLE = 3,    // fir4x4_resample_kernel<T, UP, DOWN>: one output pixel x 4 channels per lane, by rows
    FIR_GENERIC = 4,     // upfirdn2d_kernel<T>
};
struct FirShape {
    int B, C, Ho, Wo, up, down, padx0, pady0, KH, KW;
};
struct FirRoute {
    int kernel;    // FirKernel
    int UP, DOWN;  // FIR_RESAMPLE
    unsigned grid_x, grid_y;
    int threads;
    long items;        // work items: 4-channel groups of column strips / tiles / blocks / output pixels
    int partial_rows;  // fused column sum: the partial rows the launch writes (one per workgroup) ...
    ReducePlan plan;   // ... and their reduction (its scratch follows the partial rows)
};
inline unsigned fir_row_blocks(long row_items) {
    const long gx = cdivl(row_items, EW_THREADS);
    return (unsigned)(gx > FIR_ROW_BLOCKS_CAP ? FIR_ROW_BLOCKS_CAP : gx);
}
// want_colsum: only the blur kernels fuse one (the caller has refused it for every other form)
inline FirRoute fir_route(const FirShape& s, bool want_colsum, const FirKnobs& k) {
    FirRoute r{};
    r.threads = EW_THREADS;
    r.grid_y = 1;
    const long C4 = s.C / 4;
    const bool taps4 = s.KH == 4 && s.KW == 4;
    if (s.up == 1 && s.down == 1 && taps4) {
        const long strips = (long)s.B * cdivl(s.Ho, 16) * cdivl(s.Wo, 4) * C4;
        const bool rows = strips >= BLUR_ROWS_MIN_STRIPS;
        r.kernel = rows ? FIR_BLUR_ROWS : FIR_BLUR_TILED;
        r.items = rows ? strips : (long)s.B * cdivl(s.Ho, 2) * cdivl(s.Wo, 4) * C4;
        r.grid_x = (unsigned)ew_grid(r.items);
        if (want_colsum) {
            r.partial_rows = (int)r.grid_x;
            r.plan = reduce_plan(1, r.partial_rows);
        }
        return r;
    }
    if (taps4 && (long)s.B * s.Ho <= FIR_GRID_Y_MAX && ((s.up == 1 && s.down == 2) || (s.up == 2 && s.down == 1))) {
        if (k.block && s.up == 2) {
            const long nby = (s.Ho + 2 - (s.pady0 & 1)) / 2, nbx = (s.Wo + 2 - (s.padx0 & 1)) / 2;
            r.kernel = FIR_UP2_BLOCK;
            r.grid_x = fir_row_blocks(nbx * C4);
            r.grid_y = (unsigned)((long)s.B * nby);
            r.items = (long)s.B * nby * nbx * C4;
            return r;
        }
        r.kernel = FIR_RESAMPLE;
        r.UP = s.up;
        r.DOWN = s.down;
        r.grid_x = fir_row_blocks((long)s.Wo * C4);
        r.grid_y = (unsigned)((long)s.B * s.Ho);
        r.items = (long)s.B * s.Ho * s.Wo * C4;
        return r;
    }
    r.kernel = FIR_GENERIC;
    r.items = (long)s.B * s.Ho * s.Wo * C4;
    r.grid_x = (unsigned)ew_grid(r.items);
    return r;
}

}  // namespace gif_ew
