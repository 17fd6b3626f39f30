// fp32 MFMA weight-gradient kernel for gfx950 (NHWC) + unpacking of the gradient (weight PACKING: weight_pack.hip, f16x2 form below).
//
// Replaces autograd's wgrad of the F.conv2d / F.conv_transpose2d calls in
// stylegan2_common_layers.py:176, :330, :339, :345, :405-414.
//   dW[t][o][i] = sum_{b,oy,ox} small[b,oy,ox,o]*ss[b,o] * big[b, oy*s+ky-pad, ox*s+kx-pad, i]*bs[b,i]
// GEMM view per tap t: M = Cs (o), N = Cb (i), K = B*Hs*Ws pixels.  Both operands are channel-contiguous in
// HBM, i.e. K is the SLOW axis: tiles are staged as [pixel][channel] and read back with lanes along the channel
// axis (ds_read_b32, 128 contiguous bytes per half wave => conflict free), which is exactly the A[i][k] / B[k][j]
// operand shape of v_mfma_f32_32x32x2_f32 with k = pixel.
// The pixel axis is split over gridDim.z; every split writes its own partial tile (deterministic: no atomics),
// and gif_unpack_wgrad_f32 reduces the splits while scattering into the canonical [O,I,KH,KW]-style tensor.
// The per-sample scales implement the wgrad of the modulated convolution (x*s and dy*d) on the fly.
#include <stdlib.h>

#include "conv_common.h"
#include "wgrad_route.h"  // which kernel a call gets: every tile / stage / twin / family decision of the host code below
#include "wino_route.h"   // padded dims of the Winograd transforms' outputs

namespace {

namespace route = gif_wgrad;

using gif::f32x16, gif::f32x4, gif::xcd_remap;

struct WgradParams {
    const void* sm;   // small side [B,Hs,Ws,Cs]   (fp32, or f16 for the T = f16 instantiation)
    const void* bg;   // big side   [B,Hb,Wb,Cb]
    float* ws;        // [nsplit][T][RP][CP]
    const float* ss;  // [B,Cs] or null
    const float* bs;  // [B,Cb] or null
    int B, Hs, Ws, Cs, Hb, Wb, Cb;
    int KW, stride, pad, T;
    int RP, CP;
    long Ntot;   // B*Hs*Ws
    long chunk;  // pixels per split (multiple of BKP)
    int tiles_q, tiles_pq;
    int stab_nb;  // LDS scale table (scaled LDS-DMA path): samples a pixel chunk can touch
    const void* zero;   // 16 zero bytes in HBM (source of out-of-range LDS-DMA lanes), passed as an argument
    // "planes" mode (Winograd wgrad): tap t has no spatial shift but its own operand planes sm + t*sm_plane, bg + t*bg_plane
    long sm_plane, bg_plane;
    // f16x2 (common.h "h2"): gate word the kernel raises when a K group leaves the precision window; bf16x3 launch WITH a gate:
    // the guarded fallback, runs iff *gate == gate_gen
    unsigned* gate;
    unsigned gate_gen;
    unsigned* h2_stats;
    // conv_wgrad_h2v2<.., TAPS>: the 128 tile columns hold `tpt` taps x Cb channels (thin big side), `tgroups` column tiles cover the T taps
    int tpt, tgroups;
};

// GLDS = true (no per-sample scales): both operand tiles go global -> LDS directly (global_load_lds_dwordx4, lane-linear
// destination == the [pixel][channel] tile layout), no staging registers / ds_write; invalid lanes read a zero page.
// TAB = true (GLDS with per-sample scales, needs Hs*Ws % BKP == 0 so that a stage never straddles two samples): the
// scale vectors ss[b, r0:r0+BP) / bs[b, c0:c0+BQ) of the samples this chunk touches sit in an LDS table and are
// multiplied into the operand fragments (the DMA cannot scale data in flight).
// T = f16 (GLDS only): the same [pixel][channel] tiles in halfs (16-byte DMA chunk = 8 channels); v_mfma_f32_32x32x16_f16 wants
// 8 consecutive K (= pixels) of ONE channel per lane, i.e. a transposed operand, which is gathered with eight 16-bit LDS reads
// per fragment (lane = channel: the 32 lanes of a half wave read 64 contiguous bytes of one pixel row, conflict free).
// Accumulators and the partial-sum workspace stay fp32.
// X3 (T = float, GLDS): fp32 tiles, bf16 matrix cores ("bf16x3", common.h split_pair): like the f16 path every lane gathers 8
// consecutive pixels of its channel per operand tile (eight ds_read_b32, conflict free), then splits the 8 floats into the
// three bf16x8 terms; six v_mfma_f32_32x32x16_bf16 per tile pair and 16 pixels.  Both operands are activations, so neither can
// be pre-split; the split (36 VALU per fragment) overlaps with the MFMAs of the other resident waves.
// X3 = 2 ("f16x2", common.h): the same tiles, v_mfma_f32_32x32x16_f16 on two f16 terms per operand under per-CHANNEL power-of-two
// scales (a row of either operand is a channel, K runs over pixels): both operands carry a running exponent per lane, three products.
template <typename T, int BP, int BQ, int WAVES_P, int WAVES_Q, bool GLDS, int BKP, bool TAB = false, int X3 = 0>
// (f16x2, 4 waves: "at least 2 workgroups per CU" caps the budget at 256 registers, which makes hipcc keep the accumulators in
// architectural VGPRs — the rare rescale path multiplies them with VALU instructions; from AGPRs that costs 64 temporaries and the
// kernel would no longer fit two waves per SIMD)
__global__ void __launch_bounds__(64 * WAVES_P * WAVES_Q, (X3 == 2 && WAVES_P * WAVES_Q == 4) ? 2 : 1) conv_wgrad_mfma(const WgradParams p) {
    constexpr bool F16 = sizeof(T) == 2;
    if constexpr (X3 == 1) {
        if (p.gate) {  // guarded fallback of an f16x2 launch: nothing to do unless that launch raised the gate
            if (*p.gate < p.gate_gen) return;
            if (blockIdx.x == 0 && threadIdx.x == 0 && p.h2_stats) atomicAdd(p.h2_stats, 1u);
        }
    }
    static_assert(!X3 || (!F16 && GLDS && BKP % 16 == 0), "bf16x3: fp32 tiles through the LDS-DMA path, 16-pixel K steps");
    static_assert(X3 != 2 || BKP == 32, "f16x2: the software-pipelined 32-pixel stages only");
    constexpr int EPC = 16 / sizeof(T);  // elements per 16-byte chunk
    constexpr int THREADS = 64 * WAVES_P * WAVES_Q;
    constexpr int WPt = BP / WAVES_P, WQt = BQ / WAVES_Q;
    constexpr int MT = WPt / 32, NT = WQt / 32;
    constexpr int P_ROWS = THREADS / (BP / EPC), Q_ROWS = THREADS / (BQ / EPC);  // pixel rows per pass
    constexpr int P_IT = BKP / P_ROWS, Q_IT = BKP / Q_ROWS;
    static_assert(BKP % P_ROWS == 0 && BKP % Q_ROWS == 0 && P_IT >= 1 && Q_IT >= 1, "tile/thread mapping");
    static_assert(!F16 || (GLDS && BKP % 16 == 0), "f16: LDS-DMA staging, 16-pixel MFMA K steps");

    // ONE LDS object (two separate __shared__ arrays make hipcc drain the LDS-DMA with vmcnt(0) before every ds_read)
    extern __shared__ __attribute__((aligned(16))) float wg_smem[];
    typedef T PTile[BKP][BP];
    typedef T QTile[BKP][BQ];
    PTile* Ps = reinterpret_cast<PTile*>(wg_smem);                                        // [2][BKP][BP]
    QTile* Qs = reinterpret_cast<QTile*>(reinterpret_cast<T*>(wg_smem) + 2 * BKP * BP);   // [2][BKP][BQ]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wp0 = (wave / WAVES_Q) * WPt, wq0 = (wave % WAVES_Q) * WQt;
    // logical id = ((split * T) + tap) * tiles + tile: the 9 taps (and channel tiles) of one pixel chunk read the SAME
    // activations, so they are made consecutive and therefore co-resident on one XCD's L2.
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = lid % p.tiles_pq;
    const int t = (lid / p.tiles_pq) % p.T;
    const int split = lid / (p.tiles_pq * p.T);
    const int tq = tile % p.tiles_q, tp = tile / p.tiles_q;
    const int r0 = tp * BP, c0 = tq * BQ;
    const bool planes = p.sm_plane != 0;
    const int ky = planes ? 0 : t / p.KW, kx = planes ? 0 : t - ky * p.KW;
    const T* const smb = static_cast<const T*>(p.sm) + (size_t)t * p.sm_plane;
    const T* const bgb = static_cast<const T*>(p.bg) + (size_t)t * p.bg_plane;
    const T* const pzero = static_cast<const T*>(p.zero);
    const int n_begin = (int)((long)split * p.chunk);
    int n_end = n_begin + (int)p.chunk;
    if (n_end > (int)p.Ntot) n_end = (int)p.Ntot;
    const unsigned HWs = (unsigned)(p.Hs * p.Ws);

    const int p_row = tid / (BP / EPC), p_ch = r0 + (tid % (BP / EPC)) * EPC;
    const int q_row = tid / (BQ / EPC), q_ch = c0 + (tid % (BQ / EPC)) * EPC;
    const bool p_ch_ok = p_ch < p.Cs, q_ch_ok = q_ch < p.Cb;
    const bool has_ss = !TAB && p.ss != nullptr, has_bs = !TAB && p.bs != nullptr;
    float* Stab = reinterpret_cast<float*>(reinterpret_cast<T*>(wg_smem) + 2 * BKP * (BP + BQ));  // [stab_nb][BP + BQ] fp32
    int tab_row = 0, tab_rem = 0;                 // table row / pixel offset inside the sample of the stage being computed
    if (TAB) {
        const int b_first = n_begin / (int)HWs;
        for (int e = tid; e < p.stab_nb * (BP + BQ); e += THREADS) {
            int bl = e / (BP + BQ), c = e - bl * (BP + BQ);
            int b = b_first + bl;
            float v = 0.f;
            if (b < p.B) {
                if (c < BP) v = (r0 + c < p.Cs) ? (p.ss ? p.ss[(size_t)b * p.Cs + r0 + c] : 1.f) : 0.f;
                else v = (c0 + c - BP < p.Cb) ? (p.bs ? p.bs[(size_t)b * p.Cb + c0 + c - BP] : 1.f) : 0.f;
            }
            Stab[e] = v;
        }
        tab_rem = n_begin - b_first * (int)HWs;
        __syncthreads();
    }

    float4 p_reg[P_IT], ps_reg[P_IT], q_reg[Q_IT], qs_reg[Q_IT];
    unsigned p_mask = 0, q_mask = 0;

    // Per-thread pixel cursors, advanced by BKP pixels per stage with carry propagation (no divisions in the loop).
    // P side: linear pixel n (address n*Cs) and its sample index (for the per-sample scale).
    // Q side: (b, oy, ox) of the small-grid pixel; the big-grid pixel is (oy*stride+ky-pad, ox*stride+kx-pad).
    int p_n[P_IT], p_b[P_IT], p_rem[P_IT];
    int q_n[Q_IT], q_b[Q_IT], q_oy[Q_IT], q_ox[Q_IT];
#pragma unroll
    for (int it = 0; it < P_IT; ++it) {
        int n = n_begin + p_row + it * P_ROWS;
        p_n[it] = n;
        p_b[it] = (int)((unsigned)n / HWs);
        p_rem[it] = n - p_b[it] * (int)HWs;
    }
#pragma unroll
    for (int it = 0; it < Q_IT; ++it) {
        int n = n_begin + q_row + it * Q_ROWS;
        q_n[it] = n;
        unsigned b = (unsigned)n / HWs;
        unsigned r = (unsigned)n - b * HWs;
        unsigned oy = r / (unsigned)p.Ws;
        q_b[it] = (int)b; q_oy[it] = (int)oy; q_ox[it] = (int)(r - oy * (unsigned)p.Ws);
    }

    // Branch-free loads (invalid lanes read a dummy address and are zeroed at the LDS store); per-sample scales are
    // multiplied in at the LDS store, after the MFMAs of the current stage.
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto load_global = [&](int buf) __attribute__((always_inline)) {
        p_mask = 0;
        q_mask = 0;
#pragma unroll
        for (int it = 0; it < P_IT; ++it) {
            bool ok = p_ch_ok && p_n[it] < n_end;
            if (GLDS) {
                // thread tid lands at byte offset 16*tid of pass `it` (== Ps[buf][p_row + it*P_ROWS][EPC*(tid % (BP/EPC))])
                const T* g = ok ? smb + (p_n[it] * p.Cs + p_ch) : pzero;
                __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(&Ps[buf][it * P_ROWS][0] + wave_u * (1024 / (int)sizeof(T))), 16, 0, 0);
                p_n[it] += BKP;
                continue;
            }
            if constexpr (!F16) p_reg[it] = *reinterpret_cast<const float4*>(smb + (ok ? p_n[it] * p.Cs + p_ch : 0));
            if (has_ss) ps_reg[it] = *reinterpret_cast<const float4*>(p.ss + (ok ? p_b[it] * p.Cs + p_ch : 0));
            p_mask |= (ok ? 1u : 0u) << it;
            p_n[it] += BKP;
            p_rem[it] += BKP;
            while (p_rem[it] >= (int)HWs) { p_rem[it] -= (int)HWs; ++p_b[it]; }
        }
#pragma unroll
        for (int it = 0; it < Q_IT; ++it) {
            int iy = q_oy[it] * p.stride + ky - p.pad, ix = q_ox[it] * p.stride + kx - p.pad;
            bool ok = q_ch_ok && q_n[it] < n_end && (unsigned)iy < (unsigned)p.Hb && (unsigned)ix < (unsigned)p.Wb;
            if (GLDS) {
                const T* g = ok ? bgb + (((q_b[it] * p.Hb + iy) * p.Wb + ix) * p.Cb + q_ch) : pzero;
                __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(&Qs[buf][it * Q_ROWS][0] + wave_u * (1024 / (int)sizeof(T))), 16, 0, 0);
            } else {
                if constexpr (!F16)
                    q_reg[it] = *reinterpret_cast<const float4*>(
                        bgb + (ok ? ((q_b[it] * p.Hb + iy) * p.Wb + ix) * p.Cb + q_ch : 0));
                if (has_bs) qs_reg[it] = *reinterpret_cast<const float4*>(p.bs + (ok ? q_b[it] * p.Cb + q_ch : 0));
                q_mask |= (ok ? 1u : 0u) << it;
            }
            q_n[it] += BKP;
            q_ox[it] += BKP;
            if (p.Ws >= BKP) {  // uniform: at most one row wrap per stage
                const bool wx = q_ox[it] >= p.Ws;
                q_ox[it] -= wx ? p.Ws : 0;
                q_oy[it] += wx ? 1 : 0;
                const bool wy = q_oy[it] >= p.Hs;
                q_oy[it] -= wy ? p.Hs : 0;
                q_b[it] += wy ? 1 : 0;
            } else {
                while (q_ox[it] >= p.Ws) { q_ox[it] -= p.Ws; ++q_oy[it]; }
                while (q_oy[it] >= p.Hs) { q_oy[it] -= p.Hs; ++q_b[it]; }
            }
        }
    };
    auto store_lds = [&](int buf) __attribute__((always_inline)) {
        if constexpr (GLDS) return;  // the DMA already wrote the tiles
        else {
#pragma unroll
        for (int it = 0; it < P_IT; ++it) {
            float4 v = p_reg[it];
            if (has_ss) { v.x *= ps_reg[it].x; v.y *= ps_reg[it].y; v.z *= ps_reg[it].z; v.w *= ps_reg[it].w; }
            if (!((p_mask >> it) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&Ps[buf][p_row + it * P_ROWS][(tid % (BP / 4)) * 4]) = v;
        }
#pragma unroll
        for (int it = 0; it < Q_IT; ++it) {
            float4 v = q_reg[it];
            if (has_bs) { v.x *= qs_reg[it].x; v.y *= qs_reg[it].y; v.z *= qs_reg[it].z; v.w *= qs_reg[it].w; }
            if (!((q_mask >> it) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(&Qs[buf][q_row + it * Q_ROWS][(tid % (BQ / 4)) * 4]) = v;
        }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf) __attribute__((always_inline)) {
        if constexpr (X3 == 1) {
            float psv[MT], qsv[NT];
            if (TAB) {
                const float* row = Stab + tab_row * (BP + BQ);
#pragma unroll
                for (int i = 0; i < MT; ++i) psv[i] = row[wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j) qsv[j] = row[BP + wq0 + j * 32 + li];
                tab_rem += BKP;
                if (tab_rem >= (int)HWs) { tab_rem -= (int)HWs; ++tab_row; }
            }
#pragma unroll
            for (int ks = 0; ks < BKP / 16; ++ks) {
                const int k0 = 16 * ks + 8 * lh;  // this lane half's 8 pixels of the K step
                float a[MT][8], b[NT][8];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[i][e] = Ps[buf][k0 + e][wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) b[j][e] = Qs[buf][k0 + e][wq0 + j * 32 + li];
                gif::u32x4_t sa[3][MT], sb[3][NT];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x0 = a[i][2 * e], x1 = a[i][2 * e + 1];
                        if (TAB) { x0 *= psv[i]; x1 *= psv[i]; }
                        unsigned h, m, l;
                        gif::split_pair(x0, x1, h, m, l);
                        sa[0][i][e] = h; sa[1][i][e] = m; sa[2][i][e] = l;
                    }
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x0 = b[j][2 * e], x1 = b[j][2 * e + 1];
                        if (TAB) { x0 *= qsv[j]; x1 *= qsv[j]; }
                        unsigned h, m, l;
                        gif::split_pair(x0, x1, h, m, l);
                        sb[0][j][e] = h; sb[1][j][e] = m; sb[2][j][e] = l;
                    }
                // smallest terms first; mid*lo, lo*mid, lo*lo (<= 2^-23 of the product) are not formed
                constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int t6 = 0; t6 < 6; ++t6)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gif::bf16x8_t, sa[TA[t6]][i]),
                                                                                __builtin_bit_cast(gif::bf16x8_t, sb[TB[t6]][j]),
                                                                                acc[i][j], 0, 0, 0);
            }
            return;
        } else if constexpr (F16) {
            float psv[MT], qsv[NT];
            if (TAB) {
                const float* row = Stab + tab_row * (BP + BQ);
#pragma unroll
                for (int i = 0; i < MT; ++i) psv[i] = row[wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j) qsv[j] = row[BP + wq0 + j * 32 + li];
                tab_rem += BKP;
                if (tab_rem >= (int)HWs) { tab_rem -= (int)HWs; ++tab_row; }
            }
#pragma unroll
            for (int ks = 0; ks < BKP / 16; ++ks) {
                gif::f16x8_t af[MT], bf[NT];
                const int k0 = 16 * ks + 8 * lh;  // this lane half's 8 pixels of the K step
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int e = 0; e < 8; ++e) af[i][e] = Ps[buf][k0 + e][wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bf[j][e] = Qs[buf][k0 + e][wq0 + j * 32 + li];
                if (TAB) {
#pragma unroll
                    for (int i = 0; i < MT; ++i) af[i] *= (gif::f16)psv[i];
#pragma unroll
                    for (int j = 0; j < NT; ++j) bf[j] *= (gif::f16)qsv[j];
                }
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
            return;
        } else {
        // operand fragments of k-step ks+1 are fetched from LDS before the MFMAs of k-step ks (register double buffer)
        float av[2][MT], bv[2][NT];
        float psv[MT], qsv[NT];
        if (TAB) {
            const float* row = Stab + tab_row * (BP + BQ);
#pragma unroll
            for (int i = 0; i < MT; ++i) psv[i] = row[wp0 + i * 32 + li];
#pragma unroll
            for (int j = 0; j < NT; ++j) qsv[j] = row[BP + wq0 + j * 32 + li];
            tab_rem += BKP;
            if (tab_rem >= (int)HWs) { tab_rem -= (int)HWs; ++tab_row; }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) av[0][i] = Ps[buf][lh][wp0 + i * 32 + li];
#pragma unroll
        for (int j = 0; j < NT; ++j) bv[0][j] = Qs[buf][lh][wq0 + j * 32 + li];
#pragma unroll
        for (int ks = 0; ks < BKP / 2; ++ks) {
            const int c = ks & 1, n = c ^ 1;
            if (ks + 1 < BKP / 2) {
#pragma unroll
                for (int i = 0; i < MT; ++i) av[n][i] = Ps[buf][2 * ks + 2 + lh][wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j) bv[n][j] = Qs[buf][2 * ks + 2 + lh][wq0 + j * 32 + li];
            }
            if (TAB) {
#pragma unroll
                for (int i = 0; i < MT; ++i) av[c][i] *= psv[i];
#pragma unroll
                for (int j = 0; j < NT; ++j) bv[c][j] *= qsv[j];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c][i], bv[c][j], acc[i][j], 0, 0, 0);
            // pin the schedule: the LDS reads of k-step ks+1 are issued BEFORE the MFMAs of k-step ks
            __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);  // DS reads
            __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);  // MFMA
        }
        }
    };

    if constexpr (X3 && BKP == 32) {
        // ---- bf16x3 / f16x2, software-pipelined (two 16-pixel groups per stage; same schedule as conv_gather_mfma_glds' X3 path):
        //   DMA(stage+1) | MFMAs(g0) + read & split g1 | barrier | MFMAs(g1) + read & split g0 of stage+1
        // The split of the NEXT group ((MT + NT) * 4 pieces: bf16x3 11 VALU each, +2 with per-sample scales; f16x2 5 VALU + the
        // running exponents) sits piecewise between the MFMAs of the current one; sched_barrier(0) pins the interleave.
        constexpr bool H2 = X3 == 2;
        constexpr int NPL = H2 ? 2 : 3;
        constexpr int NF = MT + NT;                   // operand fragments per group: P tiles, then Q tiles
        gif::u32x4_t sa[2][NPL][MT], sb[2][NPL][NT];  // [slot][term][tile]
        float ra[MT][8], rb[NT][8];                   // raw fragments of the group being split
        float psv[MT], qsv[NT];                       // per-sample scales of the stage being split (TAB)
        // f16x2 state per fragment (h2_row.h; its "row" is a channel = lane li of the tile), one array per field of gif::H2Row: f is a
        // constant only after the group's loops are unrolled, and an array of structs indexed by it costs registers or scratch memory
        int h_ex[NF], h_dl[NF];
        float h_sc[NF], h_lim[NF], h_max[NF];
        unsigned h_gmin[NF];
        bool h_need = false;
        if constexpr (H2) {
            const gif::H2Row init;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                h_ex[f] = init.ex; h_dl[f] = init.dl;
                h_sc[f] = init.sc; h_lim[f] = init.lim;
                h_max[f] = init.max; h_gmin[f] = init.gmin;
            }
        }
        auto scales = [&]() __attribute__((always_inline)) {
            if (TAB) {
                const float* row = Stab + tab_row * (BP + BQ);
#pragma unroll
                for (int i = 0; i < MT; ++i) psv[i] = row[wp0 + i * 32 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j) qsv[j] = row[BP + wq0 + j * 32 + li];
                tab_rem += BKP;
                if (tab_rem >= (int)HWs) { tab_rem -= (int)HWs; ++tab_row; }
            }
        };
        auto read_raw = [&](int buf, int ks) __attribute__((always_inline)) {
            const int k0 = 16 * ks + 8 * lh;  // this lane half's 8 pixels of the group
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) ra[i][e] = Ps[buf][k0 + e][wp0 + i * 32 + li];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) rb[j][e] = Qs[buf][k0 + e][wq0 + j * 32 + li];
        };
        // f16x2: per-sample scale, group maximum and exponent decision of fragment f of the raw group just read
        auto track = [&](int f) __attribute__((always_inline)) {
            if constexpr (H2) {
                float* v = f < MT ? ra[f] : rb[f - MT];
                if (TAB) {
                    const float sv = f < MT ? psv[f] : qsv[f - MT];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= sv;
                }
                gif::h2_observe(h_ex[f], h_dl[f], h_sc[f], h_lim[f], h_max[f], h_gmin[f], gif::h2_group_max(v), h_need);  // the channel's 16 pixels of this group
            }
        };
        // f16x2: acc[i][j][r] *= 2^(change of its P row + change of its Q column); the column of Q tile j is this lane's own
        auto rescale = [&]() __attribute__((always_inline)) {
            if constexpr (H2) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    gif::h2_for_rows(lh, h_dl[i], [&](int r, int d) __attribute__((always_inline)) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j][r] = ldexpf(acc[i][j][r], d + h_dl[MT + j]);
                    });
            }
        };
        constexpr int NPC = NF * 4;
        auto split_piece = [&](int slot, int k) __attribute__((always_inline)) {
            const int f = k / 4, e = k % 4;
            if constexpr (H2) {
                unsigned h, l;
                // (no packed fp32 in the split, common.h: with several scales per lane hipcc kept them in register pairs and picked the
                // odd element with `op_sel:[0,1]` on v_pk_mul_f32 / v_pk_fma_f32 — the kernel then dropped products in lanes 16-31 /
                // 48-63 of the second tile of each operand whenever two of its waves shared a SIMD (correct with one workgroup per CU, and
                // with the scale as a constant: tools/probes/h2_wgrad_debug.py); cause on the hardware side not established)
                const float scv = h_sc[f];
                if (f < MT) {
                    gif::split_pair_h2(ra[f][2 * e], ra[f][2 * e + 1], scv, h, l);
                    sa[slot][0][f][e] = h; sa[slot][1][f][e] = l;
                } else {
                    gif::split_pair_h2(rb[f - MT][2 * e], rb[f - MT][2 * e + 1], scv, h, l);
                    sb[slot][0][f - MT][e] = h; sb[slot][1][f - MT][e] = l;
                }
            } else {
                unsigned h, m, l;
                if (f < MT) {
                    float x0 = ra[f][2 * e], x1 = ra[f][2 * e + 1];
                    if (TAB) { x0 *= psv[f]; x1 *= psv[f]; }
                    gif::split_pair_scalar(x0, x1, h, m, l);
                    sa[slot][0][f][e] = h; sa[slot][1][f][e] = m; sa[slot][2][f][e] = l;
                } else {
                    float x0 = rb[f - MT][2 * e], x1 = rb[f - MT][2 * e + 1];
                    if (TAB) { x0 *= qsv[f - MT]; x1 *= qsv[f - MT]; }
                    gif::split_pair_scalar(x0, x1, h, m, l);
                    sb[slot][0][f - MT][e] = h; sb[slot][1][f - MT][e] = m; sb[slot][2][f - MT][e] = l;
                }
            }
        };
        // preparation step `q` of the next group: f16x2 runs a fragment's tracking step right before its four split pieces
        constexpr int NSTEP = H2 ? NF * 5 : NPC;
        auto prep = [&](int nslot, int q) __attribute__((always_inline)) {
            if constexpr (H2) {
                if (q % 5 == 0) track(q / 5);
                else split_piece(nslot, (q / 5) * 4 + q % 5 - 1);
            } else {
                split_piece(nslot, q);
            }
        };
        constexpr int NPROD = H2 ? 3 : 6;
        constexpr int LEAD = H2 ? 3 : 6;  // MFMAs ahead of the first piece: they cover the latency of the 32 ds_read_b32 (issued as 20 ds_read2)
        auto group = [&](int slot, int nslot) __attribute__((always_inline)) {
            int n = 0, q = 0;
            if constexpr (H2) h_need = false;
#pragma unroll
            for (int t6 = 0; t6 < NPROD; ++t6)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const gif::X3Terms tm = gif::x3_terms<H2>(t6);
                        if constexpr (H2)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(gif::f16x8_t, sa[slot][tm.a][i]),
                                                                               __builtin_bit_cast(gif::f16x8_t, sb[slot][tm.b][j]),
                                                                               acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gif::bf16x8_t, sa[slot][tm.a][i]),
                                                                                __builtin_bit_cast(gif::bf16x8_t, sb[slot][tm.b][j]),
                                                                                acc[i][j], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        ++n;
                        // f16x2 has half the MFMAs to hide twice the steps under: two steps per MFMA slot
                        if (nslot >= 0 && n >= LEAD) {
#pragma unroll
                            for (int rep2 = 0; rep2 < (H2 ? 2 : 1); ++rep2)
                                if (q < NSTEP) prep(nslot, q++);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
            if (nslot >= 0) {
#pragma unroll
                for (; q < NSTEP; ++q) prep(nslot, q);
                if constexpr (H2) {
                    if (h_need) rescale();
                }
            }
        };
        if (n_begin < n_end) {
            load_global(0);
            __syncthreads();
            scales();
            read_raw(0, 0);
#pragma unroll
            for (int q = 0; q < NSTEP; ++q) prep(0, q);  // (f16x2: first exponents; the accumulators are still zero)
            int cur = 0;
            for (int n0 = n_begin; n0 + BKP < n_end; n0 += BKP) {
                load_global(cur ^ 1);  // stage n0 + BKP: its buffer was last read before the previous stage's barrier
                __builtin_amdgcn_sched_barrier(0);
                read_raw(cur, 1);
                __builtin_amdgcn_sched_barrier(0);
                group(0, 1);
                __syncthreads();
                cur ^= 1;
                scales();
                read_raw(cur, 0);
                __builtin_amdgcn_sched_barrier(0);
                group(1, 0);
            }
            read_raw(cur, 1);
            __builtin_amdgcn_sched_barrier(0);
            group(0, 1);
            group(1, -1);
        }
        if constexpr (H2) {
            bool wide_p = false, wide_q = false;  // (a narrow group only costs accuracy where the other operand is narrow too: common.h)
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if (f < MT) wide_p |= gif::h2_wide(h_max[f], h_gmin[f]);
                else wide_q |= gif::h2_wide(h_max[f], h_gmin[f]);
            }
            if (p.gate && __builtin_amdgcn_ballot_w64(wide_p) != 0 && __builtin_amdgcn_ballot_w64(wide_q) != 0 && lane == 0)
                atomicMax(p.gate, p.gate_gen);
#pragma unroll
            for (int i = 0; i < MT; ++i)
                gif::h2_for_rows(lh, h_ex[i], [&](int r, int er) __attribute__((always_inline)) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j][r] = ldexpf(acc[i][j][r], -(er + h_ex[MT + j]));
                });
        }
    } else if (n_begin < n_end) {
        load_global(0);
        store_lds(0);
        __syncthreads();
        int cur = 0;
        for (int n0 = n_begin; n0 + BKP < n_end; n0 += BKP) {
            load_global(cur ^ 1);  // stage n0 + BKP
            __builtin_amdgcn_sched_barrier(0);
            compute(cur);
            __builtin_amdgcn_sched_barrier(0);
            store_lds(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        compute(cur);
    }

    float* out = p.ws + ((size_t)split * p.T + t) * p.RP * p.CP;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int row = r0 + wp0 + i * 32 + gif::acc_row(r, lh);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                int col = c0 + wq0 + j * 32 + li;
                out[(size_t)row * p.CP + col] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------
// f16x2 weight gradient, cooperative pre-split through LDS ("v2", round 5).  In conv_wgrad_mfma<..., 2> every wave gathers its operand
// fragments with eight ds_read_b32 each and splits them itself: every element is read and split by TWO waves (2 x 2 wave layout) and the
// loop is VALU-bound (136 VALU per 12 MFMAs).  Here a stage (32 pixels x 128 + 128 channels of fp32, landed by LDS-DMA as before) is
// converted ONCE: thread c of the 256 owns channel c (0..127: small side, 128..255: big side), reads its 32 pixels (conflict free:
// consecutive threads = consecutive channels), keeps the channel's running exponent PRIVATELY (no lane exchange), splits them into
// the two f16 terms and writes them as two 64-byte rows [channel][32 pixels] — the layout of the pre-split weights of the direct
// kernel (16-byte chunks XOR-swizzled, here with the f(row) below): an MFMA operand (8 consecutive pixels of one channel) is then ONE
// ds_read_b128 per term.  Per thread and stage: ~120 VALU + 24 LDS operations for the conversion, 16 ds_read_b128 + 24 MFMAs for the
// products (before: 272 VALU, 64 ds_read_b32).  Exponent changes travel through a small LDS array: the converting thread stores its
// channel's change, raises the stage's flag, and the MFMA waves multiply their accumulators (rows and columns) before the stage's
// products.  LDS: raw fp32 stage 32 KB (single buffer: the next stage's DMA is issued once the conversion has read it) + operand
// planes 32 KB => two workgroups per CU, whose phases interleave.  128 x 128 tiles, 4 waves as 2 x 2.
// TAPS (round 5, thin big side: the 24-channel condition-noise maps): a 128 x 32 tile per tap stages 16 KB of gy for every 4 KB of x and
// sits on the LDS-DMA fill rate (13 FLOP per staged byte: 80 TFLOP/s measured).  Here the 128 tile columns are `tpt` TAPS x Cb channels
// (5 x 24): gy is staged once per 5 taps, every column's thread gathers x at ITS tap's shift; 9 taps = 2 column tiles.
// BUF (round 6): the stage's LDS-DMA pieces go through buffer descriptors.  The small side's per-lane byte offset is loop invariant (the
// stage travels in the instruction's SGPR offset; rows behind the split's end lie outside the descriptor and land as zeros): no VALU at
// all per piece.  The big side keeps (ox, oy) per piece for the padding test and a running 32-bit byte offset that advances by constants
// (+32 pixels; + a constant at a row wrap; + another at a sample wrap): ~19 VALU per piece where the 64-bit form spent ~50 — three
// multiplies, three bounds checks, a zero-page select and the (ox, oy, b) wrap with both of its code paths; the ISA of round 5 showed
// ~400 instructions per stage and wave for the addressing next to ~180 for the conversion and 24 MFMAs.  Needs both operands within
// 3.5 GiB (checked on the host: larger launches keep the 64-bit form, BUF = false).
template <bool TAB, bool TAPS = false, bool BUF = false>
__global__ void __launch_bounds__(256, 2) conv_wgrad_h2v2(const WgradParams p) {
    constexpr int BP = 128, BQ = 128, BKP = 32, THREADS = 256, MT = 2, NT = 2, P_ROWS = 8, Q_ROWS = 8, P_IT = 4, Q_IT = 4;
    extern __shared__ __attribute__((aligned(16))) float wg_smem[];
    float (*Ps)[BP] = reinterpret_cast<float (*)[BP]>(wg_smem);                         // [32][128] fp32
    float (*Qs)[BQ] = reinterpret_cast<float (*)[BQ]>(wg_smem + BKP * BP);              // [32][128] fp32
    unsigned short* Op = reinterpret_cast<unsigned short*>(wg_smem + BKP * (BP + BQ));  // [2 terms][256 channels][32 pixels] f16
    int* dexp = reinterpret_cast<int*>(Op + 2 * 256 * 32);                              // [256] exponent change of the stage
    int* fexp = dexp + 256;                                                             // [256] final exponents
    int* flags = fexp + 256;                                                            // [0], [1]: a channel changed (stage parity); [2], [3]: narrow group on the P / Q side
    float* Stab = reinterpret_cast<float*>(flags + 8);                                  // TAB: [stab_nb][256]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wp0 = (wave >> 1) * 64, wq0 = (wave & 1) * 64;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = lid % p.tiles_pq;
    const int TG = TAPS ? p.tgroups : p.T;
    const int t = (lid / p.tiles_pq) % TG;  // TAPS: the tap GROUP
    const int split = lid / (p.tiles_pq * TG);
    const int tq = tile % p.tiles_q, tp = tile / p.tiles_q;
    const int r0 = tp * BP, c0 = TAPS ? 0 : tq * BQ;
    const bool planes = !TAPS && p.sm_plane != 0;
    // TAPS: this thread's four staged columns belong to tap t * tpt + q_tl (lanes past the last tap stage zeros)
    const int q_tl = TAPS ? ((tid % (BQ / 4)) * 4) / p.Cb : 0;
    const int q_tap = TAPS ? t * p.tpt + q_tl : t;
    const int ky = planes ? 0 : q_tap / p.KW, kx = planes ? 0 : q_tap - ky * p.KW;
    const float* const smb = static_cast<const float*>(p.sm) + (TAPS ? 0 : (size_t)t * p.sm_plane);
    const float* const bgb = static_cast<const float*>(p.bg) + (TAPS ? 0 : (size_t)t * p.bg_plane);
    const float* const pzero = static_cast<const float*>(p.zero);
    const int n_begin = (int)((long)split * p.chunk);
    int n_end = n_begin + (int)p.chunk;
    if (n_end > (int)p.Ntot) n_end = (int)p.Ntot;
    const unsigned HWs = (unsigned)(p.Hs * p.Ws);

    const int p_row = tid / (BP / 4), p_ch = r0 + (tid % (BP / 4)) * 4;
    const int q_row = tid / (BQ / 4), q_ch = TAPS ? (tid % (BQ / 4)) * 4 - q_tl * p.Cb : c0 + (tid % (BQ / 4)) * 4;
    const bool p_ch_ok = p_ch < p.Cs, q_ch_ok = TAPS ? (q_tl < p.tpt && q_tap < p.T) : q_ch < p.Cb;
    int tab_row = 0, tab_rem = 0;
    if (tid < 8) flags[tid] = 0;
    if (TAB) {
        const int b_first = n_begin / (int)HWs;
        for (int e = tid; e < p.stab_nb * (BP + BQ); e += THREADS) {
            int bl = e / (BP + BQ), c = e - bl * (BP + BQ);
            int b = b_first + bl;
            float v = 0.f;
            if (b < p.B) {
                if (c < BP) v = (r0 + c < p.Cs) ? (p.ss ? p.ss[(size_t)b * p.Cs + r0 + c] : 1.f) : 0.f;
                else v = (c0 + c - BP < p.Cb) ? (p.bs ? p.bs[(size_t)b * p.Cb + c0 + c - BP] : 1.f) : 0.f;
            }
            Stab[e] = v;
        }
        tab_rem = n_begin - b_first * (int)HWs;
    }
    int p_n[P_IT], q_n[Q_IT], q_b[Q_IT], q_oy[Q_IT], q_ox[Q_IT];
    unsigned p_vo[P_IT], q_bo[Q_IT];  // BUF: byte offsets (small side: loop invariant; big side: running)
#pragma unroll
    for (int it = 0; it < P_IT; ++it) {
        p_n[it] = n_begin + p_row + it * P_ROWS;
        p_vo[it] = p_ch_ok ? (unsigned)(p_n[it] * p.Cs + p_ch) * 4u : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int it = 0; it < Q_IT; ++it) {
        int n = n_begin + q_row + it * Q_ROWS;
        q_n[it] = n;
        unsigned b = (unsigned)n / HWs;
        unsigned r = (unsigned)n - b * HWs;
        unsigned oy = r / (unsigned)p.Ws;
        q_b[it] = (int)b; q_oy[it] = (int)oy; q_ox[it] = (int)(r - oy * (unsigned)p.Ws);
        q_bo[it] = (unsigned)((((int)b * p.Hb + q_oy[it] * p.stride + ky - p.pad) * p.Wb + q_ox[it] * p.stride + kx - p.pad) * p.Cb + q_ch) * 4u;
    }
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // BUF: descriptors and the constants of the running offsets (all wave-uniform).  Small side: rows >= n_end are outside; big side: the
    // whole tensor (a stage only reaches past n_end in the LAST split, where those rows belong to sample B: outside) — planes mode: the
    // plane up to n_end (its padding rows are uninitialised memory)
    const gif::buf_rsrc_t rs_p = gif::make_buf_rsrc(smb, (unsigned)n_end * (unsigned)p.Cs * 4u);
    const gif::buf_rsrc_t rs_q = gif::make_buf_rsrc(bgb, planes ? (unsigned)n_end * (unsigned)p.Cb * 4u
                                                                  : (unsigned)p.B * (unsigned)p.Hb * (unsigned)p.Wb * (unsigned)p.Cb * 4u);
    const unsigned q_step = (unsigned)(BKP * p.stride * p.Cb) * 4u;
    const unsigned q_drow = (unsigned)((p.Wb - p.Ws) * p.stride * p.Cb) * 4u;           // on top of the linear advance, mod 2^32
    const unsigned q_dsmp = (unsigned)((p.Hb - p.Hs * p.stride) * p.Wb * p.Cb) * 4u;
    const int q_cy = ky - p.pad, q_cx = kx - p.pad;
    int p_soff = 0;
    auto load_global = [&]() __attribute__((always_inline)) {
        if constexpr (BUF) {
#pragma unroll
            for (int it = 0; it < P_IT; ++it)
                gif::buf_load_lds16(rs_p, (lptr_t)(&Ps[it * P_ROWS][0] + wave_u * 256), p_vo[it], p_soff);
            p_soff += BKP * p.Cs * 4;
#pragma unroll
            for (int it = 0; it < Q_IT; ++it) {
                const int iy = q_oy[it] * p.stride + q_cy, ix = q_ox[it] * p.stride + q_cx;
                const bool ok = q_ch_ok && (unsigned)iy < (unsigned)p.Hb && (unsigned)ix < (unsigned)p.Wb;
                gif::buf_load_lds16(rs_q, (lptr_t)(&Qs[it * Q_ROWS][0] + wave_u * 256), ok ? q_bo[it] : 0xFFFFFFFFu, 0);
                q_bo[it] += q_step;
                q_ox[it] += BKP;
                if (p.Ws >= BKP) {  // uniform: at most one row wrap per stage
                    const bool wx = q_ox[it] >= p.Ws;
                    q_ox[it] -= wx ? p.Ws : 0;
                    q_oy[it] += wx ? 1 : 0;
                    q_bo[it] += wx ? q_drow : 0u;
                    const bool wy = q_oy[it] >= p.Hs;
                    q_oy[it] -= wy ? p.Hs : 0;
                    q_bo[it] += wy ? q_dsmp : 0u;
                } else {
                    while (q_ox[it] >= p.Ws) { q_ox[it] -= p.Ws; ++q_oy[it]; q_bo[it] += q_drow; }
                    while (q_oy[it] >= p.Hs) { q_oy[it] -= p.Hs; q_bo[it] += q_dsmp; }
                }
            }
            return;
        }
#pragma unroll
        for (int it = 0; it < P_IT; ++it) {
            const bool ok = p_ch_ok && p_n[it] < n_end;
            const float* g = ok ? smb + (p_n[it] * p.Cs + p_ch) : pzero;
            __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(&Ps[it * P_ROWS][0] + wave_u * 256), 16, 0, 0);
            p_n[it] += BKP;
        }
#pragma unroll
        for (int it = 0; it < Q_IT; ++it) {
            const int iy = q_oy[it] * p.stride + ky - p.pad, ix = q_ox[it] * p.stride + kx - p.pad;
            const bool ok = q_ch_ok && q_n[it] < n_end && (unsigned)iy < (unsigned)p.Hb && (unsigned)ix < (unsigned)p.Wb;
            const float* g = ok ? bgb + (((q_b[it] * p.Hb + iy) * p.Wb + ix) * p.Cb + q_ch) : pzero;
            __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(&Qs[it * Q_ROWS][0] + wave_u * 256), 16, 0, 0);
            q_n[it] += BKP;
            q_ox[it] += BKP;
            if (p.Ws >= BKP) {  // uniform: at most one row wrap per stage
                const bool wx = q_ox[it] >= p.Ws;
                q_ox[it] -= wx ? p.Ws : 0;
                q_oy[it] += wx ? 1 : 0;
                const bool wy = q_oy[it] >= p.Hs;
                q_oy[it] -= wy ? p.Hs : 0;
                q_b[it] += wy ? 1 : 0;
            } else {
                while (q_ox[it] >= p.Ws) { q_ox[it] -= p.Ws; ++q_oy[it]; }
                while (q_oy[it] >= p.Hs) { q_oy[it] -= p.Hs; ++q_b[it]; }
            }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- this thread's channel (conversion role): running exponent and the guard's statistics, all private
    const float* const rawcol = tid < 128 ? &Ps[0][tid] : &Qs[0][tid - 128];
    unsigned short* const oprow = Op + tid * 32;
    // 16-byte chunk swizzle of the operand planes: f(row) = bit 2 | (bit 1 ^ bit 3) << 1 of the row index.  ds_write_b128 is serviced in groups
    // of 8 CONTIGUOUS lanes on 32 banks (two 64-byte rows per bank window), ds_read_b128 in the four non-contiguous 16-lane groups of the
    // microarchitecture guide's LDS table on 64 banks; this f puts both on distinct 16-byte slots (the direct kernel's (row >> 2) & 3 is
    // conflict free for the reads only: the conversion's stores ran 2-way, 109 M conflict cycles per launch in the round's PMC pass)
    const int wsw = ((tid >> 2) & 1) | ((((tid >> 1) ^ (tid >> 3)) & 1) << 1);
    gif::H2Row hr;  // (h2_row.h)
    auto convert = [&](int par) __attribute__((always_inline)) {
        float v[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = rawcol[e * 128];
        if (TAB) {
            const float sv = Stab[tab_row * (BP + BQ) + tid];
#pragma unroll
            for (int e = 0; e < 32; ++e) v[e] *= sv;
            tab_rem += BKP;
            if (tab_rem >= (int)HWs) { tab_rem -= (int)HWs; ++tab_row; }
        }
        float m0 = 0.f, m1 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) { m0 = fmaxf(m0, fabsf(v[e])); m1 = fmaxf(m1, fabsf(v[16 + e])); }
        // this channel outgrew its exponent (private state: plain divergence; rare after the first stages)
        if (gif::h2_observe_private(hr, m0, m1)) atomicOr(&flags[par], 1);
        dexp[tid] = hr.dl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // 8 pixels = one 16-byte chunk of each term
            gif::u32x4_t hi4, lo4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned h, l;
                gif::split_pair_h2(v[8 * j + 2 * k], v[8 * j + 2 * k + 1], hr.sc, h, l);
                hi4[k] = h; lo4[k] = l;
            }
            const int phys = (j ^ wsw) << 3;
            *reinterpret_cast<gif::u32x4_t*>(oprow + phys) = hi4;
            *reinterpret_cast<gif::u32x4_t*>(oprow + 256 * 32 + phys) = lo4;
        }
    };
    // ---- product role
    const int rsw = ((li >> 2) & 1) | ((((li >> 1) ^ (li >> 3)) & 1) << 1);  // f(row) of every operand row this lane reads (tile bases are multiples of 32)
    auto products = [&](int par) __attribute__((always_inline)) {
        if (flags[par] != 0) {  // workgroup-uniform: some channel of this stage changed its exponent: acc *= 2^(row change + column change)
            int dc[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) dc[j] = dexp[128 + wq0 + j * 32 + li];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = dexp[wp0 + i * 32 + gif::acc_row(r, lh)];
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j][r] = ldexpf(acc[i][j][r], dr + dc[j]);
                }
        }
        if (tid == 0) flags[par ^ 1] = 0;  // the next stage's conversions raise it again (they start behind the next barrier)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            gif::u32x4_t sa[2][MT], sb[2][NT];
            const int ch = ((2 * g + lh) ^ rsw) << 3;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int i = 0; i < MT; ++i) sa[tt][i] = *reinterpret_cast<const gif::u32x4_t*>(Op + (tt * 256 + wp0 + i * 32 + li) * 32 + ch);
#pragma unroll
                for (int j = 0; j < NT; ++j) sb[tt][j] = *reinterpret_cast<const gif::u32x4_t*>(Op + (tt * 256 + 128 + wq0 + j * 32 + li) * 32 + ch);
            }
#pragma unroll
            for (int t3 = 0; t3 < 3; ++t3) {  // lo*hi, hi*lo, hi*hi
                const gif::X3Terms tm = gif::x3_terms<true>(t3);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(gif::f16x8_t, sa[tm.a][i]),
                                                                           __builtin_bit_cast(gif::f16x8_t, sb[tm.b][j]), acc[i][j], 0, 0, 0);
            }
        }
    };

    if (n_begin < n_end) {
        load_global();
        int par = 0;
        for (int n0 = n_begin; n0 < n_end; n0 += BKP) {
            __syncthreads();  // the stage's fp32 tiles have landed (vmcnt(0) of every wave); the previous stage's operand reads are done
            convert(par);
            __syncthreads();  // operand planes complete; the raw buffer is free again
            if (n0 + BKP < n_end) load_global();
            __builtin_amdgcn_sched_barrier(0);
            products(par);
            par ^= 1;
        }
    }
    // final exponents and the guard (a narrow group only costs accuracy where the other side is narrow too: common.h)
    __syncthreads();
    fexp[tid] = hr.ex;
    if (gif::h2_wide(hr)) atomicOr(&flags[tid < 128 ? 2 : 3], 1);
    __syncthreads();
    if (tid == 0 && p.gate && flags[2] != 0 && flags[3] != 0) atomicMax(p.gate, p.gate_gen);
    int ec[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) ec[j] = fexp[128 + wq0 + j * 32 + li];
    float* out = p.ws + ((size_t)split * p.T + (TAPS ? 0 : t)) * p.RP * p.CP;
    long ocol[NT];  // column offset inside the split's [T][RP][CP] block (TAPS: the column's own tap plane), < 0: padding column
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = wq0 + j * 32 + li;
        if (TAPS) {
            const int tl = c / p.Cb, tap = t * p.tpt + tl;
            ocol[j] = (tl < p.tpt && tap < p.T) ? (long)tap * p.RP * p.CP + (c - tl * p.Cb) : -1;
        } else {
            ocol[j] = c0 + c;
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = wp0 + i * 32 + gif::acc_row(r, lh);
            const int er = fexp[rl];
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (!TAPS || ocol[j] >= 0) out[(size_t)(r0 + rl) * p.CP + ocol[j]] = ldexpf(acc[i][j][r], -(er + ec[j]));
        }
}

template <typename T, int BP, int BQ, int WP_, int WQ_, bool GLDS, int BKP, bool TAB = false, int X3 = 0>
void wgrad_launch(dim3 grid, int threads, hipStream_t s, const WgradParams& p) {
    static gif::LdsAttr attr;
    const size_t lds = (size_t)2 * BKP * (BP + BQ) * sizeof(T) + (size_t)(TAB ? p.stab_nb * (BP + BQ) : 0) * sizeof(float);
    gif::launch_lds(conv_wgrad_mfma<T, BP, BQ, WP_, WQ_, GLDS, BKP, TAB, X3>, attr, grid, dim3(threads), lds, s, p);
}

// buffer-addressed DMA of conv_wgrad_h2v2: both operands (per plane in planes mode) within 3.5 GiB; GIF_H2_WGRAD_BUF=0: the 64-bit form (A/B)
inline bool h2v2_buf_ok(const WgradParams& p) {
    static const int off = gif::knob_int("GIF_H2_WGRAD_BUF", 1) == 0;
    // byte offsets are unsigned 32-bit; rows a stage reaches past the end of a tensor (the last split's tail, < 32 pixels) must stay out of
    // range without wrapping: 512 MiB of headroom below 4 GiB (the 64-sample discriminator pass on the blurred 257^2 map is 2.16 GB)
    const long lim = (1L << 32) - (1L << 29);
    return !off && (long)p.B * p.Hs * p.Ws * p.Cs * 4 <= lim && (long)p.B * p.Hb * p.Wb * p.Cb * 4 <= lim;
}
template <bool TAB, bool TAPS>
inline void wgrad_launch_v2_t(dim3 grid, size_t lds, hipStream_t s, const WgradParams& p) {
    static gif::LdsAttr attr[2];  // one per kernel: the 64-bit form, the buffer form
    if (h2v2_buf_ok(p)) gif::launch_lds(conv_wgrad_h2v2<TAB, TAPS, true>, attr[1], grid, dim3(256), lds, s, p);
    else gif::launch_lds(conv_wgrad_h2v2<TAB, TAPS, false>, attr[0], grid, dim3(256), lds, s, p);
}
inline void wgrad_launch_v2(bool tab, dim3 grid, hipStream_t s, const WgradParams& p, bool taps = false) {
    const size_t lds = (size_t)32 * 256 * 4 + (size_t)2 * 256 * 32 * 2 + (size_t)(512 + 8) * 4 + (size_t)(tab ? p.stab_nb * 256 : 0) * sizeof(float);
    if (taps) wgrad_launch_v2_t<false, true>(grid, lds, s, p);
    else if (tab) wgrad_launch_v2_t<true, false>(grid, lds, s, p);
    else wgrad_launch_v2_t<false, false>(grid, lds, s, p);
}

// ---- f16x2 weight PACKING (operand of the forward and data-gradient kernels of conv_igemm.hip; the other packings: weight_pack.hip).
// It is in this translation unit for its device code's sake: gif::h2_exp_for (h2_row.h) takes its target as an ARGUMENT, and hipcc
// specialises the function per translation unit by the targets its callers pass.  Here those are kH2TargetW (this kernel) and kH2Target
// (the f16x2 weight-gradient kernels), so the clamp stays a v_min_i32 / s_min_i32.  With the target as a template argument (tried:
// h2_exp_for<kH2Target>, which would let this kernel move to weight_pack.hip) the clamp became an unsigned compare and a select
// everywhere: conv_wgrad_h2v2 <0,0,0> 166 -> 168, <0,0,1> 154 -> 156, <1,0,0> 162 -> 164, <1,0,1> 156 -> 158 VGPRs, other opcodes in
// conv_wgrad_h2v2 <0,1,*>, conv_wgrad_mfma <.., X3 = 2>, the three wino_gemm_h2 and both packing kernels at unchanged registers.
// f16x2 packing (common.h "h2"): one workgroup per packed row.  Header hdr[r] = the row's exponent e (row maximum over all taps and
// channels of scale * w lands in [2^14, 2^15)), hdr[RP + r] = the row's flag; planes wp2[t][2][RP][CP] (f16 bits) = hi / lo of
// scale * w * 2^e.  A 16-channel K group (the kernels' k-groups: 16 consecutive padded channels of one tap) whose maximum lies more
// than 2^kH2WindowW below the row maximum sets the flag: its values no longer carry 22 bits, launches using the row take the bf16x3
// fallback.
// planes3 != NULL: the bf16x3 packing wp3[t][3][RP][CP] of the same weights (the guarded fallback's operand) in the same pass.
// The row's T * CP values are read from HBM ONCE into LDS (the canonical tensor is walked with a stride of 9 or 9 * Cin floats:
// the second read cost as much as the first; 28.6 -> 15.5 us per pack, 86 packs per training iteration: profiles/r5_kernel_stats.md).
__global__ void __launch_bounds__(256) pack_weight_h2_kernel(const float* __restrict__ w, int* __restrict__ hdr, unsigned short* __restrict__ planes,
                                                             unsigned short* __restrict__ planes3, int R, int C, int KH, int KW, int RP, int CP,
                                                             long sr, long sc, long sky, long skx, float scale, int dense_cpt, int dense_steps) {
    // dense_cpt > 0: the tap-dense K order of a 3x3 kernel (gif_pack_weight_f32x3_tapdense): "taps" = dense_steps K steps of CP = 32
    // floats, float k of step st = float k % 4 of 16-byte chunk q = 8 st + k / 4 = tap q / cpt, channel 4 (q % cpt) + k % 4
    extern __shared__ float row_vals[];  // [KH * KW][CP]
    __shared__ float red[256];
    __shared__ int s_flag;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_flag = 0;
    const int T = dense_cpt ? dense_steps : KH * KW, n = T * CP;
    float m = 0.f;
    for (int e = tid; e < n; e += 256) {
        // (c fastest over the threads for rows = output channels: consecutive threads walk the input channels, 9 floats apart)
        int t = e / CP, c = e - t * CP;
        bool ok = r < R;
        if (dense_cpt) {
            const int q = t * 8 + c / 4;
            t = q / dense_cpt;
            c = (q - t * dense_cpt) * 4 + c % 4;
            ok = ok && t < 9;
        }
        const int ky = t / KW, kx = t - ky * KW;
        const float v = (ok && c < C) ? scale * w[r * sr + c * sc + ky * sky + kx * skx] : 0.f;
        row_vals[e] = v;
        m = fmaxf(m, fabsf(v));
    }
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
        __syncthreads();
    }
    const float rowmax = red[0];
    const int e2 = gif::h2_weight_exp(rowmax);
    const float sc2 = gif::h2_pow2(e2);
    const size_t plane = (size_t)RP * CP;
    const int gpt = CP / 16, ngroups = T * gpt;  // 16-channel groups per tap / per row
    bool narrow = false;
    for (int g = tid; g < ngroups; g += 256) {
        const int t = g / gpt, c0 = (g - t * gpt) * 16;
        const float* src = row_vals + t * CP + c0;
        unsigned short* o = planes + (size_t)t * 2 * plane + (size_t)r * CP + c0;
        float gm = 0.f;
#pragma unroll 4
        for (int k = 0; k < 16; k += 2) {
            const float v0 = src[k], v1 = src[k + 1];
            gm = fmaxf(gm, fmaxf(fabsf(v0), fabsf(v1)));
            unsigned h, l;
            gif::split_pair_h2(v0, v1, sc2, h, l);
            *reinterpret_cast<unsigned*>(o + k) = h;
            *reinterpret_cast<unsigned*>(o + plane + k) = l;
            if (planes3) {
                unsigned m3;
                gif::split_pair(v0, v1, h, m3, l);
                unsigned short* o3 = planes3 + (size_t)t * 3 * plane + (size_t)r * CP + c0 + k;
                *reinterpret_cast<unsigned*>(o3) = h;
                *reinterpret_cast<unsigned*>(o3 + plane) = m3;
                *reinterpret_cast<unsigned*>(o3 + 2 * plane) = l;
            }
        }
        gif::h2_weight_note(rowmax, gm, narrow);
    }
    if (narrow) atomicOr(&s_flag, 1);
    __syncthreads();
    if (tid == 0) {
        hdr[r] = e2;
        hdr[RP + r] = s_flag;
    }
}

__global__ void unpack_wgrad_kernel(const float* __restrict__ ws, float* __restrict__ dw, int nsplit, int R, int C,
                                    int KH, int KW, int RP, int CP, long sr, long sc, long sky, long skx,
                                    float scale) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)KH * KW * R * C;
    if (idx >= total) return;
    int c = (int)(idx % C);
    long rest = idx / C;
    int r = (int)(rest % R);
    int t = (int)(rest / R);
    int ky = t / KW, kx = t - ky * KW;
    size_t stride = (size_t)KH * KW * RP * CP;
    const float* src = ws + ((size_t)t * RP + r) * CP + c;
    // 8 independent partial sums (fixed assignment split -> lane, fixed final order): the loads of 8 splits are in flight
    // together instead of one dependent ~1 us HBM round trip per split (113 splits on the 128-channel layers)
    float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) part[k] += src[(size_t)(s + k) * stride];
    }
    for (int k = 0; s < nsplit; ++s, ++k) part[k] += src[(size_t)s * stride];
    const float acc = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    dw[r * sr + c * sc + ky * sky + kx * skx] = scale * acc;
}

// ------------------------------------------------------------------------------------------------------------------
// Small-channel weight gradient (the condition-noise convs 6->12->24: Cs <= 32, Cb <= 16, 3x3, stride 1, pad 1).
// On the 32x32-tile kernel above these layers run at 5-11 TFLOP/s: nine launches-worth of 32x32x2 MFMAs of which
// (12..24)x(8..12) entries are real.  Here ONE wave owns all 9 taps: per group of 4 consecutive pixels it loads gy[4 px][Cs]
// and the nine shifted x[4 px][Cb] straight from global memory (64-byte segments, L1/L2 resident: no LDS) as the A / B operands
// of v_mfma_f32_16x16x4_f32 (i = cout, j = cin, k = pixel) and accumulates 9 taps x 2 cout tiles = 18 accumulators.
// 1024-thread workgroups: 16 waves share a pixel range; their accumulators are reduced through LDS in a fixed order and
// written as one split of the usual [split][tap][RP][CP] workspace (deterministic, same unpack kernel).
// ------------------------------------------------------------------------------------------------------------------
struct SmallWgradParams {
    const float* sm;  // gy [B,H,W,Cs]
    const float* bg;  // x  [B,H,W,Cb]
    float* ws;        // [nsplit][9][RP][CP]
    int B, H, W, Cs, Cb, RP, CP;
    long Ntot, chunk;  // pixels, pixels per split (multiple of 64)
};

__global__ void __launch_bounds__(1024) conv_wgrad_small_mfma(const SmallWgradParams p) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [8][18][256] floats = 147 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, k = lane >> 4;
    const long n_begin = (long)blockIdx.x * p.chunk;
    long n_end = n_begin + p.chunk;
    if (n_end > p.Ntot) n_end = p.Ntot;
    f32x4 acc[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[t][ct] = (f32x4)(0.f);
    const bool cin_ok = c < p.Cb;
    const bool co_ok[2] = {c < p.Cs, 16 + c < p.Cs};
    // this lane's pixel: n = n_begin + (quad index)*4 + k ; waves take quads round-robin (16 waves => +64 pixels per step)
    long n = n_begin + wave * 4 + k;
    int x, y, b;
    {
        long hw = (long)p.H * p.W;
        b = (int)(n / hw);
        long r = n - (long)b * hw;
        y = (int)(r / p.W);
        x = (int)(r - (long)y * p.W);
    }
    float a_cur[2], b_cur[9];
    auto load = [&](float (&av)[2], float (&bv)[9]) __attribute__((always_inline)) {
        const bool ok = n < n_end;
        const float* sp = p.sm + n * p.Cs + c;
        av[0] = (ok && co_ok[0]) ? sp[0] : 0.f;
        av[1] = (ok && co_ok[1]) ? sp[16] : 0.f;
        const float* bp = p.bg + n * p.Cb + c;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const bool in = ok && cin_ok && (unsigned)(y + dy) < (unsigned)p.H && (unsigned)(x + dx) < (unsigned)p.W;
                bv[(dy + 1) * 3 + dx + 1] = in ? bp[((long)dy * p.W + dx) * p.Cb] : 0.f;
            }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        n += 64;
        x += 64;
        while (x >= p.W) { x -= p.W; ++y; }
        while (y >= p.H) { y -= p.H; ++b; }
    };
    const long steps = (n_end - n_begin + 63) / 64;
    load(a_cur, b_cur);
    for (long s = 0; s < steps; ++s) {
        float a_nxt[2], b_nxt[9];
        advance();
        load(a_nxt, b_nxt);  // prefetch of the next group runs under this group's 18 MFMAs
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                acc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[ct], b_cur[t], acc[t][ct], 0, 0, 0);
        a_cur[0] = a_nxt[0]; a_cur[1] = a_nxt[1];
#pragma unroll
        for (int t = 0; t < 9; ++t) b_cur[t] = b_nxt[t];
    }
    // fixed-order tree over the 16 waves: waves [h, 2h) hand their accumulators to waves [0, h)
    for (int h = 8; h >= 1; h >>= 1) {
        if (wave >= h && wave < 2 * h) {
            float* dst = red + (size_t)(wave - h) * 18 * 256;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    *reinterpret_cast<f32x4*>(dst + (t * 2 + ct) * 256 + lane * 4) = acc[t][ct];
        }
        __syncthreads();
        if (wave < h) {
            const float* src = red + (size_t)wave * 18 * 256;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    acc[t][ct] += *reinterpret_cast<const f32x4*>(src + (t * 2 + ct) * 256 + lane * 4);
        }
        __syncthreads();
    }
    if (wave == 0) {
        // C/D layout of the 16x16 MFMA: column j = lane & 15, rows i = 4*(lane >> 4) + r
        float* out = p.ws + (size_t)blockIdx.x * 9 * p.RP * p.CP;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = ct * 16 + 4 * k + r;
                    out[((size_t)t * p.RP + row) * p.CP + c] = acc[t][ct][r];
                }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// f16 "halo" weight gradient for the thin high-resolution layers (Cs <= 32, Cb <= 32, stride 1: the 1024^2 block of BASELINE
// configs[4] and the condition-noise / ToRGB layers, model/stg2_generator.py:159-209, stylegan2_common_layers.py:388-431).
// conv_wgrad_mfma above runs one workgroup per (pixel chunk, TAP): nine workgroups stream the same two activation chunks
// through LDS-DMA and each gathers them again — 0.86 ms for 32 x 32 channels at 1024^2, batch 8 (0.18 ms of HBM traffic).
// Here a PERSISTENT workgroup walks 16 x 16-pixel patches of one sample: the gy patch and the x patch + halo are staged in LDS
// once (double buffered: the LDS-DMA of patch k + 1 runs under the MFMAs of patch k; nothing is stored per patch, so the loop
// has no store latency in it), and all taps are formed from LDS: a K step is one patch row (16 pixels), the tap only shifts the
// row / column of the x operand.  K = pixels is the slow axis of both tiles, so an operand fragment (8 consecutive pixels of
// one channel) is gathered with eight 16-bit LDS reads as in the kernel above (lane = channel: a half wave reads 64
// contiguous bytes of one pixel, conflict free); the gy fragment is gathered once per K step for all taps.
// Each of the 4 waves owns every fourth patch row and all taps (9 accumulator tiles of 32 x 32 = 144 VGPRs); at the end the
// waves' accumulators are reduced through LDS in a fixed order and the workgroup writes ONE split of the usual
// [split][tap][RP][CP] workspace (nsplit = workgroups; deterministic, same unpack kernel).  Per-sample scales (modulated
// layers) multiply the fragments: one scalar per lane, a patch belongs to one sample.
// ------------------------------------------------------------------------------------------------------------------
struct HaloWgradParams {
    const void* sm;   // gy [B,H,W,Cs] f16
    const void* bg;   // x  [B,H,W,Cb] f16 (same spatial size: stride 1, pad = (K - 1) / 2 or 0 for 1x1)
    float* ws;        // [nsplit = gridDim.x][T][32][32]
    const float* ss;  // [B,Cs] or null
    const float* bs;  // [B,Cb] or null
    int B, Hs, Ws, Hb, Wb, Cs, Cb, KH, KW, pad;
    int tiles_x, tiles_y, ntiles;
    const void* zero;
};

constexpr int kHwPatchHalfs = 256 * 32;        // gy patch: 16 x 16 pixels x 32 channels
constexpr int kHwHaloHalfs = 5376 * 2;         // x patch + halo: 18 x 18 pixels x 32 channels, rounded up to whole DMA pieces
constexpr int kHwBufHalfs = kHwPatchHalfs + kHwHaloHalfs;

// TR: operand fragments by two transposing LDS reads (ds_read_b64_tr_b16, gfx950) instead of eight 16-bit reads.  Semantics
// (tools/probes/tr16_probe.hip): inside a 16-lane group, lane s supplies the address of an 8-byte chunk and receives element
// s % 4 of the chunks of lanes 4 j + s / 4, j = 0..3.  Lane L of the group that owns channels 16 g .. 16 g + 15 therefore
// supplies pixel k0 + L / 4, channels 16 g + 4 (L % 4) .. + 3, and lane s gets channel 16 g + s at pixels k0 .. k0 + 3.
typedef __fp16 tr_h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ gif::f16x8_t halo_frag_tr(const gif::f16* base_lo) {
    // base_lo: this lane's chunk of the first four pixels; the next four pixels are 4 * 32 halfs further
    typedef __attribute__((address_space(3))) tr_h4* lp_t;
    const tr_h4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp_t)(base_lo));
    const tr_h4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lp_t)(base_lo + 4 * 32));
    gif::f16x8_t v;
    v[0] = (gif::f16)lo[0]; v[1] = (gif::f16)lo[1]; v[2] = (gif::f16)lo[2]; v[3] = (gif::f16)lo[3];
    v[4] = (gif::f16)hi[0]; v[5] = (gif::f16)hi[1]; v[6] = (gif::f16)hi[2]; v[7] = (gif::f16)hi[3];
    return v;
}

template <bool TR>
__global__ void __launch_bounds__(256, 2) conv_wgrad_halo_f16(const HaloWgradParams p) {
    typedef gif::f16 T;
    extern __shared__ __attribute__((aligned(16))) float hw_smem[];
    T* const lds = reinterpret_cast<T*>(hw_smem);  // [2][kHwBufHalfs]
    const T* const smb = static_cast<const T*>(p.sm);
    const T* const bgb = static_cast<const T*>(p.bg);
    const T* const pzero = static_cast<const T*>(p.zero);
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int tpi = p.tiles_x * p.tiles_y;
    const int HWh = 16 + p.KW - 1;
    const int nchunks_x = (16 + p.KH - 1) * HWh * 4;
    const int T9 = p.KH * p.KW;

    // chunk e = 64 * wave + lane + 256 * pass: channel chunk e % 4 is the same in every pass, the pixel advances by 64
    const int c8 = (lane & 3) * 8;
    const int q_first = (wave * 64 + lane) >> 2;
    const int hy_first = q_first / HWh, hx_first = q_first - hy_first * HWh;
    const int dqy = 64 / HWh, dqx = 64 - dqy * HWh;
    auto issue_patch = [&](int tile, T* buf) __attribute__((always_inline)) {
        const int b = tile / tpi, tr = tile - b * tpi;
        const int ty = tr / p.tiles_x, tx = tr - ty * p.tiles_x;
        const int oy0 = ty * 16, ox0 = tx * 16;
        {   // gy patch: pixel q = 16 * ly + lx
            const T* const gb = smb + (size_t)b * p.Hs * p.Ws * p.Cs;
            int q = q_first;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int gy = oy0 + (q >> 4), gx = ox0 + (q & 15);
                const bool ok = gy < p.Hs && gx < p.Ws && c8 < p.Cs;
                const T* g = ok ? gb + ((gy * p.Ws + gx) * p.Cs + c8) : pzero;
                __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(buf + (it * 256 + wave * 64) * 8), 16, 0, 0);
                q += 64;
            }
        }
        {   // x patch + halo: rows / columns shifted by -pad
            const T* const xb = bgb + (size_t)b * p.Hb * p.Wb * p.Cb;
            const int gy0 = oy0 - p.pad, gx0 = ox0 - p.pad;
            int hy = hy_first, hx = hx_first;
            T* const xbuf = buf + kHwPatchHalfs;
            for (int e0 = wave * 64; e0 < nchunks_x; e0 += 256) {  // wave-uniform
                const int gy = gy0 + hy, gx = gx0 + hx;
                const bool ok = e0 + lane < nchunks_x && (unsigned)gy < (unsigned)p.Hb && (unsigned)gx < (unsigned)p.Wb && c8 < p.Cb;
                const T* g = ok ? xb + ((gy * p.Wb + gx) * p.Cb + c8) : pzero;
                __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(xbuf + e0 * 8), 16, 0, 0);
                hx += dqx; hy += dqy;
                if (hx >= HWh) { hx -= HWh; ++hy; }
            }
        }
    };
    auto load_scales = [&](int tile, float& sa, float& sb) __attribute__((always_inline)) {
        const int b = tile / tpi;
        sa = (p.ss && li < p.Cs) ? p.ss[(size_t)b * p.Cs + li] : 1.f;
        sb = (p.bs && li < p.Cb) ? p.bs[(size_t)b * p.Cb + li] : 1.f;
    };
    const bool scaled = p.ss != nullptr || p.bs != nullptr;
    // transposing reads: lane L = lane % 16 of channel group g = (lane >> 4) & 1 supplies pixel L / 4, channels 16 g + 4 (L % 4)
    const int tr_px = (lane & 15) >> 2, tr_ch = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int stride = (int)gridDim.x;
    int tile = xcd_remap((int)blockIdx.x, stride);
    float sa = 1.f, sb = 1.f, sa_n = 1.f, sb_n = 1.f;
    if (tile < p.ntiles) {
        issue_patch(tile, lds);
        if (scaled) load_scales(tile, sa, sb);
    }
    int cur = 0;
    for (; tile < p.ntiles; tile += stride) {
        __syncthreads();  // patch `tile` landed (vmcnt(0) of every wave); everybody is done reading the other buffer
        const int next = tile + stride;
        if (next < p.ntiles) {
            issue_patch(next, lds + (cur ^ 1) * kHwBufHalfs);
            if (scaled) load_scales(next, sa_n, sb_n);
        }
        const T* const G = lds + cur * kHwBufHalfs;      // [256 px][32]
        const T* const X = G + kHwPatchHalfs;             // [halo px][32]
        const T fa = (T)sa, fb = (T)sb;
#pragma unroll 1
        for (int row = wave; row < 16; row += 4) {  // K step = one patch row: pixels 16 * row + 8 * lh + 0..7
            gif::f16x8_t af;
            if constexpr (TR) {
                af = halo_frag_tr(G + (row * 16 + 8 * lh + tr_px) * 32 + tr_ch);
            } else {
                const T* ga = G + (row * 16 + 8 * lh) * 32 + li;
#pragma unroll
                for (int e = 0; e < 8; ++e) af[e] = ga[e * 32];
            }
            if (scaled) af *= fa;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (t < T9) {  // wave-uniform
                    const int ky = t / p.KW, kx = t - ky * p.KW;
                    gif::f16x8_t bf;
                    if constexpr (TR) {
                        bf = halo_frag_tr(X + ((row + ky) * HWh + 8 * lh + kx + tr_px) * 32 + tr_ch);
                    } else {
                        const T* xa = X + ((row + ky) * HWh + 8 * lh + kx) * 32 + li;
#pragma unroll
                        for (int e = 0; e < 8; ++e) bf[e] = xa[e * 32];
                    }
                    if (scaled) bf *= fb;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc[t], 0, 0, 0);
                }
            }
        }
        sa = sa_n; sb = sb_n;
        cur ^= 1;
    }
    // ---- fixed-order reduction of the four waves' accumulators through LDS (the patch buffers are free), then ONE split
    __syncthreads();
    float* const red = hw_smem;  // [2][9][1024] floats = 72 KB <= the two patch buffers (75.8 KB)
    for (int h = 2; h >= 1; h >>= 1) {
        if (wave >= h && wave < 2 * h) {
            float* dst = red + (size_t)(wave - h) * 9 * 1024;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * 64 + lane] = acc[t][r];
        }
        __syncthreads();
        if (wave < h) {
            const float* src = red + (size_t)wave * 9 * 1024;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] += src[(t * 16 + r) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        // C/D layout of the 32x32 MFMA: column (cin) = lane & 31, row (cout) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        float* out = p.ws + (size_t)blockIdx.x * T9 * 1024;
#pragma unroll
        for (int t = 0; t < 9; ++t)
            if (t < T9) {
#pragma unroll
                for (int r = 0; r < 16; ++r) out[(t * 32 + gif::acc_row(r, lh)) * 32 + li] = acc[t][r];
            }
    }
}

// Winograd F(3x3,2x2) output transform fused with the split reduction: dW = A'^T dU A' with
// A'^T = [1 1 1 0; 0 1 -1 0; 0 1 1 -1] (the F(3,2) matrix with the sign of the input transform's last row folded in,
// because V was produced by the F(2,3) input transform whose last row is the negative of F(3,2)'s).
__global__ void wino_unpack_wgrad_kernel(const float* __restrict__ ws, float* __restrict__ dw, int nsplit, int R, int C,
                                         int RP, int CP, long sr, long sc, long sky, long skx, float scale) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)R * C) return;
    int c = (int)(idx % C), r = (int)(idx / C);
    const size_t plane = (size_t)RP * CP, stride = 16 * plane;
    const float* src = ws + (size_t)r * CP + c;
    float u[4][4];
#pragma unroll
    for (int q = 0; q < 16; ++q) u[q >> 2][q & 3] = 0.f;
    int s = 0;
    for (; s + 2 <= nsplit; s += 2) {  // 32 independent loads in flight; splits summed in a fixed order
        const float* sp = src + (size_t)s * stride;
        float t0[16], t1[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) { t0[q] = sp[q * plane]; t1[q] = sp[stride + q * plane]; }
#pragma unroll
        for (int q = 0; q < 16; ++q) u[q >> 2][q & 3] += t0[q] + t1[q];
    }
    if (s < nsplit) {
        const float* sp = src + (size_t)s * stride;
#pragma unroll
        for (int q = 0; q < 16; ++q) u[q >> 2][q & 3] += sp[q * plane];
    }
    float t[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[0][j] = u[0][j] + u[1][j] + u[2][j];
        t[1][j] = u[1][j] - u[2][j];
        t[2][j] = u[1][j] + u[2][j] - u[3][j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float* o = dw + r * sr + c * sc + i * sky;
        o[0 * skx] = scale * (t[i][0] + t[i][1] + t[i][2]);
        o[1 * skx] = scale * (t[i][1] - t[i][2]);
        o[2 * skx] = scale * (t[i][1] + t[i][2] - t[i][3]);
    }
}

// ---- host side: knobs -> route (wgrad_route.h) -> launch ---------------------------------------------------------------------------
// The GIF_* variables of wgrad_route.h, read once per process — except GIF_CONV_VARIANT, which probe scripts set in-process: every call.
route::WgradKnobs wgrad_knobs() {
    static const route::WgradKnobs once = [] {
        route::WgradKnobs k;
        const auto num = gif::knob_int;
        k.x3_wgrad_thin = num("GIF_X3_WGRAD_THIN", k.x3_wgrad_thin);
        k.x3_wgrad_simple = num("GIF_X3_WGRAD_SIMPLE", 0) != 0;
        k.h2_wgrad_plain_tab = num("GIF_H2_WGRAD_PLAIN_TAB", 1) != 0;
        k.h2_wgrad_v2 = num("GIF_H2_WGRAD_V2", 1) != 0;
        k.h2_wgrad_taps = num("GIF_H2_WGRAD_TAPS", 1) != 0;
        k.wgrad_big = num("GIF_WGRAD_BIG", 1) != 0;
        k.small_wgrad = num("GIF_SMALL_WGRAD", 1) != 0;
        k.f16_wgrad256 = num("GIF_F16_WGRAD256", 1) != 0;
        k.f16_halo_wgrad = num("GIF_F16_HALO_WGRAD", 1) != 0;
        k.f16_halo_wgrad_tr = num("GIF_F16_HALO_WGRAD_TR", 1) != 0;
        return k;
    }();
    route::WgradKnobs k = once;
    const char* variant = gif::knob("GIF_CONV_VARIANT");
    k.conv_variant_set = variant != nullptr;
    k.conv_variant = variant ? atoi(variant) : 0;
    return k;
}

route::WgradShape wgrad_shape(const gif_conv_geom* g, bool scaled) {
    return route::WgradShape{g->B, g->Hb, g->Wb, g->Cb, g->Hs, g->Ws, g->Cs, g->KH, g->KW, g->stride, g->pad, scaled, false};
}

// launches conv_wgrad_mfma<T, ...> iff `l` names exactly this instantiation
template <typename T, int BP, int BQ, int WP, int WQ, bool GLDS, int BKP, bool TAB = false, int X3 = 0>
bool wgrad_try(const route::WgradLaunch& l, dim3 grid, hipStream_t s, const WgradParams& p) {
    if (l.f16 != (sizeof(T) == 2) || l.BP != BP || l.BQ != BQ || l.WP != WP || l.WQ != WQ || l.GLDS != GLDS || l.BKP != BKP || l.TAB != TAB ||
        l.X3 != X3)
        return false;
    wgrad_launch<T, BP, BQ, WP, WQ, GLDS, BKP, TAB, X3>(grid, l.threads, s, p);
    return true;
}

// One tiled launch of a route.  The ladder below is the complete list of conv_wgrad_mfma instantiations the library carries.
int wgrad_launch_one(const route::WgradLaunch& l, int nsplit, hipStream_t s, const WgradParams& p0) {
    WgradParams p = p0;
    if (l.unit_tab) p.stab_nb = 1;
    p.tpt = l.tpt; p.tgroups = l.tgroups;
    const dim3 grid((unsigned)(l.wgs_per_split * nsplit));
    if (l.kernel == route::WGRAD_H2V2) {
        wgrad_launch_v2(l.TAB, grid, s, p, l.TAPS);
        return 0;
    }
    using gif::f16;
    const bool launched =
        l.kernel == route::WGRAD_MFMA &&
        // f16x2 (per-wave split; the default is conv_wgrad_h2v2)
        (wgrad_try<float, 128, 32, 2, 1, true, 32, false, 2>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 32, true, 2>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 32, false, 2>(l, grid, s, p) ||
         // bf16x3
         wgrad_try<float, 128, 32, 4, 1, true, 32, false, 1>(l, grid, s, p) ||
         wgrad_try<float, 128, 32, 2, 1, true, 32, false, 1>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 32, true, 1>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 16, true, 1>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 32, false, 1>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 16, false, 1>(l, grid, s, p) ||
         // native fp32 MFMA
         wgrad_try<float, 256, 128, 2, 2, true, 16>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 16, true>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 16>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, true, 32>(l, grid, s, p) ||
         wgrad_try<float, 128, 128, 2, 2, false, 32>(l, grid, s, p) ||
         wgrad_try<float, 128, 32, 4, 1, true, 32>(l, grid, s, p) ||
         wgrad_try<float, 128, 32, 4, 1, false, 32>(l, grid, s, p) ||
         wgrad_try<float, 32, 128, 1, 4, true, 32>(l, grid, s, p) ||
         wgrad_try<float, 32, 128, 1, 4, false, 32>(l, grid, s, p) ||
         wgrad_try<float, 32, 32, 1, 1, true, 32>(l, grid, s, p) ||
         wgrad_try<float, 32, 32, 1, 1, false, 32>(l, grid, s, p) ||
         // f16 operands
         wgrad_try<f16, 256, 256, 2, 4, true, 32>(l, grid, s, p) ||
         wgrad_try<f16, 256, 256, 2, 4, true, 32, true>(l, grid, s, p) ||
         wgrad_try<f16, 128, 128, 2, 2, true, 32>(l, grid, s, p) ||
         wgrad_try<f16, 128, 128, 2, 2, true, 32, true>(l, grid, s, p) ||
         wgrad_try<f16, 128, 128, 2, 2, true, 16, true>(l, grid, s, p) ||
         wgrad_try<f16, 64, 64, 2, 2, true, 32>(l, grid, s, p) ||
         wgrad_try<f16, 64, 64, 2, 2, true, 32, true>(l, grid, s, p) ||
         wgrad_try<f16, 32, 32, 1, 1, true, 32>(l, grid, s, p) ||
         wgrad_try<f16, 32, 32, 1, 1, true, 32, true>(l, grid, s, p) ||
         wgrad_try<f16, 32, 32, 1, 1, true, 16, true>(l, grid, s, p));
    GIF_REQUIRE(launched, "conv2d_wgrad: the route names a kernel that is not built (%s %dx%d waves %dx%d glds %d stage %d tab %d x3 %d)",
                l.f16 ? "f16" : "f32", l.BP, l.BQ, l.WP, l.WQ, (int)l.GLDS, l.BKP, (int)l.TAB, l.X3);
    return 0;
}

// The tiled launches of a route: the primary one and, for an f16x2 route, its guarded bf16x3 twin (a no-op unless the primary raised
// the gate; not launched at all when the guard is switched off).  `p` carries everything but the per-launch fields.
int wgrad_dispatch(const route::WgradRoute& r, int nsplit, hipStream_t s, WgradParams p) {
    if (r.has_twin) {
        const gif::H2Gate gt = gif::h2_next_gate(s);
        if (gt.err) return gt.err;
        p.gate = gt.word; p.gate_gen = gt.gen; p.h2_stats = gif::h2_stats_words();
    }
    if (int rc = wgrad_launch_one(r.primary, nsplit, s, p)) return rc;
    if (r.has_twin && p.gate) return wgrad_launch_one(r.twin, nsplit, s, p);  // (no gate: GIF_H2_GUARD=0, unguarded)
    return 0;
}

// The f16x2 packings, one launch each: header and planes behind wp2; wp3 != NULL: the bf16x3 packing of the same weights as well;
// steps > 0: the tap-dense K order (`steps` K steps of CP = 32 floats, cpt 16-byte chunks per tap) instead of KH * KW taps of CP channels.
// The entry points have validated their arguments.
int pack_h2(const char* who, const float* w, void* wp2, void* wp3, int R, int C, int KH, int KW, int RP, int CP, int64_t sr, int64_t sc,
            int64_t sky, int64_t skx, float scale, int cpt, int steps, gif_stream_t stream) {
    int* hdr = static_cast<int*>(wp2);
    unsigned short* planes = reinterpret_cast<unsigned short*>(static_cast<char*>(wp2) + gif::h2_header_bytes(RP));
    const int T = steps ? steps : KH * KW;
    const size_t lds = (size_t)T * CP * sizeof(float);  // (tap-dense: <= 8 steps of 32 floats, always fits)
    GIF_REQUIRE(lds <= 64 * 1024, "%s: a row of %d x %d values does not fit the staging LDS", who, T, CP);
    pack_weight_h2_kernel<<<RP, 256, lds, gif::as_stream(stream)>>>(w, hdr, planes, static_cast<unsigned short*>(wp3), R, C, KH, KW, RP, CP, sr,
                                                                    sc, sky, skx, scale, cpt, steps);
    return gif::check_launch(who);
}

// everything of WgradParams but the per-launch fields (wgrad_dispatch, wgrad_launch_one), from the geometry, the route and the pointers
WgradParams wgrad_params(const route::WgradShape& g, const route::WgradRoute& r, const void* small, const void* big, float* ws,
                         const float* small_scale, const float* big_scale, const void* zero) {
    WgradParams p{};
    p.sm = small; p.bg = big; p.ws = ws; p.ss = small_scale; p.bs = big_scale;
    p.B = g.B; p.Hs = g.Hs; p.Ws = g.Ws; p.Cs = g.Cs; p.Hb = g.Hb; p.Wb = g.Wb; p.Cb = g.Cb;
    p.KW = g.KW; p.stride = g.stride; p.pad = g.pad; p.T = g.KH * g.KW;
    p.RP = r.RP; p.CP = r.CP; p.Ntot = route::wgrad_ntot(g); p.chunk = r.chunk;
    p.tiles_q = r.tiles_q; p.tiles_pq = r.tiles_pq; p.stab_nb = r.stab_nb; p.zero = zero;
    return p;
}

// The direct weight gradient behind gif_conv2d_wgrad_f32 / _f32x3 / _f32h2 (T = float; mode: 0 native fp32 MFMA, 1 bf16x3, 2 f16x2 with
// the guarded bf16x3 fallback — launch shapes f16x2 is not built for run bf16x3) and gif_conv2d_wgrad_f16 (T = f16: square tiles on the
// LDS-DMA kernel, wgrad_route_f16; fp32 partial sums, the same unpack kernel; mode unused).
template <typename T>
int conv2d_wgrad_impl(const void* small, const void* big, float* ws, const float* small_scale, const float* big_scale, const gif_conv_geom* g,
                      int nsplit, gif_stream_t stream, int mode) {
    constexpr bool F16 = sizeof(T) == 2;
    constexpr int CMULT = F16 ? 8 : 4;  // channels per 16-byte DMA chunk
    const char* const who = F16 ? "conv2d_wgrad_f16" : "conv2d_wgrad";
    GIF_REQUIRE(g && small && big && ws && nsplit >= 1, "%s: bad arguments", who);
    GIF_REQUIRE(g->Cb % CMULT == 0 && g->Cs % CMULT == 0, "%s: channels must be multiples of %d", who, CMULT);
    GIF_REQUIRE(g->KH >= 1 && g->KH <= 3 && g->KW >= 1 && g->KW <= 3 && (g->stride == 1 || g->stride == 2), "%s: unsupported kernel/stride", who);
    GIF_REQUIRE((long)g->B * g->Hs * g->Ws * g->Cs < (1L << 31) && (long)g->B * g->Hb * g->Wb * g->Cb < (1L << 31),
                "%s: tensors of >= 2^31 elements are not supported (32-bit offsets)", who);
    const bool scaled = small_scale || big_scale;
    const route::WgradShape sh = wgrad_shape(g, scaled);
    const route::WgradRoute r = F16 ? route::wgrad_route_f16(sh, nsplit, wgrad_knobs()) : route::wgrad_route(sh, mode, nsplit, wgrad_knobs());
    hipStream_t s = gif::as_stream(stream);
    const int T9 = g->KH * g->KW;
    const long Ntot = route::wgrad_ntot(sh);
    const double flops = 2.0 * Ntot * (double)g->Cs * g->Cb * T9;
    const void* zero = gif::zero_page16();
    GIF_REQUIRE(zero, "%s: zero page lookup failed", who);
    gif::ProfScope prof(r.family, flops, s, (int)Ntot, g->Cs, g->Cb, T9 * 10 + g->stride + (scaled ? 100 : 0));
    const dim3 grid((unsigned)(r.primary.wgs_per_split * nsplit)), block(r.primary.threads);
    // the two kernels outside the tiled ladder: each exists for one element type only
    if constexpr (F16) {
        if (r.primary.kernel == route::WGRAD_HALO) {
            HaloWgradParams q{};
            q.sm = small; q.bg = big; q.ws = ws; q.ss = small_scale; q.bs = big_scale;
            q.B = g->B; q.Hs = g->Hs; q.Ws = g->Ws; q.Hb = g->Hb; q.Wb = g->Wb; q.Cs = g->Cs; q.Cb = g->Cb;
            q.KH = g->KH; q.KW = g->KW; q.pad = g->pad;
            q.tiles_x = gif::cdiv(g->Ws, 16); q.tiles_y = gif::cdiv(g->Hs, 16); q.ntiles = g->B * q.tiles_x * q.tiles_y;
            q.zero = zero;
            const size_t lds = (size_t)2 * kHwBufHalfs * sizeof(gif::f16);
            static gif::LdsAttr attr, attr_tr;
            if (!r.primary.TR) gif::launch_lds(conv_wgrad_halo_f16<false>, attr, grid, block, lds, s, q);
            else gif::launch_lds(conv_wgrad_halo_f16<true>, attr_tr, grid, block, lds, s, q);
            return gif::check_launch("conv2d_wgrad_f16(halo)");
        }
    } else {
        if (r.primary.kernel == route::WGRAD_SMALL) {
            SmallWgradParams q{};
            q.sm = static_cast<const float*>(small); q.bg = static_cast<const float*>(big); q.ws = ws;
            q.B = g->B; q.H = g->Hs; q.W = g->Ws; q.Cs = g->Cs; q.Cb = g->Cb; q.RP = r.RP; q.CP = r.CP;
            q.Ntot = Ntot; q.chunk = r.chunk;
            static gif::LdsAttr attr;
            gif::launch_lds(conv_wgrad_small_mfma, attr, grid, block, (size_t)8 * 18 * 256 * sizeof(float), s, q);
            return gif::check_launch("conv2d_wgrad(small)");
        }
    }
    const WgradParams p = wgrad_params(sh, r, small, big, ws, small_scale, big_scale, zero);
    if constexpr (F16) {
        if (scaled) {
            // the scale table is indexed per stage: a stage must not straddle two samples
            const long HWs = (long)g->Hs * g->Ws;
            GIF_REQUIRE((size_t)r.stab_nb * 2 * r.tile_f16 * sizeof(float) <= 64 * 1024, "conv2d_wgrad_f16: scale table too large");
            GIF_REQUIRE(HWs % 16 == 0, "conv2d_wgrad_f16: modulated weight gradient needs Hs*Ws %% 16 == 0 (got %ld)", HWs);
        }
    }
    if (int rc = wgrad_dispatch(r, nsplit, s, p)) return rc;
    return gif::check_launch(who);
}

}  // namespace

extern "C" {

/* f16x2 packing: [RP int32 row exponents][RP int32 row flags][tap][2][RP][CP] f16 — gif_pack_weight_f32h2_bytes of device memory */
int64_t gif_pack_weight_f32h2_bytes(int KH, int KW, int RP, int CP) {
    if (KH <= 0 || KW <= 0 || RP <= 0 || CP <= 0) return 0;
    return (int64_t)gif::h2_header_bytes(RP) + (int64_t)KH * KW * 2 * RP * CP * 2;
}

int gif_pack_weight_f32h2(const float* w, void* wp2, int R, int C, int KH, int KW, int RP, int CP, int64_t sr, int64_t sc,
                          int64_t sky, int64_t skx, float scale, gif_stream_t stream) {
    GIF_REQUIRE(w && wp2 && R > 0 && C > 0 && RP >= R && CP >= C && KH > 0 && KW > 0 && RP % 32 == 0 && CP % 32 == 0,
                "pack_weight_f32h2: bad arguments");
    return pack_h2("pack_weight_f32h2", w, wp2, nullptr, R, C, KH, KW, RP, CP, sr, sc, sky, skx, scale, 0, 0, stream);
}

/* both packings of the same weights in ONE launch: wp2 (f16x2, as gif_pack_weight_f32h2) and wp3 (bf16x3, as gif_pack_weight_f32x3) */
int gif_pack_weight_f32h2x3(const float* w, void* wp2, void* wp3, int R, int C, int KH, int KW, int RP, int CP, int64_t sr, int64_t sc,
                            int64_t sky, int64_t skx, float scale, gif_stream_t stream) {
    GIF_REQUIRE(w && wp2 && wp3 && R > 0 && C > 0 && RP >= R && CP >= C && KH > 0 && KW > 0 && RP % 32 == 0 && CP % 32 == 0,
                "pack_weight_f32h2x3: bad arguments");
    return pack_h2("pack_weight_f32h2x3", w, wp2, wp3, R, C, KH, KW, RP, CP, sr, sc, sky, skx, scale, 0, 0, stream);
}

/* tap-dense K order (gif_conv2d_x3_tapdense_steps): wp2 = [2 RP int32 header][steps][2][RP][32] f16, wp3 = [steps][3][RP][32] bf16 (as
 * gif_pack_weight_f32x3_tapdense writes it), one launch */
int64_t gif_pack_weight_f32h2_tapdense_bytes(int cin_act, int KH, int KW, int RP) {
    const int steps = gif_conv2d_x3_tapdense_steps(cin_act, KH, KW);
    if (steps <= 0 || RP <= 0) return 0;
    return (int64_t)gif::h2_header_bytes(RP) + (int64_t)steps * 2 * RP * 32 * 2;
}

int gif_pack_weight_f32h2x3_tapdense(const float* w, void* wp2, void* wp3, int R, int C, int cin_act, int KH, int KW, int RP, int64_t sr,
                                     int64_t sc, int64_t sky, int64_t skx, float scale, gif_stream_t stream) {
    const int steps = gif_conv2d_x3_tapdense_steps(cin_act, KH, KW);
    GIF_REQUIRE(w && wp2 && wp3 && R > 0 && C > 0 && RP >= R && RP % 32 == 0 && cin_act >= C && steps > 0,
                "pack_weight_f32h2x3_tapdense: bad arguments");
    return pack_h2("pack_weight_f32h2x3_tapdense", w, wp2, wp3, R, C, KH, KW, RP, 32, sr, sc, sky, skx, scale, cin_act / 4, steps, stream);
}

/* ---- f16 operands (BASELINE config 5): square tiles on the LDS-DMA kernel (wgrad_route.h: wgrad_route_f16), fp32 partial sums, the
 * same unpack kernel. */
int gif_conv2d_wgrad_dims_f16(int Cs, int Cb, int* RP, int* CP) {
    GIF_REQUIRE(Cs > 0 && Cb > 0 && RP && CP, "wgrad_dims_f16: bad arguments");
    route::wgrad_dims_f16(Cs, Cb, RP, CP);
    return 0;
}

int gif_conv2d_wgrad_splits_f16(const gif_conv_geom* g) {
    if (!g || g->B <= 0) return 1;
    return route::wgrad_splits_f16(wgrad_shape(g, false), wgrad_knobs());
}

int gif_conv2d_wgrad_f16(const void* small, const void* big, float* ws, const float* small_scale, const float* big_scale,
                         const gif_conv_geom* g, int nsplit, gif_stream_t stream) {
    return conv2d_wgrad_impl<gif::f16>(small, big, ws, small_scale, big_scale, g, nsplit, stream, 0);
}

int gif_conv2d_wgrad_dims(int Cs, int Cb, int* RP, int* CP) {
    GIF_REQUIRE(Cs > 0 && Cb > 0 && RP && CP, "wgrad_dims: bad arguments");
    route::wgrad_dims(Cs, Cb, RP, CP);
    return 0;
}

// The count follows the kernel a later call is expected to launch under the PROCESS's contraction mode (wgrad_tiles_per_split takes the
// mode as a parameter: a caller that knows the mode of the call it sizes can be given a way to say so).
int gif_conv2d_wgrad_splits(const gif_conv_geom* g) {
    if (!g || g->B <= 0) return 1;
    const route::WgradShape sh = wgrad_shape(g, false);
    const route::WgradKnobs k = wgrad_knobs();
    const int mode = gif::fp32_mfma_mode();
    return route::wgrad_splits(sh, mode, k);
}

int gif_conv2d_wgrad_f32(const float* small, const float* big, float* ws, const float* small_scale,
                         const float* big_scale, const gif_conv_geom* g, int nsplit, gif_stream_t stream) {
    return conv2d_wgrad_impl<float>(small, big, ws, small_scale, big_scale, g, nsplit, stream, 0);
}

int gif_conv2d_wgrad_f32x3(const float* small, const float* big, float* ws, const float* small_scale,
                           const float* big_scale, const gif_conv_geom* g, int nsplit, gif_stream_t stream) {
    return conv2d_wgrad_impl<float>(small, big, ws, small_scale, big_scale, g, nsplit, stream, 1);
}

/* f16x2 (ABI 4): same contract; the f16x2 launch is followed by its guarded bf16x3 twin (a no-op unless the gate was raised) */
int gif_conv2d_wgrad_f32h2(const float* small, const float* big, float* ws, const float* small_scale,
                           const float* big_scale, const gif_conv_geom* g, int nsplit, gif_stream_t stream) {
    return conv2d_wgrad_impl<float>(small, big, ws, small_scale, big_scale, g, nsplit, stream, 2);
}

int gif_unpack_wgrad_f32(const float* ws, float* dw, int nsplit, int R, int C, int KH, int KW, int RP, int CP,
                         int64_t sr, int64_t sc, int64_t sky, int64_t skx, float scale, gif_stream_t stream) {
    GIF_REQUIRE(ws && dw && nsplit >= 1 && R > 0 && C > 0 && RP >= R && CP >= C, "unpack_wgrad: bad arguments");
    long total = (long)KH * KW * R * C;
    unpack_wgrad_kernel<<<gif::cdiv(total, 256), 256, 0, gif::as_stream(stream)>>>(ws, dw, nsplit, R, C, KH, KW, RP,
                                                                                     CP, sr, sc, sky, skx, scale);
    return gif::check_launch("unpack_wgrad");
}

/* ---- Winograd F(3x3,2x2) weight gradient of the stride-1 / pad-1 3x3 convolution -------------------------------------
 * dU_q[o][i] = sum_tiles Mg_q[tile][o] * V_q[tile][i] for the 16 transform positions q (a 1x1 wgrad per plane, run by
 * conv_wgrad_mfma in "planes" mode), then dW = A'^T dU A' in the unpack kernel: 16 instead of 36 multiplies per tile. */
int gif_conv3x3_winograd_wgrad_splits(int B, int H, int W, int Cs, int Cb) {
    if (B <= 0 || H <= 0 || W <= 0 || Cs <= 0 || Cb <= 0) return 1;
    const route::WgradShape planes{B, H / 2, W / 2, Cb, H / 2, W / 2, Cs, 1, 1, 1, 0, false, true};
    return route::wgrad_splits(planes, gif::fp32_mfma_mode(), wgrad_knobs());  // (the plane GEMMs' count does not depend on the mode)
}

static int conv3x3_winograd_wgrad_impl(const float* x, const float* gy, float* V, float* Mg, float* ws,
                                       const float* small_scale, const float* big_scale, int B, int H, int W, int Cs, int Cb,
                                       int nsplit, gif_stream_t stream, int mode) {
    GIF_REQUIRE(gy && V && Mg && ws && nsplit >= 1, "winograd_wgrad: bad arguments");  // x == NULL: V is already filled
    GIF_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "winograd_wgrad: bad dims (H, W must be even)");
    GIF_REQUIRE(Cs > 0 && Cb > 0 && Cs % 4 == 0 && Cb % 4 == 0, "winograd_wgrad: channels must be multiples of 4");
    hipStream_t s = gif::as_stream(stream);
    const long ntiles = (long)B * (H / 2) * (W / 2);
    const int CsP = gif_wino::padded_channels(Cs), CbP = gif_wino::padded_channels(Cb);
    const long ntiles_pad = gif_wino::padded_tiles(ntiles);
    GIF_REQUIRE(gif_wino::fits_i32(ntiles_pad * CsP) && gif_wino::fits_i32(ntiles_pad * CbP), "winograd_wgrad: tensor too large for 32-bit offsets");
    double flops = 2.0 * B * H * W * 9.0 * Cs * Cb;  // ALGORITHMIC (direct) FLOPs
    {
        gif::ProfScope prof_t(4, 4.0 * ((double)B * H * W * ((x ? Cb : 0) + Cs) + 16.0 * ntiles_pad * ((x ? CbP : 0) + CsP)), s,
                              (int)((long)B * H * W), Cb, Cs, 2);
        if (x)  // else: the caller kept the forward pass's V (same x, same modulation)
            if (int rc = gif::winograd_input_transform(x, big_scale, V, B, H, W, Cb, s)) return rc;
        if (int rc = gif::winograd_gy_transform(gy, small_scale, Mg, B, H, W, Cs, s)) return rc;
    }
    // one "image" of 1 x ntiles pixels per plane, 1x1 taps; the transforms have applied the per-sample scales
    const route::WgradShape planes{1, 1, (int)ntiles, CbP, 1, (int)ntiles, CsP, 1, 1, 1, 0, false, true};
    const route::WgradRoute r = route::wgrad_route(planes, mode, nsplit, wgrad_knobs());
    gif::ProfScope prof(r.family, flops, s, (int)((long)B * H * W), Cs, Cb, 1091 + (small_scale || big_scale ? 100 : 0));
    const void* zero = gif::zero_page16();
    GIF_REQUIRE(zero, "winograd_wgrad: zero page lookup failed");
    WgradParams p = wgrad_params(planes, r, Mg, V, ws, nullptr, nullptr, zero);
    p.T = 16;
    p.sm_plane = ntiles_pad * CsP;
    p.bg_plane = ntiles_pad * CbP;
    if (int rc = wgrad_dispatch(r, nsplit, s, p)) return rc;
    return gif::check_launch("conv3x3_winograd_wgrad");
}

int gif_conv3x3_winograd_wgrad_f32(const float* x, const float* gy, float* V, float* Mg, float* ws,
                                   const float* small_scale, const float* big_scale, int B, int H, int W, int Cs, int Cb,
                                   int nsplit, gif_stream_t stream) {
    return conv3x3_winograd_wgrad_impl(x, gy, V, Mg, ws, small_scale, big_scale, B, H, W, Cs, Cb, nsplit, stream, 0);
}

int gif_conv3x3_winograd_wgrad_f32x3(const float* x, const float* gy, float* V, float* Mg, float* ws,
                                     const float* small_scale, const float* big_scale, int B, int H, int W, int Cs, int Cb,
                                     int nsplit, gif_stream_t stream) {
    return conv3x3_winograd_wgrad_impl(x, gy, V, Mg, ws, small_scale, big_scale, B, H, W, Cs, Cb, nsplit, stream, 1);
}

int gif_conv3x3_winograd_wgrad_f32h2(const float* x, const float* gy, float* V, float* Mg, float* ws,
                                     const float* small_scale, const float* big_scale, int B, int H, int W, int Cs, int Cb,
                                     int nsplit, gif_stream_t stream) {
    return conv3x3_winograd_wgrad_impl(x, gy, V, Mg, ws, small_scale, big_scale, B, H, W, Cs, Cb, nsplit, stream, 2);
}

int gif_winograd_unpack_wgrad_f32(const float* ws, float* dw, int nsplit, int R, int C, int RP, int CP, int64_t sr,
                                  int64_t sc, int64_t sky, int64_t skx, float scale, gif_stream_t stream) {
    GIF_REQUIRE(ws && dw && nsplit >= 1 && R > 0 && C > 0 && RP >= R && CP >= C, "winograd_unpack_wgrad: bad arguments");
    long total = (long)R * C;
    wino_unpack_wgrad_kernel<<<gif::cdiv(total, 256), 256, 0, gif::as_stream(stream)>>>(ws, dw, nsplit, R, C, RP, CP, sr,
                                                                                          sc, sky, skx, scale);
    return gif::check_launch("winograd_unpack_wgrad");
}
}
