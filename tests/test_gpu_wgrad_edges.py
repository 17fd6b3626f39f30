"""-m gpu: the weight-gradient kernels of csrc/conv_wgrad.hip (conv_wgrad_mfma, conv_wgrad_h2v2, conv_wgrad_small_mfma,
conv_wgrad_halo_f16, unpack_wgrad_kernel) at the edges of their own index arithmetic, against an fp64 reference.

tests/test_gpu_conv_routes.py puts rows on the predicates of csrc/wgrad_route.h; the model-shaped tests run square maps with the
library's split count under a max-normalised error.  Here each row is computed from one expression INSIDE the kernels, and the row
chooses the split count (nsplit = None: the library's query), which ops.conv_wgrad cannot do: the C entry points are called directly
(gif_conv2d_wgrad_f32 / _f32x3 / _f32h2 / _f16, then gif_unpack_wgrad_f32).

Table of edges (sections of ROWS; each row's comment names the expression and the side):
  1 chunks   n_begin = split * chunk, n_end clamped to Ntot, `for (n0 = n_begin; n0 + BKP < n_end; ...)` + last stage, and
             steps = (n_end - n_begin + 63) / 64 of the small kernel: less than one stage, a one-pixel tail, a one-pixel split, EMPTY
             splits (they must write zeros: the workspace is poisoned), a split that starts inside a sample
  2 cursors  the (b, oy, ox) walk: `p.Ws >= BKP` (one wrap per stage) against the while loops, Ws 1 / 3 / BKP - 1 / BKP / BKP + 1 for
             the 32- and the 16-pixel stages, Hs = 1, Ws = 1, stride 2, 1x1, and the p_rem / p_b carry of the register-staged scaled path
  3 KH != KW ky = t / KW in the kernels and in the unpack: 1x3, 3x1, 2x2, 2x3, pad 0 and 1
  4 taps     conv_wgrad_h2v2<.., TAPS>: q_tl = column * 4 / Cb, q_tap = t * tpt + q_tl, the mask q_tl < tpt && q_tap < T
  5 ladder   one row per conv_wgrad_mfma / conv_wgrad_h2v2 instantiation the default knobs reach (wgrad_launch_one)
  6 table    b_first = n_begin / HWs, tab_rem, the single-`if` row advance, rows with b >= B, the 64- and 16-sample limits of tab_fits
  7 halo     513 / 1025 patches on 512 persistent workgroups (second / third patch of a workgroup, both LDS buffers), maps that are
             no multiple of 16, 511 patches (not the halo kernel), a second patch in another sample (its scales)
  8 guard    an out-of-window f16x2 launch with an empty split: the bf16x3 twin rewrites every split
  9 unpack   destination strides, wscale, R < RP, C < CP, nsplit = 1, KH != KW
Tile sizes, stage depth, table use, grouped taps, chunk and the number of empty splits are not observable from Python: CLAIMS restates
them per (row, mode) as data, and tests/test_cpu_wiring.py (test_wgrad_edges_*) holds csrc/wgrad_route.h to them on the CPU through
tests/host/wgrad_route_dump.cpp.  The profiling family (ops.prof_read) is asserted here.

How a case is run (_run): both operands and the scales sit inside larger allocations whose bands before and after (64 pixels x C: two
32-pixel stages) are NaN, so a read that should have been masked shows up as a NaN in dW; the workspace is NaN before the call, so an
unwritten (split, tap, row < R, column < C) cell reaches dW; dW is NaN before the unpack, and the rows with a strided dW assert that
the elements outside the view keep it; the call runs twice and the bits must agree (fixed reduction order, no atomics); outside the
guard test the f16x2 gate must not move.

Reference: torch.float64 on the CPU over exactly the operands the kernel reads (f16: the half-rounded tensors; the scales are the fp32
scales as passed): dW[o, i, ky, kx] = wscale * sum_{b, oy, ox} (ss[b, o] small[b, o, oy, ox]) (bs[b, i] big[b, i, oy s + ky - pad,
ox s + kx - pad]); R is the same on absolute values.  tests/test_cpu_wiring.py ties wgrad64 to autograd of F.conv2d in float64.
Bound, per element and with no element excluded (test_gpu_conv_routes._check):

    |got - ref| <= TOL * R + TINY            (R = 0, a tap that only ever reads padding: the result must be zero)

Tolerances (none is tuned to the kernels):
  f16x2 / bf16x3 / native   test_gpu_conv_routes.TOL unchanged (1.5e-6 / 2e-6 / 2e-6).
  wg16                      f16 operands, un-modulated: the native entry, 2e-6 — products of two halfs are exact in fp32 and the sums are
                            fp32, as in the native kernel.
  wg16s2 / wg16s4           f16 operands, modulated: count x 2^-11 + 2e-6 with the count of roundings to half per product.  The f16 TAB
                            branch of conv_wgrad_mfma reads the fp32 scale from the LDS table, converts it to half (`(gif::f16)psv[i]`:
                            rounding 1) and multiplies the half fragment by it in half precision (`af[i] *= ...`: rounding 2); the halo
                            kernel does the same (`fa = (T)sa`, `af *= fa`).  Two roundings per SCALED operand, none for an operand
                            without scales (the table holds 1.0f: exact) — 2 (one side scaled) or 4 (both): 9.79e-4 / 1.955e-3.
  unpack                    sums of at most 17 partial sums and one multiplication: fewer than 32 roundings of 2^-24 = 1.9e-6 -> the
                            native entry.

Observed worst |got - ref| / R on the MI355X (all cases of this module, one run) against the tolerance it is held to:
  native   3.5e-7 (lad_tab16)        ->  TOL 2e-6     (5.7 x)
  bf16x3   3.7e-7 (cu_13x3_k3)       ->  TOL 2e-6     (5.3 x)
  f16x2    2.9e-7 (lad_reg35: the native register-staged kernel; the guard test's bf16x3 twin stays below bf16x3's worst)
                                     ->  TOL 1.5e-6   (5.2 x)
  wg16     1.3e-7 (ch_sq_n16)        ->  TOL 2e-6     (15 x: fp32 sums of exact products)
  wg16s2   2.0e-4 (tb_big_only)      ->  TOL 9.79e-4  (4.9 x)
  wg16s4   7.3e-4 (lad_f16_64_4x4)   ->  TOL 1.955e-3 (2.7 x: 16 pixels per sample, little averaging of the four roundings)
  unpack   1.6e-7 (splits7)          ->  TOL 2e-6
No family needed more than the tolerance named for it.
Every case prints its ratio ("[route ratio]" lines with -s) so that a re-measurement is one run of this module.
"""
import ctypes
import zlib
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import TINY, TOL, WORST, _check

pytestmark = pytest.mark.gpu

H16 = torch.float16
FP32_MODES = ("native", "bf16x3", "f16x2")
ALL = FP32_MODES + ("f16",)
NAN = float("nan")

TOL.update({"wg16": TOL["native"], "wg16s2": 2 * 2.0 ** -11 + TOL["native"], "wg16s4": 4 * 2.0 ** -11 + TOL["native"],
            "unpack": TOL["native"]})
TINY.update({"wg16": 1e-30, "wg16s2": 1e-30, "wg16s4": 1e-30, "unpack": 1e-30})
for _fam in ("wg16", "wg16s2", "wg16s4", "unpack"):
    WORST.setdefault(_fam, (0.0, ""))  # (a first ratio of exactly 0 — a bit-for-bit copy — is no new worst: _note reads the entry)


class Row(NamedTuple):
    name: str
    geom: tuple                    # (B, Hs, Ws, Cs, Cb, KH, KW, stride, pad): the SMALL side's map; f16 rounds the channels up to 8
    modes: tuple = ALL
    nsplit: Optional[int] = None   # None: the library's query
    scaled: str = ""               # "" | both | small | big: per-sample scales
    dw: str = ""                   # "" contiguous [O, I, KH, KW] | t: a transposed view | s: a slice of a larger poisoned buffer
    wscale: float = 1.0
    ladder: bool = False           # section 5


def geom_of(row, mode):
    B, Hs, Ws, Cs, Cb, KH, KW, s, p = row.geom
    if mode == "f16":
        Cs, Cb = (Cs + 7) // 8 * 8, (Cb + 7) // 8 * 8
    return B, Hs, Ws, Cs, Cb, KH, KW, s, p


def big_hw(geom):
    B, Hs, Ws, Cs, Cb, KH, KW, s, p = geom
    return (Hs - 1) * s + KH - 2 * p, (Ws - 1) * s + KW - 2 * p


K3, K3S2, K1 = (3, 3, 1, 1), (3, 3, 2, 0), (1, 1, 1, 0)
SQ, THIN, TINYC, WIDE = (132, 36), (132, 24), (20, 24), (20, 36)  # RP x CP: 256 x 128 (second row tile: 4 real rows), 256 x 32, 32 x 32, 32 x 128

ROWS = []


def _add(name, bhw, ch, k=K3, **kw):
    ROWS.append(Row(name, (*bhw, *ch, *k), **kw))


# ---- 1. chunks: 3x3 stride 1 pad 1 on a 128 x 32 route (f16x2: grouped taps; f16: 136 channels, the 128 tile), a 128 x 128 route and a
# 32 x 32 route (f16: tile 32)
for _r, _ch in (("thin", THIN), ("sq", SQ), ("tiny", TINYC)):
    _add(f"ch_{_r}_n16", (1, 4, 4), _ch, nsplit=1)            # Ntot 16 < BKP: the loop body never runs, the last stage holds 16 masked rows
    _add(f"ch_{_r}_n33_1", (1, 3, 11), _ch, nsplit=1)         # Ntot 33, chunk 64: one full stage + a one-pixel tail stage
    _add(f"ch_{_r}_n33_2", (1, 3, 11), _ch, nsplit=2, dw="s" if _r == "thin" else "")  # chunk 32: split 1 is one pixel
    _add(f"ch_{_r}_n130_5", (2, 5, 13), _ch, nsplit=5)        # Ntot 130, chunk 32: split 4 is the two-pixel tail 128..129
    _add(f"ch_{_r}_n130_6", (2, 5, 13), _ch, nsplit=6, dw="t" if _r == "sq" else "")  # chunk 32: split 5 starts at 160 >= Ntot: EMPTY
    _add(f"ch_{_r}_b3_n2", (3, 5, 7), _ch, nsplit=2)          # Ntot 105, chunk 64: split 1 starts 29 pixels into sample 1 (35 per sample)
# conv_wgrad_small_mfma (un-modulated 3x3 s1 p1, Cs <= 32, Cb <= 16, Ntot >= 65536): 256 splits, chunk rounded to 64
_add("sm_256x257", (1, 256, 257), (20, 12), modes=FP32_MODES)   # Ntot 65792: chunk 320, splits 206..255 start past Ntot: 50 EMPTY splits
_add("sm_1x65537", (1, 1, 65537), (20, 12), modes=FP32_MODES)   # chunk 320: split 204 is 257 pixels (steps 5, the last one pixel), 51 empty;
                                                                #   a one-row map: the ky != 1 taps only read padding (R = 0: exact zeros)
_add("sm_not_255x257", (1, 255, 257), (20, 12), modes=FP32_MODES)  # Ntot 65535: the last shape on the generic 32 x 32 kernel; the library's
                                                                   #   own 113 splits of 608 pixels leave 5 EMPTY splits

# ---- 2. cursors.  32-pixel stages (bf16x3 / f16x2 / f16 on the 128 x 128 route; native there: 16-pixel stages): Ws 1, 3 (while
# loops, many wraps per stage), 31 (while loops, BKP - 1), 32 (`p.Ws >= BKP`: every stage wraps exactly once), 33 (one wrap at most),
# a one-row and a one-column map; B 2 so that the sample wraps too
for _hw in ((37, 1), (13, 3), (3, 31), (3, 32), (3, 33), (1, 40), (40, 1)):
    for _kn, _k in (("k3", K3), ("s2", K3S2), ("k1", K1)):
        _add(f"cu_{_hw[0]}x{_hw[1]}_{_kn}", (2, *_hw), SQ, _k)
    _add(f"cu_{_hw[0]}x{_hw[1]}_tiny", (2, *_hw), TINYC)            # the 32 x 32 kernel (32-pixel stages in every mode)
    if (_hw[0] * _hw[1]) % 16:
        # register-staged scaled path (GLDS = false: Hs * Ws % 16 != 0): p_rem += BKP; while (p_rem >= HWs) { p_rem -= HWs; ++p_b; }
        _add(f"cu_{_hw[0]}x{_hw[1]}_sc", (2, *_hw), SQ, modes=("native",), scaled="both")
        _add(f"cu_{_hw[0]}x{_hw[1]}_sc_s2", (2, *_hw), TINYC, K3S2, modes=("native",), scaled="both")
# 16-pixel stages with the scale table (native TAB; bf16x3 / f16 TAB with Hs * Ws % 32 == 16; f16x2 runs the bf16x3 kernel there):
# Ws 15 (while loops), 16 (`p.Ws >= BKP`, a wrap per stage), 17; Hs * Ws = 240, 48, 272
for _hw in ((16, 15), (3, 16), (16, 17)):
    for _kn, _k in (("k3", K3), ("s2", K3S2), ("k1", K1)):
        _add(f"cu16_{_hw[0]}x{_hw[1]}_{_kn}", (2, *_hw), SQ, _k, scaled="both")
    _add(f"cu16_{_hw[0]}x{_hw[1]}_plain", (2, *_hw), SQ, modes=("native",))
_add("cu_b3_1x32", (3, 1, 32), SQ)                        # Ws == BKP == Hs * Ws: every stage wraps the row AND the sample
_add("cu_b3_1x32_sc", (3, 1, 32), SQ, scaled="both")      # ... and moves to the next table row

# ---- 3. KH != KW (T = KH * KW taps, ky = t / KW): on the 128 x 128 route and on the 128 x 32 route (f16x2: grouped taps)
for _kh, _kw in ((1, 3), (3, 1), (2, 2), (2, 3)):
    for _p in (0, 1):
        _add(f"kk_{_kh}x{_kw}_p{_p}", (2, 5, 7), SQ, (_kh, _kw, 1, _p))
        _add(f"kk_{_kh}x{_kw}_p{_p}_thin", (2, 5, 7), THIN, (_kh, _kw, 1, _p), modes=FP32_MODES)

# ---- 4. grouped taps of conv_wgrad_h2v2<false, true> (f16x2, 32 < Cs, Cb <= 32, un-modulated): tpt = min(128 / Cb, T) taps per column
# tile, tgroups = ceil(T / tpt); column c belongs to tap t * tpt + c / Cb
_H2 = ("f16x2",)
_add("tp_cb4", (2, 5, 13), (68, 4), modes=_H2)     # tpt 9 (capped by T), 1 group of 9 taps, columns 36..127 unused (q_tl up to 31 >= tpt)
_add("tp_cb12", (2, 5, 13), (68, 12), modes=_H2)   # tpt 9 (128 / 12 = 10, capped by T), 1 group, columns 108..127 unused (q_tl 9, 10 masked)
_add("tp_cb16", (2, 5, 13), (68, 16), modes=_H2)   # tpt 8, 2 groups, the last holds ONE tap (q_tap 9..15 >= T masked), no unused column
_add("tp_cb20", (2, 5, 13), (68, 20), modes=_H2)   # tpt 6, 2 groups, last 3 taps, columns 120..127 unused (q_tl 6 >= tpt)
_add("tp_cb24", (2, 5, 13), (68, 24), modes=_H2)   # tpt 5, 2 groups, last 4 taps, columns 120..127 unused
_add("tp_cb28", (2, 5, 13), (68, 28), modes=_H2)   # tpt 4, 3 groups, last ONE tap, columns 112..127 unused
_add("tp_cb32", (2, 5, 13), (68, 32), modes=_H2)   # tpt 4, 3 groups, last ONE tap, no unused column
_add("tp_cb24_2x2", (2, 5, 13), (68, 24), (2, 2, 1, 0), modes=_H2)  # T 4: tpt 4 (128 / 24 = 5 capped by T), 1 group, columns 96..127 unused
_add("tp_cb24_1x3", (2, 5, 13), (68, 24), (1, 3, 1, 1), modes=_H2)  # T 3: tpt 3, 1 group, columns 72..127 unused
_add("tp_cb24_1x1", (2, 5, 13), (68, 24), K1, modes=_H2)            # T 1: not grouped: conv_wgrad_mfma<float, 128, 32, 2, 1, true, 32, false, 2>
_add("tp_cb24_rows2", (2, 5, 13), (132, 24), modes=_H2)             # RP 256: two row tiles x 2 groups per split

# ---- 5. launch ladder (wgrad_launch_one), named by template arguments <T, BP, BQ, WP, WQ, GLDS, BKP, TAB, X3> / h2v2<TAB, TAPS>
_L = dict(ladder=True)
_add("lad_big", (1, 128, 128), SQ, K1, modes=("native",), **_L)   # native <float,256,128,2,2,true,16> (Ntot 16384, RP 256, un-modulated)
_add("lad_plain32", (2, 4, 8), SQ, **_L)         # Hs*Ws 32: native <float,128,128,2,2,true,16>; bf16x3 <..,true,32,false,1>; f16x2 h2v2<true> over unit
                                                 #   scales + twin; f16 <f16,128,128,2,2,true,32>
_add("lad_plain35", (2, 5, 7), SQ, modes=FP32_MODES, **_L)         # Hs*Ws 35 (% 32 != 0): f16x2 h2v2<false, false> (plain)
_add("lad_tab32", (2, 4, 8), SQ, scaled="both", **_L)             # native <..,true,16,true>; bf16x3 <..,true,32,true,1>; f16x2 h2v2<true>; f16 <f16,128,..,32,true>
_add("lad_tab16", (2, 6, 8), SQ, scaled="both", **_L)             # Hs*Ws 48: bf16x3 (and f16x2) <..,true,16,true,1>; f16 <f16,128,128,2,2,true,16,true>
_add("lad_reg35", (2, 5, 7), SQ, modes=FP32_MODES, scaled="both", **_L)   # Hs*Ws % 16 != 0: native <float,128,128,2,2,false,32> in every mode
_add("lad_128x32", (2, 5, 7), THIN, modes=FP32_MODES, **_L)       # native <float,128,32,4,1,true,32>; bf16x3 <float,128,32,2,1,true,32,false,1>; f16x2 taps
_add("lad_128x32_k1", (2, 5, 7), THIN, K1, modes=_H2, **_L)       # f16x2 <float,128,32,2,1,true,32,false,2>
_add("lad_128x32_sc", (2, 5, 7), THIN, modes=FP32_MODES, scaled="both", **_L)    # <float,128,32,4,1,false,32> in every mode
_add("lad_32x128", (2, 5, 7), WIDE, modes=FP32_MODES, **_L)       # <float,32,128,1,4,true,32>
_add("lad_32x128_sc", (2, 5, 7), WIDE, modes=FP32_MODES, scaled="both", **_L)    # <float,32,128,1,4,false,32>
_add("lad_32x32", (2, 5, 7), TINYC, modes=FP32_MODES, **_L)       # <float,32,32,1,1,true,32>
_add("lad_32x32_sc", (2, 5, 7), TINYC, modes=FP32_MODES, scaled="both", **_L)    # <float,32,32,1,1,false,32>
_F = ("f16",)
_add("lad_f16_32", (2, 5, 7), (24, 16), modes=_F, **_L)                        # <f16,32,32,1,1,true,32>
_add("lad_f16_32_tab", (2, 4, 8), (24, 16), modes=_F, scaled="both", **_L)     # <f16,32,32,1,1,true,32,true>
_add("lad_f16_32_tab16", (2, 6, 8), (24, 16), modes=_F, scaled="both", **_L)   # <f16,32,32,1,1,true,16,true>
_add("lad_f16_64", (2, 5, 7), (40, 64), modes=_F, **_L)                        # <f16,64,64,2,2,true,32>
_add("lad_f16_64_tab", (2, 4, 8), (40, 64), modes=_F, scaled="both", **_L)     # <f16,64,64,2,2,true,32,true>
_add("lad_f16_64_4x4", (2, 4, 4), (64, 64), modes=_F, scaled="both", **_L)     # 64-channel modulated 4x4 layer: no 16-pixel-stage 64 tile ->
                                                                                #   <f16,32,32,1,1,true,16,true> on 2 x 2 tiles over the 64-padded workspace
_add("lad_f16_256", (64, 16, 16), (256, 256), K1, modes=_F, **_L)              # <f16,256,256,2,4,true,32> (Ntot 16384, channels % 256 == 0)
_add("lad_f16_256_tab", (64, 16, 16), (256, 256), K1, modes=_F, scaled="both", **_L)   # <f16,256,256,2,4,true,32,true>

# ---- 6. scale table: b_first = n_begin / HWs, tab_rem = n_begin - b_first * HWs, `tab_rem += BKP; if (tab_rem >= HWs) ...`
_add("tb_b4_n3", (4, 6, 8), SQ, nsplit=3, scaled="both")      # HWs 48, chunk 64: splits start 16 and 32 pixels into samples 1 and 2
_add("tb_small_only", (4, 6, 8), SQ, nsplit=3, scaled="small")   # the other operand's table rows hold 1.0f
_add("tb_big_only", (4, 6, 8), SQ, nsplit=3, scaled="big", wscale=-0.37)
_add("tb_b_past", (3, 4, 8), SQ, nsplit=2, scaled="both")     # HWs 32, chunk 64: split 1 starts at sample 2, table rows b = 2, 3, 4: two rows with b >= B
_add("tb_65", (128, 4, 4), SQ, modes=FP32_MODES, nsplit=2, scaled="both")   # chunk 1024: 65 samples x 1 KB > 64 KB: no table -> register-staged native kernel
_add("tb_45", (128, 4, 4), SQ, nsplit=3, scaled="both")       # chunk 704: 45 samples: the table kernels (HWs 16: a new table row every stage)
_add("tb_f16_17", (64, 16, 16), (256, 256), K1, modes=_F, nsplit=4, scaled="both")   # chunk 4096: 17 samples x 2 KB > 32 KB -> the 128-wide tile
_add("tb_f16_9", (64, 16, 16), (256, 256), K1, modes=_F, nsplit=8, scaled="both")    # chunk 2048: 9 samples -> the 256-wide tile

# ---- 7. conv_wgrad_halo_f16 (f16, stride 1, Cs, Cb <= 32, >= 512 patches of 16 x 16): 512 persistent workgroups = splits
_add("hl_513", (1, 289, 417), (24, 24), modes=_F)                        # 19 x 27 = 513 patches (one-pixel overhang both ways): workgroup 0 walks
                                                                         #   patches 0 and 512, the second through the other LDS buffer
_add("hl_513_k1_sc", (1, 289, 417), (32, 8), K1, modes=_F, scaled="both")
_add("hl_1025_sc", (1, 385, 641), (32, 32), modes=_F, scaled="both")     # 25 x 41 = 1025: workgroup 0 walks a third patch, back in its first buffer
_add("hl_1025", (1, 385, 641), (8, 24), modes=_F)
_add("hl_511", (7, 16, 1153), (24, 24), modes=_F)                        # 7 x 73 = 511 patches < 512: NOT the halo kernel (<f16,32,32,1,1,true,32>;
                                                                         #   the library's 227 splits of 576 pixels: 2 EMPTY splits)
_add("hl_xsample_sc", (2, 272, 272), (24, 32), modes=_F, scaled="both")  # 2 x 289 patches: workgroups 0..65 walk a patch of sample 0, then one of
_add("hl_xsample_k1", (2, 272, 272), (8, 32), K1, modes=_F, scaled="small")  # sample 1 (patch 512 + w >= 289): the next patch's scales

CASES = [pytest.param(r, m, id=f"{r.name}-{m}") for r in ROWS for m in r.modes]

# (row, mode) -> (launch [+ twin] as tests/host/wgrad_route_dump.cpp prints it without block size and grid, chunk, stab_nb, empty splits
# = max(0, nsplit - ceil(Ntot / chunk)), profiling family).  tests/test_cpu_wiring.py holds csrc/wgrad_route.h to every entry.
# CLAIMS-BEGIN
CLAIMS = {
    ("ch_thin_n16", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_thin_n16", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 1, 0, 9),
    ("ch_thin_n16", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 1, 0, 15),
    ("ch_thin_n16", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_thin_n33_1", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 64, 1, 0, 1),
    ("ch_thin_n33_1", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 64, 1, 0, 9),
    ("ch_thin_n33_1", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 64, 1, 0, 15),
    ("ch_thin_n33_1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 64, 1, 0, 7),
    ("ch_thin_n33_2", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_thin_n33_2", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 1, 0, 9),
    ("ch_thin_n33_2", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 1, 0, 15),
    ("ch_thin_n33_2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_thin_n130_5", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 32, 2, 0, 1),
    ("ch_thin_n130_5", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 2, 0, 9),
    ("ch_thin_n130_5", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 2, 0, 15),
    ("ch_thin_n130_5", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 2, 0, 7),
    ("ch_thin_n130_6", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 32, 2, 1, 1),
    ("ch_thin_n130_6", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 2, 1, 9),
    ("ch_thin_n130_6", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 32, 2, 1, 15),
    ("ch_thin_n130_6", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 2, 1, 7),
    ("ch_thin_b3_n2", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 64, 3, 0, 1),
    ("ch_thin_b3_n2", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 64, 3, 0, 9),
    ("ch_thin_b3_n2", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 64, 3, 0, 15),
    ("ch_thin_b3_n2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 64, 3, 0, 7),
    ("ch_sq_n16", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 32, 1, 0, 1),
    ("ch_sq_n16", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 1, 0, 9),
    ("ch_sq_n16", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 1, 0, 15),
    ("ch_sq_n16", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_sq_n33_1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 64, 1, 0, 1),
    ("ch_sq_n33_1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 64, 1, 0, 9),
    ("ch_sq_n33_1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 64, 1, 0, 15),
    ("ch_sq_n33_1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 64, 1, 0, 7),
    ("ch_sq_n33_2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 32, 1, 0, 1),
    ("ch_sq_n33_2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 1, 0, 9),
    ("ch_sq_n33_2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 1, 0, 15),
    ("ch_sq_n33_2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_sq_n130_5", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 32, 2, 0, 1),
    ("ch_sq_n130_5", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 2, 0, 9),
    ("ch_sq_n130_5", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 2, 0, 15),
    ("ch_sq_n130_5", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 2, 0, 7),
    ("ch_sq_n130_6", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 32, 2, 1, 1),
    ("ch_sq_n130_6", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 2, 1, 9),
    ("ch_sq_n130_6", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 32, 2, 1, 15),
    ("ch_sq_n130_6", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 32, 2, 1, 7),
    ("ch_sq_b3_n2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 64, 3, 0, 1),
    ("ch_sq_b3_n2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 64, 3, 0, 9),
    ("ch_sq_b3_n2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 64, 3, 0, 15),
    ("ch_sq_b3_n2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 64, 3, 0, 7),
    ("ch_tiny_n16", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n16", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n16", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n16", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_tiny_n33_1", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 1, 0, 1),
    ("ch_tiny_n33_1", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 1, 0, 1),
    ("ch_tiny_n33_1", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 1, 0, 1),
    ("ch_tiny_n33_1", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 1, 0, 7),
    ("ch_tiny_n33_2", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n33_2", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n33_2", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 1),
    ("ch_tiny_n33_2", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 1, 0, 7),
    ("ch_tiny_n130_5", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 0, 1),
    ("ch_tiny_n130_5", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 0, 1),
    ("ch_tiny_n130_5", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 0, 1),
    ("ch_tiny_n130_5", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 0, 7),
    ("ch_tiny_n130_6", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 1, 1),
    ("ch_tiny_n130_6", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 1, 1),
    ("ch_tiny_n130_6", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 1, 1),
    ("ch_tiny_n130_6", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 32, 2, 1, 7),
    ("ch_tiny_b3_n2", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 3, 0, 1),
    ("ch_tiny_b3_n2", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 3, 0, 1),
    ("ch_tiny_b3_n2", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 3, 0, 1),
    ("ch_tiny_b3_n2", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 64, 3, 0, 7),
    ("sm_256x257", "native"): ('small', 320, 0, 50, 1),
    ("sm_256x257", "bf16x3"): ('small', 320, 0, 50, 1),
    ("sm_256x257", "f16x2"): ('small', 320, 0, 50, 1),
    ("sm_1x65537", "native"): ('small', 320, 0, 51, 1),
    ("sm_1x65537", "bf16x3"): ('small', 320, 0, 51, 1),
    ("sm_1x65537", "f16x2"): ('small', 320, 0, 51, 1),
    ("sm_not_255x257", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 608, 1, 5, 1),
    ("sm_not_255x257", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 608, 1, 5, 1),
    ("sm_not_255x257", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 608, 1, 5, 1),
    ("cu_37x1_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_37x1_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_37x1_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_37x1_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_37x1_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_37x1_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_37x1_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_37x1_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_37x1_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_37x1_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_37x1_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_37x1_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_13x3_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_13x3_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_13x3_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_13x3_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_13x3_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_13x3_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_13x3_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_13x3_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_13x3_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_13x3_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_13x3_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x31_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_3x31_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x31_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x31_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_3x31_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x31_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x31_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_3x31_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x31_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x31_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x31_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x32_k3", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 2, 0, 15),
    ("cu_3x32_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x32_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x32_s2", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 2, 0, 15),
    ("cu_3x32_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x32_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_3x32_k1", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 2, 0, 15),
    ("cu_3x32_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x32_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_3x32_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_3x33_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 9),
    ("cu_3x33_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 15),
    ("cu_3x33_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 128, 2, 0, 7),
    ("cu_3x33_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 9),
    ("cu_3x33_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 15),
    ("cu_3x33_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 128, 2, 0, 7),
    ("cu_3x33_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 9),
    ("cu_3x33_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 128, 2, 0, 15),
    ("cu_3x33_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 128, 2, 0, 7),
    ("cu_3x33_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 128, 2, 0, 7),
    ("cu_3x33_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 128, 2, 0, 1),
    ("cu_3x33_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 128, 2, 0, 1),
    ("cu_1x40_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_1x40_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_1x40_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_1x40_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_1x40_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_1x40_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_1x40_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_1x40_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_1x40_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_1x40_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_1x40_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_1x40_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_40x1_k3", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_40x1_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_40x1_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_40x1_s2", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_40x1_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_40x1_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("cu_40x1_k1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("cu_40x1_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_40x1_tiny", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_tiny", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_tiny", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_tiny", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("cu_40x1_sc", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu_40x1_sc_s2", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("cu16_16x15_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x15_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_k3", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x15_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x15_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_s2", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x15_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x15_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_k1", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x15_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x15_plain", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 2, 0, 1),
    ("cu16_3x16_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 1),
    ("cu16_3x16_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_k3", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 7),
    ("cu16_3x16_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 1),
    ("cu16_3x16_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_s2", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 7),
    ("cu16_3x16_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 1),
    ("cu16_3x16_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_k1", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("cu16_3x16_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 7),
    ("cu16_3x16_plain", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("cu16_16x17_k3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x17_k3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_k3", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_k3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x17_s2", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x17_s2", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_s2", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_s2", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x17_k1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 1),
    ("cu16_16x17_k1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_k1", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 128, 2, 0, 9),
    ("cu16_16x17_k1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 128, 2, 0, 7),
    ("cu16_16x17_plain", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 2, 0, 1),
    ("cu_b3_1x32", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 3, 0, 1),
    ("cu_b3_1x32", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 3, 0, 9),
    ("cu_b3_1x32", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 3, 0, 15),
    ("cu_b3_1x32", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 3, 0, 7),
    ("cu_b3_1x32_sc", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 3, 0, 1),
    ("cu_b3_1x32_sc", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 3, 0, 9),
    ("cu_b3_1x32_sc", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 96, 3, 0, 15),
    ("cu_b3_1x32_sc", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab1 x3=0', 96, 3, 0, 7),
    ("kk_1x3_p0", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_1x3_p0", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_1x3_p0", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_1x3_p0", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_1x3_p0_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_1x3_p0_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_1x3_p0_thin", "f16x2"): ('h2v2 tab0 taps tpt3 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_1x3_p1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_1x3_p1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_1x3_p1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_1x3_p1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_1x3_p1_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_1x3_p1_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_1x3_p1_thin", "f16x2"): ('h2v2 tab0 taps tpt3 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_3x1_p0", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_3x1_p0", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_3x1_p0", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_3x1_p0", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_3x1_p0_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_3x1_p0_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_3x1_p0_thin", "f16x2"): ('h2v2 tab0 taps tpt3 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_3x1_p1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_3x1_p1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_3x1_p1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_3x1_p1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_3x1_p1_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_3x1_p1_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_3x1_p1_thin", "f16x2"): ('h2v2 tab0 taps tpt3 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x2_p0", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x2_p0", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x2_p0", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x2_p0", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_2x2_p0_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x2_p0_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x2_p0_thin", "f16x2"): ('h2v2 tab0 taps tpt4 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x2_p1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x2_p1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x2_p1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x2_p1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_2x2_p1_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x2_p1_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x2_p1_thin", "f16x2"): ('h2v2 tab0 taps tpt4 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x3_p0", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x3_p0", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x3_p0", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x3_p0", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_2x3_p0_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x3_p0_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x3_p0_thin", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x3_p1", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x3_p1", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x3_p1", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("kk_2x3_p1", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("kk_2x3_p1_thin", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("kk_2x3_p1_thin", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("kk_2x3_p1_thin", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb4", "f16x2"): ('h2v2 tab0 taps tpt9 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb12", "f16x2"): ('h2v2 tab0 taps tpt9 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb16", "f16x2"): ('h2v2 tab0 taps tpt8 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb20", "f16x2"): ('h2v2 tab0 taps tpt6 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb24", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb28", "f16x2"): ('h2v2 tab0 taps tpt4 tg3 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb32", "f16x2"): ('h2v2 tab0 taps tpt4 tg3 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb24_2x2", "f16x2"): ('h2v2 tab0 taps tpt4 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb24_1x3", "f16x2"): ('h2v2 tab0 taps tpt3 tg1 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb24_1x1", "f16x2"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("tp_cb24_rows2", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("lad_big", "native"): ('mfma f32 256x128 w2x2 glds1 bkp16 tab0 x3=0', 128, 1, 0, 1),
    ("lad_plain32", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 64, 2, 0, 1),
    ("lad_plain32", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 64, 2, 0, 9),
    ("lad_plain32", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 64, 2, 0, 15),
    ("lad_plain32", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab0 x3=0', 64, 2, 0, 7),
    ("lad_plain35", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab0 x3=0', 96, 2, 0, 1),
    ("lad_plain35", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("lad_plain35", "f16x2"): ('h2v2 tab0 + mfma f32 128x128 w2x2 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("lad_tab32", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 2, 0, 1),
    ("lad_tab32", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 64, 2, 0, 9),
    ("lad_tab32", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 64, 2, 0, 15),
    ("lad_tab32", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab1 x3=0', 64, 2, 0, 7),
    ("lad_tab16", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 1),
    ("lad_tab16", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("lad_tab16", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 96, 2, 0, 9),
    ("lad_tab16", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 96, 2, 0, 7),
    ("lad_reg35", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_reg35", "bf16x3"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_reg35", "f16x2"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_128x32", "native"): ('mfma f32 128x32 w4x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_128x32", "bf16x3"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 9),
    ("lad_128x32", "f16x2"): ('h2v2 tab0 taps tpt5 tg2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("lad_128x32_k1", "f16x2"): ('mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=2 + mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=1', 96, 2, 0, 15),
    ("lad_128x32_sc", "native"): ('mfma f32 128x32 w4x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_128x32_sc", "bf16x3"): ('mfma f32 128x32 w4x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_128x32_sc", "f16x2"): ('mfma f32 128x32 w4x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128", "native"): ('mfma f32 32x128 w1x4 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128", "bf16x3"): ('mfma f32 32x128 w1x4 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128", "f16x2"): ('mfma f32 32x128 w1x4 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128_sc", "native"): ('mfma f32 32x128 w1x4 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128_sc", "bf16x3"): ('mfma f32 32x128 w1x4 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x128_sc", "f16x2"): ('mfma f32 32x128 w1x4 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32", "native"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32", "bf16x3"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32", "f16x2"): ('mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32_sc", "native"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32_sc", "bf16x3"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_32x32_sc", "f16x2"): ('mfma f32 32x32 w1x1 glds0 bkp32 tab0 x3=0', 96, 2, 0, 1),
    ("lad_f16_32", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("lad_f16_32_tab", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab1 x3=0', 64, 2, 0, 7),
    ("lad_f16_32_tab16", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp16 tab1 x3=0', 96, 2, 0, 7),
    ("lad_f16_64", "f16"): ('mfma f16 64x64 w2x2 glds1 bkp32 tab0 x3=0', 96, 2, 0, 7),
    ("lad_f16_64_tab", "f16"): ('mfma f16 64x64 w2x2 glds1 bkp32 tab1 x3=0', 64, 2, 0, 7),
    ("lad_f16_64_4x4", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp16 tab1 x3=0', 32, 2, 0, 7),
    ("lad_f16_256", "f16"): ('mfma f16 256x256 w2x4 glds1 bkp32 tab0 x3=0', 128, 2, 0, 7),
    ("lad_f16_256_tab", "f16"): ('mfma f16 256x256 w2x4 glds1 bkp32 tab1 x3=0', 128, 2, 0, 7),
    ("tb_b4_n3", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 1),
    ("tb_b4_n3", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_b4_n3", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_b4_n3", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 7),
    ("tb_small_only", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 1),
    ("tb_small_only", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_small_only", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_small_only", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 7),
    ("tb_big_only", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 1),
    ("tb_big_only", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_big_only", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 64, 3, 0, 9),
    ("tb_big_only", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 7),
    ("tb_b_past", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 64, 3, 0, 1),
    ("tb_b_past", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 64, 3, 0, 9),
    ("tb_b_past", "f16x2"): ('h2v2 tab1 + mfma f32 128x128 w2x2 glds1 bkp32 tab1 x3=1', 64, 3, 0, 15),
    ("tb_b_past", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab1 x3=0', 64, 3, 0, 7),
    ("tb_65", "native"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 1024, 65, 0, 1),
    ("tb_65", "bf16x3"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 1024, 65, 0, 1),
    ("tb_65", "f16x2"): ('mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0', 1024, 65, 0, 1),
    ("tb_45", "native"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=0', 704, 45, 0, 1),
    ("tb_45", "bf16x3"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 704, 45, 0, 9),
    ("tb_45", "f16x2"): ('mfma f32 128x128 w2x2 glds1 bkp16 tab1 x3=1', 704, 45, 0, 9),
    ("tb_45", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp16 tab1 x3=0', 704, 45, 0, 7),
    ("tb_f16_17", "f16"): ('mfma f16 128x128 w2x2 glds1 bkp32 tab1 x3=0', 4096, 17, 0, 7),
    ("tb_f16_9", "f16"): ('mfma f16 256x256 w2x4 glds1 bkp32 tab1 x3=0', 2048, 9, 0, 7),
    ("hl_513", "f16"): ('halo tr1', 0, 0, 0, 7),
    ("hl_513_k1_sc", "f16"): ('halo tr1', 0, 0, 0, 7),
    ("hl_1025_sc", "f16"): ('halo tr1', 0, 0, 0, 7),
    ("hl_1025", "f16"): ('halo tr1', 0, 0, 0, 7),
    ("hl_511", "f16"): ('mfma f16 32x32 w1x1 glds1 bkp32 tab0 x3=0', 576, 2, 2, 7),
    ("hl_xsample_sc", "f16"): ('halo tr1', 0, 0, 0, 7),
    ("hl_xsample_k1", "f16"): ('halo tr1', 0, 0, 0, 7),
}
# CLAIMS-END


def dump_args(row, mode):
    """the `conv` argument group of tests/host/wgrad_route_dump.cpp for one case"""
    B, Hs, Ws, Cs, Cb, KH, KW, s, p = geom_of(row, mode)
    return ["conv"] + [str(v) for v in (B, Hs, Ws, Cs, Cb, KH, KW, s, p, 1 if row.scaled else 0, ALL.index(mode), row.nsplit or 0)]


def claim_of_line(line, row, mode):
    """a line of the dump in the form of a CLAIMS entry"""
    import re
    m = re.match(r"^(.*?) \| (\S+) \| ([us]) \| n(\d+) -> (.*?) ; RP\d+ CP\d+ .* stab(\d+) chunk(\d+) fam(\d+) \| tiles -?\d+ splits \d+$", line)
    assert m, line
    B, Hs, Ws = geom_of(row, mode)[:3]
    assert m.group(2) == mode and m.group(3) == ("s" if row.scaled else "u") and m.group(1).startswith(f"B{B} Hs{Hs} Ws{Ws} "), line
    launch = re.sub(r" thr\d+ wgs\d+", "", m.group(5)).replace(" + twin ", " + ")
    nsplit, chunk = int(m.group(4)), int(m.group(7))
    assert row.nsplit in (None, nsplit)
    empty = max(0, nsplit - -(-(B * Hs * Ws) // chunk)) if chunk else 0
    return (launch, chunk, int(m.group(6)), empty, int(m.group(8)))


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def wgrad64(small, big, KH, KW, stride, pad, ss=None, bs=None, wscale=1.0, absolute=False):
    """dW[o, i, ky, kx] = wscale * sum_{b, oy, ox} (ss small)[b, o, oy, ox] (bs big)[b, i, oy s + ky - pad, ox s + kx - pad] in fp64
    (NCHW CPU tensors); absolute: the same on absolute values (R)."""
    m = (lambda t: t.abs()) if absolute else (lambda t: t)
    small, big = m(small.double()), m(big.double())
    if ss is not None:
        small = small * m(ss.double())[:, :, None, None]
    if bs is not None:
        big = big * m(bs.double())[:, :, None, None]
    B, Cs, Hs, Ws = small.shape
    bp = F.pad(big, (pad, pad, pad, pad)) if pad else big
    out = small.new_zeros(Cs, big.shape[1], KH, KW)
    sm = small.permute(1, 0, 2, 3).reshape(Cs, -1)
    for ky in range(KH):
        for kx in range(KW):
            win = bp[:, :, ky:ky + (Hs - 1) * stride + 1:stride, kx:kx + (Ws - 1) * stride + 1:stride]
            out[:, :, ky, kx] = sm @ win.permute(0, 2, 3, 1).reshape(-1, big.shape[1])
    return (abs(wscale) if absolute else wscale) * out


_OPS, _REF = {}, {}


def _operands(geom, f16, scaled):
    """CPU fp32 NCHW operands (f16: rounded to half) and fp32 scales, seeded from the geometry: shared by the rows and modes that agree on it"""
    key = (geom, f16, scaled)
    if key not in _OPS:
        B, Hs, Ws, Cs, Cb, KH, KW, s, p = geom
        Hb, Wb = big_hw(geom)
        g = torch.Generator().manual_seed(zlib.crc32(repr(geom).encode()))
        r16 = (lambda t: t.to(H16).float()) if f16 else (lambda t: t)
        o = {"small": r16(torch.randn(B, Cs, Hs, Ws, generator=g)), "big": r16(torch.randn(B, Cb, Hb, Wb, generator=g))}
        ss, bs = torch.rand(B, Cs, generator=g) + 0.5, torch.rand(B, Cb, generator=g) + 0.5
        o["ss"] = ss if scaled in ("both", "small") else None
        o["bs"] = bs if scaled in ("both", "big") else None
        if len(_OPS) > 8:
            _OPS.clear()
        _OPS[key] = o
    return _OPS[key]


def _reference(geom, f16, scaled):
    key = (geom, f16, scaled)
    if key not in _REF:
        o = _operands(geom, f16, scaled)
        k = geom[5:]
        _REF[key] = (wgrad64(o["small"], o["big"], *k, o["ss"], o["bs"]), wgrad64(o["small"], o["big"], *k, o["ss"], o["bs"], absolute=True))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------------------------
def _guarded(t, dtype, band):
    """`t` (CPU, flat) inside a device allocation with `band` NaN elements before and behind it; returns (allocation, view of t)"""
    n = t.numel()
    assert band % 8 == 0
    buf = torch.full((2 * band + n,), NAN, dtype=dtype, device="cuda")
    buf[band:band + n] = t.to(dtype).cuda()
    return buf, buf[band:band + n]


def _entry(lib, mode):
    return {"native": lib.gif_conv2d_wgrad_f32, "bf16x3": lib.gif_conv2d_wgrad_f32x3, "f16x2": lib.gif_conv2d_wgrad_f32h2,
            "f16": lib.gif_conv2d_wgrad_f16}[mode]


def _bits(t):
    return t.contiguous().view(torch.int32)


SENT = 256  # sentinel floats behind the workspace


def _dw_view(kind, O, I, KH, KW):
    """(poisoned storage, the [O, I, KH, KW] view the unpack writes)"""
    if kind == "t":   # stored [KH, KW, I, O]: every stride differs from the contiguous layout's
        store = torch.full((KH, KW, I, O), NAN, device="cuda")
        return store, store.permute(3, 2, 0, 1)
    if kind == "s":   # a slice of a larger buffer
        store = torch.full((O + 3, I + 5, KH, KW + 1), NAN, device="cuda")
        return store, store[2:2 + O, 1:1 + I, :, 1:1 + KW]
    store = torch.full((O, I, KH, KW), NAN, device="cuda")
    return store, store


def _run(geom, mode, o, nsplit=None, dw_kind="", wscale=1.0):
    """One weight gradient through the C API on guarded operands, a NaN workspace and a NaN dW.  Returns (dW view, its storage, nsplit,
    (RP, CP))."""
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, Hs, Ws, Cs, Cb, KH, KW, s, p = geom
    Hb, Wb = big_hw(geom)
    f16 = mode == "f16"
    dt = H16 if f16 else torch.float32
    g = _lib.ConvGeom(B, Hb, Wb, Cb, Hs, Ws, Cs, KH, KW, s, p)
    RP, CP = ctypes.c_int(), ctypes.c_int()
    _lib.check((lib.gif_conv2d_wgrad_dims_f16 if f16 else lib.gif_conv2d_wgrad_dims)(Cs, Cb, ctypes.byref(RP), ctypes.byref(CP)), "wgrad_dims")
    if nsplit is None:
        nsplit = (lib.gif_conv2d_wgrad_splits_f16 if f16 else lib.gif_conv2d_wgrad_splits)(ctypes.byref(g))
    T = KH * KW
    hold = []  # the guarded allocations: alive until the call has run

    def dev(t, c, dtype):
        buf, view = _guarded(t.flatten(), dtype, 64 * c)
        hold.append((buf, 64 * c))
        return view

    small = dev(o["small"].permute(0, 2, 3, 1).contiguous(), Cs, dt)   # NHWC
    big = dev(o["big"].permute(0, 2, 3, 1).contiguous(), Cb, dt)
    ss = dev(o["ss"], Cs, torch.float32) if o["ss"] is not None else None
    bs = dev(o["bs"], Cb, torch.float32) if o["bs"] is not None else None
    n_ws = nsplit * T * RP.value * CP.value
    ws = torch.full((n_ws + SENT,), NAN, device="cuda")
    ws[n_ws:] = torch.arange(SENT, device="cuda", dtype=torch.float32) + 0.5
    _lib.check(_entry(lib, mode)(small.data_ptr(), big.data_ptr(), ws.data_ptr(), ops._p(ss), ops._p(bs), ctypes.byref(g), nsplit, ops._stream()),
               "conv2d_wgrad")
    store, dw = _dw_view(dw_kind, Cs, Cb, KH, KW)
    so, si, sky, skx = dw.stride()
    _lib.check(lib.gif_unpack_wgrad_f32(ws.data_ptr(), dw.data_ptr(), nsplit, Cs, Cb, KH, KW, RP.value, CP.value, so, si, sky, skx, float(wscale),
                                        ops._stream()), "unpack_wgrad")
    torch.cuda.synchronize()
    assert torch.equal(ws[n_ws:], torch.arange(SENT, device="cuda", dtype=torch.float32) + 0.5), "the sentinels behind the workspace were written"
    for buf, band in hold:
        assert torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all(), "a guard band of an operand was written"
    return dw, store, nsplit, (RP.value, CP.value)


def _outside_keeps_poison(store, dw):
    """every element of `store` the view does not cover is still NaN (the view itself is finite)"""
    n_nan = int(torch.isnan(store).sum())
    return n_nan == store.numel() - dw.numel()


@pytest.fixture(autouse=True)
def _restore():
    from gif_amd import ops
    before, guard = ops.get_fp32_mfma_mode(), ops.H2_GUARD
    ops.h2_fallback_stats(reset=True)
    yield
    ops.prof_enable(False)
    ops.set_fp32_mfma_mode(before)
    ops.H2_GUARD = guard
    ops.h2_fallback_stats(reset=True)


def _prof_begin():
    from gif_amd import ops
    ops.prof_enable(True)
    for f in range(18):
        ops.prof_read(f)  # (reading clears a family's records)


def _ran():
    from gif_amd import ops
    torch.cuda.synchronize()
    ran = {f: ops.prof_read(f)[2] for f in range(18)}
    ops.prof_enable(False)
    return {f: n for f, n in ran.items() if n}


def tol_family(mode, scaled):
    if mode != "f16":
        return mode
    return {"": "wg16", "small": "wg16s2", "big": "wg16s2", "both": "wg16s4"}[scaled]


@pytest.mark.parametrize("row,mode", CASES)
def test_wgrad_edges(row, mode):
    from gif_amd import ops
    geom = geom_of(row, mode)
    f16 = mode == "f16"
    if not f16:
        ops.set_fp32_mfma_mode(mode)
    o = _operands(geom, f16, row.scaled)
    ref, R = _reference(geom, f16, row.scaled)
    _prof_begin()
    dw, store, nsplit, _ = _run(geom, mode, o, row.nsplit, row.dw, row.wscale)
    fam = CLAIMS[row.name, mode][4]
    assert _ran() == {fam: 1}, f"{row.name} [{mode}]: expected one op in family {fam}"
    if mode == "f16x2":
        assert ops.h2_fallback_stats() == 0, f"{row.name}: well-scaled operands took the guarded bf16x3 fallback"
    assert dw.shape == (geom[3], geom[4], geom[5], geom[6]) and dw.dtype == torch.float32
    if row.dw:
        assert _outside_keeps_poison(store, dw), f"{row.name} [{mode}]: the unpack wrote outside the dW view (or left NaN inside)"
    dw2, _, _, _ = _run(geom, mode, o, row.nsplit, row.dw, row.wscale)
    assert torch.equal(_bits(dw), _bits(dw2)), f"{row.name} [{mode}]: a second call gave different bits"
    got = dw.double().cpu()
    assert torch.isfinite(got).all(), f"{row.name} [{mode}]: {int((~torch.isfinite(got)).sum())} NaN / Inf: poison or a guard band reached dW"
    _check(got, row.wscale * ref, abs(row.wscale) * R, tol_family(mode, row.scaled), f"{row.name} dW")


# ---- 6b. refusals: nothing is launched, the workspace keeps its poison
REFUSALS = [
    # f16 modulated with Hs * Ws % 16 != 0: a stage would straddle two samples
    ("f16_hws35", (2, 5, 7, 136, 40, 3, 3, 1, 1), None, r"needs Hs\*Ws % 16 == 0"),
    # f16, 128-wide tile: 65 samples x 2 x 128 floats > 64 KB (the fp32 modes fall back to the register-staged kernel: tb_65)
    ("f16_tab65", (128, 4, 4, 136, 40, 3, 3, 1, 1), 2, r"scale table too large"),
]


@pytest.mark.parametrize("name,geom,nsplit,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_wgrad_refusals(name, geom, nsplit, msg):
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, Hs, Ws, Cs, Cb, KH, KW, s, p = geom
    Hb, Wb = big_hw(geom)
    g = _lib.ConvGeom(B, Hb, Wb, Cb, Hs, Ws, Cs, KH, KW, s, p)
    if nsplit is None:
        nsplit = lib.gif_conv2d_wgrad_splits_f16(ctypes.byref(g))
    RP, CP = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.gif_conv2d_wgrad_dims_f16(Cs, Cb, ctypes.byref(RP), ctypes.byref(CP)), "wgrad_dims")
    small = torch.ones(B * Hs * Ws * Cs, device="cuda", dtype=H16)
    big = torch.ones(B * Hb * Wb * Cb, device="cuda", dtype=H16)
    ss, bs = torch.ones(B * Cs, device="cuda"), torch.ones(B * Cb, device="cuda")
    ws = torch.full((nsplit * KH * KW * RP.value * CP.value,), NAN, device="cuda")
    _prof_begin()
    with pytest.raises(_lib.GifHipError, match=msg):
        _lib.check(lib.gif_conv2d_wgrad_f16(small.data_ptr(), big.data_ptr(), ws.data_ptr(), ss.data_ptr(), bs.data_ptr(), ctypes.byref(g), nsplit,
                                            ops._stream()), "conv2d_wgrad_f16")
    torch.cuda.synchronize()
    assert torch.isnan(ws).all(), "the refused call wrote to the workspace"
    # un-modulated, the same geometry runs
    _lib.check(lib.gif_conv2d_wgrad_f16(small.data_ptr(), big.data_ptr(), ws.data_ptr(), None, None, ctypes.byref(g), nsplit, ops._stream()), "plain")
    torch.cuda.synchronize()
    assert torch.isfinite(ws).all()
    ops.prof_enable(False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. f16x2 guard with an empty split
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD_GEOM = (1, 5, 32, 132, 36, 3, 3, 1, 1)   # Ntot 160; 6 splits: chunk 32 (one image row per split), split 5 starts at 160: EMPTY
GUARD_NSPLIT = 6


def test_f16x2_guard_with_an_empty_split():
    """conv_wgrad_h2v2<true> on a 128 x 128 tile raises the gate (both operands out of window, built as in
    test_f16x2_thin_weight_gradient_guard_falls_back_per_tap: the first 16 pixels of every image row — whole 16-pixel K groups —
    2^-24 / 2^24 apart from the rest); the bf16x3 twin then rewrites EVERY split, the empty one included, and the result is bf16x3-grade."""
    from gif_amd import ops
    ops.set_fp32_mfma_mode("f16x2")
    geom = GUARD_GEOM
    g = torch.Generator().manual_seed(zlib.crc32(repr(("guard", geom)).encode()))
    B, Hs, Ws, Cs, Cb = geom[:5]
    small, big = torch.randn(B, Cs, Hs, Ws, generator=g), torch.randn(B, Cb, *big_hw(geom), generator=g)
    big[:, :, :, :16] *= 2.0 ** -24
    small[:, :, :, :16] *= 2.0 ** 24
    o = {"small": small, "big": big, "ss": None, "bs": None}
    ops.h2_fallback_stats(reset=True)
    _prof_begin()
    dw, _, _, _ = _run(geom, "f16x2", o, GUARD_NSPLIT)
    assert _ran() == {15: 1}
    assert ops.h2_fallback_stats(reset=True) == 1, "the out-of-window launch did not take the guarded fallback exactly once"
    dw2, _, _, _ = _run(geom, "f16x2", o, GUARD_NSPLIT)
    assert ops.h2_fallback_stats() == 1 and torch.equal(_bits(dw), _bits(dw2))
    got = dw.double().cpu()
    assert torch.isfinite(got).all()
    k = geom[5:]
    _check(got, wgrad64(small, big, *k), wgrad64(small, big, *k, absolute=True), "bf16x3", "guard_empty_split dW")
    # control: the same launch on well-scaled operands leaves the gate alone
    o2 = {"small": torch.randn(B, Cs, Hs, Ws, generator=g), "big": torch.randn(B, Cb, *big_hw(geom), generator=g), "ss": None, "bs": None}
    ops.h2_fallback_stats(reset=True)
    _run(geom, "f16x2", o2, GUARD_NSPLIT)
    assert ops.h2_fallback_stats() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. unpack_wgrad_kernel on a workspace of its own
# ---------------------------------------------------------------------------------------------------------------------------------
UNPACK = [
    # name, nsplit, (R, C, RP, CP), (KH, KW), wscale, dW layout
    ("one_split_copy", 1, (132, 36, 256, 128), (3, 3), 1.0, ""),      # nsplit 1, wscale 1: dW is the workspace slice bit for bit
    ("one_split_full", 1, (128, 32, 128, 32), (2, 3), 1.0, "t"),      # R = RP, C = CP; KH != KW: ky = t / KW
    ("splits7", 7, (132, 36, 256, 128), (3, 3), 0.37, ""),            # only the tail loop (s + 8 <= nsplit never holds)
    ("splits8_t", 8, (32, 32, 32, 32), (3, 1), 0.37, "t"),            # one full round of 8, no tail; a transposed dW
    ("splits17_s", 17, (20, 24, 32, 32), (2, 3), -0.37, "s"),         # two rounds + a tail of 1; a slice of a poisoned buffer; R < RP, C < CP
    ("splits9_1x1", 9, (4, 4, 32, 32), (1, 1), 0.37, "s"),
]


@pytest.mark.parametrize("name,nsplit,dims,kk,wscale,layout", UNPACK, ids=[u[0] for u in UNPACK])
def test_unpack_wgrad(name, nsplit, dims, kk, wscale, layout):
    from gif_amd import _lib, ops
    lib = _lib.load()
    R_, C_, RP, CP = dims
    KH, KW = kk
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    ws = torch.randn(nsplit, KH * KW, RP, CP, generator=g)
    wsd = ws.cuda()
    outs = []
    for _ in range(2):
        store, dw = _dw_view(layout, R_, C_, KH, KW)
        so, si, sky, skx = dw.stride()
        _lib.check(lib.gif_unpack_wgrad_f32(wsd.data_ptr(), dw.data_ptr(), nsplit, R_, C_, KH, KW, RP, CP, so, si, sky, skx, float(wscale),
                                            ops._stream()), "unpack_wgrad")
        torch.cuda.synchronize()
        assert _outside_keeps_poison(store, dw), f"{name}: the unpack wrote outside the dW view (or left NaN inside)"
        outs.append(dw)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # [split][t][r][c] -> [r][c][ky][kx]
    part = ws[:, :, :R_, :C_].reshape(nsplit, KH, KW, R_, C_).permute(0, 3, 4, 1, 2)
    if nsplit == 1 and wscale == 1.0:
        assert torch.equal(_bits(outs[0].cpu()), _bits(part[0])), f"{name}: one split with wscale 1 is a copy"
    ref, R = wscale * part.double().sum(0), abs(wscale) * part.double().abs().sum(0)
    _check(outs[0].double().cpu(), ref, R, "unpack", f"unpack {name}")
