"""-m gpu: every convolution and FIR dispatch route on both sides of its threshold, against an fp64 reference of the same operation.

The rest of the suite picks its shapes by model layer.  Here each row of the tables is a shape computed from a dispatch predicate
(gif_amd/ops.py: conv_plan and the predicates it composes, winograd_eligible, x3_conv, x3_tapdense, h2_conv; csrc/conv_route.h:
route_phase, conv_route, rows_thin_ok, halo_eligible; csrc/wgrad_route.h: small_wgrad_ok, wgrad_big_tile, the x3 / x3_thin tile rules of wgrad_route; csrc/elementwise.hip:
upfirdn2d_impl, gif::reduce_partials): the last shape that takes a route and the first that does not.  Each row's comment names the
predicate and the side.

Reference: torch.float64 conv2d / conv_transpose2d / autograd on the CPU over the operands the kernels read (f16 activations: the
half-rounded activations, residual and weights; fp32 modes: the raw fp32 operands), cached per shape and reused across modes.
Bound, per element instead of normalised by the tensor's maximum:

    |got - ref| <= TOL[mode] * R + TINY[mode]

where R is the same fp64 operation on |x| and |w| carried through the epilogue (|out_scale|, + |residual| + |bias|, x gain, x the
mask factor): the rounding error an element can honestly carry.  A wrong border pixel or tail tile fails even when the tensor's
maximum is large.  The fused column sums / dot products are held to the same bound against the sums of R.

Observed worst |got - ref| / R on the MI355X (all rows of this module, one run; fused column sums and dot products in brackets) and the
tolerance chosen from it:
  f16x2   3.1e-7 (t256_511)            [4.1e-9]  ->  TOL 1.5e-6  (4.8 x)
  bf16x3  4.2e-7 (split_tn2)           [6.3e-9]  ->  TOL 2e-6    (4.7 x)
  native  4.4e-7 (tconv_not_big)       [5.2e-9]  ->  TOL 2e-6    (4.5 x)
  f16     4.2e-4 (f16_tconv_small)     [1.8e-9]  ->  TOL 7e-4    (the f16 store alone rounds by up to 2^-11 = 4.9e-4 of |ref| <= R)
  fir32   3.1e-7 (blur_rows_513)       [8.7e-9]  ->  TOL 1.5e-6  (4.8 x)
  fir16   4.9e-4 (up2_even)            [5.4e-9]  ->  TOL 7e-4    (2^-11 again: the sums themselves are exact to fp32)
Every case prints its ratio ("[route ratio]" lines with -s) so that a re-measurement is one run of this module.

Route assertions, where the library exposes them: ops.prof_read(family) (one record per OP in the family the op ran in: it proves the
kernel family and contraction mode, not the tile size), ops.prof_winograd_calls(), gif_conv2d_f16_halo_eligible and
gif_conv2d_x3_eligible.  Tile sizes, the bulk + remainder split and the merged transposed phases are not observable from Python:
the row comment is the claim, and it is checked on the CPU.  csrc/conv_route.h (fwd / dgrad) and csrc/wgrad_route.h (weight gradient)
return the whole route as a value; tests/test_conv_route.py restates the fwd / dgrad comments as data (CLAIMS) and holds the route table
to them, tests/test_wgrad_route.py holds the weight gradient's table."""
import math
import zlib
from typing import NamedTuple, Optional

import pytest
import torch
import torch.nn.functional as F

H16 = torch.float16
CL = torch.channels_last

# per-element tolerances (see the module docstring for the measurements behind them)
TOL = {"f16x2": 1.5e-6, "bf16x3": 2e-6, "native": 2e-6, "f16": 7e-4, "fir32": 1.5e-6, "fir16": 7e-4}
TINY = {"f16x2": 1e-30, "bf16x3": 1e-30, "native": 1e-30, "f16": 2.0 ** -24, "fir32": 1e-30, "fir16": 2.0 ** -24}
WORST = {}  # mode -> (worst ratio so far, case): printed with every case, the source of the docstring's table


def _note(mode, what, ratio):
    if ratio > WORST.get(mode, (0.0, ""))[0]:
        WORST[mode] = (ratio, what)
    print(f"\n[route ratio] {mode} {what}: {ratio:.3e} (module worst so far {WORST[mode][0]:.3e} at {WORST[mode][1]})")


def _check(got, ref, R, mode, what):
    """|got - ref| <= TOL * R + TINY element-wise (all fp64 CPU tensors of one shape)."""
    assert got.shape == ref.shape == R.shape, (what, got.shape, ref.shape, R.shape)
    err = (got - ref).abs()
    ratio = (err / (R + TINY[mode])).max().item() if err.numel() else 0.0
    _note(mode, what, ratio)
    bad = err > TOL[mode] * R + TINY[mode]
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what} [{mode}]: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got "
                             f"{got[i].item():.9e} ref {ref[i].item():.9e} R {R[i].item():.3e}; worst ratio {ratio:.3e} > {TOL[mode]:.1e}")


def cpad(c, f16):
    return (c + 7) // 8 * 8 if f16 else (c + 3) // 4 * 4


def _dev(x, c, dtype):
    """CPU NCHW -> device NHWC of `dtype`, channels zero-padded to c."""
    if x.shape[1] != c:
        x = F.pad(x, (0, 0, 0, 0, 0, c - x.shape[1]))
    return x.to(dtype).cuda().contiguous(memory_format=CL)


# ---------------------------------------------------------------------------------------------------------------------------------
# Convolution route table.  The tile, launch-count, bulk-row and merge claims of the fwd / dgrad row comments are asserted by
# tests/test_conv_route.py (CLAIMS) against csrc/conv_route.h; tests/golden/conv_route_cases.txt lists these rows' library calls
# (tests/golden/make_conv_route_cases.py rewrites it when a row changes).
# ---------------------------------------------------------------------------------------------------------------------------------
# Kernel families (include/gif_hip.h, gif_prof_read): the family each mode's op must land in.
DIRECT = {"f16x2": 13, "bf16x3": 8, "native": 0}          # LDS-DMA direct kernels (contraction >= 24 in the split modes, >= 32 native)
THIN = {"f16x2": 5, "bf16x3": 5, "native": 5}             # < 24 (split modes) / < 32 (native) contraction channels: register-staged
DENSE = {"f16x2": 12, "bf16x3": 12, "native": 5}          # tap-dense bf16x3 order (f16x2 keeps the bf16x3 form: ops.H2_DENSE off)
WGRAD = {"f16x2": 15, "bf16x3": 9, "native": 1, "f16": 7}
WGRAD_NATIVE = {"f16x2": 1, "bf16x3": 1, "native": 1, "f16": 7}
WINO_FAM = (2, 10, 14)                                     # Winograd fwd / dgrad GEMM families (native, bf16x3, f16x2)
WWINO_FAM = (3, 11, 16)                                    # Winograd wgrad GEMM families


class Row(NamedTuple):
    name: str
    op: str                      # fwd | dgrad | wgrad  (dgrad of a stride-2 conv = transposed conv)
    shape: tuple                 # the FORWARD conv: (B, Cin, Cout, K, stride, pad, H, W), big side H x W
    fams: dict                   # mode -> expected kernel family (the modes the row runs in)
    epi: str = ""                # "" | full (in/out scales, bias, residual, act) | bra (bias, residual, act) | fuse (GradFuse) | scale
    halo: Optional[bool] = None  # f16 forward: gif_conv2d_f16_halo_eligible must say this
    patch: tuple = ()            # (ops attribute, value) pairs, restored after the case


ROWS = [
    # ---- launch(): tiles128 = cdiv(M, 128) * RP / 128 < 384 -> 64x64 tiles (bf16x3 / f16x2: 128x64 if cdiv(M, 128) * RP / 64 >= 256).
    # 48 -> RP 128; 33 input channels (36 active); odd H keeps winograd_eligible off.
    Row("t128_383", "fwd", (1, 33, 48, 3, 1, 1, 127, 386), DIRECT),       # M 49022: tiles128 383 < 384 -> 128x64 (split) / 64x64 (native)
    Row("t128_384", "fwd", (1, 33, 48, 3, 1, 1, 127, 387), DIRECT),       # M 49149: tiles128 384 -> not small; tiles256 192 < 512, full 0 -> 128x128
    Row("t128_383_dgrad", "dgrad", (1, 48, 33, 3, 1, 1, 127, 386), DIRECT, "full"),  # same M, data gradient (out 48, contraction 36)
    Row("t128_384_dgrad", "dgrad", (1, 48, 33, 3, 1, 1, 127, 387), DIRECT, "full"),
    Row("t64_127", "fwd", (2, 33, 48, 3, 1, 1, 63, 129), DIRECT, "full"),  # M 16254: cdiv(M,128)*2 = 254 < 256 -> 64x64 (split modes)
    Row("t64_128", "fwd", (2, 33, 48, 3, 1, 1, 63, 130), DIRECT, "full"),  # M 16380: 256 -> 128x64 (split modes)
    # ---- launch(): tiles256 = cdiv(M, 256) * tn >= 512 -> 256x128 / 8 waves (split modes); native: the 512-slot 128x128 split
    Row("t256_511", "fwd", (1, 33, 48, 3, 1, 1, 255, 513), DIRECT),       # M 130815: tiles256 511 -> 128 path; tiles128 1022: rem 510*2 > 512 -> one launch
    Row("t256_512", "fwd", (1, 33, 48, 3, 1, 1, 255, 514), DIRECT, "full"),  # M 131070: tiles256 512, rem 0 -> one 256x128 launch
    # bulk/remainder split `rem * 2 <= slots && slots % tn == 0`: split modes slots 256 on tiles256; native slots 512 on tiles128
    Row("split_rem128", "fwd", (1, 33, 48, 3, 1, 1, 255, 642), DIRECT, "full"),  # M 163710: tiles256 640 rem 128 -> bulk 131072 rows + 64x64 tail;
                                                                                  #   native tiles128 1279 rem 255 -> bulk + tail
    Row("split_rem129", "fwd", (1, 33, 48, 3, 1, 1, 255, 643), DIRECT, "full"),  # M 163965: tiles256 641 rem 129 -> one launch; native rem 257 -> one
    Row("split_rem128_dgrad", "dgrad", (1, 48, 33, 3, 1, 1, 255, 642), DIRECT),  # the same split on a data gradient
    Row("split_tn2", "fwd", (1, 33, 129, 3, 1, 1, 129, 509), DIRECT, "scale"),   # Cout 129 (RP 256, tn 2): tiles256 514 rem 2, 256 % 2 == 0 -> split;
                                                                                  #   native tiles128 1026 rem 2 -> split (bulk 65536 rows)
    Row("split_tn3", "fwd", (1, 33, 384, 3, 1, 1, 171, 255), DIRECT),    # Cout 384 (tn 3): tiles256 513 rem 1 but 256 % 3 != 0 -> NO split;
                                                                          #   native tiles128 1023, 512 % 3 != 0 -> one launch
    # ---- rows_thin_ok (f16x2 only; bf16x3 runs the same shapes on 256x32 tiles, native on the register-staged / 256x32 kernels):
    # x3 == 2, 3x3 s1 p1, RP == 32 (Cout <= 32), M % 256 == 0, W % 256 == 0 || (W >= 32 && 256 % W == 0); with GradFuse colsum + dot
    Row("thin_w32", "fwd", (2, 33, 32, 3, 1, 1, 24, 32), DIRECT, "fuse"),   # W 32: 256 % 32 == 0 -> rows_thin
    Row("thin_w64", "fwd", (1, 33, 17, 3, 1, 1, 20, 64), DIRECT, "fuse"),   # W 64 -> rows_thin (17 outputs: 3 zero-padded channels)
    Row("thin_w256", "fwd", (1, 40, 32, 3, 1, 1, 3, 256), DIRECT, "fuse"),  # W 256: W % 256 == 0 -> rows_thin
    Row("thin_w512", "fwd", (1, 33, 9, 3, 1, 1, 5, 512), DIRECT, "fuse"),   # W 512 -> rows_thin
    Row("thin_w48", "fwd", (1, 33, 32, 3, 1, 1, 16, 48), DIRECT, "fuse"),   # W 48: 256 % 48 != 0 -> 256x32 gather kernel
    Row("thin_w16", "fwd", (1, 33, 32, 3, 1, 1, 32, 16), DIRECT, "fuse"),   # W 16 < 32 -> 256x32
    Row("thin_m320", "fwd", (1, 33, 32, 3, 1, 1, 5, 64), DIRECT, "fuse"),   # M 320 % 256 != 0 -> 256x32 (mask + colsum: no dot at 320 px)
    Row("thin_dgrad_w64", "dgrad", (2, 17, 40, 3, 1, 1, 16, 64), DIRECT, "fuse"),  # data gradient, 20 outputs (RP 32) -> rows_thin
    # ---- x3_tapdense: 3x3, 8 <= cin_act < 32, cin_act >= 12 and (cout_act > 32 or cin_act < 24) (split modes; native: register-staged)
    Row("dense_c12", "fwd", (2, 12, 24, 3, 1, 1, 33, 40), DENSE, "bra"),    # cin 12 >= 12, cin < 24 -> dense
    Row("dense_c8", "fwd", (2, 8, 24, 3, 1, 1, 33, 40), THIN, "bra"),       # cin 8 < 12 -> not dense; x3_conv needs 24 -> register-staged
    Row("dense_c24_o36", "fwd", (2, 24, 33, 3, 1, 1, 33, 40), DENSE),       # cin 24, cout_act 36 > 32 -> dense
    Row("dense_c24_o32", "fwd", (2, 24, 32, 3, 1, 1, 33, 40),               # cin 24, cout 32: neither -> plain bf16x3 / f16x2 (256x32)
        {"f16x2": 13, "bf16x3": 8, "native": 5}),
    Row("dense_c9_o17", "fwd", (1, 9, 17, 3, 1, 1, 37, 29), DENSE),         # 9 -> 12 active, 17 -> 20: cin 12 < 24 -> dense
    Row("dense_c28_o33", "fwd", (2, 28, 33, 3, 1, 1, 31, 33), DENSE, "bra"),  # cin 28, cout_act 36 -> dense (7 K chunks, the last one ragged)
    Row("dense_dgrad", "dgrad", (2, 48, 20, 3, 1, 1, 33, 40), DENSE),       # data gradient: contraction 20, output 48 -> dense
    Row("dense_dgrad_s2", "dgrad", (2, 48, 20, 3, 2, 0, 33, 41), THIN),     # strided data gradient: `not (transposed and stride != 1)` -> not dense
    # ---- winograd_eligible: 3x3 s1 p1, even H/W, cin_act >= 32, cout_act >= 48, min(cin, cout) >= min_c (f16x2 256, else 0),
    # B*(H/2)*(W/2) >= 8192.  bf16x3 with cout % 128 != 0 runs the native Winograd GEMM (family 2).
    Row("wino_8192", "fwd", (2, 32, 48, 3, 1, 1, 128, 128), {"f16x2": 13, "bf16x3": 2, "native": 2}),  # 8192 tiles -> Winograd (f16x2: min_c)
    Row("wino_8190", "fwd", (2, 32, 48, 3, 1, 1, 126, 130), DIRECT),                                   # 8190 tiles -> direct
    Row("wino_odd_h", "fwd", (2, 32, 48, 3, 1, 1, 129, 128), DIRECT),                                  # H odd -> direct
    Row("wino_cin28", "fwd", (2, 28, 48, 3, 1, 1, 128, 128), DENSE),                                   # cin_act 28 < 32 -> direct (dense)
    Row("wino_cout44", "fwd", (2, 32, 44, 3, 1, 1, 128, 128), DIRECT),                                 # cout_act 44 < 48 -> direct
    Row("wino_dgrad", "dgrad", (2, 48, 32, 3, 1, 1, 128, 128), {"bf16x3": 2, "native": 2}, "full"),    # data gradient: contraction 32, output 48
    Row("wino_x3_128", "fwd", (2, 32, 128, 3, 1, 1, 128, 128), {"bf16x3": 10, "native": 2}, "full"),  # cout 128: the bf16x3 Winograd GEMM
    Row("wino_h2_c256", "fwd", (1, 256, 256, 3, 1, 1, 8, 8), {"f16x2": 14}, patch=(("WINOGRAD_MIN_TILES", 16),)),  # f16x2: min_c 256 -> Winograd
    Row("wino_h2_c252", "fwd", (1, 252, 256, 3, 1, 1, 8, 8), {"f16x2": 13}, patch=(("WINOGRAD_MIN_TILES", 16),)),  # 252 < 256 -> direct
    # ---- transposed convs (data gradient of a stride-2 conv): run_phases merges the four phases into one launch when every phase has
    # cdiv(M_i, 128) * RP/128 < 384 (small_all) or, bf16x3 / f16x2, cdiv(M_i, 256) * RP/128 >= 512 (big_all); else one launch per phase
    Row("tconv_small_all", "dgrad", (1, 48, 33, 3, 2, 0, 311, 627), DIRECT, "bra"),  # phase 0 156 x 314 = 48984 px: 383 tiles -> merged
    Row("tconv_not_small", "dgrad", (1, 48, 33, 3, 2, 0, 311, 629), DIRECT, "bra"),  # phase 0 156 x 315 = 49140: 384 -> four launches
    Row("tconv_big_all", "dgrad", (1, 48, 33, 3, 2, 0, 725, 725), DIRECT),           # smallest phase 362^2 = 131044: 512 tiles -> merged 256x128
    Row("tconv_not_big", "dgrad", (1, 48, 33, 3, 2, 0, 723, 725), DIRECT),           # smallest phase 361 x 362: 511 -> per-phase launches
    # ---- f16 activations: halo_eligible (stride 1, RP <= 64, CP <= 64, Hp and Wp >= 16, weight slices <= 36 864 bytes)
    Row("halo_16", "fwd", (2, 32, 64, 3, 1, 1, 16, 16), {"f16": 6}, "bra", halo=True),     # Hp 16: eligible (9 x 64 x 32 halfs = 36 864 B)
    Row("halo_15", "fwd", (2, 32, 64, 3, 1, 1, 15, 17), {"f16": 6}, "bra", halo=False),    # Hp 15 < 16 -> gather kernel
    Row("halo_c40_o32", "fwd", (1, 40, 32, 3, 1, 1, 17, 20), {"f16": 6}, halo=True),      # CP 64, RP 32: 36 864 B -> eligible
    Row("halo_c40_o40", "fwd", (1, 40, 40, 3, 1, 1, 17, 20), {"f16": 6}, halo=False),     # CP 64, RP 64: 73 728 B -> gather
    Row("halo_o72", "fwd", (1, 32, 72, 3, 1, 1, 17, 20), {"f16": 6}, halo=False),         # RP 128 > 64 -> gather
    Row("halo_s2", "fwd", (2, 32, 32, 3, 2, 0, 33, 35), {"f16": 6}, halo=False),          # stride 2 -> gather
    Row("halo_dot_h24", "fwd", (2, 16, 24, 3, 1, 1, 24, 32), {"f16": 6}, "fuse", halo=True),  # eligible alone; the dot needs Hp % 16 == 0 -> gather
    Row("halo_dot_512", "fwd", (2, 8, 8, 3, 1, 1, 512, 512), {"f16": 6}, "fuse", halo=True),  # dot rows 1024 per sample: reduce_partials
                                                                                               #   Y > 1, nblk >= 1024, nblk % 16 == 0 branch
    Row("halo_dot_496", "fwd", (2, 8, 8, 3, 1, 1, 496, 496), {"f16": 6}, "fuse", halo=True),  # 961 rows per sample -> the plain branch
    # ---- f16 tile rules (BN 64 for cout <= 64; 256x256 when RP % 256 == 0 and cdiv(M, 256) * RP/256 >= 512; tiles128 < 384)
    Row("f16_t256_512", "fwd", (1, 72, 256, 1, 1, 0, 255, 514), {"f16": 6}),    # M 131070: 512 tiles of 256 -> 256x256 on 8 waves
    Row("f16_t256_511", "fwd", (1, 72, 256, 1, 1, 0, 255, 513), {"f16": 6}),    # 511 -> 128x128 split path
    Row("f16_t128_383", "fwd", (1, 72, 72, 1, 1, 0, 127, 386), {"f16": 6}),     # tiles128 383 -> 64x64
    Row("f16_t128_384", "fwd", (1, 72, 72, 1, 1, 0, 127, 387), {"f16": 6}, "bra"),  # 384 -> 128x128
    Row("f16_tconv_small", "dgrad", (1, 72, 33, 3, 2, 0, 311, 627), {"f16": 6}),  # merged phases (BN 128: 72 outputs > 64)
    Row("f16_tconv_not_small", "dgrad", (1, 72, 33, 3, 2, 0, 311, 629), {"f16": 6}),
    # ---- odd corners: B = 1, H != W, channel counts 4 / 9 / 17 / 33, 1x1 and 2x2-phase kernels
    Row("b1_c4_o9", "fwd", (1, 4, 9, 3, 1, 1, 7, 5), THIN, "bra"),
    Row("c17_o33_s2", "fwd", (3, 17, 33, 3, 2, 0, 17, 23), DENSE),  # 17 -> 20 active, cout_act 36 > 32: a strided FORWARD conv stays dense
    Row("c33_o17_1x1_s2", "fwd", (2, 33, 17, 1, 2, 0, 31, 19), DIRECT, "full"),
    Row("c33_o9_dgrad_1x1_s2", "dgrad", (2, 9, 33, 1, 2, 0, 31, 19), DIRECT),   # 1x1 stride 2: three empty phases (zero-filled)
    # ---- weight gradient (csrc/wgrad_route.h, wgrad_route): bf16x3 / f16x2 need tile_of(Cs) == 128 and tile_of(Cb) == 128 or x3_thin
    # (Cb <= 32, unscaled); small_wgrad_ok: 3x3 s1 p1, Cs <= 32, Cb <= 16, B*H*W >= 65536; wgrad_big_tile: Ntot >= 16384, RP % 256 == 0
    Row("wg_x3_thin", "wgrad", (2, 24, 48, 3, 1, 1, 33, 35), WGRAD),             # Cs 48 (128), Cb 24 (32) -> x3_thin
    Row("wg_x3", "wgrad", (2, 36, 40, 3, 2, 0, 33, 35), WGRAD),                  # both > 32 -> 128x128 bf16x3 / f16x2
    Row("wg_both_thin", "wgrad", (2, 24, 20, 3, 1, 1, 33, 35), WGRAD_NATIVE),    # Cs 20 <= 32 -> native kernel in every mode
    Row("wg_small_65536", "wgrad", (1, 12, 20, 3, 1, 1, 256, 256), WGRAD_NATIVE),  # Ntot 65536 -> conv_wgrad_small_mfma
    Row("wg_small_65280", "wgrad", (1, 12, 20, 3, 1, 1, 256, 255), WGRAD_NATIVE),  # 65280 -> generic 32x32
    Row("wg_big_16384", "wgrad", (1, 36, 129, 3, 1, 1, 128, 128), WGRAD),        # native: RP 256, Ntot 16384 -> 256x128 tiles
    Row("wg_big_16383", "wgrad", (1, 36, 129, 3, 1, 1, 127, 129), WGRAD),        # native: 16383 -> 128x128
    Row("wg_f16", "wgrad", (2, 24, 48, 3, 2, 0, 33, 35), {"f16": 7}),
    Row("wg_f16_1x1", "wgrad", (2, 72, 17, 1, 1, 0, 31, 19), {"f16": 7}),
    # Winograd weight gradient: Cs, Cb >= 64 and winograd_eligible with 2048 tiles (min_c: f16x2 256, else 0)
    Row("wwino_2048", "wgrad", (2, 64, 64, 3, 1, 1, 64, 64), {"f16x2": 15, "bf16x3": 11, "native": 3}),  # 2048 tiles -> Winograd (f16x2: min_c)
    Row("wwino_2046", "wgrad", (2, 64, 64, 3, 1, 1, 62, 66), WGRAD),              # 2046 -> direct
    Row("wwino_cb60", "wgrad", (2, 60, 64, 3, 1, 1, 64, 64), WGRAD),              # Cb 60 < 64 -> direct
]
CONV_CASES = [pytest.param(r, m, id=f"{r.name}-{m}", marks=pytest.mark.gpu) for r in ROWS for m in r.fams]

# ---- fp64 references, cached per (row shape, epilogue, rounding): the fp32 modes share one
_REF = {}


def _operands(row, f16):
    """CPU fp32 operands of a row (f16: rounded to half where the kernels read half)."""
    B, Ci, Co, K, s, p, H, W = row.shape
    Hs, Ws = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    g = torch.Generator().manual_seed(zlib.crc32(repr((row.shape, row.op, row.epi)).encode()))
    r16 = (lambda t: t.to(H16).float()) if f16 else (lambda t: t)
    cin_o, cout_o = (Ci, Co) if row.op != "dgrad" else (Co, Ci)  # channels of the op's input / output
    hw_in, hw_out = ((H, W), (Hs, Ws)) if row.op == "fwd" else ((Hs, Ws), (H, W))
    o = {"w": r16(torch.randn(Co, Ci, K, K, generator=g) / math.sqrt(Ci * K * K))}
    if row.op == "wgrad":
        o["small"] = r16(torch.randn(B, Co, Hs, Ws, generator=g))
        o["big"] = r16(torch.randn(B, Ci, H, W, generator=g))
        return o
    o["x"] = r16(torch.randn(B, cin_o, *hw_in, generator=g))
    ca, cb = cpad(cin_o, f16), cpad(cout_o, f16)
    if row.epi in ("full", "scale"):
        o["in_scale"] = torch.rand(B, ca, generator=g) + 0.5
        o["out_scale"] = torch.rand(B, cb, generator=g) + 0.5
    if row.epi in ("full", "bra"):
        o["bias"] = F.pad(torch.randn(cout_o, generator=g), (0, cb - cout_o))
        o["residual"] = F.pad(r16(torch.randn(B, cout_o, *hw_out, generator=g)), (0, 0, 0, 0, 0, cb - cout_o))
        o["act"] = True
    if row.epi == "fuse":
        o["mask_src"] = F.pad(r16(torch.randn(B, cout_o, *hw_out, generator=g)), (0, 0, 0, 0, 0, cb - cout_o))
        if (hw_out[0] * hw_out[1]) % 256 == 0:  # the dot fusion needs whole 256-row tiles per sample
            o["dot_src"] = F.pad(r16(torch.randn(B, cout_o, *hw_out, generator=g)), (0, 0, 0, 0, 0, cb - cout_o))
    return o


def _reference(row, f16):
    key = (row.shape, row.op, row.epi, f16)
    if key in _REF:
        return _REF[key]
    B, Ci, Co, K, s, p, H, W = row.shape
    o = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in _operands(row, f16).items()}
    w = o["w"]
    if row.op == "wgrad":
        def wg(gy, x, w_):
            with torch.enable_grad():
                ww = torch.zeros_like(w_, requires_grad=True)
                (gw,) = torch.autograd.grad(F.conv2d(x, ww, stride=s, padding=p), ww, gy)
            return gw
        out = {"y": (wg(o["small"], o["big"], w), wg(o["small"].abs(), o["big"].abs(), w))}
        _REF[key] = out
        return out
    x = o["x"]
    if "in_scale" in o:
        x = x * o["in_scale"][:, :x.shape[1], None, None]
    if row.op == "fwd":
        conv = lambda a, b: F.conv2d(a, b, stride=s, padding=p)
        cout_o = Co
    else:
        Hs, Ws = x.shape[2:]
        op_ = (H - ((Hs - 1) * s + K - 2 * p), W - ((Ws - 1) * s + K - 2 * p))
        conv = lambda a, b: F.conv_transpose2d(a, b, stride=s, padding=p, output_padding=op_)
        cout_o = Ci
    z, R = conv(x, w), conv(x.abs(), w.abs())
    cb = cpad(cout_o, f16)
    z, R = F.pad(z, (0, 0, 0, 0, 0, cb - cout_o)), F.pad(R, (0, 0, 0, 0, 0, cb - cout_o))
    out = {}
    if "dot_src" in o:
        out["dot"] = ((z * o["dot_src"]).sum((2, 3)), (R * o["dot_src"].abs()).sum((2, 3)))
    if "out_scale" in o:
        z, R = z * o["out_scale"][:, :, None, None], R * o["out_scale"][:, :, None, None].abs()
    if "residual" in o:
        z, R = z + o["residual"], R + o["residual"].abs()
    if "bias" in o:
        z, R = z + o["bias"][None, :, None, None], R + o["bias"][None, :, None, None].abs()
    if o.get("act"):
        z, R = 2 ** 0.5 * F.leaky_relu(z, 0.2), 2 ** 0.5 * R
    if "mask_src" in o:
        f = 2 ** 0.5 * torch.where(o["mask_src"] > 0, 1.0, 0.2).double()
        z, R = z * f, R * f
        out["colsum"] = (z.sum((0, 2, 3)), R.sum((0, 2, 3)))
    out["y"] = (z[:, :cout_o], R[:, :cout_o])
    _REF[key] = out
    return out


def _run(row, mode, o):
    """One call of the op through the default entry point; returns (output, GradFuse or None)."""
    from gif_amd import ops
    B, Ci, Co, K, s, p, H, W = row.shape
    spec = ops.ConvSpec(K, K, s, p)
    f16 = mode == "f16"
    dt = H16 if f16 else torch.float32
    w = o["w"].cuda()
    if row.op == "wgrad":
        return ops.conv_wgrad(_dev(o["small"], cpad(Co, f16), dt), _dev(o["big"], cpad(Ci, f16), dt), spec, Co, Ci), None
    cin_o = Ci if row.op == "fwd" else Co
    x = _dev(o["x"], cpad(cin_o, f16), dt)
    epi = {}
    for k in ("in_scale", "out_scale", "bias"):
        if k in o:
            epi[k] = o[k].cuda().contiguous()
    if "residual" in o:
        epi["residual"] = o["residual"].to(dt).cuda().contiguous(memory_format=CL)
    if o.get("act"):
        epi["act"] = True
    fuse = None
    if "mask_src" in o:
        fuse = ops.GradFuse(mask_src=o["mask_src"].to(dt).cuda().contiguous(memory_format=CL), mask_slope=0.2, mask_gain=2 ** 0.5,
                            want_colsum=True,
                            dot_src=o["dot_src"].to(dt).cuda().contiguous(memory_format=CL) if "dot_src" in o else None)
        epi["fuse"] = fuse
    if row.op == "fwd":
        return ops.conv_fwd(x, w, spec, **epi), fuse
    return ops.conv_bwd_data(x, w, spec, (H, W), **epi), fuse


@pytest.mark.parametrize("row,mode", CONV_CASES)
def test_conv_route_vs_fp64(row, mode):
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, Ci, Co, K, s, p, H, W = row.shape
    f16 = mode == "f16"
    saved_mode = ops.get_fp32_mfma_mode()
    saved = [(k, getattr(ops, k)) for k, _ in row.patch]
    try:
        for k, v in row.patch:
            setattr(ops, k, v)
        if not f16:
            ops.set_fp32_mfma_mode(mode)
        o = _operands(row, f16)
        ref = _reference(row, f16)
        ops.h2_fallback_stats(reset=True)
        ops.prof_enable(True)
        for fam in range(18):
            ops.prof_read(fam)  # (reading clears a family's records)
        n_wino = ops.prof_winograd_calls()
        y, fuse = _run(row, mode, o)
        torch.cuda.synchronize()
        launches = {fam: ops.prof_read(fam)[2] for fam in range(18)}
        ops.prof_enable(False)
        # ---- route: the op ran once, in the family the row names
        fam = row.fams[mode]
        ran = {f: n for f, n in launches.items() if n and f != 4}  # (4: Winograd transforms, recorded beside the GEMM)
        assert ran == {fam: 1}, f"{row.name} [{mode}]: expected one op in family {fam}, got {ran}"
        wino = fam in WINO_FAM or fam in WWINO_FAM
        assert ops.prof_winograd_calls() - n_wino == (1 if wino else 0), f"{row.name} [{mode}]: Winograd route {'not ' if wino else ''}taken"
        if row.halo is not None:
            Hs, Ws = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
            assert bool(lib.gif_conv2d_f16_halo_eligible(cpad(Ci, True), cpad(Co, True), K, K, s, Hs, Ws)) == row.halo, row.name
        if fam in (8, 13) or (fam == 5 and mode in ("f16x2", "bf16x3")):
            # the direct bf16x3 / f16x2 kernels run exactly the contractions gif_conv2d_x3_eligible accepts
            c_in, c_out = (cpad(Ci, False), cpad(Co, False)) if row.op == "fwd" else (cpad(Co, False), cpad(Ci, False))
            assert lib.gif_conv2d_x3_eligible(c_out, c_in) == (1 if fam in (8, 13) else 0), row.name
        # ---- contract
        if mode == "f16x2":
            assert ops.h2_fallback_stats() == 0, f"{row.name}: well-scaled operands took the guarded bf16x3 fallback"
        if row.op == "wgrad":
            assert y.shape == (Co, Ci, K, K) and y.dtype == torch.float32
        else:
            c_out = Ci if row.op == "dgrad" else Co
            hw = (H, W) if row.op == "dgrad" else ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)
            assert y.shape == (B, cpad(c_out, f16), *hw) and y.dtype == (H16 if f16 else torch.float32), (y.shape, y.dtype)
            assert torch.count_nonzero(y[:, c_out:]).item() == 0, f"{row.name}: padded output channels are not zero"
            y2, _ = _run(row, mode, o)
            assert torch.equal(y, y2), f"{row.name} [{mode}]: a second call gave different bits"
            y = y[:, :c_out]
        got = y.double().cpu()
        assert torch.isfinite(got).all(), f"{row.name}: NaN / Inf"
        _check(got, *ref["y"], mode, f"{row.name} out")
        if fuse is not None:
            _check(fuse.colsum.double().cpu(), *ref["colsum"], mode, f"{row.name} colsum")
            if "dot" in ref:
                _check(fuse.dot.double().cpu(), *ref["dot"], mode, f"{row.name} dot")
    finally:
        ops.prof_enable(False)
        ops.set_fp32_mfma_mode(saved_mode)
        for k, v in saved:
            setattr(ops, k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# FIR and reduction routes (csrc/elementwise.hip upfirdn2d_impl, gif::reduce_partials)
# ---------------------------------------------------------------------------------------------------------------------------------
def fir64(x, k, up, down, pad0, out_hw, flip=True):
    """fp64 upfirdn2d with the entry point's (pad0, out_hw) convention, as a sum of shifted slices (no im2col: the blur rows have
    33 M elements).  test_fir64_matches_the_oracle ties it to oracle.stylegan2_ref.upfirdn2d."""
    B, C, H, W = x.shape
    KH, KW = k.shape
    Ho, Wo = out_hw
    if up > 1:
        z = x.new_zeros(B, C, H * up, W * up)
        z[:, :, ::up, ::up] = x
    else:
        z = x
    Hp, Wp = (Ho - 1) * down + KH, (Wo - 1) * down + KW
    canvas = x.new_zeros(B, C, Hp, Wp)
    h, w_ = min(z.shape[2], Hp - pad0), min(z.shape[3], Wp - pad0)
    canvas[:, :, pad0:pad0 + h, pad0:pad0 + w_] = z[:, :, :h, :w_]
    kf = torch.flip(k, [0, 1]) if flip else k
    out = x.new_zeros(B, C, Ho, Wo)
    for i in range(KH):
        for j in range(KW):
            out += kf[i, j] * canvas[:, :, i:i + (Ho - 1) * down + 1:down, j:j + (Wo - 1) * down + 1:down]
    return out


def test_fir64_matches_the_oracle():
    """The slice-sum reference of the FIR rows is the oracle's upfirdn2d (stylegan2_ref: zero insertion, pad, flipped conv2d)."""
    from oracle import stylegan2_ref as R
    g = torch.Generator().manual_seed(5)
    k = torch.rand(4, 4, generator=g, dtype=torch.float64) + 0.5
    for up, down, pad0, H, W, Ho, Wo in [(2, 1, 2, 7, 5, 14, 10), (2, 1, 1, 7, 5, 13, 9), (1, 2, 1, 9, 8, 4, 4), (1, 1, 1, 9, 6, 9, 6),
                                         (1, 1, 2, 5, 7, 6, 8), (2, 1, 2, 6, 6, 11, 11)]:
        x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        p1 = max((Ho - 1) * down + 4 - (H * up + pad0), (Wo - 1) * down + 4 - (W * up + pad0))
        want = R.upfirdn2d(x, k, up, down, (pad0, p1))[:, :, :Ho, :Wo]  # (the larger pad only extends one side's output)
        got = fir64(x, k, up, down, pad0, (Ho, Wo))
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13), (up, down, pad0, H, W)


class FirRow(NamedTuple):
    name: str
    B: int
    C: int
    H: int
    W: int
    up: int
    down: int
    pad0: int
    out: tuple
    epi: str = ""   # "" | bra (bias + residual + act) | fuse (mask + colsum: blur only)


FIR_ROWS = [
    # ---- up-by-2 block kernel (up 2, 4x4, B * Ho <= 65535): both pad parities, odd Ho / Wo
    FirRow("up2_even", 3, 8, 37, 29, 2, 1, 2, (74, 58)),            # pad0 2 (StyleGAN's upsample)
    FirRow("up2_odd", 3, 8, 37, 29, 2, 1, 1, (73, 57)),             # pad0 1: blocks open on the other parity, odd Ho / Wo
    FirRow("up2_even_bra", 3, 8, 37, 29, 2, 1, 2, (75, 59), "bra"),  # odd Ho / Wo with bias + residual + leaky ReLU
    FirRow("up2_odd_bra", 2, 16, 33, 34, 2, 1, 1, (65, 67), "bra"),
    FirRow("up2_bho_65535", 3, 8, 10923, 3, 2, 1, 2, (21845, 6)),   # B * Ho = 65535: block kernel
    FirRow("up2_bho_65536", 4, 8, 8192, 3, 2, 1, 2, (16384, 6)),    # 65536: the generic upfirdn2d kernel
    FirRow("up2_bho_65532_bra", 4, 8, 8192, 3, 2, 1, 1, (16383, 5), "bra"),  # 65532: block kernel, odd pad, with epilogue
    # ---- down-by-2 resample kernel (B * Ho <= 65535) and the generic kernel above it
    FirRow("down2", 2, 8, 37, 41, 1, 2, 1, (18, 20)),
    FirRow("down2_pad2", 3, 16, 32, 31, 1, 2, 2, (17, 16)),
    FirRow("down2_generic", 2, 8, 65542, 4, 1, 2, 1, (32770, 2)),   # B * Ho = 65540 > 65535: generic kernel
    # ---- blur (up = down = 1): rows kernel when B * cdiv(Ho,16) * cdiv(Wo,4) * C/4 >= 131072, else tiled; mask + colsum fusion.
    # The colsum reduces one partial row per workgroup: reduce_partials(Y = 1, nblk = grid): nblk > 512 -> 64 groups (+ a tail group)
    FirRow("blur_tiled_small", 2, 8, 38, 42, 1, 1, 1, (37, 41), "fuse"),    # tiled, grid 4: single-stage reduction
    FirRow("blur_tiled_tail", 1, 4, 261, 4097, 1, 1, 1, (260, 4096), "fuse"),  # tiled total 133120: grid 520 -> per 9, 57 groups + tail 7
    FirRow("blur_tiled_131008", 1, 4, 1025, 8189, 1, 1, 1, (1024, 8188), "fuse"),  # rows total 131008 < 131072 -> tiled; grid 4094:
                                                                                    #   per 64, 63 groups + tail 62
    FirRow("blur_rows_131072", 1, 4, 1025, 8190, 1, 1, 1, (1024, 8189), "fuse"),   # 131072 -> rows kernel; grid 512: single stage
    FirRow("blur_rows_513", 1, 4, 1025, 8194, 1, 1, 1, (1024, 8193), "fuse"),      # 131136 -> grid 513: 57 groups of 9, no tail
    FirRow("blur_rows_tail", 1, 4, 1041, 8190, 1, 1, 1, (1040, 8189), "fuse"),     # 133120 -> grid 520: 57 groups + tail 7
    FirRow("blur_plain_c24", 2, 24, 20, 19, 1, 1, 2, (21, 20)),             # 24 channels (no fusion: not a power of two)
]
FIR_CASES = [pytest.param(r, dt, id=f"{r.name}-{'f16' if dt == H16 else 'f32'}", marks=pytest.mark.gpu)
             for r in FIR_ROWS for dt in (torch.float32, H16) if not (dt == H16 and r.C % 8)]


@pytest.mark.parametrize("row,dt", FIR_CASES)
def test_fir_route_vs_fp64(row, dt):
    from gif_amd import ops
    mode = "fir16" if dt == H16 else "fir32"
    g = torch.Generator().manual_seed(zlib.crc32(repr(row).encode()))
    r16 = (lambda t: t.to(H16).float()) if dt == H16 else (lambda t: t)
    x = r16(torch.randn(row.B, row.C, row.H, row.W, generator=g))
    k = torch.rand(4, 4, generator=g) + 0.25  # asymmetric: a flipped or transposed tap order shows
    k = k / k.sum() * row.up ** 2
    Ho, Wo = row.out
    ref = fir64(x.double(), k.double(), row.up, row.down, row.pad0, (Ho, Wo))
    R = fir64(x.double().abs(), k.double(), row.up, row.down, row.pad0, (Ho, Wo))
    kw, fuse = {}, None
    if row.epi == "bra":
        bias = torch.randn(row.C, generator=g)
        res = r16(torch.randn(row.B, row.C, Ho, Wo, generator=g))
        kw = dict(bias=bias.cuda(), residual=res.to(dt).cuda().contiguous(memory_format=CL), act=True)
        ref = 2 ** 0.5 * F.leaky_relu(ref + res.double() + bias.double()[None, :, None, None], 0.2)
        R = 2 ** 0.5 * (R + res.double().abs() + bias.double().abs()[None, :, None, None])
    if row.epi == "fuse":
        m = r16(torch.randn(row.B, row.C, Ho, Wo, generator=g))
        fuse = ops.GradFuse(mask_src=m.to(dt).cuda().contiguous(memory_format=CL), mask_slope=0.2, mask_gain=2 ** 0.5, want_colsum=True)
        f = 2 ** 0.5 * torch.where(m > 0, 1.0, 0.2).double()
        ref, R = ref * f, R * f
        kw = dict(fuse=fuse)
    xd = x.to(dt).cuda().contiguous(memory_format=CL)
    kd = k.cuda()
    y = ops.upfirdn2d(xd, kd, row.up, row.down, row.pad0, (Ho, Wo), **kw)
    assert y.shape == (row.B, row.C, Ho, Wo) and y.dtype == dt
    if fuse is not None:
        fuse2 = ops.GradFuse(mask_src=fuse.mask_src, mask_slope=0.2, mask_gain=2 ** 0.5, want_colsum=True)
        y2 = ops.upfirdn2d(xd, kd, row.up, row.down, row.pad0, (Ho, Wo), fuse=fuse2)
        assert torch.equal(fuse.colsum, fuse2.colsum), f"{row.name}: the fused column sums changed between two calls"
    else:
        y2 = ops.upfirdn2d(xd, kd, row.up, row.down, row.pad0, (Ho, Wo), **kw)
    assert torch.equal(y, y2), f"{row.name}: a second call gave different bits"
    got = y.double().cpu()
    del y, y2
    assert torch.isfinite(got).all()
    _check(got, ref, R, mode, f"{row.name} out")
    if fuse is not None:
        _check(fuse.colsum.double().cpu(), ref.sum((0, 2, 3)), R.sum((0, 2, 3)), mode, f"{row.name} colsum")
