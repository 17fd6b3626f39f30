"""What the convolution entry points whose host bodies are shared answer to a call they refuse, without a GPU.

The weight-packing entry points run through two host functions (pack_plain in csrc/weight_pack.hip, pack_h2 in csrc/conv_wgrad.hip), the
four gif_conv2d_wgrad_* through one template and the three gif_conv3x3_winograd_wgrad_* through one implementation
(csrc/conv_wgrad.hip), and the fused column-sum / dot
workspace of the forward and data-gradient entry points (csrc/conv_igemm.hip) is carved by one helper (csrc/common.h FusedSums).  A
check dropped, reordered or given another entry's name in such a shared body changes what a refused call reports.  Every row below is
a call that a GIF_REQUIRE refuses before the first HIP call (the pointers are never dereferenced: 0x1000 stands for "not null"), or a
pure size query; the row's comment names the guard, each was read for it.  tests/golden/conv_entry_texts_golden.json
(tests/golden/make_conv_entry_texts_golden.py) holds the return code and the exact gif_last_error() text, or the returned value, of
every row as the library answered at the commit before the bodies were merged; this module compares.

The packing, dims / splits queries are also held to their values over the route tables' geometries by tests/test_conv_route.py and
tests/test_wgrad_route.py; here they appear for their refusals and degenerate arguments.
"""
import ctypes
import json
import os

import pytest

from gif_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_entry_texts_golden.json")
D = 0x1000  # a pointer that is not null
N = None
ST = [576, 9, 3, 1, 1.0]  # sr, sc, sky, skx, scale
PI = ctypes.pointer(ctypes.c_int())  # where a dims query may write


def geom(B, Hb, Wb, Cb, Hs, Ws, Cs, KH=3, KW=3, stride=1, pad=1):
    return _lib.ConvGeom(B, Hb, Wb, Cb, Hs, Ws, Cs, KH, KW, stride, pad)


def epi(**fields):
    return _lib.ConvEpilogue(**fields)


G64 = geom(2, 16, 16, 64, 16, 16, 64)     # a plain 3x3 layer
G16 = geom(2, 16, 16, 16, 16, 16, 32)     # thin big side: the tap-dense forms take it (forward)
G16T = geom(2, 16, 16, 32, 16, 16, 16)    # thin small side: the tap-dense forms take it (data gradient)
G8 = geom(2, 8, 8, 64, 8, 8, 64)          # 64 output pixels per sample
GS2 = geom(2, 16, 16, 64, 8, 8, 64, 3, 3, 2, 1)
NO_WS = epi(colsum=D)                      # column sums asked for, no red_ws
NO_WS_DOT = epi(dot=D)                     # dot asked for: no red_ws AND no dot_src — red_ws is reported
NO_SRC = epi(dot=D, red_ws=D)              # dot without dot_src
DOT = epi(dot=D, dot_src=D, red_ws=D)

# (id, kind, entry, arguments without the stream); kind "err": a refused launch, "val": a query's value, "dims": (rc, [RP, CP]),
# "modes": a query's value in each of the three fp32 contraction modes
ROWS = [
    # ---- weight_pack.hip, pack_plain<T>: the one GIF_REQUIRE, under the entry's own name
    ("pack_f32-null", "err", "gif_pack_weight_f32", [N, D, 8, 8, 3, 3, 32, 32] + ST),        # w
    ("pack_f32-rp", "err", "gif_pack_weight_f32", [D, D, 40, 8, 3, 3, 32, 32] + ST),         # RP >= R
    ("pack_f32-cp", "err", "gif_pack_weight_f32", [D, D, 8, 40, 3, 3, 32, 32] + ST),         # CP >= C
    ("pack_f32-kh", "err", "gif_pack_weight_f32", [D, D, 8, 8, 0, 3, 32, 32] + ST),          # KH > 0
    ("pack_f16-null", "err", "gif_pack_weight_f16", [D, N, 8, 8, 3, 3, 32, 32] + ST),        # wp
    ("pack_f16-rp", "err", "gif_pack_weight_f16", [D, D, 40, 8, 3, 3, 32, 32] + ST),         # RP >= R
    # gif_pack_weight_f32x3: its GIF_REQUIRE
    ("pack_f32x3-null", "err", "gif_pack_weight_f32x3", [D, N, 8, 8, 3, 3, 32, 32] + ST),    # wp3
    ("pack_f32x3-rp", "err", "gif_pack_weight_f32x3", [D, D, 40, 8, 3, 3, 32, 32] + ST),     # RP >= R
    # ---- conv_wgrad.hip, the f16x2 packings.  gif_pack_weight_f32h2: its GIF_REQUIRE, then the LDS size in pack_h2
    ("pack_f32h2-rp", "err", "gif_pack_weight_f32h2", [D, D, 40, 8, 3, 3, 32, 32] + ST),     # RP >= R
    ("pack_f32h2-rp32", "err", "gif_pack_weight_f32h2", [D, D, 8, 8, 3, 3, 48, 32] + ST),    # RP % 32
    ("pack_f32h2-cp32", "err", "gif_pack_weight_f32h2", [D, D, 8, 8, 3, 3, 32, 48] + ST),    # CP % 32
    ("pack_f32h2-lds", "err", "gif_pack_weight_f32h2", [D, D, 8, 8, 3, 3, 32, 2048] + ST),   # 9 x 2048 floats > 64 KB
    # gif_pack_weight_f32h2x3: the same with wp3
    ("pack_f32h2x3-wp3", "err", "gif_pack_weight_f32h2x3", [D, D, N, 8, 8, 3, 3, 32, 32] + ST),     # wp3
    ("pack_f32h2x3-rp", "err", "gif_pack_weight_f32h2x3", [D, D, D, 40, 8, 3, 3, 32, 32] + ST),     # RP >= R
    ("pack_f32h2x3-rp32", "err", "gif_pack_weight_f32h2x3", [D, D, D, 8, 8, 3, 3, 48, 32] + ST),    # RP % 32
    ("pack_f32h2x3-lds", "err", "gif_pack_weight_f32h2x3", [D, D, D, 8, 8, 3, 3, 32, 2048] + ST),   # pack_h2: LDS size
    # tap-dense forms (.., R, C, cin_act, KH, KW, RP, ..): their GIF_REQUIRE (f32h2x3: conv_wgrad.hip, f32x3: weight_pack.hip)
    ("pack_h2x3_td-rp", "err", "gif_pack_weight_f32h2x3_tapdense", [D, D, D, 40, 8, 16, 3, 3, 32] + ST),    # RP >= R
    ("pack_h2x3_td-rp32", "err", "gif_pack_weight_f32h2x3_tapdense", [D, D, D, 8, 8, 16, 3, 3, 48] + ST),   # RP % 32
    ("pack_h2x3_td-cin", "err", "gif_pack_weight_f32h2x3_tapdense", [D, D, D, 8, 16, 12, 3, 3, 32] + ST),   # cin_act >= C
    ("pack_h2x3_td-1x1", "err", "gif_pack_weight_f32h2x3_tapdense", [D, D, D, 8, 8, 16, 1, 1, 32] + ST),    # steps > 0 (not 3x3)
    ("pack_h2x3_td-wp3", "err", "gif_pack_weight_f32h2x3_tapdense", [D, D, N, 8, 8, 16, 3, 3, 32] + ST),    # wp3
    ("pack_x3_td-rp", "err", "gif_pack_weight_f32x3_tapdense", [D, D, 40, 8, 16, 3, 3, 32] + ST),           # RP >= R
    ("pack_x3_td-cin", "err", "gif_pack_weight_f32x3_tapdense", [D, D, 8, 16, 12, 3, 3, 32] + ST),          # cin_act >= C
    ("pack_x3_td-1x1", "err", "gif_pack_weight_f32x3_tapdense", [D, D, 8, 8, 16, 1, 1, 32] + ST),           # steps > 0 (not 3x3)
    ("pack_x3_td-cin32", "err", "gif_pack_weight_f32x3_tapdense", [D, D, 8, 8, 32, 3, 3, 32] + ST),         # steps > 0 (cin_act >= 32)
    # the packings' size queries (pure arithmetic)
    ("h2_bytes", "val", "gif_pack_weight_f32h2_bytes", [3, 3, 64, 96]),
    ("h2_bytes-1x1", "val", "gif_pack_weight_f32h2_bytes", [1, 1, 32, 32]),
    ("h2_bytes-kh0", "val", "gif_pack_weight_f32h2_bytes", [0, 3, 64, 96]),
    ("h2_bytes-rp0", "val", "gif_pack_weight_f32h2_bytes", [3, 3, 0, 96]),
    ("h2_td_bytes", "val", "gif_pack_weight_f32h2_tapdense_bytes", [16, 3, 3, 64]),
    ("h2_td_bytes-1x1", "val", "gif_pack_weight_f32h2_tapdense_bytes", [16, 1, 1, 64]),
    ("h2_td_bytes-rp0", "val", "gif_pack_weight_f32h2_tapdense_bytes", [16, 3, 3, 0]),
    ("td_steps-8", "val", "gif_conv2d_x3_tapdense_steps", [8, 3, 3]),
    ("td_steps-12", "val", "gif_conv2d_x3_tapdense_steps", [12, 3, 3]),
    ("td_steps-28", "val", "gif_conv2d_x3_tapdense_steps", [28, 3, 3]),
    ("td_steps-4", "val", "gif_conv2d_x3_tapdense_steps", [4, 3, 3]),
    ("td_steps-32", "val", "gif_conv2d_x3_tapdense_steps", [32, 3, 3]),
    ("td_steps-10", "val", "gif_conv2d_x3_tapdense_steps", [10, 3, 3]),
    ("td_steps-3x1", "val", "gif_conv2d_x3_tapdense_steps", [16, 3, 1]),
]

# ---- conv_wgrad.hip, conv2d_wgrad_impl<T>: its four GIF_REQUIREs in order, all before zero_page16() (the first HIP call)
for _e in ("f32", "f32x3", "f32h2", "f16"):
    _f = "gif_conv2d_wgrad_" + _e
    _odd = geom(2, 16, 16, 64, 16, 16, 12) if _e == "f16" else geom(2, 16, 16, 64, 16, 16, 6)
    ROWS += [
        (f"wgrad_{_e}-null", "err", _f, [D, D, N, N, N, G64, 1]),                                    # ws
        (f"wgrad_{_e}-geom", "err", _f, [D, D, D, N, N, N, 1]),                                      # g
        (f"wgrad_{_e}-nsplit0", "err", _f, [D, D, D, N, N, G64, 0]),                                 # nsplit >= 1
        (f"wgrad_{_e}-cs", "err", _f, [D, D, D, N, N, _odd, 1]),                                     # Cs % 8 (f16) / % 4
        (f"wgrad_{_e}-cb", "err", _f, [D, D, D, N, N, geom(2, 16, 16, 20 if _e == "f16" else 18, 16, 16, 64), 1]),  # Cb % 8 / % 4
        (f"wgrad_{_e}-kh4", "err", _f, [D, D, D, N, N, geom(2, 16, 16, 64, 16, 16, 64, 4, 3, 1, 1), 1]),   # KH <= 3
        (f"wgrad_{_e}-stride3", "err", _f, [D, D, D, N, N, geom(2, 16, 16, 64, 6, 6, 64, 3, 3, 3, 1), 1]),  # stride 1 or 2
        (f"wgrad_{_e}-2g", "err", _f, [D, D, D, N, N, geom(64, 1024, 1024, 8, 1024, 1024, 32), 1]),   # small side = 2^31 elements
    ]
# Cs = 12 is a multiple of 4: the fp32 forms would take it (no row: they go on to the device); Cs = 6 is refused by all four, with the
# multiple each names.
ROWS += [
    ("wgrad_f16-cs6", "err", "gif_conv2d_wgrad_f16", [D, D, D, N, N, geom(2, 16, 16, 64, 16, 16, 6), 1]),
    # the size queries of the direct weight gradient
    ("wgrad_dims", "dims", "gif_conv2d_wgrad_dims", [64, 96]),
    ("wgrad_dims-thin", "dims", "gif_conv2d_wgrad_dims", [12, 8]),
    ("wgrad_dims_f16", "dims", "gif_conv2d_wgrad_dims_f16", [64, 96]),
    ("wgrad_dims_f16-thin", "dims", "gif_conv2d_wgrad_dims_f16", [16, 8]),
    ("wgrad_dims-cs0", "err", "gif_conv2d_wgrad_dims", [0, 8, PI, PI]),            # Cs > 0
    ("wgrad_dims-null", "err", "gif_conv2d_wgrad_dims", [8, 8, N, PI]),           # RP
    ("wgrad_dims_f16-cb0", "err", "gif_conv2d_wgrad_dims_f16", [8, 0, PI, PI]),    # Cb > 0
    ("wgrad_dims_f16-null", "err", "gif_conv2d_wgrad_dims_f16", [8, 8, PI, N]),   # CP
    ("wgrad_splits", "modes", "gif_conv2d_wgrad_splits", [G64]),
    ("wgrad_splits-s2", "modes", "gif_conv2d_wgrad_splits", [GS2]),
    ("wgrad_splits-null", "modes", "gif_conv2d_wgrad_splits", [N]),
    ("wgrad_splits-b0", "modes", "gif_conv2d_wgrad_splits", [geom(0, 16, 16, 64, 16, 16, 64)]),
    ("wgrad_splits_f16", "modes", "gif_conv2d_wgrad_splits_f16", [G64]),
    ("wgrad_splits_f16-null", "modes", "gif_conv2d_wgrad_splits_f16", [N]),
    ("wino_wgrad_splits", "modes", "gif_conv3x3_winograd_wgrad_splits", [2, 16, 16, 64, 64]),
    ("wino_wgrad_splits-b0", "modes", "gif_conv3x3_winograd_wgrad_splits", [0, 16, 16, 64, 64]),
    ("wino_wgrad_splits-cb0", "modes", "gif_conv3x3_winograd_wgrad_splits", [2, 16, 16, 64, 0]),
]
# conv3x3_winograd_wgrad_impl (x, gy, V, Mg, ws, small_scale, big_scale, B, H, W, Cs, Cb, nsplit): four GIF_REQUIREs before the
# transforms' launches
for _e in ("f32", "f32x3", "f32h2"):
    _f = "gif_conv3x3_winograd_wgrad_" + _e
    ROWS += [
        (f"wino_wgrad_{_e}-null", "err", _f, [D, D, D, N, D, N, N, 2, 16, 16, 64, 64, 1]),           # Mg
        (f"wino_wgrad_{_e}-nsplit0", "err", _f, [D, D, D, D, D, N, N, 2, 16, 16, 64, 64, 0]),        # nsplit >= 1
        (f"wino_wgrad_{_e}-oddh", "err", _f, [D, D, D, D, D, N, N, 2, 15, 16, 64, 64, 1]),           # H % 2
        (f"wino_wgrad_{_e}-b0", "err", _f, [D, D, D, D, D, N, N, 0, 16, 16, 64, 64, 1]),             # B > 0
        (f"wino_wgrad_{_e}-cs6", "err", _f, [D, D, D, D, D, N, N, 2, 16, 16, 6, 64, 1]),             # Cs % 4
        (f"wino_wgrad_{_e}-2g", "err", _f, [D, D, D, D, D, N, N, 64, 2048, 2048, 32, 32, 1]),        # fits_i32(ntiles_pad * CsP)
    ]
# ---- conv_igemm.hip, fused column sums / dot: FusedSums::carve (red_ws) first, then sums_begin's own check.  Before it run check_geom,
# check_channels, the null-pointer check, check_tapdense and base_params, which reaches the runtime only for f16 (the saturation flag) and
# for f16x2 WITH a fallback packing (the gate): the fp32, bf16x3 and unguarded f16x2 (wp3 = NULL) forms are listed.
for _d, _g, _gt in (("fwd", G64, G16), ("bwd_data", G64, G16T)):
    for _e, _ptrs in (("f32", [D, D, D]), ("f32x3", [D, D, D]), ("f32h2", [D, D, N, D])):
        _f = f"gif_conv2d_{_d}_{_e}"
        ROWS += [
            (f"{_d}_{_e}-no_ws", "err", _f, _ptrs + [_g, NO_WS]),          # carve: red_ws
            (f"{_d}_{_e}-no_ws_dot", "err", _f, _ptrs + [_g, NO_WS_DOT]),  # carve: red_ws comes before the dot fusion's conditions
            (f"{_d}_{_e}-no_src", "err", _f, _ptrs + [_g, NO_SRC]),        # sums_begin: dot_src
            (f"{_d}_{_e}-hw64", "err", _f, _ptrs + [G8, DOT]),             # sums_begin: hw % 256
        ]
    for _e, _ptrs in (("f32x3_tapdense", [D, D, D]), ("f32h2_tapdense", [D, D, N, D])):
        _f = f"gif_conv2d_{_d}_{_e}"
        ROWS += [
            (f"{_d}_{_e}-no_ws", "err", _f, _ptrs + [_gt, NO_WS]),         # carve: red_ws
            (f"{_d}_{_e}-wide", "err", _f, _ptrs + [_g, N]),               # check_tapdense: gif_conv2d_x3_tapdense_steps == 0 (64 channels)
        ]
ROWS += [
    ("bwd_data_f32-s2_dot", "err", "gif_conv2d_bwd_data_f32", [D, D, D, GS2, DOT]),   # sums_begin: single phase (stride 2 has four)
    ("fwd_f32-null", "err", "gif_conv2d_fwd_f32", [D, N, D, G64, N]),                 # null pointer, before everything above
]

MODES = (0, 1, 2)  # gif_set_fp32_mfma_mode: native, bf16x3, f16x2


def answer(lib, kind, entry, args):
    """What the library answers for one row, as the golden file holds it."""
    fn = getattr(lib, entry)
    args = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args]
    if kind == "err":
        rc = fn(*args) if entry.endswith(("_dims", "_dims_f16")) else fn(*args, None)
        return {"rc": rc, "error": lib.gif_last_error().decode()}
    if kind == "dims":
        rp, cp = ctypes.c_int(), ctypes.c_int()
        return {"rc": fn(*args, ctypes.byref(rp), ctypes.byref(cp)), "value": [rp.value, cp.value]}
    if kind == "modes":
        before = lib.gif_get_fp32_mfma_mode()
        try:
            out = []
            for m in MODES:
                assert lib.gif_set_fp32_mfma_mode(m) == 0
                out.append(fn(*args))
        finally:
            lib.gif_set_fp32_mfma_mode(before)
        return {"value": out}
    return {"value": fn(*args)}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("rid,kind,entry,args", ROWS, ids=[r[0] for r in ROWS])
def test_answer_matches_the_recorded_one(rid, kind, entry, args):
    got = answer(_lib.load(), kind, entry, args)
    assert got == _golden()[rid], (entry, got)
    if kind == "err":  # every refusal is GIF_EINVAL with a text that names the check
        assert got["rc"] == -1 and got["error"]


def test_rows_and_golden_cover_the_merged_entry_points():
    assert len({r[0] for r in ROWS}) == len(ROWS) and list(_golden()) == [r[0] for r in ROWS]
    families = ("gif_pack_weight_", "gif_conv2d_wgrad_", "gif_conv3x3_winograd_wgrad_", "gif_conv2d_x3_tapdense_steps")
    assert {n for n in _lib.PROTOTYPES if n.startswith(families)} <= {r[2] for r in ROWS}
    # each entry reports under its own name: no two entry points of a family share a refusal text
    golden = _golden()
    for fam in ("gif_pack_weight_", "gif_conv2d_wgrad_f16"):
        texts = {}
        for rid, kind, entry, _ in ROWS:
            if kind == "err" and entry.startswith(fam):
                texts.setdefault(golden[rid]["error"], set()).add(entry)
        assert all(len(v) == 1 for v in texts.values()), texts
