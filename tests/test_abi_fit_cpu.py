"""The two C entry points of the FLAME fit (gif_pose_chain_bwd_f32 in flame.hip, gif_landmark_loss_f32 in flame_fit.hip) at empty sizes
and with bad arguments, without a GPU — in the manner of tests/test_abi_empty_cpu.py: every pointer null, no stream.  A no-op row
returns 0 before anything touches a device; a refusal is GIF_EINVAL (-1) with a message that names the check.  (L = 0 with B > 0
zero-fills the loss when one is given: that needs a device, tests/test_gpu_flame_fit.py runs it.)
"""
import ctypes

import pytest

from gif_amd import _lib

N = None
PARENTS5 = (ctypes.c_int32 * 5)(-1, 0, 1, 1, 1)
PARENTS1 = (ctypes.c_int32 * 1)(-1)
LATER = (ctypes.c_int32 * 5)(-1, 0, 2, 1, 1)   # joint 2 names itself
BELOW = (ctypes.c_int32 * 5)(-1, -2, 1, 1, 1)  # -2 is neither a joint nor "no parent"
ONE = ctypes.cast((ctypes.c_float * 512)(), ctypes.c_void_p).value  # a non-null address no call below reads from: each stops earlier


def chain(parents, n_shape, n_exp, B, KP, J, ptr=N, outs=(N, N, N, N, N)):
    """(J0, Jdirs, parents, shape, ld, n_shape, expr, ld, n_exp, pose, ld, neck, ld, eye, ld, g_A, g_coef, 5 outputs, B, KP, J)"""
    return [ptr, ptr, parents, N, 0, n_shape, N, 0, n_exp, N, 0, N, 0, N, 0, ptr, ptr, *outs, B, KP, J]


NOOP = [
    ("gif_pose_chain_bwd_f32", chain(N, 3, 2, 0, 41, 5), "B == 0"),
    ("gif_pose_chain_bwd_f32", chain(N, 0, 0, 0, 0, 1), "B == 0, KP == 0, J = 1"),
    ("gif_pose_chain_bwd_f32", chain(N, 3, 2, 2, 41, 5), "all five outputs null"),
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 100, 50, 7, 186, 5), "all five outputs null, parents given"),
    # (lmk, cam, target, weight, loss, g_lmk, g_cam, B, L)
    ("gif_landmark_loss_f32", [N] * 7 + [0, 68], "B == 0"),
    ("gif_landmark_loss_f32", [N] * 7 + [0, 0], "B == 0 and L == 0"),
    ("gif_landmark_loss_f32", [N] * 7 + [3, 0], "L == 0, no loss given: nothing to zero"),
]

OUT = (ONE, N, N, N, N)
REFUSED = [
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, 2, 41, 0, outs=OUT), b"bad dims"),    # J = 0
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, 2, 77, 9, outs=OUT), b"bad dims"),    # J = 9
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, -1, 41, 5, outs=OUT), b"bad dims"),   # B < 0
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, 2, 40, 5, outs=OUT), b"bad dims"),    # KP != n_shape + n_exp + 9 (J - 1)
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, 0, 40, 5), b"bad dims"),              # (refused even where nothing would run)
    ("gif_pose_chain_bwd_f32", chain(LATER, 3, 2, 2, 41, 5, ptr=ONE, outs=OUT), b"not an earlier joint"),
    ("gif_pose_chain_bwd_f32", chain(BELOW, 3, 2, 2, 41, 5, ptr=ONE, outs=OUT), b"not an earlier joint"),
    ("gif_pose_chain_bwd_f32", chain(N, 3, 2, 2, 41, 5, ptr=ONE, outs=OUT), b"null pointer"),       # parents
    ("gif_pose_chain_bwd_f32", chain(PARENTS5, 3, 2, 2, 41, 5, outs=OUT), b"null pointer"),        # J0, Jdirs, g_A, g_coef
    ("gif_pose_chain_bwd_f32", chain(PARENTS1, 0, 0, 2, 0, 1, outs=(N, N, ONE, N, N)), b"null pointer"),  # J0 and g_A (KP = 0 needs no g_coef)
    ("gif_landmark_loss_f32", [N] * 7 + [-1, 68], b"bad dims"),
    ("gif_landmark_loss_f32", [N] * 7 + [2, -1], b"bad dims"),
    ("gif_landmark_loss_f32", [N] * 7 + [2, 68], b"null pointer"),
    ("gif_landmark_loss_f32", [ONE, ONE, ONE, N, N, N, N, 2, 68], b"null pointer"),  # no loss to write to
    ("gif_landmark_loss_f32", [ONE, N, ONE, N, ONE, N, N, 2, 68], b"null pointer"),  # no camera
]


def _ids(rows):
    return [f"{r[0][4:]}-{i}" for i, r in enumerate(rows)]


@pytest.mark.parametrize("entry,args,why", NOOP, ids=_ids(NOOP))
def test_nothing_to_do_returns_0_with_every_pointer_null(entry, args, why):
    lib = _lib.load()
    rc = getattr(lib, entry)(*args, None)
    assert rc == 0, f"{entry} ({why}): rc {rc}, {lib.gif_last_error().decode(errors='replace')}"


@pytest.mark.parametrize("entry,args,text", REFUSED, ids=_ids(REFUSED))
def test_bad_arguments_are_refused_before_any_launch(entry, args, text):
    lib = _lib.load()
    assert getattr(lib, entry)(*args, None) == -1
    assert text in lib.gif_last_error(), lib.gif_last_error()


def test_both_entry_points_are_bound_and_the_abi_version_stays():
    lib = _lib.load()
    assert {"gif_pose_chain_bwd_f32", "gif_landmark_loss_f32"} <= set(_lib.PROTOTYPES)
    assert lib.gif_abi_version() == 4  # additions only
    assert {r[0] for r in NOOP} == {r[0] for r in REFUSED} == {"gif_pose_chain_bwd_f32", "gif_landmark_loss_f32"}


def test_fused_chain_keyword_and_cpu_tensors():
    import numpy as np
    import torch
    from gif_amd import fitting, flame as fl
    rng = np.random.RandomState(0)
    model = fl.synthetic_flame_model(rng.randn(9, 3) * 0.1, 3, 2)
    emb = fl.synthetic_landmark_embedding(rng.randint(0, 9, (6, 3)), 2, 3, 2, 3)
    assert fl.FlameLayer(model, 3, 2).fused_chain is False and fl.FlameLandmarkLayer(model, emb, 3, 2).fused_chain is False
    layer = fl.FlameLayer(model, 3, 2, fused_chain=True)
    assert layer.fused_chain is True and fl.FlameLandmarkLayer(model, emb, 3, 2, fused_chain=True).fused_chain is True
    with pytest.raises(_lib.GifHipError):
        layer(torch.zeros(2, 3, requires_grad=True))
    with pytest.raises(_lib.GifHipError):
        fitting.landmark_loss(torch.zeros(2, 5, 3), torch.zeros(2, 3), torch.zeros(2, 5, 2))
