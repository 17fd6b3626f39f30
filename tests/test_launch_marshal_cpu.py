"""_lib.marshal — what _lib.launch hands to ctypes — and _lib.require_device on the host: no GPU, no library load."""
import ctypes

import pytest
import torch

from gif_amd import _lib


def test_marshal_passes_addresses_and_leaves_the_rest():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    empty = torch.zeros((2, 0, 3))
    parents = (ctypes.c_int32 * 3)(-1, 0, 1)
    stride, scale = 7, 0.5
    got = _lib.marshal("gif_x_f32", (t, None, parents, stride, scale, t[1], empty, t.data_ptr()))
    assert got[0] == t.data_ptr() and got[1] is None
    assert got[2] is parents and got[3] is stride and got[4] is scale
    assert got[5] == t.data_ptr() + 16  # a contiguous view: its own address
    assert got[6] == empty.data_ptr() and got[7] == t.data_ptr()
    assert _lib.marshal("gif_x_f32", ()) == []


def test_marshal_refuses_a_non_contiguous_tensor():
    t = torch.zeros(4, 6)
    for pos, bad in ((0, t[:, :3]), (2, t.t()), (3, t[::2])):
        args = [1, None, t, 2.0]
        args[pos:pos + 1] = [bad]
        with pytest.raises(_lib.GifHipError, match=rf"gif_entry_f32: argument {pos} is not contiguous"):
            _lib.marshal("gif_entry_f32", args)


def test_require_device_names_the_argument():
    _lib.require_device("op", a=None)
    with pytest.raises(_lib.GifHipError, match=r"op needs device tensors \(no CPU fallback\): b"):
        _lib.require_device("op", a=None, b=torch.zeros(1))
    with pytest.raises(_lib.GifHipError, match="device tensors.*: c"):
        _lib.require_device("op", c=[1.0])
