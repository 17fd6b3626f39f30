"""CPU-side checks of the FLAME layer: the float64 restatement (tests/flame_ref.py) against the identities the kernels'
factorisation relies on, the synthetic model's properties, the .npz format, and the entry points' argument validation (which
happens before any launch, so it runs without a GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flame_ref
from gif_amd import _lib
from gif_amd import flame as fl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def template(V=257, seed=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    v = g["vertices"].astype(np.float64) * 0.1
    idx = np.random.RandomState(seed).permutation(v.shape[0])[:V]
    return v[np.sort(idx)]


def params(B, n_shape, n_exp, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda n, s: torch.randn(B, n, generator=g, dtype=torch.float64) * s
    return r(n_shape, 1.0), r(n_exp, 1.0), r(6, 0.15), r(3, 0.15), r(6, 0.15)


def test_joints_are_linear_in_betas():
    """joints = J_regressor . v_shaped equals J0 + betas . Jdirs (what gif_flame_joints_f32 evaluates) to 1e-12 in float64."""
    model = fl.synthetic_flame_model(template(), 20, 10, seed=3)
    c = flame_ref.constants(model, 7, 5, torch.float64)
    shape, exp, pose, neck, eye = params(3, 7, 5)
    joints = flame_ref.flame_vertices(c, shape, exp, pose, neck, eye, return_joints=True)
    _, _, J0, Jdirs = fl.joint_basis(model, 7, 5)
    lin = torch.from_numpy(J0)[None] + (torch.cat([shape, exp], 1) @ torch.from_numpy(Jdirs)).view(3, -1, 3)
    assert (joints - lin).abs().max().item() <= 1e-12
    layer = fl.FlameLayer(model, 7, 5)  # the buffers are those arrays, rounded once
    assert torch.equal(layer.J0, torch.from_numpy(J0).float().reshape(-1)) and torch.equal(layer.Jdirs, torch.from_numpy(Jdirs).float())
    assert layer.dirs.shape == (12 + 36, 3 * 257) and layer.lbs_weights.shape == (257, 5)
    sd = torch.from_numpy(model.shapedirs).float()
    assert torch.equal(layer.dirs[7 + 2].view(257, 3), sd[:, :, 20 + 2])  # expression columns start at the model's n_shape


def test_zero_parameters_give_the_template():
    """All parameters zero: dir = 0 / 1.7e-8 = 0, so every rotation is exactly I, the chain's transforms are [I | t] with
    t = (j_p + (j - j_p)) - j, and the blend is sum_j w_j [I | t_j]: the template, exactly, wherever the weights of a row sum to
    exactly 1 and t is exactly 0.  Checked exactly on the root's vertices of a model whose weights are one-hot (both hold there:
    t_0 = j_0 - j_0); elsewhere the sums (j_p + (j - j_p)) - j along a chain of depth <= 2 and sum_j w_j round a few times at
    the template's magnitude: at most 8 * 2^-52 * max|v| in float64."""
    for V, parents in ((33, fl.FLAME_PARENTS), (257, (-1, 0, 1))):
        model = fl.synthetic_flame_model(template(V), 7, 5, parents=parents)
        J = len(parents)
        onehot = np.eye(J)[np.argmax(model.lbs_weights, 1)]
        rigid = fl.FlameModel(model.v_template, model.shapedirs, model.posedirs, np.eye(J, V), onehot, parents, n_shape=7)
        z = lambda n: torch.zeros(2, n, dtype=torch.float64)
        # J_regressor = eye: the joints are vertices 0..J-1 and j_p + (j - j_p) - j is evaluated on those; one-hot rows sum exactly
        got = flame_ref.flame_vertices(flame_ref.constants(rigid, 7, 5, torch.float64), z(7), z(5), z(6), z(3), z(6))
        ref = torch.from_numpy(model.v_template).float().double()[None].expand(2, -1, -1)
        bound = 8 * 2.0 ** -52 * ref.abs().max().item()
        assert (got - ref).abs().max().item() <= bound
        root = torch.from_numpy(onehot[:, 0] == 1)
        assert root.any() and torch.equal(got[:, root], ref[:, root])  # the root's vertices: nothing to round
        # the synthetic model's weights are rounded to float32 (the layer's constants): a row sums to 1 within 2^-24 (each weight
        # moves by at most 2^-24 of itself and they sum to 1), which scales the vertex
        got = flame_ref.flame_vertices(flame_ref.constants(model, 7, 5, torch.float64), z(7), z(5), z(6), z(3), z(6))
        assert (got - ref).abs().max().item() <= 2.0 ** -24 * ref.abs().max().item() + bound


def test_global_rotation_rotates_about_the_root_joint():
    """posedirs = 0 and only pose_params[:, :3] non-zero: every joint's transform is the root's, so the mesh is v_shaped rotated
    about joint 0."""
    model = fl.synthetic_flame_model(template(), 7, 5)
    model = fl.FlameModel(model.v_template, model.shapedirs, 0 * model.posedirs, model.J_regressor, model.lbs_weights,
                          model.parents, n_shape=7)
    c = flame_ref.constants(model, 7, 5, torch.float64)
    c["lbs_weights"] = c["lbs_weights"] / c["lbs_weights"].sum(1, keepdim=True)  # (rounded to float32 a row sums to 1 +- 2^-24)
    shape, exp, pose, neck, eye = params(3, 7, 5)
    pose[:, 3:] = 0
    got = flame_ref.flame_vertices(c, shape, exp, pose, 0 * neck, 0 * eye)
    v_shaped = flame_ref.shaped(c, torch.cat([shape, exp], 1))
    j0 = flame_ref.flame_vertices(c, shape, exp, pose, neck, eye, return_joints=True)[:, :1]
    want = (v_shaped - j0) @ flame_ref.rodrigues(pose[:, :3]).transpose(1, 2) + j0
    assert (got - want).abs().max().item() <= 1e-12
    assert (got - v_shaped).abs().max().item() > 1e-3  # (the rotation did something)


def test_synthetic_model_properties():
    t = template()
    a, b, c = fl.synthetic_flame_model(t, 20, 10, seed=5), fl.synthetic_flame_model(t, 20, 10, seed=5), fl.synthetic_flame_model(t, 20, 10, seed=6)
    for k in fl.FlameModel.KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert not np.array_equal(a.shapedirs, c.shapedirs)
    assert a.shapedirs.shape == (257, 3, 30) and a.posedirs.shape == (36, 771) and (a.n_shape, a.n_exp) == (20, 10)
    assert a.parents.tolist() == [-1, 0, 1, 1, 1]
    assert a.lbs_weights.min() >= 0 and np.abs(a.lbs_weights.sum(1) - 1).max() <= 1e-12
    assert a.J_regressor.min() >= 0 and np.abs(a.J_regressor.sum(1) - 1).max() <= 1e-12
    joints = a.J_regressor @ t
    assert (joints >= t.min(0)).all() and (joints <= t.max(0)).all()
    assert np.abs(a.shapedirs).max() <= 2e-3 and np.abs(a.posedirs).max() <= 2e-3
    # smooth fall-off: the weight of a joint decreases with the distance from it, up to the row normalisation — the vertex
    # nearest to a joint weighs it more than the farthest one does
    d = np.linalg.norm(t[:, None] - joints[None], axis=2)
    for j in range(5):
        assert a.lbs_weights[d[:, j].argmin(), j] > a.lbs_weights[d[:, j].argmax(), j]
    one = fl.synthetic_flame_model(t[:1], 3, 2)  # a degenerate bounding box still gives a valid model
    assert np.isfinite(one.lbs_weights).all() and np.isfinite(one.J_regressor).all()


def test_npz_round_trip_and_shape_checks(tmp_path):
    m = fl.synthetic_flame_model(template(33), 7, 5, parents=(-1, 0, 1))
    path = str(tmp_path / "model.npz")
    m.save_npz(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(fl.FlameModel.KEYS) <= set(z.files)
    r = fl.FlameModel.from_npz(path)
    for k in fl.FlameModel.KEYS:
        assert np.array_equal(getattr(m, k), getattr(r, k)), k
    assert r.n_shape == 7 and r.n_exp == 5
    with pytest.raises(ValueError, match="topologically"):
        fl.FlameModel(m.v_template, m.shapedirs, m.posedirs, m.J_regressor, m.lbs_weights, (-1, 2, 0), n_shape=7)
    with pytest.raises(ValueError, match="posedirs"):
        fl.FlameModel(m.v_template, m.shapedirs, m.posedirs[:9], m.J_regressor, m.lbs_weights, m.parents, n_shape=7)
    with pytest.raises(ValueError, match="lbs_weights"):
        fl.FlameModel(m.v_template, m.shapedirs, m.posedirs, m.J_regressor, m.lbs_weights.T, m.parents, n_shape=7)
    with pytest.raises(ValueError, match="n_shape"):
        fl.FlameModel(m.v_template, m.shapedirs, m.posedirs, m.J_regressor, m.lbs_weights, m.parents)  # K != 400: no default
    with pytest.raises(ValueError, match="asked for"):
        fl.FlameLayer(m, 8, 5)
    np.savez(path, **{k: getattr(m, k) for k in fl.FlameModel.KEYS if k != "parents"})
    with pytest.raises(ValueError, match="missing keys"):
        fl.FlameModel.from_npz(path)


def test_layer_refuses_cpu_tensors():
    layer = fl.FlameLayer(fl.synthetic_flame_model(template(33), 7, 5), 7, 5)
    with pytest.raises(_lib.GifHipError):
        layer(torch.zeros(2, 7), torch.zeros(2, 5), torch.zeros(2, 6))
    with pytest.raises(_lib.GifHipError):
        layer()


def test_argument_validation_without_gpu():
    lib = _lib.load()
    skin, bwd, joints = lib.gif_flame_skin_f32, lib.gif_flame_skin_bwd_f32, lib.gif_flame_joints_f32
    # empty work is a no-op
    assert skin(None, None, None, None, None, None, None, 0, 33, 48, 5, None) == 0
    assert skin(None, None, None, None, None, None, None, 2, 0, 48, 5, None) == 0
    assert bwd(None, None, None, None, None, None, None, 0, 33, 48, 5, None, None) == 0
    assert bwd(None, None, None, None, None, None, None, 2, 0, 48, 5, None, None) == 0
    # J outside 1..8, KP < P = 9 (J - 1), null required pointers
    for J in (0, 9):
        assert skin(None, None, None, None, None, None, None, 2, 33, 100, J, None) == -1 and b"J in 1..8" in lib.gif_last_error()
        assert bwd(None, None, None, None, None, None, None, 2, 33, 100, J, None, None) == -1 and b"J in 1..8" in lib.gif_last_error()
    assert skin(None, None, None, None, None, None, None, 2, 33, 35, 5, None) == -1 and b"KP >= 9" in lib.gif_last_error()
    assert bwd(None, None, None, None, None, None, None, 2, 33, 35, 5, None, None) == -1 and b"KP >= 9" in lib.gif_last_error()
    assert skin(None, None, None, None, None, None, None, 2, 33, 48, 5, None) == -1 and b"null pointer" in lib.gif_last_error()
    assert bwd(None, None, None, None, None, None, None, 2, 33, 48, 5, None, None) == -1 and b"null pointer" in lib.gif_last_error()
    assert lib.gif_flame_skin_bwd_workspace_bytes(0, 33, 48, 5) == 0
    # partial rows of both reductions (32 / 64 vertices per workgroup) + the 64 rows a long second pass may need
    assert lib.gif_flame_skin_bwd_workspace_bytes(3, 5023, 186, 5) == ((157 + 64) * 3 * 186 + (79 + 64) * 3 * 60) * 4
    par = lambda *p: (ctypes.c_int32 * len(p))(*p)
    j = lambda parents, B, ns, ne, KP, J: joints(None, None, parents, None, 0, ns, None, 0, ne, None, 0, None, 0, None, 0,
                                                 None, None, B, KP, J, None)
    assert j(par(-1, 0, 1, 1, 1), 0, 7, 5, 48, 5) == 0
    assert j(par(-1, 0, 1, 1, 1), 2, 7, 5, 48, 9) == -1 and b"J in 1..8" in lib.gif_last_error()
    assert j(par(-1, 0, 1, 1, 1), 2, 7, 5, 47, 5) == -1 and b"n_shape + n_exp + 9" in lib.gif_last_error()
    assert j(par(-1, 0, 2, 1, 1), 2, 7, 5, 48, 5) == -1 and b"parents[2]" in lib.gif_last_error()
    assert j(None, 2, 7, 5, 48, 5) == -1 and b"null parents" in lib.gif_last_error()
    assert j(par(-1, 0, 1, 1, 1), 2, 7, 5, 48, 5) == -1 and b"null pointer" in lib.gif_last_error()
