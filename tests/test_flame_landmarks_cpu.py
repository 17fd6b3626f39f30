"""CPU-side checks of the FLAME landmarks: the embedding's format and validation, the synthetic embedding's properties, the row rule
and the chain product of the float64 restatement (tests/flame_landmarks_ref.py), the entry points' argument validation (before
any launch, so it runs without a GPU), and the layer's constants with and without the new arguments."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import flame_landmarks_ref as lref
import flame_ref
from gif_amd import _lib
from gif_amd import flame as fl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAWS = (0.0, -0.2, 12.3, 38.7, 45.0, -1.0, -12.3, -38.7, -45.0)
ROWS = (0, 0, 12, 39, 39, 40, 51, 78, 78)


def body(V=257):
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    v, f = g["vertices"].astype(np.float64) * 0.1, g["faces"].astype(np.int64)
    return v[:V], f[(f < V).all(1)]


def small_embedding(seed=0, **kw):
    return fl.synthetic_landmark_embedding(body()[1], n_dynamic=3, n_static=4, n_full=5, n_rows=5, seed=seed, **kw)


def test_npz_round_trip_and_missing_keys(tmp_path):
    e = small_embedding()
    path = str(tmp_path / "lmk.npz")
    e.save_npz(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(fl.FlameLandmarkEmbedding.KEYS) <= set(z.files)
    r = fl.FlameLandmarkEmbedding.from_npz(path)
    for k in fl.FlameLandmarkEmbedding.KEYS:
        assert np.array_equal(getattr(e, k), getattr(r, k)), k
    assert r.dynamic_vid.shape == (5, 3, 3) and r.yaw_joint == 1
    np.savez(path, **{k: getattr(e, k) for k in fl.FlameLandmarkEmbedding.KEYS if k != "dynamic_bary"})
    with pytest.raises(ValueError, match=r"missing keys \['dynamic_bary'\]"):
        fl.FlameLandmarkEmbedding.from_npz(path)


def test_embedding_validation_names_the_problem():
    e = small_embedding()
    args = lambda **kw: [kw.get(k, getattr(e, k)) for k in fl.FlameLandmarkEmbedding.KEYS[:-1]]
    E = fl.FlameLandmarkEmbedding
    with pytest.raises(ValueError, match="R = 4 rows: R must be odd"):
        E(*args(dynamic_vid=e.dynamic_vid[:4], dynamic_bary=e.dynamic_bary[:4]))
    with pytest.raises(ValueError, match=r"static_vid must be \[L,3\]"):
        E(*args(static_vid=e.static_vid[:, :2]))
    with pytest.raises(ValueError, match=r"dynamic_vid must be \[R,Ld,3\]"):
        E(*args(dynamic_vid=e.dynamic_vid[0]))
    with pytest.raises(ValueError, match="full_bary must have full_vid's shape"):
        E(*args(full_bary=e.full_bary[:3]))
    with pytest.raises(ValueError, match="static_vid must hold integers"):
        E(*args(static_vid=e.static_vid.astype(np.float64)))
    bad = e.full_vid.copy()
    bad[2, 1] = -1
    with pytest.raises(ValueError, match="full_vid holds the negative vertex id -1"):
        E(*args(full_vid=bad))
    nan = e.dynamic_bary.copy()
    nan[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="dynamic_bary holds non-finite"):
        E(*args(dynamic_bary=nan))
    with pytest.raises(ValueError, match="yaw_joint = 8 outside"):
        E(*args(), yaw_joint=8)
    # ids < V once V is known: check_vertices, which the layers call
    top = int(e.vertex_ids().max())
    e.check_vertices(top + 1)
    with pytest.raises(ValueError, match=rf"holds vertex id {top}, outside 0\.\.{top - 1}"):
        e.check_vertices(top)
    v, _ = body()
    model = fl.synthetic_flame_model(v[:top], 3, 2)
    with pytest.raises(ValueError, match="outside 0.."):
        fl.FlameLayer(model, 3, 2, landmarks=e)
    with pytest.raises(ValueError, match="outside 0.."):
        fl.FlameLandmarkLayer(model, e, 3, 2)
    chain = fl.synthetic_flame_model(v, 3, 2, parents=(-1,))
    with pytest.raises(ValueError, match="yaw_joint = 1 outside 0..0"):
        fl.FlameLayer(chain, 3, 2, landmarks=e)
    with pytest.raises(ValueError, match="vertex_ids outside 0..256"):
        fl.FlameLayer(fl.synthetic_flame_model(v, 3, 2), 3, 2, vertex_ids=[0, 257])
    # an even R is fine when there are no dynamic columns
    E(e.static_vid, e.static_bary, np.zeros((2, 0, 3), np.int64), np.zeros((2, 0, 3)), e.full_vid, e.full_bary)


def test_from_face_embedding_equals_a_hand_gather():
    _, faces = body()
    rng = np.random.RandomState(3)
    st, dy, fu = rng.randint(0, len(faces), 4), rng.randint(0, len(faces), (3, 2)), rng.randint(0, len(faces), (1, 5))
    bs, bd, bf = rng.rand(4, 3), rng.rand(3, 2, 3), rng.rand(1, 5, 3)
    e = fl.FlameLandmarkEmbedding.from_face_embedding(faces, st, bs, dy, bd, fu, bf, yaw_joint=2)
    for l in range(4):
        assert e.static_vid[l].tolist() == faces[st[l]].tolist()
    for r in range(3):
        for l in range(2):
            assert e.dynamic_vid[r, l].tolist() == faces[dy[r, l]].tolist()
    for l in range(5):  # (the file's leading 1 is dropped)
        assert e.full_vid[l].tolist() == faces[fu[0, l]].tolist()
    assert np.array_equal(e.static_bary, bs) and np.array_equal(e.dynamic_bary, bd) and np.array_equal(e.full_bary, bf[0])
    assert e.yaw_joint == 2
    ids = e.vertex_ids()
    assert np.array_equal(ids, np.unique(np.concatenate([faces[st].ravel(), faces[dy].ravel(), faces[fu].ravel()])))
    c = e.remapped(ids)
    assert np.array_equal(ids[c.static_vid], e.static_vid) and np.array_equal(ids[c.dynamic_vid], e.dynamic_vid)
    assert np.array_equal(ids[c.full_vid], e.full_vid) and c.vertex_ids().tolist() == list(range(len(ids)))
    with pytest.raises(ValueError, match="missing from ids"):
        e.remapped(ids[1:])
    with pytest.raises(ValueError, match=rf"static_faces_idx outside 0\.\.{len(faces) - 1}"):
        fl.FlameLandmarkEmbedding.from_face_embedding(faces, [len(faces)], bs[:1], dy, bd, fu, bf)


def test_synthetic_embedding_properties():
    v, faces = body()
    a, b, c = (fl.synthetic_landmark_embedding(faces, seed=s) for s in (0, 0, 1))
    for k in fl.FlameLandmarkEmbedding.KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert not np.array_equal(a.dynamic_vid, c.dynamic_vid)
    assert a.dynamic_vid.shape == (79, 17, 3) and a.static_vid.shape == (51, 3) and a.full_vid.shape == (68, 3) and a.yaw_joint == 1
    for name in ("static", "dynamic", "full"):
        vid, bary = getattr(a, name + "_vid"), getattr(a, name + "_bary")
        assert vid.min() >= 0 and vid.max() < len(v)
        assert bary.min() > 0 and np.abs(bary.sum(-1) - 1).max() <= 1e-12
    # neighbouring rows share faces, and so do neighbouring columns of a row: collisions for the backward
    shared = [len(set(map(tuple, a.dynamic_vid[r])) & set(map(tuple, a.dynamic_vid[r + 1]))) for r in range(78)]
    assert min(shared) >= 1
    assert all(len(set(map(tuple, a.dynamic_vid[r]))) < 17 for r in range(79))
    one = fl.synthetic_landmark_embedding(np.array([[0, 1, 2]]), 2, 3, 4, 3)  # a single face: everything collides
    assert set(one.vertex_ids().tolist()) == {0, 1, 2}


def test_row_rule():
    yaw = torch.tensor(YAWS, dtype=torch.float64)
    assert lref.select_row(yaw, 39).tolist() == list(ROWS)
    assert lref.select_row(yaw, 0).tolist() == [0] * len(YAWS)  # R = 1
    # half-way cases round to even; -0.4 rounds to -0, which counts as 0; non-finite yaws select row 0
    assert lref.select_row(torch.tensor([0.5, 1.5, 2.5, -0.4, -0.5, -1.5, -38.5, -39.5]), 39).tolist() == [0, 2, 2, 0, 0, 41, 77, 78]
    assert lref.select_row(torch.tensor([math.nan, math.inf, -math.inf]), 39).tolist() == [0, 0, 0]
    # the definition's sign: a rotation about y by -t has yaw_degrees = t for |t| < 90 (Rodrigues' 1e-8 guard on each component
    # moves the angle by at most sqrt(3) 1e-8 rad = 1e-6 degrees)
    for t in YAWS:
        R = flame_ref.rodrigues(torch.tensor([[0.0, -math.radians(t), 0.0]], dtype=torch.float64))
        assert abs(lref.yaw_degrees(R).item() - t) <= 2e-6


def test_chain_product_is_the_world_rotation_flame_ref_builds():
    """Four vertices (origin and the unit axes) that follow joint `yaw_joint` rigidly, no blend shapes: flame_ref's vertices are
    G_j [v, 1] with G_j the world transform its chain of 4x4 products builds, so the differences of the outputs to the first one
    are the columns of its world rotation.  The chain product of flame_landmarks_ref equals it at 1e-12 in float64."""
    tmpl = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    g = torch.Generator().manual_seed(4)
    for parents, yaw_joint in (((-1, 0, 1, 1, 1), 1), ((-1, 0, 1), 1), ((-1, 0, 1), 2), ((-1, 0, 1, 1, 1), 4)):
        J = len(parents)
        rng = np.random.RandomState(J)
        jr = rng.rand(J, 4)
        model = fl.FlameModel(tmpl, np.zeros((4, 3, 2)), np.zeros((9 * (J - 1), 12)), jr / jr.sum(1, keepdims=True),
                              np.eye(J)[[yaw_joint] * 4], parents, n_shape=1)
        c = flame_ref.constants(model, 1, 1, torch.float64)
        r = lambda n: torch.randn(3, n, generator=g, dtype=torch.float64) * 0.5
        z = torch.zeros(3, 1, dtype=torch.float64)
        pose, neck, eye = r(6), r(3), r(6)
        v = flame_ref.flame_vertices(c, z, z, pose, neck, eye)
        built = (v[:, 1:] - v[:, :1]).transpose(1, 2)  # columns: images of the unit axes
        got = lref.neck_rotation(c, pose, neck, eye, yaw_joint)
        assert (got - built).abs().max().item() <= 1e-12
        assert (got - torch.eye(3, dtype=torch.float64)).abs().max().item() > 0.1  # (the poses did something)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    N = None
    # (B, V, J, yaw_joint, R, Ld, Ls)
    fwd = lambda *dims: lib.gif_flame_landmarks_f32(N, N, N, N, N, N, N, N, *dims, N)
    # (B, V, R, Ld, Ls)
    bwd = lambda *dims: lib.gif_flame_landmarks_bwd_f32(N, N, N, N, N, N, N, *dims, N)
    err = lib.gif_last_error
    # empty work is a no-op
    assert fwd(0, 33, 5, 1, 79, 17, 51) == 0
    assert fwd(2, 33, 5, 1, 79, 0, 0) == 0
    assert fwd(2, 33, 5, 1, 2, 0, 0) == 0  # (an even R without dynamic columns is nothing)
    assert bwd(0, 33, 79, 17, 51) == 0
    assert bwd(2, 0, 79, 17, 51) == 0
    # J outside 1..8
    for J in (0, 9):
        assert fwd(2, 33, J, 0, 79, 17, 51) == -1 and b"J in 1..8" in err()
    # yaw_joint outside 0..J-1
    for yj in (-1, 5):
        assert fwd(2, 33, 5, yj, 79, 17, 51) == -1 and b"yaw_joint = %d outside 0..J-1 = 4" % yj in err()
    # R even with dynamic columns (R = 0 included)
    for R in (0, 2, 78):
        assert fwd(2, 33, 5, 1, R, 17, 51) == -1 and b"R = %d rows" % R in err() and b"odd" in err()
        assert bwd(2, 33, R, 17, 51) == -1 and b"R = %d rows" % R in err() and b"odd" in err()
    assert fwd(2, 33, 5, 1, 78, 0, 51) == -1 and b"null pointer" in err()  # (R even, Ld = 0: legal, so it gets as far as the pointers)
    # negative sizes
    assert fwd(-1, 33, 5, 1, 79, 17, 51) == -1 and b"bad dims" in err()
    assert fwd(2, 33, 5, 1, 79, -1, 51) == -1 and b"bad dims" in err()
    assert bwd(2, -3, 79, 17, 51) == -1 and b"bad dims" in err()
    # null pointers with work to do; R = 1 is legal (it gets as far as the pointers)
    assert fwd(2, 33, 5, 1, 79, 17, 51) == -1 and b"flame_landmarks: null pointer" in err()
    assert fwd(2, 33, 5, 1, 1, 1, 0) == -1 and b"flame_landmarks: null pointer" in err()
    assert fwd(2, 33, 1, 0, 1, 0, 1) == -1 and b"flame_landmarks: null pointer" in err()
    assert bwd(2, 33, 79, 17, 51) == -1 and b"flame_landmarks_bwd: null pointer" in err()
    assert bwd(2, 33, 1, 0, 0) == -1 and b"flame_landmarks_bwd: null pointer" in err()  # (no landmarks: g_verts is still zero-filled)
    # one null among valid pointers: host memory stands in, nothing is launched before the check fails
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gif_flame_landmarks_f32(p, p, p, p, N, p, p, N, 2, 3, 5, 1, 1, 1, 1, N) == -1 and b"null pointer" in err()
    assert lib.gif_flame_landmarks_f32(p, N, p, p, p, p, p, N, 2, 3, 5, 1, 1, 1, 1, N) == -1 and b"null pointer" in err()
    assert lib.gif_flame_landmarks_bwd_f32(p, N, p, p, p, p, p, 2, 3, 1, 1, 1, N) == -1 and b"null pointer" in err()


def test_layers_refuse_cpu_tensors():
    v, faces = body(33)
    model = fl.synthetic_flame_model(v, 3, 2)
    e = fl.synthetic_landmark_embedding(faces, 2, 3, 4, 3)
    z = [torch.zeros(2, 3), torch.zeros(2, 2), torch.zeros(2, 6)]
    with pytest.raises(_lib.GifHipError):
        fl.FlameLayer(model, 3, 2, landmarks=e)(*z)
    with pytest.raises(_lib.GifHipError):
        fl.FlameLandmarkLayer(model, e, 3, 2)(*z)
    t = lref.tables(e, torch.float32)
    with pytest.raises(_lib.GifHipError):
        fl._FlameLandmarksFn.apply(torch.zeros(2, 33, 3), torch.zeros(2, 5, 12), 1, 3, 2, 3, t["dynamic_vid"].int(), t["dynamic_bary"],
                                   t["static_vid"].int(), t["static_bary"])


def test_project_landmarks_is_plain_torch():
    g = torch.Generator().manual_seed(0)
    lmk, cam = torch.randn(2, 5, 3, generator=g, dtype=torch.float64), torch.randn(2, 3, generator=g, dtype=torch.float64)
    want = cam[:, None, 0:1] * torch.cat([lmk[:, :, :2] + cam[:, None, 1:], lmk[:, :, 2:]], 2)
    want[:, :, 1:] *= -1
    assert torch.equal(fl.project_landmarks(lmk, cam), want)


def test_vertex_ids_gathers_the_rows_and_keeps_the_joints():
    v, faces = body()
    model = fl.synthetic_flame_model(v, 7, 5, seed=2)
    full = fl.FlameLayer(model, 5, 3)
    ids = np.array([200, 3, 3, 17, 256, 0])
    sub = fl.FlameLayer(model, 5, 3, vertex_ids=ids)
    KP = full.dirs.shape[0]
    assert sub.n_vertices == 6 and sub.dirs.shape == (KP, 18)
    assert torch.equal(sub.v_template.view(6, 3), full.v_template.view(257, 3)[ids])
    assert torch.equal(sub.dirs.view(KP, 6, 3), full.dirs.view(KP, 257, 3)[:, ids])
    assert torch.equal(sub.lbs_weights, full.lbs_weights[ids])
    assert torch.equal(sub.J0, full.J0) and torch.equal(sub.Jdirs, full.Jdirs)
    e = fl.synthetic_landmark_embedding(faces, 2, 3, 4, 3, seed=5)
    lm = fl.FlameLandmarkLayer(model, e, 5, 3)
    want = e.vertex_ids()
    assert torch.equal(lm.lbs_weights, full.lbs_weights[want]) and torch.equal(lm.J0, full.J0)
    assert torch.equal(torch.from_numpy(want)[lm.lmk_dyn_vid.long()], torch.from_numpy(e.dynamic_vid))
    assert lm.lmk_st_vid.shape == (7, 3) and lm.lmk_st_vid.dtype == torch.int32  # static, then full: one table
    assert torch.equal(lm.lmk_st_bary, torch.from_numpy(np.concatenate([e.static_bary, e.full_bary])).float())


def test_layer_without_the_new_arguments_is_unchanged():
    """Buffer names and values of FlameLayer(model): the five constants, formed as before the landmark arguments existed."""
    v, _ = body()
    model = fl.synthetic_flame_model(v, 7, 5, seed=2)
    layer = fl.FlameLayer(model, 5, 3)
    assert [k for k, _ in layer.named_buffers()] == ["v_template", "dirs", "lbs_weights", "J0", "Jdirs"]
    assert list(layer.state_dict()) == ["v_template", "dirs", "lbs_weights", "J0", "Jdirs"]
    tmpl, sd, J0, Jdirs = fl.joint_basis(model, 5, 3)
    dirs = np.concatenate([sd.reshape(3 * 257, -1).T, model.posedirs.astype(np.float32)], 0)
    for name, a in (("v_template", tmpl.reshape(-1)), ("dirs", dirs), ("lbs_weights", model.lbs_weights.astype(np.float32)),
                    ("J0", J0.astype(np.float32).reshape(-1)), ("Jdirs", Jdirs.astype(np.float32))):
        assert torch.equal(getattr(layer, name), torch.from_numpy(np.ascontiguousarray(a))), name
    with_lmk = fl.FlameLayer(model, 5, 3, landmarks=fl.synthetic_landmark_embedding(body()[1], 2, 3, 4, 3))
    assert [k for k, _ in with_lmk.named_buffers()][5:] == ["lmk_dyn_vid", "lmk_dyn_bary", "lmk_st_vid", "lmk_st_bary"]
    for name in ("v_template", "dirs", "lbs_weights", "J0", "Jdirs"):
        assert torch.equal(getattr(with_lmk, name), getattr(layer, name))
