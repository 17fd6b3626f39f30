"""The FLAME layer on HIP kernels: (shape, expression, pose) -> vertices, differentiable with respect to all three.

The reference keeps its FLAME layer in the absent `photometric_optimization` submodule and the model file is licensed, but the
algorithm is public (FLAME, Li et al. 2017, in the smplx formulation): shape / expression blend shapes, pose-corrective blend
shapes, joint regression, a kinematic chain and linear blend skinning.  This module is that algorithm with the call signature
FlameTextureSpace.forward uses (model/stg2_generator.py:362-364); DESIGN.md §3l has the layout and the measurements.

* FlameModel            — the six constant arrays of a model; .npz in and out (what a licensed model file is converted into).
* synthetic_flame_model — a model with FLAME's structure over any template mesh (no assets needed to build, test or measure).
* FlameLayer            — nn.Module, `FlameLayer(model)(shape_params, expression_params, pose_params) -> (vertices, None, None)`;
                          drops into render.FlameConditionRenderer(flame=...).  With `landmarks=` an embedding the outputs are
                          (vertices, landmarks2d, landmarks3d), the reference layer's three.
* FlameLandmarkEmbedding — the landmark tables in vertex-id form (.npz in and out; from_face_embedding converts the layout of
                          `landmark_embedding.npy`); synthetic_landmark_embedding builds one over any face list.
* FlameLandmarkLayer    — (landmarks2d, landmarks3d) alone: the layer restricted to the few hundred vertices the tables name.
* project_landmarks     — orthographic projection with y and z flipped, as the reference draws landmarks.
Kernels: gif_flame_joints_f32, gif_pose_chain_bwd_f32, gif_flame_skin_f32, gif_flame_skin_bwd_f32 (csrc/flame.hip),
gif_flame_landmarks_f32, gif_flame_landmarks_bwd_f32 (csrc/flame_landmarks.hip).  No CPU fallback.
"""
import ctypes

import numpy as np
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

FLAME_PARENTS = (-1, 0, 1, 1, 1)  # global, neck, jaw, left eye, right eye
MAX_JOINTS = 8


class FlameModel:
    """Constants of a FLAME-style model:
      v_template [V,3]; shapedirs [V,3,K] (the `n_shape` shape columns first, then the expression columns); posedirs [P,3V],
      P = 9 (J - 1); J_regressor [J,V]; lbs_weights [V,J]; parents [J] (parents[0] = -1, parents[j] < j).
    `n_shape` is the number of SHAPE columns of shapedirs (300 of the 400 in the public FLAME files, the default for K = 400)."""

    KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents")

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents, n_shape=None):
        self.v_template = np.asarray(v_template, np.float64)
        self.shapedirs = np.asarray(shapedirs, np.float64)
        self.posedirs = np.asarray(posedirs, np.float64)
        self.J_regressor = np.asarray(J_regressor, np.float64)
        self.lbs_weights = np.asarray(lbs_weights, np.float64)
        self.parents = np.asarray(parents, np.int64).reshape(-1)
        if self.v_template.ndim != 2 or self.v_template.shape[1] != 3:
            raise ValueError(f"v_template must be [V,3], got {self.v_template.shape}")
        V, J = self.v_template.shape[0], self.parents.shape[0]
        if not 1 <= J <= MAX_JOINTS:
            raise ValueError(f"{J} joints: the kernels take 1..{MAX_JOINTS}")
        if self.shapedirs.ndim != 3 or self.shapedirs.shape[:2] != (V, 3):
            raise ValueError(f"shapedirs must be [{V},3,K], got {self.shapedirs.shape}")
        for name, want in (("posedirs", (9 * (J - 1), 3 * V)), ("J_regressor", (J, V)), ("lbs_weights", (V, J))):
            if getattr(self, name).shape != want:
                raise ValueError(f"{name} must be {list(want)}, got {list(getattr(self, name).shape)}")
        if self.parents[0] != -1 or any(not 0 <= self.parents[j] < j for j in range(1, J)):
            raise ValueError(f"parents {self.parents.tolist()} is not topologically ordered (parents[0] = -1, parents[j] < j)")
        K = self.shapedirs.shape[2]
        if n_shape is None:
            if K != 400:
                raise ValueError(f"n_shape (the number of shape columns among the {K} of shapedirs) is needed")
            n_shape = 300
        if not 0 <= int(n_shape) <= K:
            raise ValueError(f"n_shape = {n_shape} outside 0..{K}")
        self.n_shape = int(n_shape)

    @property
    def n_exp(self):
        return self.shapedirs.shape[2] - self.n_shape

    def save_npz(self, path):
        with open(path, "wb") as f:
            np.savez(f, n_shape=np.int64(self.n_shape), **{k: getattr(self, k) for k in self.KEYS})

    @classmethod
    def from_npz(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: missing keys {missing}")
            return cls(*[z[k] for k in cls.KEYS], n_shape=int(z["n_shape"]) if "n_shape" in z.files else None)


def synthetic_flame_model(template, n_shape=100, n_exp=50, seed=0, amplitude=2e-3, parents=FLAME_PARENTS):
    """A model with FLAME's structure over `template` [V,3]: smooth low-amplitude blend shapes (the fields of
    data.SyntheticFlame.basis), pose correctives a quarter of that size, joints inside the template's bounding box (a
    non-negative J_regressor whose rows sum to 1) and skinning weights that fall off smoothly with the distance from each joint
    (rows non-negative, summing to 1).  Deterministic per seed.  NOT a face model: the structure and the arithmetic of one."""
    rng = np.random.RandomState(seed)
    t = np.asarray(template, np.float64)
    V, J = t.shape[0], len(parents)

    def basis(n, amp):
        freq = rng.randn(n, 3) * 3.0
        phase = rng.rand(n, 1) * 2 * np.pi
        direction = rng.randn(n, 1, 3)
        direction /= np.linalg.norm(direction, axis=2, keepdims=True)
        return amp * np.sin(freq @ t.T + phase)[:, :, None] * direction  # [n,V,3]

    shapedirs = basis(n_shape + n_exp, amplitude).transpose(1, 2, 0)  # [V,3,K]
    posedirs = basis(9 * (J - 1), 0.25 * amplitude).reshape(9 * (J - 1), 3 * V)
    lo, hi = t.min(0), t.max(0)
    sigma = max(0.25 * float(np.linalg.norm(hi - lo)), 1e-6)
    frac = np.array([(0.5, 0.3, 0.4), (0.5, 0.2, 0.4), (0.5, 0.4, 0.5), (0.35, 0.7, 0.7), (0.65, 0.7, 0.7)])
    frac = np.concatenate([frac, 0.2 + 0.6 * rng.rand(max(J - 5, 0), 3)])[:J]

    def falloff(points, s):  # [n,3] -> weights [n,V]: Gaussian in the distance, rows sum to 1
        d2 = ((points[:, None, :] - t[None]) ** 2).sum(2) / (2 * s * s)
        w = np.exp(-(d2 - d2.min(1, keepdims=True)))
        return w / w.sum(1, keepdims=True)

    J_regressor = falloff(lo + frac * (hi - lo), 0.5 * sigma)
    joints = J_regressor @ t
    d2 = ((joints[:, None, :] - t[None]) ** 2).sum(2).T / (2 * sigma * sigma)  # [V,J]
    w = np.exp(-(d2 - d2.min(1, keepdims=True)))
    return FlameModel(t, shapedirs, posedirs, J_regressor, w / w.sum(1, keepdims=True), parents, n_shape=n_shape)


class FlameLandmarkEmbedding:
    """Landmark tables in vertex-id form.  A landmark is sum_i bary[i] * vertex[vid[i]]:
      static_vid [Ls,3] int, static_bary [Ls,3]        the static landmarks of `landmarks2d` (FLAME: Ls = 51);
      dynamic_vid [R,Ld,3] int, dynamic_bary [R,Ld,3]  the contour landmarks, R = 2M + 1 rows, one chosen per sample from the yaw of
                                                      joint `yaw_joint` (FLAME: R = 79, Ld = 17, joint 1 = the neck);
      full_vid [Lf,3] int, full_bary [Lf,3]            the static "full" set, `landmarks3d` (FLAME: Lf = 68).
    Shapes, R odd, ids >= 0 and finite weights are checked here; ids < V by check_vertices(V), which the layers call."""

    KEYS = ("static_vid", "static_bary", "dynamic_vid", "dynamic_bary", "full_vid", "full_bary", "yaw_joint")

    def __init__(self, static_vid, static_bary, dynamic_vid, dynamic_bary, full_vid, full_bary, yaw_joint=1):
        for name, vid, bary, nd in (("static", static_vid, static_bary, 2), ("dynamic", dynamic_vid, dynamic_bary, 3),
                                    ("full", full_vid, full_bary, 2)):
            vid, bary = np.asarray(vid), np.asarray(bary, np.float64)
            want = "[R,Ld,3]" if nd == 3 else "[L,3]"
            if vid.ndim != nd or vid.shape[-1] != 3:
                raise ValueError(f"{name}_vid must be {want}, got {list(vid.shape)}")
            if bary.shape != vid.shape:
                raise ValueError(f"{name}_bary must have {name}_vid's shape {list(vid.shape)}, got {list(bary.shape)}")
            if vid.size and not np.issubdtype(vid.dtype, np.integer):
                raise ValueError(f"{name}_vid must hold integers, got {vid.dtype}")
            vid = vid.astype(np.int64)
            if vid.size and vid.min() < 0:
                raise ValueError(f"{name}_vid holds the negative vertex id {int(vid.min())}")
            if not np.isfinite(bary).all():
                raise ValueError(f"{name}_bary holds non-finite weights")
            setattr(self, name + "_vid", vid)
            setattr(self, name + "_bary", bary)
        R, Ld = self.dynamic_vid.shape[:2]
        if Ld > 0 and R % 2 == 0:
            raise ValueError(f"dynamic tables have R = {R} rows: R must be odd (2M + 1, rows for yaw 0..M, then -1..-M)")
        self.yaw_joint = int(yaw_joint)
        if not 0 <= self.yaw_joint < MAX_JOINTS:
            raise ValueError(f"yaw_joint = {yaw_joint} outside 0..{MAX_JOINTS - 1}")

    @classmethod
    def from_face_embedding(cls, faces, static_faces_idx, static_bary, dynamic_faces_idx, dynamic_bary, full_faces_idx, full_bary,
                            yaw_joint=1):
        """From face indices into `faces` [F,3], the layout of the FLAME distribution's `landmark_embedding.npy`.  That file is a
        pickled dict (this library loads no pickle; the caller does, `np.load(path, allow_pickle=True, encoding="latin1")[()]`):
          static_lmk_faces_idx [51], static_lmk_bary_coords [51,3]            -> static_faces_idx, static_bary
          dynamic_lmk_faces_idx [79,17], dynamic_lmk_bary_coords [79,17,3]    -> dynamic_faces_idx, dynamic_bary
          full_lmk_faces_idx [1,68], full_lmk_bary_coords [1,68,3]            -> full_faces_idx, full_bary (a leading 1 is dropped)
        and `faces` is the model's face list."""
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3:
            raise ValueError(f"faces must be [F,3], got {list(faces.shape)}")
        full_faces_idx, full_bary = np.asarray(full_faces_idx), np.asarray(full_bary)
        if full_faces_idx.ndim == 2 and full_faces_idx.shape[0] == 1:
            full_faces_idx, full_bary = full_faces_idx[0], full_bary.reshape(full_bary.shape[-2:])
        vids = []
        for name, idx in (("static", static_faces_idx), ("dynamic", dynamic_faces_idx), ("full", full_faces_idx)):
            idx = np.asarray(idx)
            if idx.size and not np.issubdtype(idx.dtype, np.integer):
                raise ValueError(f"{name}_faces_idx must hold integers, got {idx.dtype}")
            idx = idx.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= faces.shape[0]):
                raise ValueError(f"{name}_faces_idx outside 0..{faces.shape[0] - 1}")
            vids.append(faces[idx].reshape(idx.shape + (3,)))
        return cls(vids[0], static_bary, vids[1], dynamic_bary, vids[2], full_bary, yaw_joint)

    def check_vertices(self, V):
        """Raise unless every vertex id is in 0..V-1."""
        for name in ("static", "dynamic", "full"):
            vid = getattr(self, name + "_vid")
            if vid.size and vid.max() >= V:
                raise ValueError(f"{name}_vid holds vertex id {int(vid.max())}, outside 0..{V - 1}")

    def vertex_ids(self):
        """Sorted unique vertex ids over all tables."""
        return np.unique(np.concatenate([self.static_vid.reshape(-1), self.dynamic_vid.reshape(-1), self.full_vid.reshape(-1)]))

    def remapped(self, ids):
        """The same tables over the compact vertex list `ids` (sorted, unique, a superset of vertex_ids()): id -> its position."""
        ids = np.asarray(ids, np.int64)
        pos = lambda vid: np.searchsorted(ids, vid).reshape(vid.shape)
        for vid in (self.static_vid, self.dynamic_vid, self.full_vid):
            if vid.size and not np.array_equal(ids[np.minimum(pos(vid), len(ids) - 1)], vid):
                raise ValueError("remapped: a vertex id of the tables is missing from ids")
        return FlameLandmarkEmbedding(pos(self.static_vid), self.static_bary, pos(self.dynamic_vid), self.dynamic_bary,
                                      pos(self.full_vid), self.full_bary, self.yaw_joint)

    def save_npz(self, path):
        with open(path, "wb") as f:
            np.savez(f, **{k: np.asarray(getattr(self, k)) for k in self.KEYS})

    @classmethod
    def from_npz(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: missing keys {missing}")
            return cls(*[z[k] for k in cls.KEYS[:-1]], yaw_joint=int(z["yaw_joint"]))


def synthetic_landmark_embedding(faces, n_dynamic=17, n_static=51, n_full=68, n_rows=79, seed=0):
    """An embedding with FLAME's structure over `faces` [F,3]: positive barycentric weights that sum to 1, and dynamic faces drawn
    from one sequence, face[r, c] = seq[(r + c) // 2], so neighbouring rows share faces and neighbouring columns of a row sit on
    one face (the collisions of a profile view).  Deterministic per seed.  NOT a face's landmarks: their structure."""
    faces = np.asarray(faces, np.int64)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError(f"faces must be [F,3] with F >= 1, got {list(faces.shape)}")
    rng = np.random.RandomState(seed)
    F = faces.shape[0]

    def bary(*shape):
        w = 0.1 + rng.rand(*shape, 3)
        return w / w.sum(-1, keepdims=True)

    seq = rng.randint(0, F, (n_rows + n_dynamic + 1) // 2 + 1)
    dyn_idx = seq[(np.arange(n_rows)[:, None] + np.arange(n_dynamic)[None, :]) // 2]
    st_idx, full_idx = rng.randint(0, F, n_static), rng.randint(0, F, n_full)
    return FlameLandmarkEmbedding.from_face_embedding(faces, st_idx, bary(n_static), dyn_idx, bary(n_rows, n_dynamic), full_idx,
                                                      bary(n_full))


def project_landmarks(lmk, cam):
    """Landmarks [B,L,3] under the orthographic camera [B,3] = (s, tx, ty), components 1 and 2 negated: render.batch_orth_proj
    and the flip the reference applies before it draws them (plots/voca/generate_voca_gt.py:68-69).  Plain torch."""
    from .render import batch_orth_proj
    p = batch_orth_proj(lmk, cam)
    return torch.cat([p[:, :, :1], -p[:, :, 1:]], 2)


def joint_basis(model, n_shape, n_exp):
    """(tmpl [V,3], sd [V,3,K], J0 [J,3], Jdirs [K,3J]): the layer's fp32 template and selected blend-shape columns, and the
    joints as a linear function of betas — joints = J0 + betas . Jdirs with J0 = J_regressor . v_template and Jdirs =
    J_regressor . shapedirs, in float64 from the fp32-rounded arrays (the model IS its fp32 constants)."""
    cols = np.concatenate([np.arange(n_shape), model.n_shape + np.arange(n_exp)]).astype(np.int64)
    sd = np.asarray(model.shapedirs, np.float32)[:, :, cols]
    tmpl = np.asarray(model.v_template, np.float32)
    jr = np.asarray(model.J_regressor, np.float32).astype(np.float64)
    J0 = jr @ tmpl.astype(np.float64)
    Jdirs = np.einsum("jv,vik->kji", jr, sd.astype(np.float64)).reshape(sd.shape[2], 3 * jr.shape[0])  # (no -1: K may be 0)
    return tmpl, sd, J0, Jdirs


def rodrigues(r):
    """Axis-angle [N,3] -> rotations [N,3,3] in the smplx form: angle = |r + 1e-8|, dir = r / angle, R = I + sin K + (1 - cos) K^2."""
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    x, y, z = (r / angle).unbind(1)
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], 1).view(-1, 3, 3)
    s, c = torch.sin(angle)[:, :, None], torch.cos(angle)[:, :, None]
    return torch.eye(3, dtype=r.dtype, device=r.device)[None] + s * K + (1 - c) * torch.bmm(K, K)


class _FlameSkinFn(Function):
    """verts = skin(template + dirs^T coef, A): steps 2, 7 and 9 of the layer on gif_flame_skin_f32 / gif_flame_skin_bwd_f32."""

    @staticmethod
    def forward(ctx, coef, A, tmpl, dirs, lbs_w):
        B, KP = coef.shape
        V, J = lbs_w.shape
        coef, A = coef.contiguous().float(), A.contiguous().float()
        keep = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        verts = torch.empty((B, V, 3), device=coef.device, dtype=torch.float32)
        v_posed = torch.empty_like(verts) if keep else None
        _lib.launch("gif_flame_skin_f32", coef.device, tmpl, dirs, lbs_w, coef, A, verts, v_posed, B, V, KP, J)
        if keep:
            ctx.save_for_backward(A, v_posed, dirs, lbs_w)
        ctx.dtypes = (coef.dtype, A.dtype)
        return verts

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, g_verts):
        A, v_posed, dirs, lbs_w = ctx.saved_tensors
        B, V, _ = v_posed.shape
        KP, J = dirs.shape[0], lbs_w.shape[1]
        need_c, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g_verts.contiguous().float()
        dev = g.device
        g_coef = torch.empty((B, KP), device=dev, dtype=torch.float32) if need_c else None
        g_A = torch.empty((B, J, 12), device=dev, dtype=torch.float32) if need_a else None
        ws = _lib.workspace(_lib.load().gif_flame_skin_bwd_workspace_bytes(B, V, KP, J), dev)
        _lib.launch("gif_flame_skin_bwd_f32", dev, dirs, lbs_w, A, g, v_posed, g_coef, g_A, B, V, KP, J, ws)
        return g_coef, g_A, None, None, None


def _group_args(ins):
    """(address, row stride) per parameter group for the joints kernels, and the tensors that must stay alive until the launch is
    queued.  A float32 tensor whose columns are adjacent goes in as it is (a column slice of a wider tensor is not copied)."""
    keep, args = [], []
    for t in ins:
        if t is None:
            args += [None, 0]
            continue
        if t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
            t = t.float().contiguous()
        keep.append(t)
        args += [t.data_ptr(), t.stride(0)]
    return args, keep


def _launch_pose_chain_bwd(dev, *args):
    """The one place gif_pose_chain_bwd_f32 is launched from."""
    _lib.launch("gif_pose_chain_bwd_f32", dev, *args)


class _FlameJointsFn(Function):
    """(coef [B,KP], A [B,J,12]) = gif_flame_joints_f32 of the five parameter groups (None = zeros), the launch of the no-grad path;
    backward: gif_pose_chain_bwd_f32 on the g_coef / g_A that _FlameSkinFn hands back, one launch for all groups.  Nothing but the
    inputs themselves is kept: the backward kernel recomputes joints, rotations and the chain."""

    @staticmethod
    def forward(ctx, consts, dims, shape, exp, pose, neck, eye):
        J0, Jdirs, parents_c = consts
        B, n_shape, n_exp, KP, J = dims
        dev = J0.device
        ins = [None if t is None else t.detach() for t in (shape, exp, pose, neck, eye)]
        args, keep = _group_args(ins)
        coef = torch.empty((B, KP), device=dev, dtype=torch.float32)
        A = torch.empty((B, J, 12), device=dev, dtype=torch.float32)
        _lib.launch("gif_flame_joints_f32", dev, J0, Jdirs, parents_c, *args[0:2], n_shape, *args[2:4], n_exp, *args[4:], A, coef,
                    B, KP, J)
        ctx.consts, ctx.dims = consts, dims
        ctx.save_for_backward(*[t for t in ins if t is not None])
        ctx.present = [t is not None for t in ins]
        return coef, A

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly
    def backward(ctx, g_coef, g_A):
        need = ctx.needs_input_grad[2:7]
        if not any(need):
            return (None,) * 7
        J0, Jdirs, parents_c = ctx.consts
        B, n_shape, n_exp, KP, J = ctx.dims
        dev = J0.device
        saved = iter(ctx.saved_tensors)
        ins = [next(saved) if have else None for have in ctx.present]
        args, keep = _group_args(ins)
        outs = [torch.empty((B, n), device=dev, dtype=torch.float32) if want else None
                for want, n in zip(need, (n_shape, n_exp, 6, 3, 6))]
        _launch_pose_chain_bwd(dev, J0, Jdirs, parents_c, *args[0:2], n_shape, *args[2:4], n_exp, *args[4:],
                               g_A.contiguous().float(), g_coef.contiguous().float(), *outs, B, KP, J)
        return (None, None) + tuple(outs)


def _launch_landmarks_bwd(g_lmk, row, tables, g_verts, B, V, R, Ld, Ls):
    """The one place gif_flame_landmarks_bwd_f32 is launched from (on g_verts' device and its current stream)."""
    _lib.launch("gif_flame_landmarks_bwd_f32", g_verts.device, g_lmk, row, *tables, g_verts, B, V, R, Ld, Ls)


class _FlameLandmarksFn(Function):
    """lmk [B,Ld+Ls,3] = cat(dynamic[row(A[:, yaw_joint])], static) landmarks of verts, on gif_flame_landmarks_f32 /
    gif_flame_landmarks_bwd_f32.  tables = (dyn_vid [R,Ld,3] int32, dyn_bary, st_vid [Ls,3] int32, st_bary); an empty table is
    None.  The gradient goes to verts alone: the row choice is piecewise constant in A."""

    @staticmethod
    def forward(ctx, verts, A, yaw_joint, R, Ld, Ls, dyn_vid, dyn_bary, st_vid, st_bary):
        _lib.require_device("flame landmarks", verts=verts, A=A)
        B, V, _ = verts.shape
        J = A.shape[1]
        verts, A = verts.contiguous().float(), A.contiguous().float()
        tables = (dyn_vid, dyn_bary, st_vid, st_bary)
        lmk = torch.empty((B, Ld + Ls, 3), device=verts.device, dtype=torch.float32)
        row = torch.empty((B,), device=verts.device, dtype=torch.int32)
        _lib.launch("gif_flame_landmarks_f32", verts.device, verts, A, *tables, lmk, row, B, V, J, yaw_joint, R, Ld, Ls)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(row, *[t for t in tables if t is not None])
            ctx.present = [t is not None for t in tables]
        ctx.dims = (B, V, R, Ld, Ls)
        ctx.mark_non_differentiable(row)
        return lmk, row

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly
    def backward(ctx, g_lmk, _g_row):
        if not ctx.needs_input_grad[0]:
            return (None,) * 10  # nothing to launch: A receives no gradient
        row, *rest = ctx.saved_tensors
        rest = iter(rest)
        tables = [next(rest) if have else None for have in ctx.present]
        B, V, R, Ld, Ls = ctx.dims
        g = g_lmk.contiguous().float()
        g_verts = torch.empty((B, V, 3), device=g.device, dtype=torch.float32)
        _launch_landmarks_bwd(g, row, tables, g_verts, B, V, R, Ld, Ls)
        return (g_verts,) + (None,) * 9


class FlameLayer(nn.Module):
    """FLAME layer over a FlameModel: the first `n_shape` shape columns and the first `n_exp` expression columns of its
    shapedirs.  forward(shape_params [B,n_shape], expression_params [B,n_exp], pose_params [B,6] = (global, jaw) axis-angle,
    neck_pose [B,3], eye_pose [B,6]) -> (vertices [B,V,3], landmarks2d, landmarks3d); missing arguments are zeros.  A model with
    J != 5 joints takes the first 3 J entries of cat(global, neck, jaw, eyes) (zeros past the fifth).

    `landmarks`: a FlameLandmarkEmbedding over the layer's vertices -> landmarks2d [B,Ld+Ls,3] = cat(the dynamic contour row chosen
    from the yaw of joint `yaw_joint`, the static landmarks) and landmarks3d [B,Lf,3] (the static "full" set): one more launch
    (gif_flame_landmarks_f32) on the vertices and the chain's transforms A, both already on the device; differentiable through
    the vertices.  None (the default): both outputs are None and nothing else changes.
    `vertex_ids`: keep only these rows of the model's vertices (template rows, the three dirs columns per vertex, lbs_weights
    rows); the joints still come from the full model (J0, Jdirs), so the kept vertices move exactly as they do in the full layer.
    The landmark tables then index the kept list.

    No input requires a gradient: two launches (gif_flame_joints_f32, gif_flame_skin_f32).  Otherwise the joints, the rotations
    and the chain run as torch ops on [B,J,.] tensors — the same J0 + Jdirs . betas form, so both paths compute one function —
    and autograd carries the skin kernels' g_coef / g_A back through them.  The constants receive no gradient.
    `fused_chain=True`: a forward that needs gradients runs the no-grad path's two launches instead (v_posed kept),
    and the backward of the joints launch is one launch too, gif_pose_chain_bwd_f32, for whichever groups require a gradient."""

    def __init__(self, model, n_shape=100, n_exp=50, landmarks=None, vertex_ids=None, fused_chain=False):
        super().__init__()
        self.fused_chain = bool(fused_chain)
        if not (0 <= n_shape <= model.n_shape and 0 <= n_exp <= model.n_exp):
            raise ValueError(f"model has {model.n_shape} shape and {model.n_exp} expression columns; asked for {n_shape}, {n_exp}")
        self.n_shape, self.n_exp = n_shape, n_exp
        f32 = lambda a: np.asarray(a, np.float32)
        V, J = model.lbs_weights.shape
        tmpl, sd, J0, Jdirs = joint_basis(model, n_shape, n_exp)  # (computed in fp64, rounded once)
        dirs = np.concatenate([sd.reshape(3 * V, -1).T, f32(model.posedirs)], 0)  # [KP,3V], k-major
        lbs_w = f32(model.lbs_weights)
        if vertex_ids is not None:
            ids = np.asarray(vertex_ids)
            if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
                raise ValueError(f"vertex_ids must be a 1-D integer array, got {ids.dtype} {list(ids.shape)}")
            ids = ids.astype(np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= V):
                raise ValueError(f"vertex_ids outside 0..{V - 1}")
            tmpl, lbs_w = tmpl[ids], lbs_w[ids]
            dirs = dirs.reshape(dirs.shape[0], V, 3)[:, ids].reshape(dirs.shape[0], 3 * len(ids))
            V = len(ids)
        self.parents = tuple(int(p) for p in model.parents)
        self._parents_c = (ctypes.c_int32 * J)(*self.parents)
        for name, a in (("v_template", tmpl.reshape(-1)), ("dirs", dirs), ("lbs_weights", lbs_w),
                        ("J0", f32(J0).reshape(-1)), ("Jdirs", f32(Jdirs))):
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a)))
        self._lmk = None
        if landmarks is not None:
            landmarks.check_vertices(V)
            if not landmarks.yaw_joint < J:
                raise ValueError(f"landmarks.yaw_joint = {landmarks.yaw_joint} outside 0..{J - 1}")
            # one static table: the Ls static landmarks of landmarks2d, then the Lf of landmarks3d — one launch yields both
            st_vid = np.concatenate([landmarks.static_vid, landmarks.full_vid], 0)
            st_bary = np.concatenate([landmarks.static_bary, landmarks.full_bary], 0)
            R, Ld = landmarks.dynamic_vid.shape[:2]
            self._lmk = (landmarks.yaw_joint, R, Ld, landmarks.static_vid.shape[0], landmarks.full_vid.shape[0])
            for name, a, dt in (("lmk_dyn_vid", landmarks.dynamic_vid, np.int32), ("lmk_dyn_bary", landmarks.dynamic_bary, np.float32),
                                ("lmk_st_vid", st_vid, np.int32), ("lmk_st_bary", st_bary, np.float32)):
                self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))))

    @property
    def n_vertices(self):
        return self.lbs_weights.shape[0]

    def _rows(self, t, n, name, B):
        if t is not None and (t.ndimension() != 2 or t.shape != (B, n)):
            raise ValueError(f"{name} must be [{B},{n}], got {list(t.shape)}")
        return t

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None):
        _lib.require_device("FlameLayer", layer=self.dirs, shape_params=shape_params, expression_params=expression_params,
                            pose_params=pose_params, neck_pose=neck_pose, eye_pose=eye_pose)
        given = [t for t in (shape_params, expression_params, pose_params, neck_pose, eye_pose) if t is not None]
        B = given[0].shape[0] if given else 1
        ins = [self._rows(t, n, name, B) for t, n, name in (
            (shape_params, self.n_shape, "shape_params"), (expression_params, self.n_exp, "expression_params"),
            (pose_params, 6, "pose_params"), (neck_pose, 3, "neck_pose"), (eye_pose, 6, "eye_pose"))]
        if torch.is_grad_enabled() and any(t.requires_grad for t in given):
            verts, A = self._forward_fused(B, ins) if self.fused_chain else self._forward_grad(B, *ins)
        else:
            verts, A = self._forward_nograd(B, ins)
        return (verts,) + self._landmarks(verts, A)

    def _forward_nograd(self, B, ins):
        dev = self.dirs.device
        V, J = self.lbs_weights.shape
        KP = self.dirs.shape[0]
        args, keep = _group_args(ins)  # views such as flame_batch[:, 0:100] go in as they are; `keep` lives until both launches are queued
        coef = torch.empty((B, KP), device=dev, dtype=torch.float32)
        A = torch.empty((B, J, 12), device=dev, dtype=torch.float32)
        verts = torch.empty((B, V, 3), device=dev, dtype=torch.float32)
        _lib.launch("gif_flame_joints_f32", dev, self.J0, self.Jdirs, self._parents_c, *args[0:2], self.n_shape, *args[2:4],
                    self.n_exp, *args[4:], A, coef, B, KP, J)
        _lib.launch("gif_flame_skin_f32", dev, self.v_template, self.dirs, self.lbs_weights, coef, A, verts, None, B, V, KP, J)
        return verts, A

    def _forward_fused(self, B, ins):
        KP, J = self.dirs.shape[0], self.lbs_weights.shape[1]
        coef, A = _FlameJointsFn.apply((self.J0, self.Jdirs, self._parents_c), (B, self.n_shape, self.n_exp, KP, J), *ins)
        return _FlameSkinFn.apply(coef, A, self.v_template, self.dirs, self.lbs_weights), A

    def _forward_grad(self, B, shape, exp, pose, neck, eye):
        dev = self.dirs.device
        J = self.lbs_weights.shape[1]
        z = lambda t, n: torch.zeros((B, n), device=dev, dtype=torch.float32) if t is None else t.float()
        pose = z(pose, 6)
        betas = torch.cat([z(shape, self.n_shape), z(exp, self.n_exp)], 1)
        joints = (self.J0[None] + betas @ self.Jdirs).view(B, J, 3)
        full = torch.cat([pose[:, :3], z(neck, 3), pose[:, 3:6], z(eye, 6)], 1)
        if J > 5:
            full = torch.cat([full, full.new_zeros(B, 3 * (J - 5))], 1)
        R = rodrigues(full[:, :3 * J].reshape(B * J, 3)).view(B, J, 3, 3)
        pose_feature = (R[:, 1:] - torch.eye(3, device=dev)).reshape(B, 9 * (J - 1))
        GR, Gt = [R[:, 0]], [joints[:, 0]]
        for j in range(1, J):
            p = self.parents[j]
            GR.append(GR[p] @ R[:, j])
            Gt.append((GR[p] @ (joints[:, j] - joints[:, p])[:, :, None])[:, :, 0] + Gt[p])
        GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
        A = torch.cat([GR, (Gt - (GR @ joints[..., None])[..., 0])[..., None]], 3).reshape(B, J, 12)
        return _FlameSkinFn.apply(torch.cat([betas, pose_feature], 1), A, self.v_template, self.dirs, self.lbs_weights), A

    def _landmarks(self, verts, A):
        """(landmarks2d, landmarks3d) of the layer's vertices: one launch over the concatenated static table, split into views."""
        if self._lmk is None:
            return None, None
        yaw_joint, R, Ld, Ls, Lf = self._lmk
        if Ld + Ls + Lf == 0:
            return verts.new_empty((verts.shape[0], 0, 3)), verts.new_empty((verts.shape[0], 0, 3))
        some = lambda t: t if t.numel() else None
        lmk, _ = _FlameLandmarksFn.apply(verts, A, yaw_joint, R, Ld, Ls + Lf, some(self.lmk_dyn_vid), some(self.lmk_dyn_bary),
                                         some(self.lmk_st_vid), some(self.lmk_st_bary))
        return lmk[:, :Ld + Ls], lmk[:, Ld + Ls:]


class FlameLandmarkLayer(FlameLayer):
    """(landmarks2d, landmarks3d) alone: a FlameLayer over embedding.vertex_ids() — the few hundred vertices the tables name — with
    the tables remapped to that compact list, so a landmark fit skins those vertices instead of all V, forward and backward.  Same
    arguments as FlameLayer.forward; the landmarks are those of FlameLayer(model, landmarks=embedding)."""

    def __init__(self, model, embedding, n_shape=100, n_exp=50, fused_chain=False):
        embedding.check_vertices(model.lbs_weights.shape[0])
        ids = embedding.vertex_ids()
        super().__init__(model, n_shape, n_exp, landmarks=embedding.remapped(ids), vertex_ids=ids, fused_chain=fused_chain)

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None):
        return super().forward(shape_params, expression_params, pose_params, neck_pose, eye_pose)[1:]
