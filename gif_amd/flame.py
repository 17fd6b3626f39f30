"""The FLAME layer on HIP kernels: (shape, expression, pose) -> vertices, differentiable with respect to all three.

The reference keeps its FLAME layer in the absent `photometric_optimization` submodule and the model file is licensed, but the
algorithm is public (FLAME, Li et al. 2017, in the smplx formulation): shape / expression blend shapes, pose-corrective blend
shapes, joint regression, a kinematic chain and linear blend skinning.  This module is that algorithm with the call signature
FlameTextureSpace.forward uses (model/stg2_generator.py:362-364); DESIGN.md §3l has the layout and the measurements.

* FlameModel            — the six constant arrays of a model; .npz in and out (what a licensed model file is converted into).
* synthetic_flame_model — a model with FLAME's structure over any template mesh (no assets needed to build, test or measure).
* FlameLayer            — nn.Module, `FlameLayer(model)(shape_params, expression_params, pose_params) -> (vertices, None, None)`;
                          drops into render.FlameConditionRenderer(flame=...).
Kernels (csrc/flame.hip): gif_flame_joints_f32, gif_flame_skin_f32, gif_flame_skin_bwd_f32.  No CPU fallback.
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


def joint_basis(model, n_shape, n_exp):
    """(tmpl [V,3], sd [V,3,K], J0 [J,3], Jdirs [K,3J]): the layer's fp32 template and selected blend-shape columns, and the
    joints as a linear function of betas — joints = J0 + betas . Jdirs with J0 = J_regressor . v_template and Jdirs =
    J_regressor . shapedirs, in float64 from the fp32-rounded arrays (the model IS its fp32 constants)."""
    cols = np.concatenate([np.arange(n_shape), model.n_shape + np.arange(n_exp)]).astype(np.int64)
    sd = np.asarray(model.shapedirs, np.float32)[:, :, cols]
    tmpl = np.asarray(model.v_template, np.float32)
    jr = np.asarray(model.J_regressor, np.float32).astype(np.float64)
    J0 = jr @ tmpl.astype(np.float64)
    Jdirs = np.einsum("jv,vik->kji", jr, sd.astype(np.float64)).reshape(sd.shape[2], -1)
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
        with torch.cuda.device(coef.device):  # launch on the operands' device and its current stream
            _lib.check(_lib.load().gif_flame_skin_f32(tmpl.data_ptr(), dirs.data_ptr(), lbs_w.data_ptr(), coef.data_ptr(),
                                                      A.data_ptr(), verts.data_ptr(), v_posed.data_ptr() if keep else None,
                                                      B, V, KP, J, torch.cuda.current_stream().cuda_stream), "flame_skin")
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
        lib = _lib.load()
        dev = g.device
        g_coef = torch.empty((B, KP), device=dev, dtype=torch.float32) if need_c else None
        g_A = torch.empty((B, J, 12), device=dev, dtype=torch.float32) if need_a else None
        ws = torch.empty((max(lib.gif_flame_skin_bwd_workspace_bytes(B, V, KP, J) // 4, 1),), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.gif_flame_skin_bwd_f32(dirs.data_ptr(), lbs_w.data_ptr(), A.data_ptr(), g.data_ptr(), v_posed.data_ptr(),
                                                  g_coef.data_ptr() if need_c else None, g_A.data_ptr() if need_a else None,
                                                  B, V, KP, J, ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "flame_skin_bwd")
        return g_coef, g_A, None, None, None


class FlameLayer(nn.Module):
    """FLAME layer over a FlameModel: the first `n_shape` shape columns and the first `n_exp` expression columns of its
    shapedirs.  forward(shape_params [B,n_shape], expression_params [B,n_exp], pose_params [B,6] = (global, jaw) axis-angle,
    neck_pose [B,3], eye_pose [B,6]) -> (vertices [B,V,3], None, None); missing arguments are zeros; the landmark outputs are
    not computed.  A model with J != 5 joints takes the first 3 J entries of cat(global, neck, jaw, eyes) (zeros past the fifth).

    No input requires a gradient: two launches (gif_flame_joints_f32, gif_flame_skin_f32).  Otherwise the joints, the rotations
    and the chain run as torch ops on [B,J,.] tensors — the same J0 + Jdirs . betas form, so both paths compute one function —
    and autograd carries the skin kernels' g_coef / g_A back through them.  The constants receive no gradient."""

    def __init__(self, model, n_shape=100, n_exp=50):
        super().__init__()
        if not (0 <= n_shape <= model.n_shape and 0 <= n_exp <= model.n_exp):
            raise ValueError(f"model has {model.n_shape} shape and {model.n_exp} expression columns; asked for {n_shape}, {n_exp}")
        self.n_shape, self.n_exp = n_shape, n_exp
        f32 = lambda a: np.asarray(a, np.float32)
        V, J = model.lbs_weights.shape
        tmpl, sd, J0, Jdirs = joint_basis(model, n_shape, n_exp)  # (computed in fp64, rounded once)
        dirs = np.concatenate([sd.reshape(3 * V, -1).T, f32(model.posedirs)], 0)  # [KP,3V], k-major
        self.parents = tuple(int(p) for p in model.parents)
        self._parents_c = (ctypes.c_int32 * J)(*self.parents)
        for name, a in (("v_template", tmpl.reshape(-1)), ("dirs", dirs), ("lbs_weights", f32(model.lbs_weights)),
                        ("J0", f32(J0).reshape(-1)), ("Jdirs", f32(Jdirs))):
            self.register_buffer(name, torch.from_numpy(np.ascontiguousarray(a)))

    @property
    def n_vertices(self):
        return self.lbs_weights.shape[0]

    def _rows(self, t, n, name, B):
        if t is None:
            return None
        if not t.is_cuda:
            raise _lib.GifHipError(f"FlameLayer needs device tensors ({name} is on the CPU; no CPU fallback)")
        if t.ndimension() != 2 or t.shape != (B, n):
            raise ValueError(f"{name} must be [{B},{n}], got {list(t.shape)}")
        if t.device != self.dirs.device:
            raise _lib.GifHipError(f"{name} is on {t.device}, the layer's constants on {self.dirs.device}")
        return t

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None):
        given = [t for t in (shape_params, expression_params, pose_params, neck_pose, eye_pose) if t is not None]
        if not self.dirs.is_cuda or any(not t.is_cuda for t in given):
            raise _lib.GifHipError("FlameLayer needs device tensors and a layer moved to the device (no CPU fallback)")
        B = given[0].shape[0] if given else 1
        ins = [self._rows(t, n, name, B) for t, n, name in (
            (shape_params, self.n_shape, "shape_params"), (expression_params, self.n_exp, "expression_params"),
            (pose_params, 6, "pose_params"), (neck_pose, 3, "neck_pose"), (eye_pose, 6, "eye_pose"))]
        if torch.is_grad_enabled() and any(t.requires_grad for t in given):
            return self._forward_grad(B, *ins), None, None
        return self._forward_nograd(B, ins), None, None

    def _forward_nograd(self, B, ins):
        dev = self.dirs.device
        V, J = self.lbs_weights.shape
        KP = self.dirs.shape[0]
        args = []
        for t in ins:  # (pointer, row stride): views such as flame_batch[:, 0:100] go in as they are
            if t is None:
                args += [None, 0]
                continue
            if t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
                t = t.float().contiguous()
            args += [t, t.stride(0)]
        ptr = lambda t: None if t is None else t.data_ptr()
        coef = torch.empty((B, KP), device=dev, dtype=torch.float32)
        A = torch.empty((B, J, 12), device=dev, dtype=torch.float32)
        verts = torch.empty((B, V, 3), device=dev, dtype=torch.float32)
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(lib.gif_flame_joints_f32(self.J0.data_ptr(), self.Jdirs.data_ptr(), self._parents_c,
                                                ptr(args[0]), args[1], self.n_shape, ptr(args[2]), args[3], self.n_exp,
                                                ptr(args[4]), args[5], ptr(args[6]), args[7], ptr(args[8]), args[9],
                                                A.data_ptr(), coef.data_ptr(), B, KP, J, stream), "flame_joints")
            _lib.check(lib.gif_flame_skin_f32(self.v_template.data_ptr(), self.dirs.data_ptr(), self.lbs_weights.data_ptr(),
                                              coef.data_ptr(), A.data_ptr(), verts.data_ptr(), None, B, V, KP, J, stream),
                       "flame_skin")
        return verts

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
        return _FlameSkinFn.apply(torch.cat([betas, pose_feature], 1), A, self.v_template, self.dirs, self.lbs_weights)
