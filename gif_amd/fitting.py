"""FLAME landmark fitting on the device: detected 2-D landmarks -> FLAME parameters and an orthographic camera.

* landmark_loss        — [B] = sum_l w |project(lmk, cam)[:2] - target|^2 on gif_landmark_loss_f32: the projection, the distance and
                         both gradients in one launch; the backward only scales what the forward stored.
* FlameLandmarkFitter  — the loop: FlameLandmarkLayer(fused_chain=True) -> landmark_loss -> Adam, first the global rotation and the
                         camera alone, then every enabled group.  Ordinary autograd over the public pieces; no iteration copies
                         anything to the host.
No CPU fallback.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .flame import FlameLandmarkLayer, project_landmarks


class _LandmarkLossFn(Function):
    @staticmethod
    def forward(ctx, lmk, cam, target, weight):
        B, L = lmk.shape[0], lmk.shape[1]
        dev = lmk.device
        f = lambda t: t.detach().contiguous().float()
        need_l, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        loss = torch.empty((B,), device=dev, dtype=torch.float32)
        g_lmk = torch.empty((B, L, 3), device=dev, dtype=torch.float32) if need_l else None
        g_cam = torch.empty((B, 3), device=dev, dtype=torch.float32) if need_c else None
        _lib.launch("gif_landmark_loss_f32", dev, f(lmk), f(cam), f(target), None if weight is None else f(weight), loss, g_lmk,
                    g_cam, B, L)
        ctx.save_for_backward(*[g for g in (g_lmk, g_cam) if g is not None])
        ctx.have = (need_l, need_c)
        return loss

    @staticmethod
    @once_differentiable  # the stored gradients carry no history: a double backward must fail loudly
    def backward(ctx, up):
        saved = iter(ctx.saved_tensors)
        g_lmk, g_cam = [next(saved) if have else None for have in ctx.have]
        up = up.float()
        return (None if g_lmk is None else g_lmk * up[:, None, None], None if g_cam is None else g_cam * up[:, None], None, None)


def landmark_loss(lmk, cam, target, weight=None):
    """lmk [B,L,3], cam [B,3] = (s, tx, ty), target [B,L,2], weight [B,L] or None (ones) -> loss [B] =
    sum_l weight |p - target|^2 with p = (s (x + tx), -s (y + ty)), project_landmarks' first two components; no normalisation.
    Differentiable with respect to lmk and cam (not target, not weight).  A landmark of weight exactly 0 contributes exact zeros
    even where its target is NaN or infinite: that is how a missing detection is marked."""
    _lib.require_device("landmark_loss", lmk=lmk, cam=cam, target=target, weight=weight)
    if lmk.dim() != 3 or lmk.shape[2] != 3:
        raise ValueError(f"lmk must be [B,L,3], got {list(lmk.shape)}")
    B, L = lmk.shape[:2]
    for name, t, want in (("cam", cam, (B, 3)), ("target", target, (B, L, 2)), ("weight", weight, (B, L))):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"{name} must be {list(want)}, got {list(t.shape)}")
    return _LandmarkLossFn.apply(lmk, cam, target, weight)


class FlameLandmarkFitter:
    """Fits shape, expression, pose (global rotation and jaw), neck and eye poses and a camera (s, tx, ty) per sample to 2-D
    landmarks `target2d [B,L,2]`, L = the embedding's Ld + Ls landmarks2d in the layer's order, in the coordinates of
    project_landmarks (x right, y up negated).  `weight [B,L]`: per-landmark weights; 0 marks a missing detection (its target may
    be NaN).

    Loss: sum_b landmark_loss_b + reg_shape |shape|^2 + reg_exp |expression|^2.  Adam (torch.optim.Adam over the six parameter
    tensors, DESIGN.md §3q says why).  The first `rigid_steps` iterations move the global rotation (pose[:, :3]) and the camera only:
    the other groups go into the layer detached, so nothing is computed for them, and the jaw's half of the pose gradient is zeroed.
    After that every enabled group moves (`fit_neck`, `fit_eyes`; a disabled group stays at its initial value).
    Start: zeros and cam = (s0, 0, 0), or `init`: a dict with any of shape, expression, pose, neck_pose, eye_pose, cam.

    fit() returns a dict of device tensors: shape, expression, pose, neck_pose, eye_pose, cam, loss_history [steps,B] (per sample:
    the landmark term plus the sample's share of the two regularisers, evaluated BEFORE the iteration's update) and landmarks2d
    [B,L,2], the projected landmarks of the result."""

    GROUPS = ("shape", "expression", "pose", "neck_pose", "eye_pose", "cam")

    def __init__(self, model, embedding, n_shape=100, n_exp=50, lr=0.01, steps=200, rigid_steps=50, reg_shape=1e-4, reg_exp=1e-4,
                 fit_neck=True, fit_eyes=False, s0=1.0, device="cuda"):
        if not 0 <= rigid_steps <= steps:
            raise ValueError(f"rigid_steps = {rigid_steps} outside 0..steps = {steps}")
        self.layer = FlameLandmarkLayer(model, embedding, n_shape, n_exp, fused_chain=True).to(device)
        self.n_shape, self.n_exp = n_shape, n_exp
        self.lr, self.steps, self.rigid_steps = lr, steps, rigid_steps
        self.reg_shape, self.reg_exp = reg_shape, reg_exp
        self.fit_neck, self.fit_eyes, self.s0 = fit_neck, fit_eyes, s0

    def _start(self, B, init):
        dev = self.layer.dirs.device
        widths = dict(zip(self.GROUPS, (self.n_shape, self.n_exp, 6, 3, 6, 3)))
        init = dict(init or {})
        unknown = set(init) - set(self.GROUPS)
        if unknown:
            raise ValueError(f"init: unknown entries {sorted(unknown)}")
        x = {}
        for name, n in widths.items():
            t = torch.zeros((B, n), device=dev, dtype=torch.float32)
            if name in init:
                _lib.require_device("FlameLandmarkFitter", **{name: init[name]})
                if tuple(init[name].shape) != (B, n):
                    raise ValueError(f"init[{name!r}] must be [{B},{n}], got {list(init[name].shape)}")
                t.copy_(init[name])
            elif name == "cam":
                t[:, 0] = self.s0
            x[name] = t.requires_grad_(True)
        return x

    def step_loss(self, x, target2d, weight, rigid):
        """[B]: one iteration's loss per sample at the parameters `x` (a dict of the six tensors)."""
        moves = lambda t, enabled=True: t if enabled and not rigid else t.detach()
        shape, exp = moves(x["shape"]), moves(x["expression"])
        neck, eye = moves(x["neck_pose"], self.fit_neck), moves(x["eye_pose"], self.fit_eyes)
        l2d = self.layer(shape, exp, x["pose"], neck, eye)[0]
        per = landmark_loss(l2d, x["cam"], target2d, weight)
        return per + self.reg_shape * (shape * shape).sum(1) + self.reg_exp * (exp * exp).sum(1)

    def iterate(self, x, opt, target2d, weight, rigid, record=None, loss_fn=None):
        """One iteration: loss, backward, Adam step; the per-sample loss goes into `record` [B] (a device tensor) when given.
        `loss_fn`: another implementation of step_loss (tools/fit_bench.py times the loop around an unfused one)."""
        opt.zero_grad(set_to_none=True)
        per = (loss_fn or self.step_loss)(x, target2d, weight, rigid)
        if record is not None:
            record.copy_(per.detach())
        per.sum().backward()
        if rigid:
            x["pose"].grad[:, 3:].zero_()  # the jaw waits with the other groups
        opt.step()

    def fit(self, target2d, weight=None, init=None):
        _lib.require_device("FlameLandmarkFitter", target2d=target2d, weight=weight)
        if target2d.dim() != 3 or target2d.shape[2] != 2:
            raise ValueError(f"target2d must be [B,L,2], got {list(target2d.shape)}")
        B = target2d.shape[0]
        x = self._start(B, init)
        opt = torch.optim.Adam([x[name] for name in self.GROUPS], lr=self.lr)
        history = torch.zeros((self.steps, B), device=target2d.device, dtype=torch.float32)
        for it in range(self.steps):
            self.iterate(x, opt, target2d, weight, it < self.rigid_steps, history[it])
        out = {name: t.detach() for name, t in x.items()}
        with torch.no_grad():
            l2d = self.layer(out["shape"], out["expression"], out["pose"], out["neck_pose"], out["eye_pose"])[0]
            out["landmarks2d"] = project_landmarks(l2d, out["cam"])[:, :, :2]
        out["loss_history"] = history
        return out
