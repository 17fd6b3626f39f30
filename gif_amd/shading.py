"""The shaded half of GIF's condition: the FLAME albedo texture, sampled through the mesh's UV chart and lit by nine
spherical-harmonics coefficients per colour channel — what OverLayViz.get_rendered_mesh(flame_params=(shape, exp, pose, light_code,
texture_code)) renders (my_utils/visualize_flame_overlay.py:17-33; label columns 159:209 texture code, 209:236 light code,
constants.py DECA_IDX).  The renderer itself sits in the reference's absent `photometric_optimization` submodule; the definition
used here is the public one DECA's light codes are written for (second-order SH irradiance, Ramamoorthi & Hanrahan 2001), stated in
include/gif_hip.h and DESIGN.md §3m.

Deferred shading in image space: the two rasteriser passes the condition needs anyway deliver an interpolated UV coordinate and an
interpolated normal per pixel; one pointwise kernel turns them into the lit texture.

* sh_shade                      — autograd Function over gif_shade_sh_f32 / gif_shade_sh_bwd_f32 (csrc/shade.hip).
* rasterize_face_attributes     — the attribute rasteriser for per-face-corner attributes (UV charts have seams).
* render_shaded_condition       — vertices, UVs, albedo, light -> the 6-channel condition, like render.render_condition.
* FlameTextureModel             — mean + linear basis of the albedo texture; .npz in and out; decode by one addmm.
* synthetic_texture_model, synthetic_face_uvs — stand-ins with the right structure (no assets needed to build, test or measure).
* ShadedFlameConditionRenderer  — flame_batch [N, >=236] -> (rend_flm, norma_map_img); drops into InterpolatedTextureLoss.
No CPU fallback.  Deterministic except the gradient to the albedo (fp32 atomics), which only texture fitting asks for.
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import render

N_LABEL_COLUMNS = 236  # shape 0:100, expression 100:150, pose 150:156, camera 156:159, texture 159:209, light 209:236


class _ShShadeFn(Function):
    @staticmethod
    def forward(ctx, uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul, nrm_add):
        B, _, H, W = uv_img.shape
        uv, nrm = uv_img.contiguous().float(), normal_img.contiguous().float()
        alb, sh = albedo.contiguous().float(), sh_coeff.contiguous().float()
        m8 = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else (mask != 0).contiguous().view(torch.uint8)
        out = torch.empty((B, 3, H, W), device=uv.device, dtype=torch.float32)
        _lib.launch("gif_shade_sh_f32", uv.device, uv, nrm, m8, alb, sh, out, B, alb.shape[0], H, W, alb.shape[2], nrm_mul, nrm_add)
        ctx.save_for_backward(uv, nrm, m8, alb, sh)
        ctx.scale = (float(nrm_mul), float(nrm_add))
        ctx.dtypes = (uv_img.dtype, normal_img.dtype, albedo.dtype, sh_coeff.dtype)
        return out

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, g_out):
        uv, nrm, m8, alb, sh = ctx.saved_tensors
        B, _, H, W = uv.shape
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        g = g_out.contiguous().float()
        outs = [torch.empty_like(t) if n else None for t, n in zip((uv, nrm, alb, sh), need)]  # only what autograd asks for
        ws = _lib.workspace(_lib.load().gif_shade_sh_bwd_workspace_bytes(B, H, W), g.device) if need[3] else None
        _lib.launch("gif_shade_sh_bwd_f32", g.device, uv, nrm, m8, alb, sh, g, *outs, B, alb.shape[0], H, W, alb.shape[2],
                    *ctx.scale, ws)
        g_uv, g_nrm, g_alb, g_sh = (None if t is None else t.to(dt) for t, dt in zip(outs, ctx.dtypes))
        return g_uv, g_nrm, None, g_alb, g_sh, None, None


def sh_shade(uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul=1.0, nrm_add=0.0):
    """Lit texture [B,3,H,W]: at every pixel of `mask` (bool [B,1,H,W], what rasterize_attributes returns), the bilinear sample of
    `albedo` [Ba,3,T,T] (Ba = 1: one texture for the batch, or Ba = B) at grid coordinate uv_img[:, :2] — the semantics of
    F.grid_sample(bilinear, zeros, align_corners=False) — times the SH irradiance sum_i k_i basis_i(n) sh_coeff[b,i,c] of
    n = nrm_mul * normal_img + nrm_add (not re-normalised); 0 outside the mask.  Differentiable with respect to uv_img, normal_img,
    albedo and sh_coeff; only the gradients autograd asks for are computed.  The gradient to `albedo` is accumulated with float
    atomics (last bits vary from run to run); everything else is deterministic."""
    _lib.require_device("sh_shade", uv_img=uv_img, normal_img=normal_img, mask=mask, albedo=albedo, sh_coeff=sh_coeff)
    if uv_img.ndimension() != 4 or uv_img.shape[1] != 3:
        raise ValueError(f"uv_img must be [B,3,H,W], got {list(uv_img.shape)}")
    B, _, H, W = uv_img.shape
    if normal_img.shape != uv_img.shape:
        raise ValueError(f"normal_img must be {list(uv_img.shape)}, got {list(normal_img.shape)}")
    if tuple(mask.shape) != (B, 1, H, W):
        raise ValueError(f"mask must be [{B},1,{H},{W}], got {list(mask.shape)}")
    if albedo.ndimension() != 4 or albedo.shape[0] not in (1, B) or albedo.shape[1] != 3 or albedo.shape[2] != albedo.shape[3]:
        raise ValueError(f"albedo must be [1 or {B},3,T,T], got {list(albedo.shape)}")
    if tuple(sh_coeff.shape) != (B, 9, 3):
        raise ValueError(f"sh_coeff must be [{B},9,3], got {list(sh_coeff.shape)}")
    return _ShShadeFn.apply(uv_img, normal_img, mask, albedo, sh_coeff, float(nrm_mul), float(nrm_add))


def rasterize_face_attributes(vertices_ndc, faces, face_attributes, h, w):
    """render.rasterize_attributes for attributes given per FACE CORNER, [F,3,3] (shared by the batch) or [B,F,3,3]: a UV chart has
    its own topology (two faces that share a vertex across a seam give it different coordinates), so the attribute cannot be
    per vertex.  Same launches (render._RasterizeColorsFn), same conventions, same limits of the gradient (inside each pixel's
    winning face), which goes to vertices_ndc and, if asked, to face_attributes.  -> (images [B,3,h,w], mask [B,1,h,w])."""
    _lib.require_device("rasterize_face_attributes", vertices_ndc=vertices_ndc, face_attributes=face_attributes)
    F = faces.shape[-2]
    want = ((F, 3, 3), (vertices_ndc.shape[0], F, 3, 3))
    if tuple(face_attributes.shape) not in want:
        raise ValueError(f"face_attributes must be {list(want[0])} or {list(want[1])}, got {list(face_attributes.shape)}")
    return render._RasterizeColorsFn.apply(vertices_ndc, face_attributes, faces, h, w, False, "rasterize_face_attributes")[:2]


def render_shaded_condition(vertices_ndc, faces, face_uvs, albedo, sh_coeff, h=256, w=256, straight_through=False):
    """6-channel generator condition cat(shaded texture render, normal render) in [-1,1] — render.render_condition's channel order,
    8-bit quantisation and scaling, with the texture render computed instead of given: face_uvs [F,3,2] are grid coordinates in
    [-1,1] into albedo [1 or B,3,T,T]; sh_coeff [B,9,3].  Three passes: the normal render (vertex normals rasterised as n*0.5+0.5,
    exactly render_condition's), the UV render, and sh_shade on the un-quantised normal image (nrm_mul = 2, nrm_add = -1).  The
    texture render is clamp(shaded, 0, 1), quantised.  Differentiable with respect to vertices_ndc, face_uvs, albedo and sh_coeff;
    straight_through as in render_condition."""
    quant = render._quantize_straight_through if straight_through else render.quantize_8bit
    if face_uvs.ndimension() != 3 or tuple(face_uvs.shape[1:]) != (3, 2) or face_uvs.shape[0] != faces.shape[-2]:
        raise ValueError(f"face_uvs must be [{faces.shape[-2]},3,2], got {list(face_uvs.shape)}")
    normals = render.vertex_normals(vertices_ndc, faces)
    normal_img, mask = render.rasterize_attributes(vertices_ndc, faces, normals * 0.5 + 0.5, h, w)
    face_attr = torch.cat((face_uvs.float(), face_uvs.new_zeros((face_uvs.shape[0], 3, 1), dtype=torch.float32)), 2)
    uv_img, _ = rasterize_face_attributes(vertices_ndc, faces, face_attr, h, w)
    shaded = sh_shade(uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul=2.0, nrm_add=-1.0)
    tex_img = quant(shaded.clamp(0, 1)) * 2 - 1
    normal_img = quant(normal_img) * 2 - 1
    return torch.cat((tex_img, normal_img), dim=1)


class FlameTextureModel:
    """Linear albedo model: texture = mean + sum_k code_k basis_k, with mean [3,T,T] and basis [K,3,T,T] in RGB, [0,1] units.
    This is what a licensed FLAME_texture.npz is converted into: that file stores `mean` [T,T,3] and `tex_dir` [T,T,3,K] with the
    channels in BGR order and values in 0..255, so the conversion flips the channel axis (BGR -> RGB), divides by 255 and moves
    the channels in front (mean[:, :, ::-1].transpose(2, 0, 1) / 255, tex_dir[:, :, ::-1].transpose(3, 2, 0, 1) / 255)."""

    KEYS = ("mean", "basis")

    def __init__(self, mean, basis):
        self.mean = np.asarray(mean, np.float32)
        self.basis = np.asarray(basis, np.float32)
        if self.mean.ndim != 3 or self.mean.shape[0] != 3 or self.mean.shape[1] != self.mean.shape[2]:
            raise ValueError(f"mean must be [3,T,T], got {list(self.mean.shape)}")
        T = self.mean.shape[1]
        if self.basis.ndim != 4 or self.basis.shape[1:] != (3, T, T):
            raise ValueError(f"basis must be [K,3,{T},{T}], got {list(self.basis.shape)}")
        self._device_copies = {}

    @property
    def size(self):
        return self.mean.shape[1]

    @property
    def n_tex(self):
        return self.basis.shape[0]

    def save_npz(self, path):
        with open(path, "wb") as f:
            np.savez(f, **{k: getattr(self, k) for k in self.KEYS})

    @classmethod
    def from_npz(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: missing keys {missing}")
            return cls(*[z[k] for k in cls.KEYS])

    def _on(self, device):
        key = str(device)
        if key not in self._device_copies:
            K, T = self.n_tex, self.size
            self._device_copies[key] = (torch.from_numpy(self.mean.reshape(-1)).to(device),
                                        torch.from_numpy(self.basis.reshape(K, 3 * T * T)).to(device))
        return self._device_copies[key]

    def decode(self, tex_code):
        """tex_code [B,K] -> albedo [B,3,T,T] = mean + tex_code . basis, on tex_code's device: one torch.addmm (a single pass over
        the basis; plumbing, not a kernel of this library).  Differentiable with respect to tex_code."""
        if tex_code.ndimension() != 2 or tex_code.shape[1] != self.n_tex:
            raise ValueError(f"tex_code must be [B,{self.n_tex}], got {list(tex_code.shape)}")
        mean, basis = self._on(tex_code.device)
        return torch.addmm(mean, tex_code.float(), basis).view(tex_code.shape[0], 3, self.size, self.size)


def synthetic_texture_model(T=64, K=50, seed=0, amplitude=0.02):
    """A texture model with the structure of FLAME's: a smooth mean in [0.3, 0.7] and K smooth low-amplitude basis fields.
    Deterministic per seed.  NOT a skin texture: the arithmetic of one."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, T), np.linspace(-1, 1, T), indexing="ij")
    pts = np.stack([x, y], 0).reshape(2, -1)  # [2,T*T]

    def fields(n, freq):
        f = rng.randn(n, 3, 2) * freq
        phase = rng.rand(n, 3, 1) * 2 * np.pi
        return np.sin(f @ pts + phase).reshape(n, 3, T, T)

    mean = 0.5 + 0.2 * fields(1, 2.0)[0]
    return FlameTextureModel(mean, amplitude * fields(K, 3.0))


def synthetic_face_uvs(template, faces, seed=0):
    """A UV chart for any mesh, as grid coordinates [F,3,2] (float32 tensor): the template's x, y extent mapped into
    [-0.75, 0.75]^2 (y flipped: image rows grow downwards) plus a per-face offset of up to 0.05, so the chart stays inside
    [-0.8, 0.8]^2 and two faces that share a vertex give it different coordinates, as at a seam.  Deterministic per seed."""
    t = np.asarray(template, np.float64)
    f = np.asarray(faces, np.int64)
    lo, hi = t[:, :2].min(0), t[:, :2].max(0)
    uv = ((t[:, :2] - lo) / np.maximum(hi - lo, 1e-12) * 2 - 1) * 0.75 * np.array([1.0, -1.0])
    offset = np.random.RandomState(seed).uniform(-0.05, 0.05, (f.shape[0], 1, 2))
    return torch.from_numpy((uv[f] + offset).astype(np.float32))


class ShadedFlameConditionRenderer(render.FlameConditionRenderer):
    """callable flame_batch [N, >=236] -> (rend_flm, norma_map_img), both [N,3,h,w] in [-1,1]: render.FlameConditionRenderer's
    contract (it drops into InterpolatedTextureLoss(render_condition=...) and GifTrainer(texture_loss=...)) with the texture
    render GIF conditions on.  Label columns: 0:159 as there (shape, expression, pose, camera); 159:209 the texture code ->
    texture_model.decode; 209:236 the light code -> [N,9,3].  shared_appearance=True uses row 0's texture and light code for the
    whole batch (loss_functions/losses.py:200-207): one albedo is decoded and shaded for every sample.  `face_uvs` [F,3,2]: grid
    coordinates of every face corner in the texture."""

    def __init__(self, flame, faces, face_uvs, texture_model, h=256, w=256, straight_through=False, shared_appearance=False):
        super().__init__(flame, faces, None, h, w, straight_through)
        self.face_uvs, self.texture_model, self.shared_appearance = face_uvs, texture_model, shared_appearance

    def appearance(self, flame_batch):
        """(albedo [1 or N,3,T,T], sh_coeff [N,9,3]) of a label batch."""
        N = flame_batch.shape[0]
        tex_code, light = flame_batch[:, 159:209], flame_batch[:, 209:236]
        if self.shared_appearance:
            tex_code, light = tex_code[:1], light[:1].expand(N, -1)
        return self.texture_model.decode(tex_code), light.reshape(N, 9, 3)

    def __call__(self, flame_batch):
        if flame_batch.ndimension() != 2 or flame_batch.shape[1] < N_LABEL_COLUMNS:
            raise ValueError(f"flame_batch must be [N, >={N_LABEL_COLUMNS}] (texture code 159:209, light code 209:236), "
                             f"got {list(flame_batch.shape)}")
        _, v_ndc, _ = self.vertices(flame_batch)
        albedo, sh_coeff = self.appearance(flame_batch)
        cond = render_shaded_condition(v_ndc, self.faces, self.face_uvs, albedo, sh_coeff, self.h, self.w,
                                       straight_through=self.straight_through)
        return cond[:, :3], cond[:, 3:]
