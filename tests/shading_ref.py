"""The shaded condition's shading step in plain torch, dtype-generic — a helper module, not a test.

Written from the definition in include/gif_hip.h (second-order spherical-harmonics irradiance, Ramamoorthi & Hanrahan 2001, times
a bilinear albedo sample), NOT from the kernels: F.grid_sample does the sampling, one einsum the nine-term sum.  In float64 it is
the reference of tests/test_gpu_shading.py and tests/test_shading_cpu.py; in float32 on the CPU it is their error yardstick; in
float32 on the device it is the arm tools/shade_bench.py compares gif_amd.shading.sh_shade against.
"""
import math

import torch
import torch.nn.functional as F

# k_i = A_l * Y_lm with A = (1, 2 pi / 3, pi / 4): the table DECA's light codes are written for (band 0 carries no factor pi)
SH_K = (1 / math.sqrt(4 * math.pi),
        *([(2 * math.pi / 3) * math.sqrt(3 / (4 * math.pi))] * 3),
        *([(math.pi / 4) * 3 * math.sqrt(5 / (12 * math.pi))] * 3),
        (math.pi / 4) * (3 / 2) * math.sqrt(5 / (12 * math.pi)),
        (math.pi / 4) * (1 / 2) * math.sqrt(5 / (4 * math.pi)))

# (B, Ba, H, W, T) of tests/test_gpu_shading.py
CASES = {
    "one_pixel": (1, 1, 1, 1, 1),
    "5x7_t2": (1, 1, 5, 7, 2),
    "shared_33x65_t3": (3, 1, 33, 65, 3),
    "64x64_t257": (3, 3, 64, 64, 257),
    "16x300_t16": (2, 2, 16, 300, 16),
}


def sh_basis(n):
    """n [...,3] -> k_i * basis_i(n) [...,9], basis = (1, x, y, z, xy, xz, yz, x^2 - y^2, 3 z^2 - 1)."""
    x, y, z = n.unbind(-1)
    basis = torch.stack([torch.ones_like(x), x, y, z, x * y, x * z, y * z, x * x - y * y, 3 * z * z - 1], -1)
    return basis * torch.tensor(SH_K, dtype=n.dtype, device=n.device)


def sh_shade(uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul=1.0, nrm_add=0.0):
    """gif_amd.shading.sh_shade's signature and definition in the operands' dtype: uv_img, normal_img [B,3,H,W], mask [B,1,H,W],
    albedo [1 or B,3,T,T], sh_coeff [B,9,3] -> [B,3,H,W]."""
    B = uv_img.shape[0]
    n = nrm_mul * normal_img + nrm_add
    a = F.grid_sample(albedo.expand(B, -1, -1, -1), uv_img[:, :2].permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros",
                      align_corners=False)
    shading = torch.einsum("bhwi,bic->bchw", sh_basis(n.permute(0, 2, 3, 1)), sh_coeff)
    return torch.where(mask.bool(), a * shading, torch.zeros((), dtype=a.dtype, device=a.device))


def sh_shade_in(dtype):
    """sh_shade computed in `dtype` behind casts (float32 operands in, float32 out): drops into gif_amd.shading.sh_shade's place."""
    def fn(uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul=1.0, nrm_add=0.0):
        return sh_shade(uv_img.to(dtype), normal_img.to(dtype), mask, albedo.to(dtype), sh_coeff.to(dtype), nrm_mul,
                        nrm_add).to(uv_img.dtype)
    return fn


def make_case(B, Ba, H, W, T, seed=0):
    """Inputs of one case, float32 on the CPU, from a seeded generator: (uv, nrm, mask, albedo, sh, upstream gradient, cells).
    Texel position = an integer in [-1, T-1] plus a fraction in [0.05, 0.95] — taps outside on both sides, and float32 and
    float64 agree on the cell (`cells` [B,2,H,W], what tests/test_shading_cpu.py checks) — converted to grid coordinates in
    float64 and rounded to float32; normals of length 0.8 .. 1.2; about 70 % coverage, pixel (0, 0) always covered; sh[:, 0] += 2.5."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 5 * Ba + 3 * H + 2 * W + T)
    cells = torch.randint(-1, T, (B, 2, H, W), generator=g)
    pos = cells.double() + 0.05 + 0.9 * torch.rand(B, 2, H, W, generator=g, dtype=torch.float64)
    uv = torch.cat([((2 * pos + 1) / T - 1).float(), torch.zeros(B, 1, H, W)], 1)
    d = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    nrm = (d / d.norm(dim=1, keepdim=True) * (0.8 + 0.4 * torch.rand(B, 1, H, W, generator=g, dtype=torch.float64))).float()
    mask = torch.rand(B, 1, H, W, generator=g) < 0.7
    mask[:, :, 0, 0] = True  # (every sample covers a pixel, the one-pixel case included)
    albedo = torch.rand(Ba, 3, T, T, generator=g)
    sh = torch.randn(B, 9, 3, generator=g)
    sh[:, 0] += 2.5
    up = torch.randn(B, 3, H, W, generator=g)
    return uv, nrm, mask, albedo, sh, up, cells


def texel_cells(uv, T, dtype):
    """floor of grid_sample's texel position ((g + 1) T - 1) / 2, evaluated in `dtype` from the float32 coordinates."""
    return torch.floor(((uv[:, :2].to(dtype) + 1) * T - 1) / 2).long()
