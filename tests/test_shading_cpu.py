"""CPU-side checks of the shaded condition (gif_amd/shading.py, csrc/shade.hip): the entry points' argument validation (it
happens before any launch, so it runs without a GPU), the SH constants of the float64 restatement (tests/shading_ref.py) against an
independent evaluation, the inputs tests/test_gpu_shading.py uses, the texture model's file format and arithmetic, and the
renderer's label slicing."""
import ctypes
import os

import numpy as np
import pytest
import torch

import shading_ref
from gif_amd import _lib
from gif_amd import shading as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_validation_without_gpu():
    lib = _lib.load()
    fwd, bwd, ws = lib.gif_shade_sh_f32, lib.gif_shade_sh_bwd_f32, lib.gif_shade_sh_bwd_workspace_bytes
    one = ctypes.c_void_p(16)  # a non-null pointer the validation never follows
    f = lambda B, Ba, H, W, T, p=None: fwd(p, p, p, p, p, p, B, Ba, H, W, T, 1.0, 0.0, None)
    b = lambda B, Ba, H, W, T, p=None, outs=(None,) * 4, w=None: bwd(p, p, p, p, p, p, *outs, B, Ba, H, W, T, 1.0, 0.0, w, None)
    err = lambda: lib.gif_last_error()
    for call in (f, b):
        for dims in ((-1, 1, 4, 4, 2), (2, 2, -4, 4, 2), (2, 2, 4, -4, 2), (2, 2, 4, 4, -2)):
            assert call(*dims) == -1 and b"bad dims" in err()
        for Ba in (0, 2, 4):
            assert call(3, Ba, 4, 4, 2) == -1 and b"must be 1 or B" in err()
        assert call(2, 1, 32768, 16384, 2) == -1 and b"below 2^31" in err()  # B * 3 * H * W = 3 * 2^30
        # nothing to do: no pointer is looked at
        assert call(0, 1, 4, 4, 2) == 0 and call(0, 0, 4, 4, 2) == 0 and call(2, 2, 0, 4, 2) == 0 and call(2, 1, 4, 0, 2) == 0
    assert f(2, 2, 4, 4, 2) == -1 and b"null pointer" in err()
    assert b(2, 2, 4, 4, 2) == 0  # no output asked for: no work either
    assert b(2, 2, 4, 4, 2, outs=(one, None, None, None)) == -1 and b"null pointer" in err()
    assert b(2, 2, 4, 4, 2, p=one, outs=(None, None, None, one)) == -1 and b"needs the workspace" in err()
    assert b(2, 2, 4, 4, 0, p=one, outs=(None, None, one, None)) == -1 and b"T = 0" in err()
    assert b(0, 0, 4, 4, 0, outs=(None, None, one, None)) == -1 and b"T = 0" in err()
    # the workspace: positive, and it does not shrink when B, H or W grows
    assert ws(0, 4, 4) == 0 and ws(2, 0, 4) == 0 and ws(-1, 4, 4) == 0
    assert ws(1, 1, 1) > 0
    sizes = [1, 2, 3, 16, 31, 32, 33, 255, 256, 257, 1024]
    for fixed in ((1, 1), (3, 65), (32, 256)):
        for k in range(3):
            got = [ws(*(fixed[:k] + (n,) + fixed[k:])) for n in sizes]
            assert all(x > 0 for x in got) and got == sorted(got), (fixed, k, got)
    # one partial row of 27 floats per 1024 pixels of a sample, and room for the fixed-order sum's intermediate rows
    assert ws(32, 256, 256) >= 32 * 64 * 27 * 4


def real_sh(theta, phi):
    """The nine real spherical harmonics up to l = 2 from the angles (colatitude theta, azimuth phi), in the order of the
    kernel's basis: Y00; Y1 (x, y, z) = (m = 1, -1, 0); Y2 (xy, xz, yz, x^2 - y^2, 3z^2 - 1) = (m = -2, 1, -1, 2, 0)."""
    s, c, pi = np.sin(theta), np.cos(theta), np.pi
    y1 = np.sqrt(3 / (4 * pi))
    return np.stack([np.full_like(theta, 0.5 * np.sqrt(1 / pi)),
                     y1 * s * np.cos(phi), y1 * s * np.sin(phi), y1 * c,
                     0.25 * np.sqrt(15 / pi) * s * s * np.sin(2 * phi),
                     0.5 * np.sqrt(15 / pi) * s * c * np.cos(phi),
                     0.5 * np.sqrt(15 / pi) * s * c * np.sin(phi),
                     0.25 * np.sqrt(15 / pi) * s * s * np.cos(2 * phi),
                     0.25 * np.sqrt(5 / pi) * (3 * c * c - 1)], -1)


def test_basis_constants_against_spherical_harmonics():
    """k_i * basis_i(n) = A_l * Y_lm(n) on unit normals: the harmonics evaluated from the angles, the restatement from the
    Cartesian polynomials.  A = (1, 2 pi / 3, pi / 4): the constants as the definition lists them (DECA's table) — k_0 =
    1 / sqrt(4 pi) is Y_00 itself, the irradiance kernel's band-0 factor pi is left to the light code."""
    rng = np.random.RandomState(0)
    theta, phi = np.arccos(rng.uniform(-1, 1, 1000)), rng.uniform(0, 2 * np.pi, 1000)
    n = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    A = np.array([1.0] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5)
    got = shading_ref.sh_basis(torch.from_numpy(n)).numpy()
    assert got.dtype == np.float64 and np.abs(got - A * real_sh(theta, phi)).max() <= 1e-12


@pytest.mark.parametrize("name", list(shading_ref.CASES))
def test_gpu_case_inputs(name):
    """The inputs of tests/test_gpu_shading.py: float32 and float64 put every coordinate into the cell it was drawn for, the cells
    reach outside the texture on both sides, the fractions keep 0.05 from a cell border, the normals' lengths and the coverage."""
    B, Ba, H, W, T = shading_ref.CASES[name]
    uv, nrm, mask, albedo, sh, up, cells = shading_ref.make_case(B, Ba, H, W, T)
    assert uv.dtype == torch.float32 and uv.shape == (B, 3, H, W) and albedo.shape == (Ba, 3, T, T) and sh.shape == (B, 9, 3)
    assert torch.equal(shading_ref.texel_cells(uv, T, torch.float32), cells)
    assert torch.equal(shading_ref.texel_cells(uv, T, torch.float64), cells)
    frac = ((uv[:, :2].double() + 1) * T - 1) / 2 - cells
    assert frac.min().item() >= 0.05 - 1e-4 and frac.max().item() <= 0.95 + 1e-4
    assert cells.min().item() >= -1 and cells.max().item() <= T - 1
    if B * H * W >= 35:
        assert cells.min().item() == -1 and cells.max().item() == T - 1  # taps outside on both sides
        assert 0.5 < mask.float().mean().item() < 0.9
    length = nrm.double().norm(dim=1)
    assert length.min().item() >= 0.8 - 1e-6 and length.max().item() <= 1.2 + 1e-6
    assert mask.dtype == torch.bool and mask[:, :, 0, 0].all()


def test_texture_model_npz_round_trip_and_shape_checks(tmp_path):
    m = sd.synthetic_texture_model(8, 5, seed=3)
    assert m.mean.shape == (3, 8, 8) and m.basis.shape == (5, 3, 8, 8) and (m.size, m.n_tex) == (8, 5)
    assert 0.3 - 1e-6 <= m.mean.min() and m.mean.max() <= 0.7 + 1e-6 and np.abs(m.basis).max() <= 0.02 + 1e-7
    same, other = sd.synthetic_texture_model(8, 5, seed=3), sd.synthetic_texture_model(8, 5, seed=4)
    assert np.array_equal(m.basis, same.basis) and not np.array_equal(m.basis, other.basis)
    path = str(tmp_path / "texture.npz")
    m.save_npz(path)
    r = sd.FlameTextureModel.from_npz(path)
    for k in sd.FlameTextureModel.KEYS:
        assert np.array_equal(getattr(m, k), getattr(r, k)), k
    with pytest.raises(ValueError, match="mean"):
        sd.FlameTextureModel(m.mean[:, :, :7], m.basis)
    with pytest.raises(ValueError, match="mean"):
        sd.FlameTextureModel(m.mean[:2], m.basis)
    with pytest.raises(ValueError, match="basis"):
        sd.FlameTextureModel(m.mean, m.basis[:, :, :7])
    with pytest.raises(ValueError, match="basis"):
        sd.FlameTextureModel(m.mean, m.basis[0])
    np.savez(path, mean=m.mean)
    with pytest.raises(ValueError, match="missing keys"):
        sd.FlameTextureModel.from_npz(path)
    with pytest.raises(ValueError, match="tex_code"):
        m.decode(torch.zeros(2, 4))


def test_texture_decode_against_numpy():
    m = sd.synthetic_texture_model(8, 5, seed=1)
    code = torch.randn(3, 5, generator=torch.Generator().manual_seed(0))
    got = m.decode(code)
    want = m.mean.astype(np.float64)[None] + np.einsum("bk,kcyx->bcyx", code.double().numpy(), m.basis.astype(np.float64))
    assert got.shape == (3, 3, 8, 8) and got.dtype == torch.float32
    # five products of magnitude <= 0.02 * 4 and a mean below 1, each rounded to float32
    assert np.abs(got.numpy() - want).max() <= 8 * 2.0 ** -24
    code.requires_grad_(True)
    m.decode(code).sum().backward()
    assert np.allclose(code.grad.numpy(), np.broadcast_to(m.basis.astype(np.float64).sum((1, 2, 3)), (3, 5)), rtol=1e-5, atol=1e-6)


def test_synthetic_face_uvs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    v, f = g["vertices"].astype(np.float64) * 0.1, g["faces"].astype(np.int64)
    uv = sd.synthetic_face_uvs(v, f, seed=2)
    assert uv.shape == (f.shape[0], 3, 2) and uv.dtype == torch.float32
    assert uv.abs().max().item() <= 0.8
    assert torch.equal(uv, sd.synthetic_face_uvs(v, f, seed=2)) and not torch.equal(uv, sd.synthetic_face_uvs(v, f, seed=3))
    # seams: two faces that share a vertex give it different coordinates; inside a face the chart is the planar one
    f0 = f[0]
    other = next(k for k in range(1, f.shape[0]) if f0[0] in f[k])
    assert not torch.equal(uv[0, 0], uv[other, list(f[other]).index(f0[0])])
    span = (v[:, :2].max(0) - v[:, :2].min(0))
    want = (v[f0[1], :2] - v[f0[0], :2]) / span * 1.5 * np.array([1.0, -1.0])
    assert np.allclose((uv[0, 1] - uv[0, 0]).numpy(), want, atol=1e-6)


class _StubFlame:
    def __call__(self, shape_params, expression_params, pose_params):
        self.seen = (shape_params, expression_params, pose_params)
        return torch.zeros(shape_params.shape[0], 4, 3) + shape_params[:, :1, None], None, None


def test_renderer_slices_the_labels(monkeypatch):
    """Columns 159:209 go through texture_model.decode, 209:236 become [N,9,3]; shared_appearance takes both from row 0 and hands
    ONE albedo to the shading.  The rasteriser passes and sh_shade are stubs here (they need the device)."""
    from gif_amd import render
    seen = {}

    def stub_shade(uv_img, normal_img, mask, albedo, sh_coeff, nrm_mul=1.0, nrm_add=0.0):
        seen.update(albedo=albedo, sh=sh_coeff, scale=(nrm_mul, nrm_add))
        return sh_coeff[:, 0, :, None, None].expand(-1, -1, 4, 4) * 0.1

    img = lambda v: (torch.full((v.shape[0], 3, 4, 4), 0.5), torch.ones(v.shape[0], 1, 4, 4, dtype=torch.bool))
    monkeypatch.setattr(render, "vertex_normals", lambda v, f: torch.zeros_like(v))
    monkeypatch.setattr(render, "rasterize_attributes", lambda v, f, a, h, w: img(v))
    monkeypatch.setattr(sd, "rasterize_face_attributes", lambda v, f, a, h, w: img(v))
    monkeypatch.setattr(sd, "sh_shade", stub_shade)
    model = sd.synthetic_texture_model(4, 50, seed=0)
    faces = torch.tensor([[0, 1, 2], [1, 2, 3]])
    uvs = torch.zeros(2, 3, 2)
    fb = torch.randn(3, 240, generator=torch.Generator().manual_seed(0))
    flame = _StubFlame()
    rend, nrm = sd.ShadedFlameConditionRenderer(flame, faces, uvs, model, 4, 4)(fb)
    assert rend.shape == (3, 3, 4, 4) and nrm.shape == (3, 3, 4, 4)
    assert torch.equal(flame.seen[0], fb[:, 0:100]) and torch.equal(flame.seen[1], fb[:, 100:150]) and torch.equal(flame.seen[2], fb[:, 150:156])
    assert torch.equal(seen["sh"], fb[:, 209:236].reshape(3, 9, 3)) and seen["scale"] == (2.0, -1.0)
    assert seen["albedo"].shape == (3, 3, 4, 4) and torch.equal(seen["albedo"], model.decode(fb[:, 159:209]))
    # the texture render: clamp, floor quantisation, [-1,1]; the normal render of the 0.5 image
    want = torch.floor((fb[:, 209:212] * 0.1).clamp(0, 1) * 255) / 255 * 2 - 1
    assert torch.equal(rend, want[:, :, None, None].expand(-1, -1, 4, 4))
    assert torch.equal(nrm, torch.floor(torch.full((3, 3, 4, 4), 0.5) * 255) / 255 * 2 - 1)
    sd.ShadedFlameConditionRenderer(flame, faces, uvs, model, 4, 4, shared_appearance=True)(fb)
    assert seen["albedo"].shape == (1, 3, 4, 4) and torch.equal(seen["albedo"], model.decode(fb[:1, 159:209]))
    assert torch.equal(seen["sh"], fb[:1, 209:236].reshape(1, 9, 3).expand(3, -1, -1))
    for bad in (fb[:, :235], fb[:, :159], fb[0]):
        with pytest.raises(ValueError, match="236"):
            sd.ShadedFlameConditionRenderer(flame, faces, uvs, model, 4, 4)(bad)


def test_no_cpu_fallback():
    uv, nrm, mask, albedo, sh, _, _ = shading_ref.make_case(*shading_ref.CASES["5x7_t2"])
    with pytest.raises(_lib.GifHipError):
        sd.sh_shade(uv, nrm, mask, albedo, sh)
    with pytest.raises(_lib.GifHipError):
        sd.rasterize_face_attributes(torch.zeros(1, 4, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 3, 3), 4, 4)
    with pytest.raises(_lib.GifHipError):
        sd.render_shaded_condition(torch.zeros(1, 4, 3), torch.tensor([[0, 1, 2]]), torch.zeros(1, 3, 2), albedo, sh[:1], 4, 4)
