"""CPU: the per-sample arithmetic of the pose-chain backward (gif_amd/csrc/flame_chain.h: Rodrigues and its derivative, the world
rotations, the reverse walk), the code gif_pose_chain_bwd_f32 runs on the device, against float64 autograd of the restatement.

tests/host/flame_chain_check.cpp includes only that header.  It is built here host-only under AddressSanitizer and UBSan and run as
a stand-alone program; it prints its inputs and the two gradients (dL/d joints, dL/d axis-angles) for every case, and each case is
recomputed from the printed inputs by tests/flame_chain_ref.py (the lines of tests/flame_ref.py in front of the skinning).
Rule: err <= 4 * err32 + 2^-23, err = relative Frobenius error of a gradient against float64, err32 = the same for
float32 autograd of the restatement on the same inputs.
Cases: J in {1, 3, 5, 8}; the chains (-1,0,1), (-1,0,1,1,1), an 8-joint tree and a forest with two roots; poses of exact zeros, an
angle within 1e-3 of pi, an angle of 1e-6, and one chain with one joint of each.
MEASURED err / err32 (this file prints them with -s): joints 0.39 .. 1.63 (the forest), axis-angles 0.52 .. 1.50 (one joint, zero pose).
"""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flame_chain_ref as cref  # noqa: E402
import flame_ref  # noqa: E402

M_RULE, FLOOR = 4, 2.0 ** -23
WANT = {"j1": (1, (-1,)), "j3_chain": (3, (-1, 0, 1)), "j5_flame": (5, (-1, 0, 1, 1, 1)), "j8": (8, (-1, 0, 1, 1, 1, 0, 5, 2)),
        "j5_forest": (5, (-1, 0, -1, 2, 2)), "j1_zero": (1, (-1,)), "j3_zero": (3, (-1, 0, 1)), "j5_zero": (5, (-1, 0, 1, 1, 1)),
        "j3_near_pi": (3, (-1, 0, 1)), "j5_near_pi": (5, (-1, 0, 1, 1, 1)), "j3_tiny": (3, (-1, 0, 1)), "j5_tiny": (5, (-1, 0, 1, 1, 1)),
        "j5_mixed": (5, (-1, 0, 1, 1, 1)), "j8_mixed": (8, (-1, 0, 1, 1, 1, 0, 5, 2))}


def _floats(words):
    return np.array([struct.unpack("<f", struct.pack("<I", int(w, 16)))[0] for w in words], np.float32)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flame_chain") / "flame_chain_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "flame_chain_check.cpp"),
                                     "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # (either sanitizer ends the program with an error status)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    out, cur = {}, None
    for line in ran.stdout.splitlines():
        m = re.match(r"case (\w+) J=(\d+) parents=([-0-9,]+)$", line)
        if m:
            cur = out.setdefault(m.group(1), {"J": int(m.group(2)), "parents": tuple(int(p) for p in m.group(3).split(","))})
            continue
        key, *words = line.split()
        cur[key] = _floats(words)
    return out


def _reference(c, dtype):
    """(g_jt, g_r) by autograd of the restatement in `dtype` on the printed inputs."""
    J = c["J"]
    t = lambda a, *shape: torch.from_numpy(a).to(dtype).reshape(*shape)
    jt, r = t(c["jt"], 1, J, 3).requires_grad_(True), t(c["r"], 1, J, 3).requires_grad_(True)
    A, F = cref.chain(jt, r, c["parents"])
    loss = (A * t(c["gA"], 1, J, 12)).sum() + (F * t(c["gF"], 1, 9 * (J - 1))).sum()
    return [g.reshape(-1) for g in torch.autograd.grad(loss, [jt, r])]


def _rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def test_the_list_of_cases_is_the_one_asked_for(cases):
    assert {k: (c["J"], c["parents"]) for k, c in cases.items()} == WANT
    for name, c in cases.items():
        J = c["J"]
        assert [len(c[k]) for k in ("jt", "r", "gA", "gF", "gjt", "gr")] == [3 * J, 3 * J, 12 * J, 9 * (J - 1), 3 * J, 3 * J], name
        angles = np.linalg.norm(c["r"].reshape(J, 3).astype(np.float64), axis=1)
        if name.endswith("_zero"):
            assert (c["r"] == 0).all()
        if name.endswith("_near_pi"):
            assert (np.abs(angles - np.pi) < 1e-3).all() and (angles < np.pi).all()
        if name.endswith("_tiny"):
            assert np.allclose(angles, 1e-6, rtol=1e-3)
        if name.endswith("_mixed"):
            assert angles[0] == 0 and abs(angles[1] - np.pi) < 1e-3 and abs(angles[2] - 1e-6) < 1e-9


@pytest.mark.parametrize("name", list(WANT))
def test_gradients_match_float64_autograd(cases, name):
    c = cases[name]
    ref, ref32 = _reference(c, torch.float64), _reference(c, torch.float32)
    msgs, bad = [], []
    for label, got, want, w32 in (("joints", c["gjt"], ref[0], ref32[0]), ("axis-angles", c["gr"], ref[1], ref32[1])):
        got = torch.from_numpy(got)
        assert torch.isfinite(got).all(), label
        if want.norm().item() == 0:  # (every R = I: each A is the identity wherever the joints are)
            assert name.endswith("_zero") and label == "joints" and w32.abs().max().item() == 0 and got.abs().max().item() == 0
            continue
        e, e32 = _rel(got, want), _rel(w32, want)
        msgs.append(f"{label} {e:.2e} (err32 {e32:.2e}, x{e / max(e32, 1e-30):.2f})")
        if not e <= M_RULE * e32 + FLOOR:
            bad.append(f"{label}: {e:.3e} > {M_RULE * e32 + FLOOR:.3e}")
    print(f"\n[flame chain host] {name}: " + "  ".join(msgs))
    assert not bad, "; ".join(bad)


def test_zero_pose_gives_the_finite_gradient_autograd_gives(cases):
    """r = 0: R = I up to 1e-16, and dL/dr is the antisymmetric part of dL/dR, read off the inputs without any formula of the header."""
    c = cases["j1_zero"]
    g = c["gA"].astype(np.float64).reshape(3, 4)
    gR = g[:, :3] - np.outer(g[:, 3], c["jt"].astype(np.float64))
    want = np.array([gR[2, 1] - gR[1, 2], gR[0, 2] - gR[2, 0], gR[1, 0] - gR[0, 1]])
    assert np.abs(c["gr"] - want).max() <= 1e-6 * np.abs(want).max()


def test_the_restated_chain_is_flame_refs():
    """Skinning with flame_chain_ref's transforms gives flame_ref.flame_vertices: the helper restates the reference, nothing else."""
    from gif_amd import flame as fl
    rng = np.random.RandomState(0)
    for parents in ((-1,), (-1, 0, 1), (-1, 0, 1, 1, 1), (-1, 0, 1, 1, 1, 0, 5, 2)):
        model = fl.synthetic_flame_model(rng.randn(19, 3) * 0.1, 4, 3, seed=1, parents=parents)
        c = flame_ref.constants(model, 4, 3, torch.float64)
        g = torch.Generator().manual_seed(len(parents))
        x = [torch.randn(2, n, generator=g, dtype=torch.float64) * s for n, s in ((4, 1.0), (3, 1.0), (6, 0.3), (3, 0.3), (6, 0.3))]
        want = flame_ref.flame_vertices(c, *x)
        J = len(parents)
        joints = flame_ref.flame_vertices(c, *x, return_joints=True)
        A, F = cref.chain(joints, flame_ref.full_pose(x[2], x[3], x[4], J).reshape(2, J, 3), parents)
        v_posed = flame_ref.shaped(c, torch.cat(x[:2], 1)) + (F @ c["posedirs"]).view(2, -1, 3)
        T = torch.einsum("vj,bjrc->bvrc", c["lbs_weights"], A.view(2, J, 3, 4))
        got = torch.einsum("bvrc,bvc->bvr", T, torch.cat([v_posed, v_posed.new_ones(2, v_posed.shape[1], 1)], 2))
        assert (got - want).abs().max().item() <= 1e-12
        # and the joints in the kernels' form, J0 + betas . Jdirs
        _, _, J0, Jdirs = fl.joint_basis(model, 4, 3)
        coef, A2 = cref.joints_step(torch.from_numpy(J0), torch.from_numpy(Jdirs), parents, *x)
        assert (A2 - A).abs().max().item() <= 1e-12 and torch.equal(coef[:, :7], torch.cat(x[:2], 1))
