"""The part of tests/flame_ref.py in front of the skinning, on its own and dtype-generic — a helper module, not a test.

flame_ref.flame_vertices does not hand out the chain's transforms, so its lines for them are restated here (4x4 products, the
homogeneous joint with w = 0), with flame_ref's own rodrigues and full_pose; tests/test_flame_chain_cpu.py checks that skinning with
these transforms reproduces flame_ref.flame_vertices.  In float64 it is the reference of the pose-chain backward
(gif_pose_chain_bwd_f32, gif_amd/csrc/flame_chain.h); in float32 on the CPU the error yardstick.
"""
import torch

import flame_ref


def chain(joints, r, parents):
    """joints [B,J,3], axis-angles r [B,J,3] -> (A [B,J,12] the relative transforms row-major 3x4, F [B,9(J-1)] the pose feature)."""
    B, J = joints.shape[:2]
    dt, dev = joints.dtype, joints.device
    R = flame_ref.rodrigues(r.reshape(B * J, 3)).view(B, J, 3, 3)
    F = (R[:, 1:] - torch.eye(3, dtype=dt, device=dev)).reshape(B, 9 * (J - 1))
    bottom = torch.tensor([0, 0, 0, 1], dtype=dt, device=dev).expand(B, 1, 4)
    G = []
    for j, p in enumerate(parents):
        rel = joints[:, j] if p < 0 else joints[:, j] - joints[:, p]
        local = torch.cat([torch.cat([R[:, j], rel[:, :, None]], 2), bottom], 1)
        G.append(local if p < 0 else torch.bmm(G[p], local))
    G = torch.stack(G, 1)
    jh = torch.cat([joints, joints.new_zeros(B, J, 1)], 2)[..., None]
    A = G - torch.nn.functional.pad(torch.matmul(G, jh), (3, 0))
    return A[:, :, :3, :].reshape(B, J, 12), F


def joints_step(J0, Jdirs, parents, shape, exp, pose, neck, eye):
    """What gif_flame_joints_f32 computes: J0 [J,3], Jdirs [K,3J], parameters [B,.] -> (coef [B,KP], A [B,J,12])."""
    B, J = pose.shape[0], len(parents)
    betas = torch.cat([shape, exp], 1)
    joints = J0[None] + (betas @ Jdirs).view(B, J, 3)
    A, F = chain(joints, flame_ref.full_pose(pose, neck, eye, J).reshape(B, J, 3), parents)
    return torch.cat([betas, F], 1), A
