"""FLAME landmarks in plain torch, dtype-generic — a helper module, not a test.

Written from the definition (include/gif_hip.h; smplx lbs.vertices2landmarks / find_dynamic_lmk_idx_and_bcoords), NOT from the
kernels: a landmark is sum_i bary_i * verts[vid_i]; the dynamic contour landmarks take one row of a table of R = 2M + 1 rows,
chosen from the yaw of the world rotation of one joint, and that rotation is formed here as the product of the joints' rotations
along the kinematic chain (no skinning transforms involved).  In float64 it is the reference of tests/test_gpu_flame_landmarks.py and
tests/test_flame_landmarks_cpu.py; in float32 on the CPU their error yardstick; in float32 on the device the arm
tools/landmark_bench.py compares the kernels against.
"""
import math

import torch

import flame_ref


def tables(emb, dtype, device="cpu"):
    """The embedding's arrays as the layer sees them (weights rounded to float32 once) in `dtype`; ids as int64."""
    w = lambda a: torch.from_numpy(a).float().to(device=device, dtype=dtype)
    i = lambda a: torch.from_numpy(a).long().to(device)
    return {"static_vid": i(emb.static_vid), "static_bary": w(emb.static_bary), "dynamic_vid": i(emb.dynamic_vid),
            "dynamic_bary": w(emb.dynamic_bary), "full_vid": i(emb.full_vid), "full_bary": w(emb.full_bary),
            "yaw_joint": emb.yaw_joint}


def world_rotation(R, parents, joint):
    """R [B,J,3,3] local rotations -> the world rotation of `joint`: the product along the chain from the root down to it."""
    chain = []
    while joint >= 0:
        chain.append(joint)
        joint = parents[joint]
    Rw = R[:, chain[-1]]
    for j in reversed(chain[:-1]):
        Rw = torch.bmm(Rw, R[:, j])
    return Rw


def yaw_degrees(Rw):
    return -torch.atan2(-Rw[:, 2, 0], torch.sqrt(Rw[:, 0, 0] ** 2 + Rw[:, 1, 0] ** 2)) * (180.0 / math.pi)


def select_row(yaw_deg, M):
    """yaw in degrees [B] -> row [B] (int64) of a table of 2M + 1 rows: 0..M for yaw >= 0, M+1..2M for -1..-M."""
    y = torch.round(torch.clamp(yaw_deg, max=float(M)))  # torch.round: half to even
    row = torch.where(y >= 0, y, torch.where(y < -M, torch.full_like(y, 2.0 * M), M - y))
    return torch.where(torch.isfinite(yaw_deg), row, torch.zeros_like(row)).long()


def gather(verts, vid, bary):
    """verts [B,V,3]; vid, bary [L,3] (shared) or [B,L,3] (per sample) -> landmarks [B,L,3]."""
    if vid.dim() == 2:
        corners = verts[:, vid]  # [B,L,3 corners,3]
        return (corners * bary[None, :, :, None]).sum(2)
    b = torch.arange(verts.shape[0], device=verts.device)[:, None, None]
    return (verts[b, vid] * bary[:, :, :, None]).sum(2)


def landmarks_of(t, verts, Rw):
    """t: tables(); verts [B,V,3]; Rw [B,3,3] the yaw joint's world rotation -> (landmarks2d, landmarks3d, row)."""
    R, Ld = t["dynamic_vid"].shape[:2]
    B = verts.shape[0]
    if Ld > 0:
        row = select_row(yaw_degrees(Rw), (R - 1) // 2)
        dyn = gather(verts, t["dynamic_vid"][row], t["dynamic_bary"][row])
    else:
        row = torch.zeros(B, dtype=torch.long, device=verts.device)
        dyn = verts.new_zeros(B, 0, 3)
    l2d = torch.cat([dyn, gather(verts, t["static_vid"], t["static_bary"])], 1)
    return l2d, gather(verts, t["full_vid"], t["full_bary"]), row


def neck_rotation(c, pose_params, neck_pose, eye_pose, yaw_joint):
    B, J = pose_params.shape[0], len(c["parents"])
    R = flame_ref.rodrigues(flame_ref.full_pose(pose_params, neck_pose, eye_pose, J).reshape(B * J, 3)).view(B, J, 3, 3)
    return world_rotation(R, c["parents"], yaw_joint)


def flame_landmarks(c, t, shape_params, expression_params, pose_params, neck_pose, eye_pose):
    """c: flame_ref.constants(); t: tables(); parameters [B,.] -> (vertices, landmarks2d, landmarks3d, row)."""
    verts = flame_ref.flame_vertices(c, shape_params, expression_params, pose_params, neck_pose, eye_pose)
    Rw = neck_rotation(c, pose_params, neck_pose, eye_pose, t["yaw_joint"])
    return (verts,) + landmarks_of(t, verts, Rw)
