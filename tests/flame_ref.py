"""The FLAME layer's algorithm in plain torch, dtype-generic — a helper module, not a test.

Written from the published description (blend shapes, joint regression over the shaped vertices, Rodrigues in the smplx form,
pose correctives, a kinematic chain of 4x4 products, skinning as one einsum), NOT from the kernels' factorisation: no
precomputed joint basis, no 3x4 shortcuts, no k-major layout.  In float64 it is the reference of tests/test_gpu_flame.py and
tests/test_flame_cpu.py; in float32 on the CPU it is their error yardstick; in float32 on the device it is the arm
tools/flame_bench.py compares the layer against.
"""
import torch


def constants(model, n_shape, n_exp, dtype, device="cpu"):
    """The model's arrays as the layer sees them (rounded to float32 once, the selected blend-shape columns) in `dtype`."""
    t = lambda a: torch.from_numpy(a).float().to(device=device, dtype=dtype)
    sd = t(model.shapedirs)
    return {"v_template": t(model.v_template),
            "shapedirs": torch.cat([sd[:, :, :n_shape], sd[:, :, model.n_shape:model.n_shape + n_exp]], 2),
            "posedirs": t(model.posedirs), "J_regressor": t(model.J_regressor), "lbs_weights": t(model.lbs_weights),
            "parents": [int(p) for p in model.parents]}


def rodrigues(r):
    angle = torch.norm(r + 1e-8, dim=1, keepdim=True)
    d = r / angle
    K = torch.zeros(r.shape[0], 3, 3, dtype=r.dtype, device=r.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -d[:, 2], d[:, 1], d[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -d[:, 0], -d[:, 1], d[:, 0]
    ident = torch.eye(3, dtype=r.dtype, device=r.device)[None]
    return ident + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * torch.bmm(K, K)


def full_pose(pose_params, neck_pose, eye_pose, J):
    """cat(global, neck, jaw, eyes) [B,15], cut or zero-padded to the model's 3 J entries."""
    full = torch.cat([pose_params[:, :3], neck_pose, pose_params[:, 3:6], eye_pose], 1)
    if J > 5:
        full = torch.cat([full, full.new_zeros(full.shape[0], 3 * (J - 5))], 1)
    return full[:, :3 * J]


def shaped(c, betas):
    return c["v_template"][None] + torch.einsum("vik,bk->bvi", c["shapedirs"], betas)


def flame_vertices(c, shape_params, expression_params, pose_params, neck_pose, eye_pose, return_joints=False):
    """c: constants(); parameters [B,.] in c's dtype -> vertices [B,V,3]."""
    B, J = shape_params.shape[0], len(c["parents"])
    dt, dev = shape_params.dtype, shape_params.device
    betas = torch.cat([shape_params, expression_params], 1)
    v_shaped = shaped(c, betas)
    joints = torch.einsum("jv,bvi->bji", c["J_regressor"], v_shaped)
    if return_joints:
        return joints
    R = rodrigues(full_pose(pose_params, neck_pose, eye_pose, J).reshape(B * J, 3)).view(B, J, 3, 3)
    pose_feature = (R[:, 1:] - torch.eye(3, dtype=dt, device=dev)).reshape(B, 9 * (J - 1))  # (no -1: B may be 0)
    v_posed = v_shaped + (pose_feature @ c["posedirs"]).view(B, v_shaped.shape[1], 3)
    bottom = torch.tensor([0, 0, 0, 1], dtype=dt, device=dev).expand(B, 1, 4)
    G = []
    for j, p in enumerate(c["parents"]):
        rel = joints[:, j] if p < 0 else joints[:, j] - joints[:, p]
        local = torch.cat([torch.cat([R[:, j], rel[:, :, None]], 2), bottom], 1)  # [B,4,4]
        G.append(local if p < 0 else torch.bmm(G[p], local))
    G = torch.stack(G, 1)  # [B,J,4,4]
    jh = torch.cat([joints, joints.new_zeros(B, J, 1)], 2)[..., None]  # homogeneous with w = 0: G . [j, 0] = G.R j
    A = G - torch.nn.functional.pad(torch.matmul(G, jh), (3, 0))
    T = torch.einsum("vj,bjrc->bvrc", c["lbs_weights"], A)
    vh = torch.cat([v_posed, v_posed.new_ones(B, v_posed.shape[1], 1)], 2)
    return torch.einsum("bvrc,bvc->bvr", T, vh)[:, :, :3]
