"""The gradient oracle of the differentiable SMPL layer: torch autograd through oracle.tepose_ref's batch_rodrigues -> lbs ->
smpl_joints49 on the CPU, fp64 by default.  The same helper in fp32 is the yardstick for what fp32 arithmetic alone costs.  Plain torch; no GPU.

tests/test_smpl_bwd_host.py pins this helper against central finite differences of the fp64 forward; tests/test_gpu_smpl_bwd.py holds the HIP backward
to it."""
import functools

import numpy as np
import torch

from oracle import tepose_ref as O
from tepose_amd import synth


@functools.lru_cache(maxsize=4)
def tables(skin_nnz=4, seed=0):
    return synth.synthetic_smpl(seed, skin_nnz=skin_nnz)


def forward(smpl_t, pose, betas, pose2rot):
    """pose [N,72] axis-angle (pose2rot) or [N,24,3,3]; betas [N,10] -> verts [N,6890,3], joints [N,49,3] in the dtype of the inputs."""
    N = betas.shape[0]
    R = O.batch_rodrigues(pose.reshape(-1, 3)).view(N, 24, 3, 3) if pose2rot else pose.reshape(N, 24, 3, 3)
    verts, posed = O.lbs(smpl_t, betas, R)
    return verts, O.smpl_joints49(smpl_t, verts, posed)


def grads(smpl_np, pose, betas, pose2rot, g_verts=None, g_joints=None, dtype=torch.float64):
    """d<g_verts, verts> + <g_joints, joints> / d(pose, betas) by autograd in `dtype` on the CPU.  Arguments: numpy arrays or tensors (any float
    dtype; None for a gradient-in = zeros).  Returns (g_pose shaped like pose, g_betas [N,10]) as `dtype` tensors."""
    cv = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype).clone()
    smpl_t = O.smpl_tensors(smpl_np, dtype)
    pose_t, betas_t = cv(pose).requires_grad_(True), cv(betas).requires_grad_(True)
    verts, joints = forward(smpl_t, pose_t, betas_t, pose2rot)
    outs, gouts = [], []
    if g_verts is not None:
        outs.append(verts); gouts.append(cv(g_verts))
    if g_joints is not None:
        outs.append(joints); gouts.append(cv(g_joints))
    g_pose, g_betas = torch.autograd.grad(outs, [pose_t, betas_t], gouts)
    return g_pose.detach(), g_betas.detach()


def rel_err(got, ref):
    """max|got - ref| / max|ref|: the figure the fp32 budget (1e-4) is stated in."""
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    return float((got - ref).abs().max() / ref.abs().max())
