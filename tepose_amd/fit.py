"""Fitting through the differentiable SMPL layer: `fit_keypoints`, the first user of SMPL.forward's autograd.

This is NOT the reference demo's Temporal SMPLify (demo.py:264-293 calls a module that is absent from the reference tree, so nothing here is pinned
to it): no pose prior, no temporal term, no camera initialisation -- one loss, one optimiser."""
import torch

from .spin import projection      # lib/models/spin.py:307-351 with R = I, centre 0: plain torch, differentiable, any device and dtype


def keypoint_loss(pred_2d, kp_2d, conf):
    """The reference's confidence-weighted 2-D reprojection loss, lib/core/loss.py:182-195 with openpose_weight = gt_weight = 1:
    mean over every (person, joint, coordinate) of conf * (pred - gt)^2.  conf [N,J]."""
    return (conf[:, :, None] * (pred_2d - kp_2d) ** 2).mean()


def fit_loop(joints_fn, pose_aa, betas, cam, kp_2d, conf, steps, lr, optimise=('pose', 'betas', 'cam')):
    """The optimisation of fit_keypoints for any differentiable joints_fn(pose_aa [N,72], betas [N,10]) -> joints [N,49,3] (tests run the same loop
    on the fp64 oracle).  Returns (pose_aa, betas, cam, losses): refined copies and the loss before each of the `steps` Adam steps."""
    bad = set(optimise) - {'pose', 'betas', 'cam'}
    if bad or not optimise:
        raise ValueError("optimise must name some of 'pose', 'betas', 'cam', got %r" % (tuple(optimise),))
    par = {'pose': pose_aa.detach().clone(), 'betas': betas.detach().clone(), 'cam': cam.detach().clone()}
    for k in optimise:
        par[k].requires_grad_(True)
    opt = torch.optim.Adam([par[k] for k in ('pose', 'betas', 'cam') if k in optimise], lr=lr)
    losses = []
    for _ in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        loss = keypoint_loss(projection(joints_fn(par['pose'], par['betas']), par['cam']), kp_2d, conf)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return par['pose'].detach(), par['betas'].detach(), par['cam'].detach(), losses


def fit_keypoints(smpl, pose_aa, betas, cam, kp_2d, conf, steps, lr, optimise=('pose', 'betas', 'cam')):
    """Refine SMPL parameters against 2-D keypoints.

    smpl: a tepose_amd.smpl.SMPL; pose_aa [N,72] axis-angle (global orient first), betas [N,10], cam [N,3] weak-perspective (s, tx, ty): the start;
    kp_2d [N,49,2] targets in the normalised image coordinates of `spin.projection`, conf [N,49] their confidences -- all on one cuda device.
    Minimises keypoint_loss (lib/core/loss.py:182-195) of spin.projection (lib/models/spin.py:307-351) of the layer's 49 joints with torch.optim.Adam
    over the parameters named in `optimise`, `steps` steps at learning rate `lr`.  The joints and their gradient come from the HIP library
    (SMPL.forward -> tepose_smpl_fwd / tepose_smpl_bwd); projection and loss are plain torch on the device.
    Returns (pose_aa, betas, cam, losses) -- refined copies (the inputs are not written) and the loss before each step.

    This is not Temporal SMPLify: that module is absent from the reference tree and nothing here is pinned to it (no priors, no temporal term)."""
    def joints_fn(pose, b):
        return smpl(betas=b, body_pose=pose[:, 3:], global_orient=pose[:, :3], pose2rot=True).joints
    return fit_loop(joints_fn, pose_aa, betas, cam, kp_2d, conf, steps, lr, optimise)
