"""Autograd through the standalone SMPL layer: forward = Engine.smpl_fwd, backward = Engine.smpl_bwd (tepose_smpl_bwd, csrc/smpl_bwd.hip; DESIGN.md
section 19).  Recorded by SMPL.forward only when a tensor the caller passed requires grad."""
import torch
from torch.autograd.function import once_differentiable


class SmplFunction(torch.autograd.Function):
    """(eng, pose2rot, full [N,72] | [N,24,3,3], betas [N,10]) -> (verts [N,6890,3], joints [N,49,3]); fp32, contiguous, on the engine's device.

    The backward is stateless on the library's side: it is handed (full, betas) again and recomputes what it needs, so nothing but the two small
    inputs is saved.  It receives whichever of the two output gradients exist (the other travels as NULL) and computes only the input gradients
    that are needed.  Its workspace is the engine's own growable one, unless the forward ran inside Engine.use_workspace(ws): then the backward
    runs in that same caller-owned tensor (it must hold Engine.smpl_bwd_workspace_bytes(N); too small raises) -- what a captured graph needs, whose
    kernels keep the workspace address.  Double backward is not supported: differentiating the backward raises (once_differentiable)."""

    @staticmethod
    def forward(ctx, eng, pose2rot, full, betas):
        ctx.eng, ctx.pose2rot = eng, bool(pose2rot)
        ctx.ws = eng._ws_private          # a caller-owned workspace (Engine.use_workspace) pins the backward too, wherever backward() is called from
        if ctx.ws is not None and ctx.ws.numel() < eng.smpl_bwd_workspace_bytes(full.shape[0]):      # say so now, not when backward() runs
            raise RuntimeError('the caller-owned workspace (%d bytes) is too small for the SMPL backward of %d persons (%d bytes)'
                               % (ctx.ws.numel(), full.shape[0], eng.smpl_bwd_workspace_bytes(full.shape[0])))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(full, betas)
        return eng.smpl_fwd(full, betas, pose2rot)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_verts, g_joints):
        full, betas = ctx.saved_tensors
        want_pose, want_betas = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if (g_verts is None and g_joints is None) or not (want_pose or want_betas):
            return None, None, None, None
        g_verts = None if g_verts is None else g_verts.to(torch.float32).contiguous()
        g_joints = None if g_joints is None else g_joints.to(torch.float32).contiguous()
        with torch.cuda.device(full.device):
            g_pose, g_betas = ctx.eng.smpl_bwd(full, betas, ctx.pose2rot, g_verts, g_joints, want_pose, want_betas, ws=ctx.ws)
        return None, None, g_pose, g_betas
