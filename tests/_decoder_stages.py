"""The decoder half stage by stage (plain torch on the CPU): an fp64 restatement of every stage tepose_decoder_tap can copy out of a finished
tepose_regressor_fwd[_init] / tepose_forward / tepose_smpl_fwd, and of the five outputs behind them; the componentwise bound of each; and the checker
tests/test_gpu_decoder_stages.py runs over the taps.  tests/test_decoder_stages_helper.py checks this file on its own (no GPU).  Modelled on
tests/_encoder_stages.py, whose product coefficient (ES.coef) every product here uses.

EVERY STAGE IS JUDGED IN ISOLATION: its fp64 reference is computed from the device's own value of the stage before it (a tap or an output), so a
stage's error is the error of the one kernel (or kernel section) that made it and nothing is propagated from stage to stage.  The tables are the
caller's (tepose_amd.synth / the state dict), never the packed blob: the pack-time constants (J0, JS, the blend table, the collapsed matrices, the CSR
and compact skin tables) are under test with the kernels that read them.

u = 2^-24.  A bound is never tuned on a kernel; each formula below is what the op sequence in csrc/smpl.hip / forward.hip allows.  A NaN anywhere scores
infinity (the GPU test poisons workspace and outputs first).

xs [N][160] = [pose6d 144 | shape 10 | cam 3 | 0 0 0], by how the call made it (Src.how):
    'collapsed'       feat Mf^T + k0.  Mf, k0 are formed HERE in fp64 (the affine map of three iterations evaluated on 0 and the unit vectors).
                      c = coef(2048, width-first split kernel) + u (Mf is stored in fp32 before it is split), A = |feat| |Mf|^T + |k0|.
    'tail_collapsed'  relu-tail Mt^T + kt, Mt = Mf [W_lf | W_lr] / 2, kt = k0 + Mf (b_lf + b_lr) / 2; K = 3 Hp; the tail is the encoder tap's.
    'loop', n_iter 1  h1 = feat W1a^T + b1 + init W1b^T     two products, K = 2048 and 160: coef(2048) (|feat| |W1a|^T + |b1|) + coef(160) (|init| |W1b|^T + |base|)
                      h2 = h1 W2^T + b2                      from the TAPPED h1, K = 1024
                      xs = init + h2 Wdec^T + bdec            from the TAPPED h2, K = 1024, A includes |init|; 160 columns: always the width-first kernel
    'loop', n_iter 3  h2 from the tapped h1 as above; h1 and xs finite (their inputs are not kept)
    'init' (n_iter 0) xs bit-equal to the init rows
    pad columns 157 .. 159 are exactly 0 always.  Where reg_seq_kernel ran, h1 / h2 exist as hi + lo planes only: + 2^-22 |v| + 2^-36 (ES's tail fact).
rotmat [N][24][3][3] from xs[:, :144] (rot6d_to_rotmat, fp contract off: every op rounds once; v = a1, w = a2 of a joint, k2 = |w| / max(|w - (b1.w) b1|, 1e-6)):
    n1 = |v|: 3 u relative (a sum of three rounded squares, its root);  b1 = v / n1: 4 u |b1_i| + 1.5 * 2^-126 / max(n1, 1e-6)^2 (squares that underflow)
    dp = b1 . w: 7 u |w|;   t = w - dp b1: 13 u |w| per component;   n2 = |t|: sqrt(3) 13 u |w| + 3 u n2
    b2 = t / n2: (13 + 22.6) u k2 + 4 u <= 40 u k2;   b3 = b1 x b2: 2 * 4 u + 2 * 40 u k2 + 6 u <= 94 u k2
    A joint whose |v| or |t| is below the clamp (1e-6 (1 + 2^-10)) is no normalisation any more and its conditioning is unbounded: finite only.
    Modes 1 / 2 (tepose_smpl_fwd) return no rotmat: R is read as pf + I (root: amat's rotation part, which IS R), which is R to u |R - I| on the
    diagonal; mode 2 must be the given matrices to that, mode 1 Rodrigues64(aa + 1e-8) to (8 angle + 50) u + that: angle = |aa + 1e-8| 4 u relative,
    axis 5 u, sin / cos 2 ulp (4 u) on top of the angle's error, K^2 13 u, the final sum 3 roundings on <= 3.
pf rows [N][224]: exact facts -- pf[:, 0] == 1; pf[:, 1:11], theta[:, 75:] bit-equal to the shape slots and theta[:, :3] to the cam slots of xs;
    pf[:, 218:] == 0; pf[:, 11 + 9 (j - 1) + 3 r + c] is the fp32 value rotmat - I.
pf_planes / pf16 from the pf rows: 2^-22 |v| + 2^-36 (blocked: the low half's fp16 subnormal step 2^-24, halved, / 2048) | + 2^-38 max|row| (scaled: the row
    is brought to [2^13, 2^14) first, the low half's step 2^-25 in those units; forward.hip "elements below 2^-3").  Pad columns exactly 0.
theta[:, 3:75] from rotmat: directly against the fp64 restatement of rotmat_to_aa on the device's R where |angle - pi| > 1e-2: quaternion component 6 u
    (t >= 1 in the chosen branch: 12 u on t, a difference 2 u, the divide), |xyz| 13.4 u, the half angle (13.4 + 6) u + 2 ulp of atan2 <= 26 u, aa =
    xyz (2 half / |xyz|): 19 u + 52 u + pi 13.4 u + 2 u <= 128 u.  As a rotation on every regular row: Rodrigues64(aa) against R itself, 3 * 128 u
    (each entry of exp has a gradient <= 1 per component) + 85 E, E = |R^T R - I|_F: R is orthonormal only to its own rounding, the quaternion of a
    matrix E away from a rotation is <= 2 E off per component, through the same chain 28 E, times 3, + E.
posed [N][24][3], amat [N][24][3][4] from R and beta.  Rest joints in the reference: J_regressor (v_template + shapedirs beta), NOT J0 + JS beta.
    e_J = 11 u (|J0| + |JS| |beta|): the fp32 storage of J0 / JS and 10 fmas.  rel = J - J_parent: e_J + e_J' + u |rel|.  Down the tree, level by level,
    G = P [R | rel]:  e_rot = e_P |R| + |P| e_R + 3 u |P| |R|   (product, fma, fma);  e_t = e_Prot |rel| + |P| e_rel + e_Pt + 4 u (|P| |rel| + |P_t|)
    (product, fma, fma, add).  posed = G_t.  amat: rotation e_rot; translation G_t - G J: e_t + e_rot |J| + |G| e_J + 4 u (|G| |J| + |G_t|).
vposed [N][20670] = pf blendW^T in fp64 from the tapped pf rows, K = 218 real columns of 224: the product bound of the plan's family at K = 224
    (scaled planes: + 2^-38 max|pf row| sum_k |W|).
verts from amat, vposed and the fp32 weight table: (nnz + 4) u (sum_j |w_j| |A_j|) (|v|, 1), nnz = 4 (compact kernel) or 24 (dense).  Under the
    one-launch small-N kernel vposed is not kept: it is restated from pf = [1 | beta | fp32(R - I)] with (224 + 3) u |pf| |W|^T (224 fmas + 3 shuffle
    adds) carried through |T|.
kp_3d: the 24 + 21 copied joints bit-equal to posed / verts; a regressed row (ceil(nnz / 64) + 6 + 1) u sum |w| |v| (per-lane chain, 6 shuffle adds).
kp_2d from kp_3d and cam = xs[:, 154:157], the kernel's formula (1e-9f is the fp32 constant): tz = 10000 / (224 s + 1e-9): rho = u (|224 s| + |den|) /
    |den| + u relative; 5000 (px / pz) / 112: |r| (5 u + |tz| rho / |pz|) -- relative, so it holds for s = 1e-3, 0 and negative s.
"""
import collections
import math

import numpy as np
import torch

import _encoder_stages as ES
from oracle import tepose_ref as O

U = ES.U
STAGES = ('xs', 'h1', 'h2', 'pf', 'pf_planes', 'pf16', 'amat', 'posed', 'vposed')
STAGE_ID = {n: i for i, n in enumerate(STAGES)}
WIDTH = dict(xs=160, h1=1024, h2=1024, pf=224, pf_planes=224, pf16=224, amat=288, posed=72, vposed=20670)
ORDER = ('xs', 'h1', 'h2', 'rotmat', 'pf', 'pf_planes', 'pf16', 'theta', 'posed', 'amat', 'vposed', 'verts', 'kp_3d', 'kp_2d')
NV, NJ, KB, KREAL = 6890, 24, 224, 218
CLAMP = 1e-6 * (1 + 2.0 ** -10)
WIDTH_FIRST = 'skinny_gemm_h3_kernel'
F32 = torch.float32
F64 = torch.float64

# how xs was made: how = 'collapsed' | 'tail_collapsed' | 'loop' | 'init' | 'pose'; feat [N, 2048]; tail ([N, 3 Hp], form) and H; n_iter; init = the
# [N, 160] initial rows; mode 1 / 2 with pose [N, 72] / [N, 24, 3, 3] and betas [N, 10] for 'pose' (tepose_smpl_fwd: no xs at all)
Src = collections.namedtuple('Src', 'how feat tail H n_iter init mode pose betas', defaults=(None,) * 8)
# taps[name] = (fp32 [N, WIDTH[name]], form); out: theta / verts / kp_3d / kp_2d / rotmat fp32 (tepose_smpl_fwd: verts and kp_3d only); J: the [17, 6890]
# evaluation regressor or None
Run = collections.namedtuple('Run', 'N taps out src J')


class StageMismatch(AssertionError):
    def __init__(self, failures):
        self.failures = failures
        more = '' if len(failures) <= 8 else '\n... and %d more' % (len(failures) - 8)
        super().__init__('%d stage(s) failed, first: %s\n%s%s' % (len(failures), failures[0]['stage'], '\n'.join(format_record(f) for f in failures[:8]), more))


def _record(stage, kernel, form, ratio, bound=None, note=''):
    """ratio [N, ...]: error / bound per element (NaN = infinite); the record holds its maximum, the person and element it is at and the bound there"""
    r = torch.where(torch.isnan(ratio), torch.full_like(ratio, float('inf')), ratio).reshape(ratio.shape[0], -1)
    at = int(torch.argmax(r))
    row, col = at // r.shape[1], at % r.shape[1]
    b, full = float('nan'), None
    if bound is not None:
        full = torch.as_tensor(bound, dtype=F64).expand(ratio.shape).reshape(r.shape)
        b = float(full[row, col])
    if _KEEP is not None:
        _KEEP[stage] = full
    return {'stage': stage, 'kernel': kernel, 'form': form, 'ratio': float(r.max()), 'row': row, 'col': col, 'bound': b,
            'n_bad': int((~(r <= 1.0)).sum()), 'n': r.numel(), 'note': note}


_KEEP = None           # check_stages(bounds = a dict): every stage's bound tensor [N, elements] (None where the stage is exact facts only) is left in it


def format_record(r):
    return '%-10s %-44s %-9s worst error / bound %9.4f at (person %d, element %d) bound there %.2e%s%s' % (
        r['stage'], r['kernel'], r['form'], r['ratio'], r['row'], r['col'], r['bound'], '; %d of %d over' % (r['n_bad'], r['n']) if r['n_bad'] else '', r['note'])


def format_records(records, tag=''):
    lines = ['%s%s' % (tag, format_record(r)) for r in records]
    worst = max(records, key=lambda r: r['ratio'])
    return lines + ['%sworst: %s %.4f' % (tag, worst['stage'], worst['ratio'])]


def _exact(got, want):
    """0 where bit-equal as values, infinity elsewhere (and for anything not finite)"""
    ok = (got == want) & torch.isfinite(got)
    return torch.where(ok, torch.zeros(got.shape, dtype=F64), torch.full(got.shape, float('inf'), dtype=F64))


def _finite(got):
    return torch.where(torch.isfinite(got), torch.zeros(got.shape, dtype=F64), torch.full(got.shape, float('inf'), dtype=F64))


def _ratio(got, want, bound):
    return (got.double() - want).abs() / bound.clamp_min(1e-300)


def coef(K, kernel):
    """ES.coef; reg_seq_kernel adds its 8 waves' K-partial sums like the width-first kernels"""
    return ES.coef(K, WIDTH_FIRST if 'reg_seq' in kernel else kernel)


def families(plan, dense):
    """(tail product family, its 160-column kernel, blend-shape family | None under the small kernel, skinning kernel) from tepose_select_kernels' words"""
    tr, sm = plan['tail_regressor'], plan['smpl']
    exact = 'gemm_kernel' in tr or 'f32' in tr
    fam = 'reg_seq_kernel' if tr.startswith('reg_seq') else tr.split(' ')[0].rstrip(':')
    if fam == 'collapsed':
        fam = WIDTH_FIRST
    blend = None if sm == 'smpl_small_kernel' else sm.split('+')[1]
    skin = 'smpl_small_kernel' if blend is None else 'smpl_skin_kernel' if dense else 'smpl_skin4_kernel'
    return fam, (fam if exact or 'reg_seq' in fam else WIDTH_FIRST), blend, skin


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def tables(smpl_np):
    """fp64 views of the caller's SMPL tables and what the bounds need of them (cached per table set)"""
    hit = _TABLES.get(id(smpl_np))
    if hit is not None and hit['src'] is smpl_np:
        return hit
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in smpl_np.items() if k != 'parents'}
    vt, sd, pd = t['v_template'].reshape(-1), t['shapedirs'].reshape(3 * NV, 10), t['posedirs']
    W = torch.cat([vt[:, None], sd, pd.t()], dim=1)                           # [20670, 218]: rows (v, c), columns [1 | beta | R - I]
    Jr = t['J_regressor']
    w32 = torch.from_numpy(np.ascontiguousarray(smpl_np['lbs_weights']))
    nnz = int((w32 != 0).sum(dim=1).max())
    parents = [int(p) for p in smpl_np['parents']]
    depth = [0] * NJ
    for j in range(1, NJ):
        depth[j] = depth[parents[j]] + 1
    out = dict(src=smpl_np, W=W, Wabs=W.abs(), Jreg=Jr, J0=Jr @ t['v_template'], JS=torch.einsum('jv,vcl->jcl', Jr, t['shapedirs']),
               vt=t['v_template'], sd=t['shapedirs'], lbs=t['lbs_weights'], dense=nnz > 4, parents=parents, depth=depth, extra=t['J_regressor_extra'])
    if len(_TABLES) > 6:
        _TABLES.clear()
    _TABLES[id(smpl_np)] = out
    return out


_MAPS = {}


def collapsed_maps(state):
    """Mf [160, 2048], k0 [160] of xs = feat Mf^T + k0 after three iterations from the model's own init, in fp64 from the fp32 weights: the iteration
    is affine in feat, so its value at 0 and at the unit vectors is the map"""
    hit = _MAPS.get(id(state))
    if hit is not None and hit[0] is state:
        return hit[1], hit[2]
    reg = O.split_state_dict(state, F64)[1]
    probe = torch.cat([torch.zeros(1, 2048, dtype=F64), torch.eye(2048, dtype=F64)])
    y = torch.nn.functional.pad(torch.cat(O.regressor_iterations(reg, probe, 3), dim=1), (0, 3))
    k0, Mf = y[0], (y[1:] - y[0]).t().contiguous()
    if len(_MAPS) > 4:
        _MAPS.clear()
    _MAPS[id(state)] = (state, Mf, k0)
    return Mf, k0


def init_rows(state, N, pose=None, shape=None, cam=None):
    """the [N, 160] fp32 rows the FC loop starts from: the caller's per-call rows where given, else the model's means; pad 0"""
    f = lambda given, key: torch.from_numpy(np.ascontiguousarray(state['regressor.' + key])).float().expand(N, -1) if given is None else torch.as_tensor(given).float()
    return torch.cat([f(pose, 'init_pose'), f(shape, 'init_shape'), f(cam, 'init_cam'), torch.zeros(N, 3)], dim=1).contiguous()


def _reg64(state):
    reg = O.split_state_dict(state, F64)[1]
    W1 = reg['fc1.weight']
    Wd = torch.cat([reg['decpose.weight'], reg['decshape.weight'], reg['deccam.weight']])
    bd = torch.cat([reg['decpose.bias'], reg['decshape.bias'], reg['deccam.bias']])
    return dict(W1a=W1[:, :2048], W1b=W1[:, 2048:], b1=reg['fc1.bias'], W2=reg['fc2.weight'], b2=reg['fc2.bias'], Wd=Wd, bd=bd)


# ---- geometry in fp64 -----------------------------------------------------------------------------------------------------------------------------------
def rot6d64(x144):
    """[N, 144] -> R [N, 24, 3, 3] (oracle), the bound of the module docstring [N, 24, 3, 3] and which joints are regular [N, 24]"""
    N = x144.shape[0]
    x = x144.double().reshape(N * 24, 3, 2)
    v, w = x[:, :, 0], x[:, :, 1]
    R = O.rot6d_to_rotmat(x144.double().reshape(-1, 6)).reshape(N, 24, 3, 3)
    n1 = v.norm(dim=1)
    b1 = v / n1.clamp_min(1e-6)[:, None]
    t = w - (b1 * w).sum(1, keepdim=True) * b1
    n2 = t.norm(dim=1)
    k2 = w.norm(dim=1) / n2.clamp_min(1e-6)
    e1 = 4 * U * b1.abs() + 1.5 * 2.0 ** -126 / n1.clamp_min(1e-6)[:, None] ** 2
    e2 = (40 * U * k2)[:, None].expand(-1, 3)
    e3 = (94 * U * k2.clamp_min(1.0))[:, None].expand(-1, 3)
    bound = torch.stack([e1, e2, e3], dim=-1).reshape(N, 24, 3, 3)
    return R, bound, ((n1 >= CLAMP) & (n2 >= CLAMP)).reshape(N, 24)


def rodrigues64(aa):
    """[M, 3] (fp64) -> [M, 3, 3], smplx's aa + 1e-8"""
    return O.batch_rodrigues(aa.double())


def exp64(aa):
    """the exact rotation of an axis-angle vector [M, 3] (no + 1e-8; well-conditioned at 0 through the series' limit)"""
    ang = aa.norm(dim=1, keepdim=True).clamp_min(1e-300)
    d = aa / ang
    z = torch.zeros_like(d[:, 0])
    K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], dim=1).view(-1, 3, 3)
    return torch.eye(3, dtype=F64)[None] + torch.sin(ang)[:, :, None] * K + (1 - torch.cos(ang))[:, :, None] * (K @ K)


def chain64(R, eR, beta, T):
    """The 24-joint chain in fp64 from R [N, 24, 3, 3] (its uncertainty eR, elementwise) and beta [N, 10] with the rest joints THE LONG WAY (J_regressor
    applied to the shaped template).  Returns posed, amat [N, 24, 3, 4] and their running componentwise bounds (module docstring)."""
    N = R.shape[0]
    v_shaped = T['vt'][None] + torch.einsum('bl,vcl->bvc', beta, T['sd'])
    J = torch.einsum('jv,bvc->bjc', T['Jreg'], v_shaped)
    eJ = 11 * U * (T['J0'].abs()[None] + torch.einsum('jcl,bl->bjc', T['JS'].abs(), beta.abs())) + 2.0 ** -40 * J.abs()
    par = T['parents']
    G = [None] * NJ
    eG = [None] * NJ
    Ra = R.abs()
    for j in sorted(range(NJ), key=lambda j: T['depth'][j]):
        if par[j] < 0:
            G[j] = torch.cat([R[:, j], J[:, j, :, None]], dim=2)
            eG[j] = torch.cat([eR[:, j], eJ[:, j, :, None]], dim=2)
            continue
        p = par[j]
        rel = J[:, j] - J[:, p]
        erel = eJ[:, j] + eJ[:, p] + U * rel.abs()
        P, eP = G[p], eG[p]
        Pa = P[:, :, :3].abs() + eP[:, :, :3]
        rot = P[:, :, :3] @ R[:, j]
        erot = eP[:, :, :3] @ Ra[:, j] + Pa @ eR[:, j] + 3 * U * (Pa @ Ra[:, j])
        t = (P[:, :, :3] @ rel[:, :, None])[:, :, 0] + P[:, :, 3]
        et = (eP[:, :, :3] @ rel.abs()[:, :, None])[:, :, 0] + (Pa @ erel[:, :, None])[:, :, 0] + eP[:, :, 3] \
            + 4 * U * ((Pa @ rel.abs()[:, :, None])[:, :, 0] + P[:, :, 3].abs())
        G[j] = torch.cat([rot, t[:, :, None]], dim=2)
        eG[j] = torch.cat([erot, et[:, :, None]], dim=2)
    G, eG = torch.stack(G, dim=1), torch.stack(eG, dim=1)                       # [N, 24, 3, 4]
    Gr, eGr = G[..., :3], eG[..., :3]
    GJ = torch.einsum('bjik,bjk->bji', Gr, J)
    at = G[..., 3] - GJ
    eat = eG[..., 3] + torch.einsum('bjik,bjk->bji', eGr, J.abs()) + torch.einsum('bjik,bjk->bji', Gr.abs() + eGr, eJ) \
        + 4 * U * (torch.einsum('bjik,bjk->bji', Gr.abs() + eGr, J.abs()) + G[..., 3].abs())
    amat = torch.cat([Gr, at[..., None]], dim=3)
    eamat = torch.cat([eGr, eat[..., None]], dim=3)
    return G[..., 3], eG[..., 3], amat, eamat


def skin64(amat, vposed, T, evp=None, chunk=32):
    """fp64 LBS from amat [N, 24, 3, 4] and vposed [N, 6890, 3] with the fp32 weight table; returns verts and the magnitude (sum |w| |A|) (|v|, 1)
    (+ |T| evp where vposed carries its own bound)"""
    N = amat.shape[0]
    w = T['lbs']
    verts, mag = torch.empty(N, NV, 3, dtype=F64), torch.empty(N, NV, 3, dtype=F64)
    extra = None if evp is None else torch.empty(N, NV, 3, dtype=F64)
    for a in range(0, N, chunk):
        A = amat[a:a + chunk].reshape(-1, NJ, 12)
        Tv = torch.einsum('vj,bjk->bvk', w, A).reshape(-1, NV, 3, 4)
        Ta = torch.einsum('vj,bjk->bvk', w.abs(), A.abs()).reshape(-1, NV, 3, 4)
        v = vposed[a:a + chunk]
        verts[a:a + chunk] = torch.einsum('bvik,bvk->bvi', Tv[..., :3], v) + Tv[..., 3]
        mag[a:a + chunk] = torch.einsum('bvik,bvk->bvi', Ta[..., :3], v.abs()) + Ta[..., 3]
        if extra is not None:
            extra[a:a + chunk] = torch.einsum('bvik,bvk->bvi', Ta[..., :3], evp[a:a + chunk])
    return verts, mag, extra


def project64(kp3, cam):
    """the joints kernel's projection in fp64 and its relative bound (module docstring)"""
    s, tx, ty = cam[:, 0:1].double(), cam[:, 1:2].double(), cam[:, 2:3].double()
    den = 224.0 * s + float(np.float32(1e-9))
    tz = 10000.0 / den
    rho = U * ((224.0 * s).abs() + den.abs()) / den.abs() + U
    q = kp3.double()
    pz = q[:, :, 2] + tz
    r = torch.stack([5000.0 * ((q[:, :, 0] + tx) / pz) / 112.0, 5000.0 * ((q[:, :, 1] + ty) / pz) / 112.0], dim=-1)
    return r, r.abs() * (5 * U + tz.abs() * rho / pz.abs())[:, :, None] + 2.0 ** -149


def regressed64(verts, Jrows):
    """fp64 rows of a sparse joint regressor applied to the device's verts, and (ceil(nnz / 64) + 7) u sum |w| |v|"""
    nnz = (Jrows != 0).sum(dim=1)
    c = (torch.ceil(nnz.double() / 64) + 7) * U
    v = verts.double()
    return torch.einsum('jv,bvc->bjc', Jrows, v), c[None, :, None] * torch.einsum('jv,bvc->bjc', Jrows.abs(), v.abs())


# ---- the checker ----------------------------------------------------------------------------------------------------------------------------------------
def check_stages(run, state, smpl_np, plan, raise_on_fail=True, stages=None, bounds=None):
    """Every stage of `run` against its fp64 restatement.  state: the reference-keyed numpy state dict (None for tepose_smpl_fwd); plan: the dict of
    tepose_select_kernels for the call's shape.  Returns the records in ORDER; raises StageMismatch unless raise_on_fail is False, in which case
    (records, failures) is returned.  stages: judge only these (the others' references are not computed where they are costly)."""
    global _KEEP
    _KEEP = bounds
    try:
        return _check_stages(run, state, smpl_np, plan, raise_on_fail, stages)
    finally:
        _KEEP = None


def _check_stages(run, state, smpl_np, plan, raise_on_fail, stages):
    T = tables(smpl_np)
    heavy = stages is None or bool(set(stages) & {'vposed', 'verts'})
    N, taps, out, src = run.N, run.taps, run.out, run.src
    fam, fam160, blend, skin = families(plan, T['dense'])
    small = blend is None
    records = []
    tap = lambda n: taps[n][0]
    form = lambda n: ES.FORMS[taps[n][1]]
    planes = lambda n: taps[n][1] in ES.PLANES
    for n, (t, _) in taps.items():
        assert tuple(t.shape) == (N, WIDTH[n]) and t.dtype == F32, (n, tuple(t.shape))

    # ---- xs and the FC activations
    if src.how != 'pose':
        xs = tap('xs')
        if src.how == 'init':
            records.append(_record('xs', 'init_state_rows', form('xs'), _exact(xs, src.init)))
        elif src.how in ('collapsed', 'tail_collapsed'):
            Mf, k0 = collapsed_maps(state)
            if src.how == 'collapsed':
                a, M, k, K = src.feat.double(), Mf, k0, 2048
            else:
                enc = O.split_state_dict(state, F64)[0]
                H, Hp = src.H, ES.hp_of(src.H)
                a = ES._gates(src.tail[0], H, Hp)[0].double().reshape(N, 3 * H)
                Wc = torch.cat([enc['linear_fwd.weight'], enc['linear_rec.weight']], dim=1)
                M, k, K = Mf @ Wc / 2, k0 + Mf @ (enc['linear_fwd.bias'] + enc['linear_rec.bias']) / 2, 3 * Hp
            want = a @ M.t() + k
            bound = (coef(K, WIDTH_FIRST) + U) * (a.abs() @ M.abs().t() + k.abs())
            ratio = _ratio(xs, want, bound)
            ratio[:, 157:] = _exact(xs[:, 157:], torch.zeros(N, 3))
            records.append(_record('xs', '%s (%s)' % (src.how, WIDTH_FIRST), form('xs'), ratio, bound))
        else:
            w = _reg64(state)
            init = src.init.double()
            h1, h2 = tap('h1'), tap('h2')
            pl = lambda n, want: (2.0 ** -22 * want.abs() + 2.0 ** -36) if planes(n) else 0.0
            if src.n_iter == 1:
                f = src.feat.double()
                base = f @ w['W1a'].t() + w['b1']
                want = base + init[:, :157] @ w['W1b'].t()
                bound = coef(2048, fam) * (f.abs() @ w['W1a'].abs().t() + w['b1'].abs()) + coef(160, fam) * (init[:, :157].abs() @ w['W1b'].abs().t() + base.abs())
                bound = bound + pl('h1', want)
                records.append(_record('h1', fam, form('h1'), _ratio(h1, want, bound), bound))
            else:
                records.append(_record('h1', fam, form('h1'), _finite(h1), note='  [its state row is not kept: finite only]'))
            a = h1.double()
            want = a @ w['W2'].t() + w['b2']
            bound = coef(1024, fam) * (a.abs() @ w['W2'].abs().t() + w['b2'].abs())
            bound = bound + pl('h2', want)
            records.append(_record('h2', fam, form('h2'), _ratio(h2, want, bound), bound))
            if src.n_iter == 1:
                a = h2.double()
                want = init[:, :157] + a @ w['Wd'].t() + w['bd']
                bound = coef(1024, fam160) * (a.abs() @ w['Wd'].abs().t() + w['bd'].abs() + init[:, :157].abs())
                ratio = torch.cat([_ratio(xs[:, :157], want, bound), _exact(xs[:, 157:], torch.zeros(N, 3))], dim=1)
                records.append(_record('xs', fam160, form('xs'), ratio, torch.nn.functional.pad(bound, (0, 3))))
            else:
                ratio = torch.cat([_finite(xs[:, :157]), _exact(xs[:, 157:], torch.zeros(N, 3))], dim=1)
                records.append(_record('xs', fam160, form('xs'), ratio, note='  [the state row before it is not kept: finite and pads only]'))
        beta32, cam32 = xs[:, 144:154], xs[:, 154:157]
    else:
        beta32, cam32 = torch.as_tensor(src.betas).float(), None

    # ---- rotations
    eye = torch.eye(3, dtype=F64)
    if src.how != 'pose':
        rot = out['rotmat'].reshape(N, 24, 3, 3)
        want, bound, regular = rot6d64(xs[:, :144])
        ratio = torch.where(regular[:, :, None, None], _ratio(rot, want, bound), _finite(rot))
        records.append(_record('rotmat', 'rot6d', 'rows', ratio, bound, '' if bool(regular.all()) else '  [%d joint(s) at the clamp: finite only]' % int((~regular).sum())))
        R, eR = rot.double(), torch.zeros(N, 24, 3, 3, dtype=F64)
    else:
        regular = torch.ones(N, 24, dtype=torch.bool)
        if small:                                                         # nothing of the rotations is kept but amat's root: the given pose is R
            R = (rodrigues64(torch.as_tensor(src.pose).double().reshape(-1, 3)) if src.mode == 1 else torch.as_tensor(src.pose).double()).reshape(N, 24, 3, 3)
            ang = torch.as_tensor(src.pose).double().reshape(N, 24, -1).norm(dim=2) if src.mode == 1 else torch.zeros(N, 24, dtype=F64)
            eR = ((8 * ang + 50) * U)[:, :, None, None].expand(N, 24, 3, 3).contiguous() if src.mode == 1 else torch.zeros(N, 24, 3, 3, dtype=F64)
        else:
            pf = tap('pf')
            R = torch.cat([tap('amat').reshape(N, 24, 3, 4)[:, :1, :, :3].double(), pf[:, 11:KREAL].double().reshape(N, 23, 3, 3) + eye], dim=1)
            eR = (U * (R - eye).abs() * eye).contiguous()
            eR[:, 0] = 0
            if src.mode == 1:
                aa = torch.as_tensor(src.pose).double().reshape(-1, 3)
                want = rodrigues64(aa).reshape(N, 24, 3, 3)
                bound = ((8 * (aa + 1e-8).norm(dim=1) + 50) * U).reshape(N, 24, 1, 1) + eR
            else:
                want, bound = torch.as_tensor(src.pose).double().reshape(N, 24, 3, 3), eR + 2.0 ** -149
            records.append(_record('rotmat', 'rodrigues' if src.mode == 1 else 'given matrices', 'pf + I', (R - want).abs() / bound, bound))

    # ---- pose features: exact facts, then the plane forms
    if not small:
        pf = tap('pf')
        wantpf = torch.zeros(N, KB)
        wantpf[:, 0] = 1
        wantpf[:, 1:11] = beta32
        if src.how != 'pose':
            wantpf[:, 11:KREAL] = (out['rotmat'].reshape(N, 24, 3, 3)[:, 1:] - torch.eye(3)).reshape(N, 207)
        else:
            wantpf[:, 11:KREAL] = pf[:, 11:KREAL]                            # (judged as a rotation above)
        ratio = _exact(pf, wantpf)
        records.append(_record('pf', 'smpl_prep_kernel', 'rows', ratio))
        m = pf.double().abs().max(dim=1, keepdim=True).values
        for n, absolute in (('pf_planes', 2.0 ** -36), ('pf16', 2.0 ** -38 * m)):
            if n in taps:
                bound = 2.0 ** -22 * pf.double().abs() + absolute
                ratio = _ratio(tap(n), pf.double(), bound)
                ratio[:, KREAL:] = _exact(tap(n)[:, KREAL:], torch.zeros(N, KB - KREAL))
                records.append(_record(n, 'smpl_prep_kernel' if n == 'pf_planes' else 'split_rows_kernel', form(n), ratio, bound))
    if src.how != 'pose':
        th = out['theta']
        facts = torch.cat([_exact(th[:, :3], cam32), _exact(th[:, 75:], beta32)], dim=1)
        Rf = R.reshape(-1, 3, 3)
        aa64 = O.rotmat_to_angle_axis(Rf)
        got = th[:, 3:75].double().reshape(-1, 3)
        ang = aa64.norm(dim=1)
        E = (Rf.transpose(1, 2) @ Rf - eye).reshape(-1, 9).norm(dim=1)
        reg = regular.reshape(-1) & torch.isfinite(aa64).all(dim=1)
        direct = torch.where((reg & ((ang - math.pi).abs() > 1e-2))[:, None], (got - aa64).abs() / (128 * U), _finite(got))
        asrot = (exp64(got) - Rf).abs().reshape(-1, 9).max(dim=1).values / (3 * 128 * U + 85 * E)
        direct = torch.maximum(direct, torch.where(reg, asrot, torch.zeros_like(asrot))[:, None])
        ratio = torch.cat([facts[:, :3], direct.reshape(N, 72), facts[:, 3:]], dim=1)
        records.append(_record('theta', 'rotmat_to_aa', 'rows', ratio, 128 * U))

    # ---- the chain
    posed64, eposed, amat64, eamat = chain64(R, eR, beta32.double(), T)
    chain_kernel = 'smpl_small_kernel' if small else 'smpl_prep_kernel'
    # (a joint at the clamp: its R is still the chain's input, exactly)
    records.append(_record('posed', chain_kernel, 'rows', _ratio(tap('posed').reshape(N, 24, 3), posed64, eposed), eposed))
    records.append(_record('amat', chain_kernel, 'rows', _ratio(tap('amat').reshape(N, 24, 3, 4), amat64, eamat), eamat))

    # ---- blend shapes and skinning
    verts = out['verts'].reshape(N, NV, 3)
    if heavy:
        A = tap('amat').double().reshape(N, 24, 3, 4)
        if not small:
            a = tap('pf')[:, :KREAL].double()
            want = a @ T['W'].t()
            bound = coef(KB, blend) * (a.abs() @ T['Wabs'].t())
            if 'h3s' in blend:
                bound = bound + 2.0 ** -38 * a.abs().max(dim=1, keepdim=True).values * T['Wabs'].sum(dim=1)[None]
            records.append(_record('vposed', blend, 'rows', _ratio(tap('vposed'), want, bound), bound))
            del want, bound
            want, mag, _ = skin64(A, tap('vposed').double().reshape(N, NV, 3), T)
            bound = ((24 if T['dense'] else 4) + 4) * U * mag
        else:
            pf32 = torch.zeros(N, KREAL)
            pf32[:, 0] = 1
            pf32[:, 1:11] = beta32
            pf32[:, 11:] = (R.float() - torch.eye(3))[:, 1:].reshape(N, 207) if src.how == 'pose' else (out['rotmat'].reshape(N, 24, 3, 3)[:, 1:] - torch.eye(3)).reshape(N, 207)
            a = pf32.double()
            vp = (a @ T['W'].t()).reshape(N, NV, 3)
            evp = ((KB + 3) * U * (a.abs() @ T['Wabs'].t())).reshape(N, NV, 3)
            if src.how == 'pose':                                              # R itself is only known to eR: |dR| |W| on top
                evp = evp + (torch.nn.functional.pad(eR[:, 1:].reshape(N, 207), (11, 0)) @ T['Wabs'].t()).reshape(N, NV, 3)
            want, mag, extra = skin64(A, vp, T, evp)
            bound = 8 * U * mag + extra
        records.append(_record('verts', skin, 'rows', _ratio(verts, want, bound), bound))
        del want, bound, mag

    # ---- joints and projection
    kp3 = out['kp_3d']
    if run.J is not None:
        Jh = torch.from_numpy(np.ascontiguousarray(run.J)).double()[O.H36M_TO_J14]
        want, bound = regressed64(verts, Jh)
        ratio = _ratio(kp3, want, bound)
    else:
        want, bound = regressed64(verts, T['extra'])
        ratio, b49 = torch.empty(N, 49, 3, dtype=F64), torch.zeros(N, 49, 3, dtype=F64)
        posed32 = tap('posed').reshape(N, 24, 3)
        for k, s in enumerate(O.JOINT_MAP_49):
            if s < 24:
                ratio[:, k] = _exact(kp3[:, k], posed32[:, s])
            elif s < 45:
                ratio[:, k] = _exact(kp3[:, k], verts[:, O.EXTRA_VERTEX_IDS[s - 24]])
            else:
                ratio[:, k] = _ratio(kp3[:, k], want[:, s - 45], bound[:, s - 45])
                b49[:, k] = bound[:, s - 45]
        bound = b49
    records.append(_record('kp_3d', 'smpl_joints_kernel', 'rows', ratio, bound))
    if 'kp_2d' in out:
        want, bound = project64(kp3, cam32)
        records.append(_record('kp_2d', 'smpl_joints_kernel', 'rows', _ratio(out['kp_2d'], want, bound), bound))

    records = sorted((r for r in records if stages is None or r['stage'] in stages), key=lambda r: ORDER.index(r['stage']))
    failures = [r for r in records if not r['ratio'] <= 1.0]
    if not raise_on_fail:
        return records, failures
    if failures:
        raise StageMismatch(failures)
    return records


# ---- the stand-in for a device: what taps and outputs would hold, had torch computed every stage in fp32 on the CPU ------------------------------------
def _planes32(v):
    hi = v.half().float()
    return hi + ((v - hi) * 2048.0).half().float() / 2048.0


def _planes16(v):
    m = v.abs().max(dim=1, keepdim=True).values
    ex = torch.frexp(m)[1]
    sc, inv = torch.ldexp(torch.ones_like(m), 14 - ex), torch.ldexp(torch.ones_like(m), ex - 14)
    s = v * sc
    hi = s.half().float()
    return (hi + (s - hi).half().float()) * inv


def standin_run(state, smpl_np, src, plan, J=None, JS_fault=None):
    """A Run of an fp32 emulation: torch fp32 products (the split families' operands rounded to hi + lo fp16 first), the op sequences of smpl.hip in
    fp32, the pack-time constants as the library forms them (fp64 sums stored in fp32).  JS_fault = (j, c, l, delta) perturbs one JS entry at 'pack time'."""
    T = tables(smpl_np)
    fam, fam160, blend, skin = families(plan, T['dense'])
    small = blend is None
    split = fam160 not in ES.EXACT_KERNELS
    q = ES.split22 if split else (lambda t: t)
    taps = {}
    if src.how == 'pose':
        N = int(torch.as_tensor(src.pose).shape[0])
        beta = torch.as_tensor(src.betas).float()
        if src.mode == 1:
            aa = torch.as_tensor(src.pose).float().reshape(-1, 3)
            R = O.batch_rodrigues(aa).reshape(N, 24, 3, 3)
        else:
            R = torch.as_tensor(src.pose).float().reshape(N, 24, 3, 3).clone()
        xs = None
    else:
        N = int((src.feat if src.feat is not None else src.init if src.tail is None else src.tail[0]).shape[0])
        w = {k: v.float() for k, v in _reg64(state).items()} if state is not None else None
        if src.how == 'init':
            xs = src.init.clone()
        elif src.how == 'collapsed':
            Mf, k0 = collapsed_maps(state)
            xs = q(src.feat) @ q(Mf.float()).t() + k0.float()
        elif src.how == 'tail_collapsed':
            Mf, k0 = collapsed_maps(state)
            enc = O.split_state_dict(state, F64)[0]
            H, Hp = src.H, ES.hp_of(src.H)
            Wc = torch.cat([enc['linear_fwd.weight'], enc['linear_rec.weight']], dim=1)
            M, k = (Mf @ Wc / 2).float(), (k0 + Mf @ (enc['linear_fwd.bias'] + enc['linear_rec.bias']) / 2).float()
            xs = q(ES._gates(src.tail[0], H, Hp)[0].reshape(N, 3 * H)) @ q(M).t() + k
        else:
            x = src.init[:, :157].clone()
            base = q(src.feat) @ q(w['W1a']).t() + w['b1']
            for _ in range(src.n_iter):
                h1 = base + q(x) @ q(w['W1b']).t()
                h2 = q(h1) @ q(w['W2']).t() + w['b2']
                x = x + q(h2) @ q(w['Wd']).t() + w['bd']
            seq = 'reg_seq' in fam
            taps['h1'] = (_planes32(h1), 3) if seq else (h1, 0)
            taps['h2'] = (_planes32(h2), 3) if seq else (h2, 0)
            xs = torch.nn.functional.pad(x, (0, 3))                       # (q(h) is the planes' value: the consumers read what the tap reads)
        if xs.shape[1] == 157:
            xs = torch.nn.functional.pad(xs, (0, 3))
        xs = xs.contiguous()
        xs[:, 157:] = 0
        taps['xs'] = (xs, 0)
        beta = xs[:, 144:154]
        R = O.rot6d_to_rotmat(xs[:, :144].reshape(-1, 6)).reshape(N, 24, 3, 3)
    # the chain in fp32, rest joints from the fp32-stored constants
    J0, JS = T['J0'].float(), T['JS'].float().clone()
    if JS_fault is not None:
        JS[JS_fault[0], JS_fault[1], JS_fault[2]] += JS_fault[3]
    Jr = J0[None] + torch.einsum('jcl,bl->bjc', JS, beta)
    par = T['parents']
    G = [None] * NJ
    for j in sorted(range(NJ), key=lambda j: T['depth'][j]):
        if par[j] < 0:
            G[j] = torch.cat([R[:, j], Jr[:, j, :, None]], dim=2)
        else:
            P, rel = G[par[j]], Jr[:, j] - Jr[:, par[j]]
            G[j] = torch.cat([P[:, :, :3] @ R[:, j], ((P[:, :, :3] @ rel[:, :, None])[:, :, 0] + P[:, :, 3])[:, :, None]], dim=2)
    G = torch.stack(G, dim=1)
    amat = torch.cat([G[..., :3], (G[..., 3] - torch.einsum('bjik,bjk->bji', G[..., :3], Jr))[..., None]], dim=3).contiguous()
    posed = G[..., 3].contiguous()
    taps['amat'], taps['posed'] = (amat.reshape(N, 288), 0), (posed.reshape(N, 72), 0)
    pf = torch.zeros(N, KB)
    pf[:, 0] = 1
    pf[:, 1:11] = beta
    pf[:, 11:KREAL] = (R[:, 1:] - torch.eye(3)).reshape(N, 207)
    W32 = T['W'].float()
    if not small:
        taps['pf'] = (pf, 0)
        if 'h3' in blend:
            taps['pf_planes'] = (_planes32(pf), 3)
        if 'h3s' in blend:
            taps['pf16'] = (_planes16(pf), 4)
        a = pf[:, :KREAL]
        vp = (q(a) @ q(W32).t()) if 'h3' in blend else a @ W32.t()
        taps['vposed'] = (vp.contiguous(), 0)
    else:
        vp = pf[:, :KREAL] @ W32.t()
    lbs = T['lbs'].float()
    Tv = torch.zeros(N, NV, 12)
    for j in range(NJ):                                                   # the kernels' order: ascending joints, one fma each (zeros add nothing)
        Tv = Tv + lbs[None, :, j, None] * amat.reshape(N, 1, NJ, 12)[:, :, j]
    Tv = Tv.reshape(N, NV, 3, 4)
    verts = (torch.einsum('bvik,bvk->bvi', Tv[..., :3], vp.reshape(N, NV, 3)) + Tv[..., 3]).contiguous()
    out = {'verts': verts}

    def regress(rows):                                                     # a lane's chain over its entries, then the six shuffle adds
        res = torch.zeros(N, rows.shape[0], 3)
        for r in range(rows.shape[0]):
            idx = torch.nonzero(rows[r] != 0)[:, 0]
            n = (len(idx) + 63) // 64 * 64
            wv = torch.zeros(n)
            wv[:len(idx)] = rows[r, idx].float()
            vv = torch.zeros(N, n, 3)
            vv[:, :len(idx)] = verts[:, idx]
            acc = torch.zeros(N, 64, 3)
            for c in range(n // 64):
                acc = acc + wv[None, c * 64:(c + 1) * 64, None] * vv[:, c * 64:(c + 1) * 64]
            o = 32
            while o:
                acc = acc[:, :o] + acc[:, o:2 * o]
                o //= 2
            res[:, r] = acc[:, 0]
        return res
    if J is not None:
        kp3 = regress(torch.from_numpy(np.ascontiguousarray(J)).double())[:, O.H36M_TO_J14].contiguous()
    else:
        reg = regress(T['extra'])
        j54 = torch.cat([posed, verts[:, O.EXTRA_VERTEX_IDS], reg], dim=1)
        kp3 = j54[:, O.JOINT_MAP_49].contiguous()
    out['kp_3d'] = kp3
    if xs is not None:
        cam = xs[:, 154:157]
        tz = np.float32(10000.0) / (np.float32(224.0) * cam[:, 0:1] + np.float32(1e-9))
        px, py, pz = kp3[:, :, 0] + cam[:, 1:2], kp3[:, :, 1] + cam[:, 2:3], kp3[:, :, 2] + tz
        out['kp_2d'] = torch.stack([(5000.0 * (px / pz)) / 112.0, (5000.0 * (py / pz)) / 112.0], dim=-1)
        out['rotmat'] = R.contiguous()
        aa = O.rotmat_to_angle_axis(R.reshape(-1, 3, 3)).reshape(N, 72)
        out['theta'] = torch.cat([cam, aa, beta], dim=1).contiguous()
    return Run(N, taps, out, src, J)


def standin_plan(N, split=True, dense=False, reg='collapsed', blend16=False):
    """a plan as tepose_select_kernels words it, for the emulation"""
    tr = {'collapsed': 'collapsed: one product (skinny_gemm_h3_kernel)', 'seq': 'reg_seq_kernel', 'loop': 'skinny_gemm_h3_kernel loop',
          'tiled': 'gemm_h3_kernel loop'}[reg] if split else 'skinny_gemm_kernel x (2 + 1 + 9)'
    mid = ('gemm_h3s_persist16c_kernel<1>' if blend16 else 'gemm_h3_kernel') if split else 'skinny_gemm_kernel'
    return {'tail_regressor': tr, 'smpl': 'smpl_small_kernel' if N <= 4 and not dense else 'smpl_prep_kernel+%s+smpl_skin4_kernel' % mid}


def output_tests_see(run_a, run_b, tol=1e-4):
    """what the output comparisons of the other tests (1e-4 absolute on the five outputs) would report between two runs: the largest difference, and
    whether it is over"""
    worst = max(float((run_a.out[k].double() - run_b.out[k].double()).abs().max()) for k in run_a.out)
    return worst, worst >= tol
