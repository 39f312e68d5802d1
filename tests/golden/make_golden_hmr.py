"""Generate tests/golden/hmr_features_N3.npz and hmr_state_keys.npz by running the REFERENCE's own HMR class on the CPU.

Run only in the build container (needs the reference checkout; never on the GPU box):

    python tests/golden/make_golden_hmr.py

The reference's `HMR(Bottleneck, [3, 4, 6, 3], ...)` (lib/models/spin.py:16-206) is imported through the stubs of make_golden.py (stand-in
SMPL = the oracle's LBS over the synthetic tables) and executed in fp64 and in fp32 on the seeded weights / images of tests/_hmr_synth.py.
The fixtures hold seeds and expected outputs only -- no weights, no reference source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import _hmr_synth as HS  # noqa: E402

N = 3


def digest(out):
    v = out['verts'].double().numpy()
    return {'theta': out['theta'].double().numpy(), 'kp_3d': out['kp_3d'].double().numpy(), 'kp_2d': out['kp_2d'].double().numpy(),
            'verts_sub': v[:, ::108][:, :64].copy(), 'verts_sum': v.sum(axis=1), 'verts_l2': np.sqrt((v * v).sum(axis=(1, 2)))}


def main():
    MG.install_stubs()
    import lib.models.spin as P
    model = P.HMR(P.Bottleneck, [3, 4, 6, 3], P.SMPL_MEAN_PARAMS).eval()
    sd = model.state_dict()
    names = [k for k in sd if not k.startswith('smpl.')]
    shapes = np.full((len(names), 4), -1, dtype=np.int64)
    for i, k in enumerate(names):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    MG.save('hmr_state_keys', names=np.array(names), shapes=shapes, ndim=np.array([sd[k].dim() for k in names], dtype=np.int64))

    syn = HS.state_dict_np({k: tuple(sd[k].shape) for k in names})
    assert sum(1 for k in syn if HS.is_backbone_key(k)) == 265 and all(k in syn for k in names if 'num_batches_tracked' not in k), 'recipe misses a tensor'
    MG.load_synth(model, syn)
    x = torch.from_numpy(HS.images(N))
    ip, ish, ic = (torch.from_numpy(a) for a in HS.init_state(N))

    amax = [0.0]
    hooks = [m.register_forward_hook(lambda m, i, o: amax.__setitem__(0, max(amax[0], float(o.detach().abs().max()))) if torch.is_tensor(o) else None)
             for m in model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d, P.Bottleneck))]
    m64 = model.double()
    cases = (('default', {}, 3), ('init', {'init_pose': ip, 'init_shape': ish, 'init_cam': ic}, 3), ('it0', {'init_pose': ip, 'init_shape': ish, 'init_cam': ic}, 0))
    with torch.no_grad():
        torch.set_default_dtype(torch.float64)                     # the tensors the reference creates on the way (projection's eye / zeros) follow
        feat64 = m64.feature_extractor(x.double())
        out64 = {tag: digest(m64(x.double(), n_iter=it, **{k: v.double() for k, v in kw.items()})[0]) for tag, kw, it in cases}
        xf, o = m64(x.double(), return_features=True)
        assert torch.equal(xf, feat64)
        torch.set_default_dtype(torch.float32)
        m32 = model.float()
        feat32 = m32.feature_extractor(x)
        out32 = {tag: digest(m32(x, n_iter=it, **kw)[0]) for tag, kw, it in cases}
    for h in hooks:
        h.remove()
    feat64, feat32 = feat64.numpy(), feat32.numpy()
    e32 = float(np.abs(feat32.astype(np.float64) - feat64).max() / np.abs(feat64).max())
    print('max |activation| %.3g   features: max %.3g, non-zero per image %s   e32 %.3g' % (amax[0], np.abs(feat64).max(), (feat64 != 0).sum(axis=1), e32))
    # on the reference alone; if one fails, change the recipe (tests/_hmr_synth.py), not the assertion
    assert amax[0] < 1e3, amax[0]
    assert ((feat64 != 0).sum(axis=1) >= 1024).all()
    for tag in out64:
        for k in ('theta', 'kp_3d', 'kp_2d', 'verts_sub'):
            gap = float(np.abs(out32[tag][k] - out64[tag][k]).max())
            print('  %-8s %-9s fp32 - fp64 %.3g' % (tag, k, gap))
            assert gap <= 2.5e-5, (tag, k, gap)
    d = {'seeds': np.array([HS.SEED_W, HS.SEED_X], dtype=np.int64), 'feat64': feat64, 'feat32': feat32, 'e32': np.array(e32)}
    for tag in out64:
        for k, v in out64[tag].items():
            d['%s_%s' % (tag, k)] = v
    MG.save('hmr_features_N3', **d)
    print('wrote hmr_features_N3', {k: v.shape for k, v in d.items()})


if __name__ == '__main__':
    main()
