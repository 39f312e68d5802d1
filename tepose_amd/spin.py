"""Drop-in for the reference's lib/models/spin.py: `Regressor` (lib/models/spin.py:209-291), `projection` (:307-351) and the
`HMR` model with its ResNet-50 feature extractor (:59-206, `hmr` :294-304, `get_pretrained_hmr` :354-360).
"""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from .engine import Engine, on_device, warn_if_training
from .smpl import SMPL, SMPL_MEAN_PARAMS, SMPL_MODEL_DIR, H36M_TO_J14  # noqa: F401


class Regressor(nn.Module):
    """Same parameters, buffers and forward signature as the reference class; the forward
    (3x fc1/fc2/decoders, rot6d->R, SMPL LBS, joints, projection, R->axis-angle) is one call
    into libtepose_hip.so.

    Extra keyword `smpl=` takes a ready `SMPL` (the licence-gated model files are absent in
    this repo); `smpl_mean_params` may also be a dict with 'pose','shape','cam'."""

    def __init__(self, smpl_mean_params=SMPL_MEAN_PARAMS, smpl=None, _engine=None):
        super().__init__()
        npose = 24 * 6
        self.fc1 = nn.Linear(512 * 4 + npose + 13, 1024)
        self.drop1 = nn.Dropout()
        self.fc2 = nn.Linear(1024, 1024)
        self.drop2 = nn.Dropout()
        self.decpose = nn.Linear(1024, npose)
        self.decshape = nn.Linear(1024, 10)
        self.deccam = nn.Linear(1024, 3)
        nn.init.xavier_uniform_(self.decpose.weight, gain=0.01)
        nn.init.xavier_uniform_(self.decshape.weight, gain=0.01)
        nn.init.xavier_uniform_(self.deccam.weight, gain=0.01)
        self.smpl = smpl if smpl is not None else SMPL(SMPL_MODEL_DIR, batch_size=64, create_transl=False)
        mean_params = smpl_mean_params if isinstance(smpl_mean_params, dict) else np.load(smpl_mean_params)
        init_pose = torch.from_numpy(np.asarray(mean_params['pose'][:], dtype=np.float32)).unsqueeze(0)
        init_shape = torch.from_numpy(np.asarray(mean_params['shape'][:]).astype('float32')).unsqueeze(0)
        init_cam = torch.from_numpy(np.asarray(mean_params['cam'], dtype=np.float32)).unsqueeze(0)
        self.register_buffer('init_pose', init_pose)
        self.register_buffer('init_shape', init_shape)
        self.register_buffer('init_cam', init_cam)
        object.__setattr__(self, '_engine', _engine if _engine is not None else Engine(1, 64))

    def forward(self, x, init_pose=None, init_shape=None, init_cam=None, n_iter=3, is_train=False,
                J_regressor=None):
        warn_if_training(self, x)
        if not x.is_cuda:
            raise RuntimeError('tepose_amd runs on MI355X only: move the model and input to a cuda device')
        x = x.float().contiguous()
        eng = self._engine
        with on_device(x.device):
            eng.pack_regressor(self, x.device)
            use_j = J_regressor if (not is_train and J_regressor is not None) else None
            return [eng.regressor_fwd(x, n_iter, use_j, init=(init_pose, init_shape, init_cam))]


def warm_start_from_spin(regressor, ckpt_path):
    """Initialise the regressor from a SPIN checkpoint's 'model' entry, non-strictly, when the file
    exists -- what TePose.__init__ / VIBE.__init__ do with `pretrained`
    (lib/models/tepose.py:115-118, lib/models/vibe.py:97-101)."""
    import os
    if not ckpt_path or not os.path.isfile(ckpt_path):
        return False
    from .data import load_checkpoint
    weights = load_checkpoint(ckpt_path)['model']
    regressor.load_state_dict(weights, strict=False)
    print("=> loaded pretrained model from '%s'" % ckpt_path)
    return True


def projection(pred_joints, pred_camera):
    """lib/models/spin.py:307-320 with R = I and zero camera centre (host-side helper for
    callers; the model forward computes kp_2d on the GPU)."""
    t = torch.stack([pred_camera[:, 1], pred_camera[:, 2],
                     2 * 5000. / (224. * pred_camera[:, 0] + 1e-9)], dim=-1)
    p = pred_joints + t.unsqueeze(1)
    p = p / p[:, :, -1].unsqueeze(-1)
    return (5000. * p[:, :, :-1]) / (224. / 2.)


# ResNet-50 as (planes, blocks, stride of the first block) per stage; a bottleneck is 1x1 -> 3x3 (carries the stride) -> 1x1 with 4 x planes outputs.
# (The C library walks its own table of the same network, csrc/hmr.h; this one only names the parameter containers.)
_STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))
_EXPANSION = 4
HMR_IMAGE = 224
HMR_PASS = 64            # images per pass of tepose_hmr_features (csrc/hmr.hip runs N > 64 in passes of 64 on one workspace)


def _conv_bn(holder, conv_name, bn_name, cin, cout, k, stride):
    setattr(holder, conv_name, nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False))
    setattr(holder, bn_name, nn.BatchNorm2d(cout))


class HMR(nn.Module):
    """Same constructor, state-dict keys and forward signature as the reference class (lib/models/spin.py:59-206); `block` is accepted
    and ignored (the bottleneck of spin.py:16-56 is the only one the reference passes).  The members are parameter containers and
    are never called: `feature_extractor` is one call into libtepose_hip.so (53 convolutions with their inference batch norms
    folded in at pack time), `forward` adds the regressor entry that `Regressor` uses.  Inference only: train-mode batch norm is
    not offered.  Extra keyword `smpl=` as in `Regressor`."""

    def __init__(self, block=None, layers=(3, 4, 6, 3), smpl_mean_params=SMPL_MEAN_PARAMS, smpl=None):
        super().__init__()
        if list(layers) != [n for _, n, _ in _STAGES]:
            raise ValueError('HMR is built for ResNet-50: layers must be [3, 4, 6, 3], got %r' % (list(layers),))
        npose = 24 * 6
        _conv_bn(self, 'conv1', 'bn1', 3, 64, 7, 2)
        inplanes = 64
        for i, (planes, blocks, stride) in enumerate(_STAGES):
            stage = nn.Sequential()
            for b in range(blocks):
                blk = nn.Module()
                _conv_bn(blk, 'conv1', 'bn1', inplanes, planes, 1, 1)
                _conv_bn(blk, 'conv2', 'bn2', planes, planes, 3, stride if b == 0 else 1)
                _conv_bn(blk, 'conv3', 'bn3', planes, planes * _EXPANSION, 1, 1)
                if b == 0:
                    blk.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * _EXPANSION, kernel_size=1, stride=stride, bias=False),
                                                   nn.BatchNorm2d(planes * _EXPANSION))
                inplanes = planes * _EXPANSION
                stage.add_module(str(b), blk)
            setattr(self, 'layer%d' % (i + 1), stage)
        self.fc1 = nn.Linear(512 * _EXPANSION + npose + 13, 1024)
        self.drop1 = nn.Dropout()
        self.fc2 = nn.Linear(1024, 1024)
        self.drop2 = nn.Dropout()
        self.decpose = nn.Linear(1024, npose)
        self.decshape = nn.Linear(1024, 10)
        self.deccam = nn.Linear(1024, 3)
        nn.init.xavier_uniform_(self.decpose.weight, gain=0.01)
        nn.init.xavier_uniform_(self.decshape.weight, gain=0.01)
        nn.init.xavier_uniform_(self.deccam.weight, gain=0.01)
        self.smpl = smpl if smpl is not None else SMPL(SMPL_MODEL_DIR, batch_size=64, create_transl=False)
        for m in self.modules():                                   # spin.py:94-100
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, np.sqrt(2. / n))
        mean_params = smpl_mean_params if isinstance(smpl_mean_params, dict) else np.load(smpl_mean_params)
        self.register_buffer('init_pose', torch.from_numpy(np.asarray(mean_params['pose'][:], dtype=np.float32)).unsqueeze(0))
        self.register_buffer('init_shape', torch.from_numpy(np.asarray(mean_params['shape'][:]).astype('float32')).unsqueeze(0))
        self.register_buffer('init_cam', torch.from_numpy(np.asarray(mean_params['cam'], dtype=np.float32)).unsqueeze(0))
        object.__setattr__(self, '_engine', Engine(1, 64, kind='hmr'))

    def conv_bn_pairs(self):
        """(conv, bn) of the 53 convolutions in state-dict order: the order tepose_pack_hmr_backbone takes them in."""
        pairs = [(self.conv1, self.bn1)]
        for i in range(len(_STAGES)):
            for blk in getattr(self, 'layer%d' % (i + 1)):
                pairs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
                if hasattr(blk, 'downsample'):
                    pairs.append((blk.downsample[0], blk.downsample[1]))
        return pairs

    def _check(self, x):
        warn_if_training(self, x)
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (3, HMR_IMAGE, HMR_IMAGE):
            raise ValueError('input must be a [N, 3, %d, %d] tensor (AvgPool2d(7) + view + fc1, lib/models/spin.py:76,139-140, accept no other size), got %s'
                             % (HMR_IMAGE, HMR_IMAGE, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        if not x.is_cuda:
            raise RuntimeError('tepose_amd runs on MI355X only: move the model and input to a cuda device')
        return x.float().contiguous()

    def feature_extractor(self, x):
        x = self._check(x)
        eng = self._engine
        with on_device(x.device):
            eng.pack_backbone(self, x.device)
            return eng.hmr_features(x)

    def features_from_frames(self, frames_u8, frame_index, bboxes, scale=1.2):
        """The reference's CropDataset + feature loop (demo.py:171-198): frames_u8 [F,H,W,3] torch.uint8 cuda (RGB), frame_index int[n],
        bboxes [n,4] (c_x, c_y, w, h) -> [n,2048].  Crops (tepose_amd.crop, 224 x 224 at `scale`) and extracts in passes of 64 through one
        reused [64,3,224,224] buffer: a 1 000-frame tracklet never holds 600 MB of crops.  A row equals
        `feature_extractor(crop_frames(...))`'s: in split mode bit for bit (rows do not depend on the pass they ride in)."""
        from . import crop as C
        warn_if_training(self, frames_u8)
        C.check_frames(frames_u8)
        idx = C.check_index(frame_index, int(frames_u8.shape[0]))
        _, minv = C.crop_transform(C.check_boxes(bboxes, idx.shape[0]), scale, HMR_IMAGE)
        frames_u8 = C.on_gpu(frames_u8)
        n, dev, eng = idx.shape[0], frames_u8.device, self._engine
        feats = torch.empty((n, 2048), dtype=torch.float32, device=dev)
        if n == 0:
            return feats
        buf = torch.empty((min(n, HMR_PASS), 3, HMR_IMAGE, HMR_IMAGE), dtype=torch.float32, device=dev)
        with on_device(dev):
            eng.pack_backbone(self, dev)
            for i in range(0, n, HMR_PASS):
                k = min(HMR_PASS, n - i)
                C.crop_into(frames_u8, idx[i:i + k], minv[i:i + k], HMR_IMAGE, buf[:k], None)
                feats[i:i + k] = eng.hmr_features(buf[:k])
        return feats

    def forward(self, x, init_pose=None, init_shape=None, init_cam=None, n_iter=3, return_features=False):
        x = self._check(x)
        eng = self._engine
        with on_device(x.device):
            eng.pack_backbone(self, x.device)
            eng.pack_regressor(self, x.device)
            xf = eng.hmr_features(x)
            out = eng.regressor_fwd(xf, n_iter, None, init=(init_pose, init_shape, init_cam))
        out.pop('rotmat')                                          # spin.py:196-201: theta, verts, kp_2d, kp_3d
        return (xf, [out]) if return_features else [out]


_warned_imagenet = [False]


def hmr(smpl_mean_params=SMPL_MEAN_PARAMS, pretrained=True, **kwargs):
    """lib/models/spin.py:294-304 without its download: with `pretrained`, ImageNet ResNet-50 weights are taken from the local torch
    hub checkpoint directory (`resnet50-*.pth`) when a file is there; otherwise that initialisation is skipped with one warning --
    both reference callers overwrite every backbone weight with the SPIN checkpoint on their next line (demo.py:116-121)."""
    model = HMR(None, [3, 4, 6, 3], smpl_mean_params, **kwargs)
    if pretrained:
        import glob
        from torch.hub import get_dir
        found = sorted(glob.glob(os.path.join(get_dir(), 'checkpoints', 'resnet50-*.pth')))
        if found:
            from .data import load_checkpoint
            model.load_state_dict(load_checkpoint(found[0]), strict=False)
        elif not _warned_imagenet[0]:
            _warned_imagenet[0] = True
            warnings.warn('tepose_amd.hmr: no resnet50-*.pth in %s -- the ImageNet initialisation is skipped (nothing is downloaded); '
                          'load a SPIN checkpoint next, as the reference callers do' % os.path.join(get_dir(), 'checkpoints'), RuntimeWarning)
    return model


def get_pretrained_hmr():
    """lib/models/spin.py:354-360: hmr() with the SPIN checkpoint's 'model' entry loaded non-strictly, in eval mode."""
    from .data import load_checkpoint
    from .smpl import BASE_DATA_DIR
    model = hmr().to('cuda')
    checkpoint = load_checkpoint(os.path.join(BASE_DATA_DIR, 'spin_model_checkpoint.pth.tar'))
    model.load_state_dict(checkpoint['model'], strict=False)
    model.eval()
    return model
