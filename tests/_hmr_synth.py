"""Seeded synthetic weights, batch-norm statistics and images for the HMR backbone tests and their fixture generator
(tests/golden/make_golden_hmr.py).  One numpy Generator per tensor, keyed by (seed, tensor name): a tensor's values do not depend on
which other tensors were drawn.  Shapes come from the state dict the caller passes in, so nothing here lists the network.

Recipe (chosen so that the reference's own activations stay O(1 - 100) through 16 residual blocks and its fp32 run stays within a
quarter of the 1e-4 parity budget of its fp64 run -- the generator asserts both):
  conv weight      He-normal over the fan-in
  bn weight        U(0.5, 1.5); the last batch norm of every block (bn3) and the downsample one x 0.35 / x 0.7, so the residual sum does not grow
  bn bias          N(0, 0.3)
  running_mean     N(0, 0.3)
  running_var      U(0.5, 2.0)
  head             the synthetic regressor of tepose_amd.synth (fc1 .. deccam, init_*), as the Regressor fixtures use it
  images           N(0, 1) clipped to the range of ImageNet-normalised pixels, [-2.12, 2.64]
"""
import zlib

import numpy as np

from tepose_amd import synth

SEED_W, SEED_X = 11, 12


def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def backbone_tensor(name, shape, seed=SEED_W):
    """The synthetic value of one backbone state-dict entry (None for `num_batches_tracked`)."""
    g = _rng(seed, name)
    leaf = name.rsplit('.', 1)[-1]
    owner = name.rsplit('.', 1)[0]
    if leaf == 'num_batches_tracked':
        return None
    if len(shape) == 4:                                           # convolution, OIHW
        fan_in = shape[1] * shape[2] * shape[3]
        return (g.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    if leaf == 'weight':
        scale = 0.35 if owner.endswith('bn3') else (0.7 if owner.endswith('downsample.1') else 1.0)
        return (g.uniform(0.5, 1.5, shape) * scale).astype(np.float32)
    if leaf in ('bias', 'running_mean'):
        return (g.standard_normal(shape) * 0.3).astype(np.float32)
    if leaf == 'running_var':
        return g.uniform(0.5, 2.0, shape).astype(np.float32)
    raise KeyError(name)


def is_backbone_key(k):
    return k.startswith(('conv1.', 'bn1.', 'layer'))


def state_dict_np(shapes, seed=SEED_W):
    """{name: array} for every entry of `shapes` ({name: shape}, an HMR state dict's) that the recipe covers: the backbone and the head."""
    head = {k[len('regressor.'):]: v for k, v in synth.synthetic_state_dict(1, 64, seed).items() if k.startswith('regressor.')}
    out = {}
    for k, shp in shapes.items():
        if is_backbone_key(k):
            v = backbone_tensor(k, tuple(shp), seed)
            if v is not None:
                out[k] = v
        elif k in head and tuple(head[k].shape) == tuple(shp):
            out[k] = head[k]
    return out


def images(n, seed=SEED_X):
    g = _rng(seed, 'images')
    return np.clip(g.standard_normal((n, 3, 224, 224)), -2.12, 2.64).astype(np.float32)


def init_state(n, seed=SEED_X):
    """Caller-given initial pose (6D) / shape / camera rows around the synthetic mean parameters."""
    mean = synth.synthetic_mean_params(0)
    g = _rng(seed, 'init')
    pose = np.asarray(mean['pose'], dtype=np.float32)[None] + 0.15 * g.standard_normal((n, 144)).astype(np.float32)
    shape = 0.5 * g.standard_normal((n, 10)).astype(np.float32)
    cam = np.array([0.9, 0., 0.], dtype=np.float32)[None] + 0.1 * g.standard_normal((n, 3)).astype(np.float32)
    return pose.astype(np.float32), shape, cam.astype(np.float32)
