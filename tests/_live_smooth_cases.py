"""The feeds of tests/test_gpu_live_smooth.py, in a module of their own so that one and the same feed can be run on two builds (the digests of the
unsmoothed sessions in profiles/live_smoothing.txt were made with these functions on the parent commit's tree).  S = 3 slots, seqlen 4, 6 ticks:

    tick      0    1    2    3    4    5
    slot 0    A    A    A    A    A    A          A: joins at tick 0
    slot 1    B    -    B    .    C    C          B: joins at tick 0, has no feature at tick 1 (held), leaves after tick 2; C takes the slot at tick 4
    slot 2    .    .    .    .    .    .          idle throughout

Nothing here names `smooth` unless it is asked for: the parent's constructors do not know the argument."""
import hashlib

import numpy as np
import torch

from tepose_amd import synth

T, S, TICKS = 4, 3, 6
SLOT = {'A': 0, 'B': 1, 'C': 1}
PRESENT = {'A': (0, 1, 2, 3, 4, 5), 'B': (0, 2), 'C': (4, 5)}
JOIN = {'A': 0, 'B': 0, 'C': 4}
LEAVE = {'B': 3}                                  # before the push of this tick
SEED = {'A': 411, 'B': 412, 'C': 413}
KEYS = ('theta', 'kp_3d', 'verts', 'kp_2d')


def clip(person):
    """features [TICKS, 2048] (row = tick) and the history (features [T-1, 2048], theta [T-1, 85]) of a person."""
    w = synth.synthetic_windows(1, TICKS + T - 1, SEED[person])[0]
    return torch.from_numpy(w[T - 1:, :2048].copy()), (torch.from_numpy(w[:T - 1, :2048].copy()), torch.from_numpy(w[:T - 1, 2048:].copy()))


def feature_run(model, graph=True, **kw):
    """The schedule above on a MultiStreamSession(model, T, S, keep=KEYS, graph=graph, **kw).  -> {person: {key: [ticks present, ...]}}, the session."""
    from tepose_amd.stream import MultiStreamSession
    ses = MultiStreamSession(model, T, S, keep=KEYS, graph=graph, **kw)
    clips = {p: clip(p) for p in SLOT}
    rows = {p: {k: [] for k in KEYS} for p in SLOT}
    for j in range(TICKS):
        for p, t in LEAVE.items():
            if t == j:
                ses.leave(SLOT[p])
        for p, t in JOIN.items():
            if t == j:
                ses.join(SLOT[p], *clips[p][1])
        fed = [p for p in SLOT if j in PRESENT[p]]
        out = ses.push({SLOT[p]: clips[p][0][j] for p in fed})
        assert sorted(out) == sorted(SLOT[p] for p in fed), j
        for p in fed:
            for k in KEYS:
                rows[p][k].append(out[SLOT[p]][k].clone())
    return {p: {k: torch.stack(v) for k, v in d.items()} for p, d in rows.items()}, ses


# ------------------------------------------------------------------ from pixels: two ragged tracklets
H, W, NF, SCALE = 96, 128, 12, 1.2
PIXEL_KEYS = ('theta', 'kp_3d', 'verts')


def box(person, f):
    """Person `person`'s box in frame f: 40 - 70 px, w != h, drifting."""
    cx, cy, w, h = [(38.3, 44.6, 41.0, 62.5), (96.7, 51.2, 55.4, 47.9)][person]
    return np.array([cx + 1.9 * f, cy + 0.8 * f, w + 0.7 * f, h + 0.4 * f])


def frames():
    return torch.from_numpy(np.random.default_rng(18).integers(0, 256, (NF, H, W, 3), dtype=np.uint8))


def tracks():
    """A: frames 0 .. 11 in slot 0.  B: frames 3 .. 10 in slot 1 with no box in frame 8 (held there)."""
    fa, fb = np.arange(0, 12), np.array([3, 4, 5, 6, 7, 9, 10])
    return {'A': {'frames': fa, 'bbox': np.stack([box(0, f) for f in fa])}, 'B': {'frames': fb, 'bbox': np.stack([box(1, f) for f in fb])}}


def pixel_run(model, hmr, vibe, frames_u8, **kw):
    """The two tracklets on a PixelSession of 2 slots: per person the bootstrap rows of join_from_frames, then its tick rows, as one sequence.
    -> {person: {key: numpy [frames of the tracklet, ...]}} with the keys PIXEL_KEYS, 'orig_cam', 'bbox'."""
    from tepose_amd.live import PixelSession
    ses = PixelSession(model, hmr, vibe, T, 2, frame_size=(H, W), bbox_scale=SCALE, keep=PIXEL_KEYS, **kw)
    tr, slot = tracks(), {'A': 0, 'B': 1}
    rows = {p: [] for p in tr}

    def take(p, o):
        rows[p].append({k: np.array(torch.as_tensor(o[k]).numpy(), copy=True) for k in PIXEL_KEYS + ('orig_cam', 'bbox')})

    for f in range(NF):
        for p, t in tr.items():
            if f == t['frames'][T - 1]:
                first = t['frames'][:T - 1]
                boot = ses.join_from_frames(slot[p], frames_u8[first], t['bbox'][:T - 1])
                for j in range(T - 1):
                    take(p, {k: boot[k][j] for k in boot})
        fed = {p: t['bbox'][list(t['frames']).index(f)] for p, t in tr.items() if f in t['frames'][T - 1:]}
        if not fed:
            continue
        out = ses.push(frames_u8[f], {slot[p]: b for p, b in fed.items()})
        for p in fed:
            take(p, out[slot[p]])
    return {p: {k: torch.from_numpy(np.stack([r[k] for r in rows[p]])) for k in rows[p][0]} for p in tr}


def digest(rows):
    """sha256 over every person's rows, key by key, as the raw bytes of their own type."""
    h = hashlib.sha256()
    for p in sorted(rows):
        for k in sorted(rows[p]):
            h.update(np.ascontiguousarray(rows[p][k].numpy()).tobytes())
    return h.hexdigest()
