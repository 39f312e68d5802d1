"""The window ops of a multi-person live session (csrc/session.hip) restated in numpy: what tepose_session_advance and
tepose_session_commit must produce, bit for bit -- they only move fp32 values.  No GPU needed."""
import numpy as np

HOLD, ADVANCE, JOIN, CLEAR = 0, 1, 2, 3


def advance(win, ops, feat, hist=None):
    """win [S,T,2133], ops [S], feat [S,2048], hist [S,T-1,2133] or None -> (new win, saved).  `saved` is every window as it stood; any op
    code outside 1 .. 3 holds, and so does a join without hist."""
    win = np.asarray(win, dtype=np.float32)
    S, T, W = win.shape
    assert W == 2133 and T >= 2 and len(ops) == S and feat.shape == (S, 2048)
    saved, new = win.copy(), win.copy()
    for s in range(S):
        op = int(ops[s])
        if op == JOIN and hist is None:
            op = HOLD
        if op == ADVANCE:
            new[s, :T - 1] = win[s, 1:]
        elif op == JOIN:
            new[s, :T - 1] = hist[s]
        elif op == CLEAR:
            new[s] = 0
        if op in (ADVANCE, JOIN):
            new[s, T - 1, :2048] = feat[s]
            new[s, T - 1, 2048:] = 0
    return new, saved


def commit(win, ops, theta):
    """theta [S,85] -> the newest row's theta columns of the slots that advanced or joined; nothing else changes."""
    new = np.array(win, dtype=np.float32, copy=True)
    for s in range(new.shape[0]):
        if int(ops[s]) in (ADVANCE, JOIN):
            new[s, -1, 2048:] = theta[s]
    return new


def random_case(S, T, seed, shift=0):
    """Windows, ops (all four codes and out-of-range ones, in random places), features, history, theta: finite values and a few odd bit patterns
    (-0.0, a denormal, inf, NaN), which a copy must carry unchanged."""
    g = np.random.default_rng(seed)
    win = g.standard_normal((S, T, 2133)).astype(np.float32)
    feat = g.standard_normal((S, 2048)).astype(np.float32)
    hist = g.standard_normal((S, T - 1, 2133)).astype(np.float32)
    theta = g.standard_normal((S, 85)).astype(np.float32)
    odd = np.array([-0.0, 1e-42, np.inf, np.nan], dtype=np.float32)
    for a in (win, feat, hist, theta):
        flat = a.reshape(-1)
        flat[g.integers(0, flat.size, 8)] = odd[g.integers(0, 4, 8)]
    codes = np.array([0, 1, 2, 3, 4, -1, 7, 1 << 20], dtype=np.int32)
    ops = codes[(g.permutation(S) + shift) % len(codes)].copy()      # S >= 8: every code; below: `shift` 0 .. 7 walks each slot through all of them
    return win, ops, feat, hist, theta


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
