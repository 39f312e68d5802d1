"""Whole-batch comparisons against the fp64 oracle on batches built for it (helper module of tests/test_gpu_all_rows.py, tests/test_all_rows_helper.py and
tests/_fuzz_parity.py; not a conftest, not collected).

The oracle cannot afford 8192 windows of the published architecture, but it can afford 128.  A batch whose B rows are copies of D distinct windows has
an fp64 answer for EVERY row after one oracle run on the D windows -- so a fault that is local to one row tile, one unit tile, the second tile a
workgroup takes or a stale ring slot shows up as rows over tolerance, with their indices.

Why the replication does not hide a row mix-up: `assignment` lays the windows out as independent permutations of range(D), one per aligned block of D
rows.  A row that received another row's data fails unless that other row happens to hold the same window: 1 in D per row, and independently so in every
D-block, because the blocks are different permutations (a fault that repeats per tile would have to hit a copy in every tile).  That argument needs the
distinct windows' outputs to be far apart compared with the tolerance; `assert_separated` checks it for the D windows of every case.

What replication cannot see at all: a row overwritten by ANOTHER COPY OF THE SAME WINDOW (tests/test_all_rows_helper.py plants one and shows that it
passes)."""
from collections import namedtuple

import numpy as np
import torch

from tepose_amd import synth

TILE = 128            # rows of the large-batch kernels' row tile (gemm_h3s_persist16c_kernel, gru_step16_kernel)

Report = namedtuple('Report', 'name rows worst row tile window n_over tol bad_tiles')


def assignment(B, D, seed):
    """int64[B]: the source window of every row -- concatenated independent fixed-seed permutations of range(D), cut to B.  Every window occurs (B >= D),
    the D rows from any multiple of D on are all different, and no two aligned D-blocks are the same permutation."""
    assert B >= D >= 2, (B, D)
    rng = np.random.RandomState(seed)
    blocks, seen = [], set()
    while len(blocks) * D < B:
        p = rng.permutation(D)
        if p.tobytes() in seen:          # (D! orders: only a tiny D can draw one twice)
            continue
        seen.add(p.tobytes())
        blocks.append(p)
    return np.concatenate(blocks)[:B].astype(np.int64)


def replicated_windows(B, T, D, seed, device):
    """(x [B, T, 2133] on `device`, the D distinct windows as numpy [D, T, 2133], src int64[B]): synth.synthetic_windows(D, T, seed) uploaded once and
    gathered on the device (the benchmark shape is 1.1 GB: never built on the host)."""
    xw = synth.synthetic_windows(D, T, seed)
    src = assignment(B, D, seed)
    x = torch.from_numpy(xw).to(device)[torch.from_numpy(src).to(device)].contiguous()
    return x, xw, src


def _rows64(a, device):
    a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device).reshape(a.shape[0], -1)


def compare_all_rows(got, ref, src, tol, name='', raise_on_fail=True, chunk=1024):
    """got [B, ...] against ref [D, ...][src], every row, in float64 on got's device.  Returns a Report: the worst absolute error, the row it is in, that
    row's 128-row tile and source window, the number of rows that are not < tol (a NaN counts), and the tiles those rows lie in.  Raises AssertionError
    with all of that unless raise_on_fail is False -- a failure has to say WHERE, since locality is the finding."""
    dev = got.device
    B = got.shape[0]
    src_t = torch.as_tensor(np.asarray(src), dtype=torch.int64, device=dev)
    assert src_t.shape == (B,) and tuple(got.shape[1:]) == tuple(ref.shape[1:]), (name, tuple(got.shape), tuple(ref.shape), tuple(src_t.shape))
    g, r = _rows64(got, dev), _rows64(ref, dev).double()
    err = torch.empty(B, dtype=torch.float64, device=dev)
    for a in range(0, B, chunk):
        e = (g[a:a + chunk].double() - r[src_t[a:a + chunk]]).abs().amax(1)
        err[a:a + chunk] = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)
    bad = torch.nonzero(~(err < tol)).flatten()
    row = int(err.argmax())
    rep = Report(name, B, float(err[row]), row, row // TILE, int(src_t[row]), int(bad.numel()), tol,
                 sorted(set((bad // TILE).tolist())))
    if raise_on_fail and rep.n_over:
        raise AssertionError(describe(rep))
    return rep


def describe(rep):
    s = '%s: worst |got - fp64| = %.3e in row %d (128-row tile %d, source window %d); %d of %d rows not < %g' % (
        rep.name, rep.worst, rep.row, rep.tile, rep.window, rep.n_over, rep.rows, rep.tol)
    if rep.bad_tiles:
        s += '; tiles with such rows: %s%s' % (rep.bad_tiles[:16], ' ...' if len(rep.bad_tiles) > 16 else '')
    return s


def _copy_groups(src):
    """Rows grouped by how many earlier rows hold the same window: inside one group every window occurs at most once."""
    src = np.asarray(src)
    order = np.argsort(src, kind='stable')
    first = np.r_[0, np.nonzero(np.diff(src[order]))[0] + 1]
    rank = np.empty(len(src), dtype=np.int64)
    rank[order] = np.arange(len(src)) - np.repeat(first, np.diff(np.r_[first, len(src)]))
    return [np.nonzero(rank == k)[0] for k in range(int(rank.max()) + 1)]


def copies_spread(got, src):
    """max over windows of the max abs difference between the copies of one window (0.0: the copies agree in value everywhere; NaN if any is NaN)."""
    dev = got.device
    g = got.reshape(got.shape[0], -1)
    D = int(np.asarray(src).max()) + 1
    hi = torch.full((D, g.shape[1]), float('-inf'), dtype=g.dtype, device=dev)
    lo = torch.full((D, g.shape[1]), float('inf'), dtype=g.dtype, device=dev)
    for rows in _copy_groups(src):
        rows_t = torch.from_numpy(rows).to(dev)
        w = torch.as_tensor(np.asarray(src)[rows], device=dev)
        hi[w] = torch.maximum(hi[w], g[rows_t])
        lo[w] = torch.minimum(lo[w], g[rows_t])
    return float((hi - lo).max())


def copies_bit_identical(got, src):
    """Every copy of a window equals the first copy of that window bit for bit (float32 words compared as integers)."""
    src = np.asarray(src)
    first = np.zeros(int(src.max()) + 1, dtype=np.int64)
    windows, rows = np.unique(src, return_index=True)          # the first row of every window
    first[windows] = rows
    g =got.reshape(got.shape[0], -1).contiguous().view(torch.int32)
    return bool(torch.equal(g, g[torch.from_numpy(first[src]).to(got.device)]))


# ---- the distinct windows must be far apart -------------------------------------------------------------------------------------------------------
# Smallest separation (min over pairs of windows of the max abs difference of their fp64 outputs) as a multiple of the comparison's tolerance.  With
# these, a swapped row cannot pass on any compared output and fails by a wide margin on two.  A case that does not reach them gets another seed or D.
SEPARATION = {'feature': 1000.0, 'feature_train': 1000.0, 'verts': 50.0}
SEPARATION_OTHER = 2.0


def separation(ref):
    """min over pairs (i != j) of max |ref[i] - ref[j]|."""
    r = _rows64(ref, 'cpu').double()
    best = float('inf')
    for i in range(r.shape[0] - 1):
        best = min(best, float((r[i + 1:] - r[i]).abs().amax(1).min()))
    return best


def assert_separated(refs, tols):
    """refs: name -> fp64 oracle output [D, ...]; tols: name -> tolerance of its comparison.  Returns name -> separation / tolerance."""
    out = {}
    for k, ref in refs.items():
        ratio = separation(ref) / tols[k]
        need = SEPARATION.get(k, SEPARATION_OTHER)
        assert ratio >= need if k in SEPARATION else ratio > need, \
            'distinct windows too close on %s: separation %.1f x tolerance, need %g x (change the seed or D, not this)' % (k, ratio, need)
        out[k] = ratio
    return out
