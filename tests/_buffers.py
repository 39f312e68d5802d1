"""Poisoned, guarded buffers for the tests of the buffer contract (include/tepose_amd.h, conventions): a forward's results do not depend on what its
workspace held before, and it writes only inside [workspace, workspace + bytes) and inside the first B rows of each output.

A buffer handed to the library is a view into the MIDDLE of a larger allocation whose two ends -- the guards -- hold a byte no pattern uses; after
the call every guard byte is compared.  Nothing here needs a GPU: tests/test_buffers_helper.py runs the same code on CPU tensors.

Guard sizes are derived from what the kernels can do wrong, not guessed: a kernel that ignores the row count of its last tile writes at most one
whole row tile past (or before) the owned rows, and the widest row tile of any kernel here is 128 rows.
  workspace: the widest buffer a forward carves is a gate pre-activation matrix of 9 Hp fp32 columns (csrc/state.h g0), so
             guard = 128 rows x 9 Hp columns x 4 bytes                                                        (workspace_guard_bytes)
  outputs:   guard = 128 rows of that output                                                                  (GUARD_ROWS)"""
import torch

GUARD_ROWS = 128             # the tallest row tile of any kernel (gemm_h3 / gemm_h3s / gru_step16: 128 rows)
GUARD_BYTE = 0xA5            # differs from every byte of every pattern below
PATTERNS = {
    'zeros': (0x00, 0x00),   # what a fresh allocation often holds: the case every other test sees
    'ones': (0xFF, 0xFF),    # NaN as fp32 and as fp16; all-ones as a counter, tag or index
    'finite': (0x00, 0x3C),  # little-endian 0x3C00 repeated: 1.0 as fp16, 0.0078... (0x3C003C00) as fp32
}
assert all(GUARD_BYTE not in p for p in PATTERNS.values())


def workspace_guard_bytes(Hp):
    """One full 128-row tile of the widest workspace buffer: 128 x 9 Hp x 4 bytes, Hp = the hidden size rounded up to 64 (Engine.gate_width / 9): a
    multiple of 256."""
    return GUARD_ROWS * 9 * int(Hp) * 4


class Guard:
    """`base`: the whole uint8 allocation; the owned region is base[lo:hi]."""

    def __init__(self, base, lo, hi, name):
        self.base, self.lo, self.hi, self.name = base, lo, hi, name

    def changed(self):
        """Byte offsets RELATIVE TO THE OWNED REGION of the first and the last changed guard byte (negative: in front of it; >= hi - lo: behind it), and
        how many changed; None if both guards are intact."""
        bad = []
        for a, b in ((0, self.lo), (self.hi, self.base.numel())):
            idx = (self.base[a:b] != GUARD_BYTE).nonzero().flatten()
            if idx.numel():
                bad.append((int(idx[0]) + a - self.lo, int(idx[-1]) + a - self.lo, int(idx.numel())))
        if not bad:
            return None
        return bad[0][0], bad[-1][1], sum(n for _, _, n in bad)


def _fill(base, lo, hi, pattern):
    base.fill_(GUARD_BYTE)
    b0, b1 = PATTERNS[pattern]
    own = base[lo:hi]
    if b0 == b1:
        own.fill_(b0)
        return
    n2 = (hi - lo) // 2 * 2                              # (lo is a multiple of 256: the 16-bit view is aligned)
    v16 = b0 | b1 << 8
    own[:n2].view(torch.int16).fill_(v16 - 65536 if v16 >= 32768 else v16)
    if n2 != hi - lo:
        own[n2] = b0


def poisoned(nbytes, pattern, device, guard_bytes=workspace_guard_bytes(1024), name='workspace'):
    """A workspace of exactly `nbytes` filled with `pattern`: a view at an offset that is a multiple of 256 into a larger uint8 allocation whose
    guards -- at least `guard_bytes` (rounded up to 256) on each side -- hold GUARD_BYTE.  The view carries its Guard as `.guard`.  (The device
    allocator hands out 256-byte-aligned blocks; a host allocation may not be one: the offset then grows by what brings the ADDRESS to a multiple of
    256, which is what the library's carve relies on.)"""
    g = (int(guard_bytes) + 255) // 256 * 256
    base = torch.empty(g + int(nbytes) + g + 256, dtype=torch.uint8, device=device)
    lo = g + (-base.data_ptr()) % 256
    _fill(base, lo, lo + int(nbytes), pattern)
    ws = base[lo:lo + int(nbytes)]
    assert ws.data_ptr() % 256 == 0
    ws.guard = Guard(base, lo, lo + int(nbytes), '%s (%s)' % (name, pattern))
    return ws


def refill(ws, pattern):
    """The same workspace again, with another pattern (guards rewritten too)."""
    _fill(ws.guard.base, ws.guard.lo, ws.guard.hi, pattern)
    ws.guard.name = ws.guard.name.split(' (')[0] + ' (%s)' % pattern
    return ws


def untouched(ws):
    """True if the workspace still holds, byte for byte, the pattern it was last filled with: the call under test did not use it at all."""
    b0, b1 = PATTERNS[ws.guard.name.rsplit('(', 1)[1][:-1]]
    return bool((ws[0::2] == b0).all()) and bool((ws[1::2] == b1).all())


def guarded_like(shape, B, device, name='out', guard_rows=GUARD_ROWS, dtype=torch.float32):
    """An output tensor of trailing shape shape[1:] whose rows [0, B) are owned: a contiguous row slice of a larger tensor with `guard_rows` guard rows
    in front of them and behind them.  The returned view STARTS at the first owned row and keeps the tail guard rows (shape[0] = B + guard_rows): what
    Engine._out_views takes as "a tensor whose first B rows are written"; `.own` is the [B, ...] slice, `.guard` the Guard."""
    tail = tuple(int(s) for s in shape[1:])
    esz = torch.empty((), dtype=dtype).element_size()
    row = esz
    for s in tail:
        row *= s
    G, B = int(guard_rows), int(B)
    base = torch.empty((G + B + G) * row, dtype=torch.uint8, device=device)
    base.fill_(GUARD_BYTE)
    base[G * row:(G + B) * row] = 0xFF                   # owned rows start as NaN: a row the forward leaves out shows
    t = base[G * row:].view(dtype).view((B + G,) + tail)
    assert t.is_contiguous()
    t.guard = Guard(base, G * row, (G + B) * row, name)
    t.own = t[:B]
    return t


def guards_of(*things):
    """The Guards of tensors made here (dicts and lists of them and None are accepted)."""
    out = []
    for t in things:
        if t is None:
            continue
        if isinstance(t, dict):
            out += guards_of(*t.values())
        elif isinstance(t, (list, tuple)):
            out += guards_of(*t)
        elif isinstance(t, Guard):
            out.append(t)
        else:
            out.append(t.guard)
    return out


def assert_guards_intact(*things, what=''):
    """Bitwise check of every guard; a failure names the buffer and the first and last changed byte offsets relative to its owned region."""
    for g in guards_of(*things):
        c = g.changed()
        assert c is None, ('%s: %s written outside its owned %d bytes: %d guard bytes changed, first at offset %d, last at offset %d'
                           % (what, g.name, g.hi - g.lo, c[2], c[0], c[1]))


def same_bits(a, b):
    """Bitwise equality (NaN == NaN of the same payload, -0.0 != 0.0), for tensors of one dtype and shape."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Frozen:
    """Clones of a call's inputs, taken before it: a forward never writes its inputs."""

    def __init__(self, **tensors):
        self.live = {k: t for k, t in tensors.items() if t is not None}
        self.copy = {k: t.clone() for k, t in self.live.items()}

    def assert_unchanged(self, what=''):
        for k, t in self.live.items():
            assert same_bits(t, self.copy[k]), '%s: input %r was written' % (what, k)
