"""Live-stream sessions: frames arrive one at a time (BASELINE.json config 5; reference loop: demo.py:238-252).

The reference's demo slides a `seqlen` window over one tracked person: window k holds the features of frames k .. k+seqlen-1
and, in its theta slots, the predictions of the first seqlen-1 of them (the newest frame's slots are zero); the prediction for
the newest frame is appended to the theta history and the window moves on by one frame.  `tepose_amd.driver.run_clips` runs
that loop when the whole clip is known up front.  A live stream is not: frames ARRIVE, and what matters is the time from a
frame's arrival on the host to its result being readable on the host.

A session owns its windows on the device, pinned staging for what arrives and pinned result rows; one `push` is one TICK --
upload, window shift, forward, theta into the history, D2H of the kept outputs -- queued as ONE captured hipGraph replay and
followed by one event wait.  No allocation and no host sync inside; the forward inside the graph is the same C entry point on
the same operands as the eager driver, so the results are bit-identical to `run_clips` (tests/test_gpu_stream.py).

`_Session` is everything that is not "what a tick does", written once: construction (the session's own stream and workspace),
the weight watch, the captured graphs, the warm-up and the run loop with its recovery.  `StreamSession` (one person, the torch
copy chain at B = 1), `MultiStreamSession` (S slots, csrc/session.hip) and `tepose_amd.live.PixelSession` (the same from
pixels) each supply a tick.

Failure contract (include/tepose_amd.h, "failure channel"): a replayed graph is not status-checked by `Engine._run`, so the run
loop reads the handle's fault word (one host-memory read) after its wait; on a give-up the model is switched to the
step-per-launch kernels, the windows are restored, the graph is re-captured and the tick is run again -- never a NaN result.
"""

import math
import operator

import torch

from . import _lib
from .engine import NUM_VERTS, OUT_TAILS, n_joints, on_device, out_shapes

# the per-push weight check reads both of every watched tensor (~0.1 us each): C-level getters, mapped without a Python frame per tensor
_VERSION, _ADDRESS = operator.attrgetter('_version'), torch.Tensor.data_ptr


class _Session:
    """What every live session shares.  A subclass checks its arguments, calls `__init__` (device, stream, pack, workspace), makes
    its buffers and calls `_warm_up`; it supplies `_tick(variant)` -- one tick queued on the current stream as a single chain, what a
    graph captures -- and `_restore()`, which puts its windows back from `saved`.  It may extend `_pack` (the full weight check) and
    `_signature` (what a captured graph depends on)."""

    def __init__(self, model, batch, seqlen, J_regressor, keep, graph):
        self.model, self.T, self.J, self.keep, self.use_graph = model, int(seqlen), J_regressor, tuple(keep), bool(graph)
        self.eng, self.dev, self._batch = model._engine, next(model.parameters()).device, int(batch)
        self.stream = torch.cuda.Stream(device=self.dev)      # non-blocking: nothing orders it after the caller's stream implicitly
        self._on_stream = torch.cuda.stream(self.stream)      # entered once per push (never nested): made once, off the frame's critical path
        self.done = torch.cuda.Event()
        self.graphs = {}                                    # variant (what a tick uploads, e.g. 'host') -> captured tick
        self._captured_for = None
        self._pushes_since_full = 0
        with torch.no_grad():
            self._pack()                                      # on the caller's stream; the workspace size depends on what is packed
        # A workspace of the session's own: a captured graph bakes its address into every kernel argument (the status words the run
        # loop reads live in it too), and the engine's shared workspace moves whenever another call on the model needs more bytes or
        # the weights are re-packed.  Two sessions on one model do not share scratch either.
        self.ws = torch.empty(self.eng.workspace_bytes(self._batch, self.T), dtype=torch.uint8, device=self.dev)

    def _warm_up(self):
        """Last step of construction: one eager tick (packed blob, workspace and caches settle; a subclass may create its pinned result
        rows in it), retried once after a give-up, which has switched the model to the step kernels (warned); the windows are put
        back; with graph=True the 'host' tick is captured."""
        eng = self.eng
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))      # the subclass's buffers were filled on the caller's stream
        with torch.no_grad(), torch.cuda.stream(self.stream), eng.use_workspace(self.ws):
            for attempt in (0, 1):
                with eng.lazy_status():
                    self._tick('host')
                self.stream.synchronize()
                try:
                    eng.check_status()
                    break
                except _lib.TeposeTimeout:
                    if attempt:
                        raise
                finally:
                    self._restore()
            self._captured_for = self._signature()
            if self.use_graph:
                self._capture('host')
        self.stream.synchronize()

    def _cheap_sig(self):
        return list(map(_VERSION, self._watch)), list(map(_ADDRESS, self._watch))

    def _pack(self):
        """The full weight check, on the current stream: the engine re-fetches every tensor from its module by name (~35 us) and
        re-packs what changed -- a no-op while its signatures stand; the watch list is taken anew."""
        self.eng.pack_model(self.model, self.dev)
        self._watch = self.eng.watched_tensors(self.model)
        self._watch_sig = self._cheap_sig()

    def _signature(self):
        eng = self.eng
        return (eng.packed_generation, eng.blob.data_ptr() if eng.blob is not None else 0, self.ws.data_ptr())

    def _refresh(self, variant):
        """Before a tick, graph and eager sessions alike.  Re-pack if the model's parameters changed in place since the last pack --
        outside any capture: a replay would go on using the old packed blob without a sign.  Grow the workspace if the packed model now
        needs more, drop graphs captured against another blob or workspace, capture the variant this tick needs.

        Per push, on the frame's critical path: the in-place version counter and the address of every watched tensor (an address moves
        without a version bump under `p.data = ...`).  The full check runs when those moved, and every 32nd push as a backstop for what
        they cannot show (a parameter OBJECT replaced by assignment); it waits for the caller's current stream first, where the change
        was queued."""
        self._pushes_since_full += 1
        if self._cheap_sig() != self._watch_sig or self._pushes_since_full >= 32:
            self._pushes_since_full = 0
            self.stream.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(self.stream):
                self._pack()
        if self._signature() != self._captured_for:
            need = self.eng.workspace_bytes(self._batch, self.T)
            if self.ws.numel() < need:
                self.stream.synchronize()
                self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            self.graphs = {}
            self._captured_for = self._signature()
        if self.use_graph and variant not in self.graphs:
            with torch.cuda.stream(self.stream):
                self._capture(variant)

    def _capture(self, variant='host'):
        """Capture one tick with the session's own workspace; remembers what it was captured against (`_refresh` compares).  'host' is the variant
        every session has (StreamSession: its only one)."""
        g = torch.cuda.CUDAGraph()
        with self.eng.use_workspace(self.ws), torch.cuda.graph(g, stream=self.stream):
            self._tick(variant)
        self.graphs[variant] = g
        self._captured_for = self._signature()

    def _run(self, variant):
        """Queue the staged tick -- one replay, or the eager tick -- and block until its results are in pinned memory."""
        eng = self.eng
        for attempt in (0, 1):
            with self._on_stream:
                if self.use_graph:
                    self.graphs[variant].replay()                        # the workspace is baked into it
                else:
                    with eng.use_workspace(self.ws), eng.lazy_status():
                        self._tick(variant)
            self.done.record(self.stream)
            self.done.synchronize()
            if eng.lib.tepose_status_peek(eng.handle) != _lib.E_TIMEOUT:
                return
            what = type(self).__name__
            if attempt:
                _lib.check(_lib.E_TIMEOUT, what + '.push')
            # a persistent kernel gave up inside the tick: clear, switch kernels, put the windows back, re-capture, run the same tick
            # again (whatever it uploads is still staged in pinned memory)
            eng.lib.tepose_status(eng.handle, self.stream.cuda_stream)
            eng._raise_if_kernel_fault(what + '.push')                   # code 4: not a residency problem -- no switch, no re-run
            eng._degrade(what + ' recomputes this push and re-captures its graph')
            with torch.cuda.stream(self.stream):
                self._restore()
                if self.use_graph:
                    self.graphs = {}
                    self._capture(variant)
            self.stream.synchronize()


def _smooth_args(smooth, J_regressor):
    """`smooth` of a live session: None, or (min_cutoff, beta) as run_tracklets spells it -> None or two floats.  No device is touched."""
    if smooth is None:
        return None
    try:
        mc, beta = (float(v) for v in smooth)
    except (TypeError, ValueError):
        raise ValueError('smooth must be None or (min_cutoff, beta), got %r' % (smooth,))
    if not (math.isfinite(mc) and math.isfinite(beta) and mc >= 0.0 and beta >= 0.0):
        raise ValueError('smooth = (min_cutoff, beta) must be two finite numbers >= 0, got %r' % (smooth,))
    if J_regressor is not None:
        raise ValueError('smooth goes with the 49 joints of the demo path, not with a J_regressor (the reference smooths in demo.py only; the '
                         "14-joint evaluation has the slerp filter: tepose_amd.filters.smooth_pose_mat)")
    return mc, beta


class StreamSession(_Session):
    """One live clip.  `theta_init` [seqlen-1, 85] and `feature_init` [seqlen-1, 2048] are the history a stream starts from
    (demo.py:229-237 takes both from the VIBE bootstrap over the first frames).  `push(feature)` returns a dict of pinned host
    tensors for the newest frame (valid until the next push): keys `keep`, e.g. theta[85], kp_3d[J,3], verts[6890,3].

    No `smooth` here: a one-slot `MultiStreamSession(model, seqlen, 1, smooth=...)` is the smoothed single-person session."""

    def __init__(self, model, seqlen, feature_init, theta_init, J_regressor=None, keep=('theta', 'kp_3d', 'verts'), graph=True):
        T = int(seqlen)
        if T < 2 or tuple(feature_init.shape) != (T - 1, 2048) or tuple(theta_init.shape) != (T - 1, 85):
            raise ValueError('feature_init / theta_init must be [seqlen-1, 2048] / [seqlen-1, 85] with seqlen >= 2')
        super().__init__(model, 1, T, J_regressor, keep, graph)
        dev = self.dev
        # the window as the model sees it (slot T-1 = the newest frame) and a scratch copy for the one-frame shift
        self.win = torch.zeros(1, T, 2133, device=dev)
        self.win[0, 1:, :2048] = feature_init.to(dev, torch.float32)      # after the first push's shift they sit in slots 0 .. T-2
        self.win[0, 1:, 2048:] = theta_init.to(dev, torch.float32)
        self.tmp = torch.empty_like(self.win)
        self.saved = torch.empty_like(self.win)                           # the window before a push (recompute after a give-up)
        self.feat_host = torch.zeros(2048, dtype=torch.float32).pin_memory()
        self.out_host = {}                                                # the pinned result rows: made by the warm-up tick
        self.frames = 0
        self._warm_up()

    @property
    def graph(self):
        """The captured tick, or None (graph=False)."""
        return self.graphs.get('host')

    def _tick(self, variant):
        T = self.T
        self.saved.copy_(self.win)                                   # the recompute point, should this tick give up
        # shift by one frame (slots 1 .. T-1 -> 0 .. T-2, through tmp: the ranges overlap); the arriving feature goes into slot
        # T-1 straight from the pinned staging row, its theta slots are zero (evaluate.py:248-252, demo.py:239-241)
        self.tmp[0, :T - 1].copy_(self.win[0, 1:])
        self.tmp[0, T - 1, :2048].copy_(self.feat_host, non_blocking=True)
        self.tmp[0, T - 1, 2048:].zero_()
        self.win.copy_(self.tmp)
        out = self.model(self.win, J_regressor=self.J)[0]
        self.win[0, T - 1, 2048:].copy_(out['theta'][0])             # history: this frame's theta, in a window from the next push on
        for k in self.keep:
            if k not in self.out_host:
                self.out_host[k] = torch.empty(out[k][0].shape, dtype=torch.float32).pin_memory()
            self.out_host[k].copy_(out[k][0], non_blocking=True)

    def _restore(self):
        self.win.copy_(self.saved)

    @torch.no_grad()
    def push(self, feature):
        """feature: [2048] (host tensor / numpy / device tensor).  Blocks until the newest frame's outputs are in the pinned
        result tensors and returns them."""
        if torch.is_tensor(feature) and feature.is_cuda:
            feature = feature.cpu()
        self.feat_host.copy_(torch.as_tensor(feature, dtype=torch.float32).reshape(2048))
        self._refresh('host')
        self._run('host')
        self.frames += 1
        return self.out_host


class MultiStreamSession(_Session):
    """Several live people on one model: a fixed number of SLOTS, each a sliding window like `StreamSession`'s.  A person
    joins a slot, advances with every arriving frame, may miss a frame, and leaves; one tick of the whole session -- `push` -- is ONE captured
    graph replay and one event wait, whatever happened to the slots in it.

        ses = MultiStreamSession(model, seqlen, slots)
        ses.join(slot, feature_init[T-1, 2048], theta_init[T-1, 85])    # staged: the slot's first push loads the history, then advances
        ses.leave(slot)                                                  # staged: the next push clears the window
        out = ses.push({slot: feature[2048], ...})                       # or push(tensor[S, 2048], slots=(...)): which rows are real
        out[slot]['verts']                                               # pinned host row, valid until the next push

    `out` holds the slots that got a feature in this tick.  A joined slot without one is held: its window does not move, nothing is fed back, and
    it is not in `out`.  A `[S, 2048]` tensor on the device (say from `HMR.features_from_frames`) is copied device to device, ordered after the
    caller's current stream, and never visits the host.

    COST: the forward always runs on all S windows (idle ones are all zero), so a tick costs what a batch of B = S costs, however many people are
    present: the caller picks the capacity.  1 <= slots <= 64, the range of the persistent small-batch kernels.

    A tick is the FEED (`_feed`: the upload of op codes and features, by variant) and the rest, which a subclass with another feed keeps.  After a
    give-up every window is restored and the same ops run again (joins reload from hist, which no tick writes).

    smooth=(min_cutoff, beta): the reference's --smooth (demo.py:307-313) inside the tick -- a one-euro step on the pose per slot
    (`tepose_session_smooth`: the filter state, 2 x 72 floats per slot, lives on the device and follows the op codes; a join starts it from the
    history, as `run_tracklets(smooth=...)` starts a tracklet), then SMPL on the filtered pose.  The rows `theta`, `verts` and `kp_3d` are then the
    smoothed ones; `kp_2d` and `rotmat` stay the model's (demo.py does not recompute them either), and so does what is fed back into the windows:
    the windows of a smoothed and an unsmoothed session are the same.  Still one replay and one event wait per tick.  Not with a J_regressor."""

    def __init__(self, model, seqlen, slots, J_regressor=None, keep=('theta', 'kp_3d', 'verts'), graph=True, smooth=None):
        S, T, keep = int(slots), int(seqlen), tuple(keep)
        if not 1 <= S <= 64:
            raise ValueError('slots must be in [1, 64] (the range of the persistent small-batch kernels), got %d' % S)
        if T < 2:
            raise ValueError('seqlen must be >= 2')
        if not keep or any(k not in OUT_TAILS for k in keep):
            raise ValueError('keep must name outputs among %s' % (tuple(OUT_TAILS),))
        self.smooth = _smooth_args(smooth, J_regressor)
        self.S = S                          # before the base's constructor: `_pack` sizes by it
        self.ws_hat = None                  # with smooth: the workspace of the SMPL launch on the filtered pose, the session's own (made by `_pack`)
        super().__init__(model, S, T, J_regressor, keep, graph)
        dev = self.dev
        self.win = torch.zeros(S, T, 2133, device=dev)                    # idle windows are all zero
        self.saved = torch.zeros_like(self.win)                           # every window before a tick (recompute after a give-up)
        self.hist = torch.zeros(S, T - 1, 2133, device=dev)               # what a join loads
        self.hist_host = torch.zeros(S, T - 1, 2133).pin_memory()
        self._alloc_feed()
        self.out_dev = {k: torch.empty((S,) + tail, device=dev) for k, tail in out_shapes(n_joints(J_regressor)).items()}
        self.rows_dev = dict(self.out_dev)                                # what a tick copies into the pinned rows
        if self.smooth is not None:
            self.fstate = torch.zeros(S, 2, 72, device=dev)               # per slot (x^, dx^) of the one-euro filter
            self.fsaved = torch.zeros_like(self.fstate)                   # ... before a tick (recompute after a give-up)
            self.theta_hat, self.pose_hat, self.betas_hat = torch.zeros(S, 85, device=dev), torch.zeros(S, 72, device=dev), torch.zeros(S, 10, device=dev)
            self.verts_hat, self.joints_hat = torch.empty(S, NUM_VERTS, 3, device=dev), torch.empty(S, 49, 3, device=dev)
            self.rows_dev.update(theta=self.theta_hat, verts=self.verts_hat, kp_3d=self.joints_hat)
        self.out_host = {k: torch.empty(self.out_dev[k].shape).pin_memory() for k in self.keep}
        self._rows = [{k: self.out_host[k][s] for k in self.keep} for s in range(S)]      # what push returns: views, made once
        self.occupied = [False] * S
        self._join = [False] * S            # staged: the slot's next push with a feature is op 2
        self._clear = [False] * S           # staged: the window still holds a person who left
        self.ticks = 0
        self._warm_up()                     # all-zero windows, every op 0: no window changes

    def _alloc_feed(self):
        """What `_feed` uploads, as ONE pinned block and one device block: S op codes (int32), then S feature rows -- one H2D copy in the graph.
        Leaves `ops`, `feat` (device) and `_ops_np` (the pinned op codes, as numpy) for the rest of the tick and for `push`."""
        S, dev = self.S, self.dev
        self.stage = torch.zeros(S * (1 + 2048), dtype=torch.float32, device=dev)
        self.stage_host = torch.zeros(S * (1 + 2048), dtype=torch.float32).pin_memory()
        self.ops, self.feat = self.stage[:S].view(torch.int32), self.stage[S:].view(S, 2048)
        self.ops_host, self.feat_host = self.stage_host[:S].view(torch.int32), self.stage_host[S:].view(S, 2048)
        self._ops_np = self.ops_host.numpy()                              # the same memory

    def _feed(self, variant):
        if variant == 'host':
            self.stage.copy_(self.stage_host, non_blocking=True)         # op codes and features
        else:
            self.ops.copy_(self.ops_host, non_blocking=True)             # the features are on the device already

    def _tick(self, variant):
        eng, S, T = self.eng, self.S, self.T
        self._feed(variant)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        # hist is always given: the library cannot see on the host whether an op is 2, and a join without hist would act as a hold
        _lib.check(eng.lib.tepose_session_advance(self.win.data_ptr(), self.saved.data_ptr(), S, T, self.ops.data_ptr(), self.feat.data_ptr(),
                                                  self.hist.data_ptr(), st), 'tepose_session_advance')
        with on_device(self.dev):
            eng.forward(self.win, self.J, out=self.out_dev)           # B = S, the forward run_clips and StreamSession call
        _lib.check(eng.lib.tepose_session_commit(self.win.data_ptr(), S, T, self.ops.data_ptr(), self.out_dev['theta'].data_ptr(), st),
                   'tepose_session_commit')
        if self.smooth is not None:
            # after the commit: the model's theta is what is fed back (the reference smooths after its window loop)
            _lib.check(eng.lib.tepose_session_smooth(self.out_dev['theta'].data_ptr(), self.hist.data_ptr(), S, T, self.ops.data_ptr(), self.fstate.data_ptr(),
                                                     self.fsaved.data_ptr(), self.smooth[0], self.smooth[1], 1.0, self.theta_hat.data_ptr(),
                                                     self.pose_hat.data_ptr(), self.betas_hat.data_ptr(), st), 'tepose_session_smooth')
            # the path filters.smooth_pose reaches through SMPL, at N = S (held and idle slots: pose 0, betas 0)
            _lib.check(eng.lib.tepose_smpl_fwd(eng.handle, 1, self.pose_hat.data_ptr(), self.betas_hat.data_ptr(), S, self.verts_hat.data_ptr(),
                                               self.joints_hat.data_ptr(), self.ws_hat.data_ptr(), self.ws_hat.numel(), st), 'tepose_smpl_fwd')
        for k in self.keep:
            self.out_host[k].copy_(self.rows_dev[k], non_blocking=True)

    def _restore(self):
        self.win.copy_(self.saved)
        if self.smooth is not None:
            self.fstate.copy_(self.fsaved)

    def _pack(self):
        """With smooth, the full check also sizes the SMPL workspace: what is packed can change the bytes a launch needs."""
        super()._pack()
        if self.smooth is not None:
            need = max(self.eng.workspace_bytes(max(1, (self.S + 1) // 2), 1), self.eng.workspace_bytes(self.S, 1))      # as Engine.smpl_fwd sizes it, or more
            if self.ws_hat is None or self.ws_hat.numel() < need:
                self.stream.synchronize()
                self.ws_hat = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def _signature(self):
        sig = super()._signature()
        if self.smooth is not None:         # the addresses the two extra launches of a captured tick hold
            sig += (self.ws_hat.data_ptr(), self.fstate.data_ptr(), self.theta_hat.data_ptr(), self.verts_hat.data_ptr(), self.joints_hat.data_ptr())
        return sig

    def _slot(self, slot):
        s = int(slot)
        if not 0 <= s < self.S:
            raise ValueError('slot %r out of range [0, %d)' % (slot, self.S))
        return s

    def join(self, slot, feature_init, theta_init):
        """A person takes an idle slot (one left in this same interval counts as idle).  feature_init [seqlen-1, 2048] and theta_init [seqlen-1, 85]:
        the history a stream starts from, as for StreamSession.  Staged in pinned memory; loaded by the slot's first push."""
        s = self._slot(slot)
        if self.occupied[s]:
            raise ValueError('slot %d is occupied' % s)
        T = self.T
        if tuple(feature_init.shape) != (T - 1, 2048) or tuple(theta_init.shape) != (T - 1, 85):
            raise ValueError('feature_init / theta_init must be [seqlen-1, 2048] / [seqlen-1, 85]')
        self.hist_host[s, :, :2048].copy_(torch.as_tensor(feature_init).to(torch.float32))
        self.hist_host[s, :, 2048:].copy_(torch.as_tensor(theta_init).to(torch.float32))
        self.occupied[s], self._join[s] = True, True

    def leave(self, slot):
        s = self._slot(slot)
        if not self.occupied[s]:
            raise ValueError('slot %d is idle' % s)
        self.occupied[s] = False
        if self._join[s]:
            self._join[s] = False            # never pushed: the window holds nothing of this person
        else:
            self._clear[s] = True

    @torch.no_grad()
    def push(self, features, slots=None):
        """features: {slot: feature[2048]} (host tensors / numpy), or a [S, 2048] tensor, on the host or the device, with `slots` naming the rows that
        are real (None: every occupied slot).  Blocks until the tick's outputs are in pinned memory; returns {slot: {key: row}} for those slots."""
        S = self.S
        if isinstance(features, dict):
            if slots is not None:
                raise ValueError('slots= goes with a [S, 2048] tensor, not with a dict')
            active = sorted(self._slot(s) for s in features)
            rows, variant = {self._slot(s): f for s, f in features.items()}, 'host'
        else:
            if not torch.is_tensor(features):
                features = torch.as_tensor(features)
            if tuple(features.shape) != (S, 2048):
                raise ValueError('a feature tensor must be [slots, 2048] = [%d, 2048], got %s' % (S, tuple(features.shape)))
            active = sorted(set(self._slot(s) for s in slots)) if slots is not None else [s for s in range(S) if self.occupied[s]]
            rows, variant = None, 'device' if features.is_cuda else 'host'
        for s in active:
            if not self.occupied[s]:
                raise ValueError('a feature for idle slot %d' % s)
        ops = self._stage_ops(active)
        if rows is not None:
            for s in active:
                self.feat_host[s].copy_(torch.as_tensor(rows[s], dtype=torch.float32).reshape(2048))
        elif variant == 'host':
            self.feat_host.copy_(features)
        return self._run_staged(variant, active, ops, features if variant == 'device' else None)

    def _stage_ops(self, active):
        """The op code of every slot for a tick in which the (occupied) slots `active` advance, written to the pinned op codes."""
        got = set(active)
        ops = [(2 if self._join[s] else 1) if s in got else (3 if self._clear[s] else 0) for s in range(self.S)]
        self._ops_np[:] = ops
        return ops

    def _run_staged(self, variant, active, ops, features=None):
        """Run the tick whose op codes and feed are staged; `features`: a device tensor to copy into `feat` in front of it.  -> {slot: rows}."""
        self._refresh(variant)
        if features is not None or 2 in ops:
            if features is not None:
                # the caller's stream, taken BEFORE the session's becomes current: whatever is still writing `features` there finishes first
                self.stream.wait_stream(torch.cuda.current_stream(features.device))
            with torch.cuda.stream(self.stream):
                if features is not None:
                    self.feat.copy_(features, non_blocking=True)
                for s in active:
                    if ops[s] == 2:          # outside the graph, before the replay: the graph itself never changes
                        self.hist[s].copy_(self.hist_host[s], non_blocking=True)
        self._run(variant)
        for s in range(self.S):
            if ops[s] == 2:
                self._join[s] = False
            if ops[s] >= 2:
                self._clear[s] = False       # a join overwrites the whole window, as a clear does
        self.ticks += 1
        return {s: self._rows[s] for s in active}
