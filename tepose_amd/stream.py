"""Frame-at-a-time live-stream session (BASELINE.json config 5; reference loop: demo.py:238-252).

The reference's demo slides a `seqlen` window over one tracked person: window k holds the features of frames k .. k+seqlen-1
and, in its theta slots, the predictions of the first seqlen-1 of them (the newest frame's slots are zero); the prediction for
the newest frame is appended to the theta history and the window moves on by one frame.  `tepose_amd.driver.run_clips` runs
that loop when the whole clip is known up front.  A live stream is not: frames ARRIVE, one at a time, and what matters is the
time from a frame's arrival on the host to its result being readable on the host.

`StreamSession.push(feature[2048])` is that step.  The session owns the window on the device (features + theta history), a
pinned staging row for the arriving feature and pinned result rows; one push is ONE captured hipGraph replay --

    H2D copy of the feature -> shift the window by one frame, newest theta slots zero -> TePose.forward (B = 1: the
    persistent small-batch HIP kernels) -> predicted theta into the history slot -> D2H copy of the kept outputs

-- followed by one event wait.  No allocation, no Python-side tensor work and no host sync inside the step; the host pays
one graph launch per frame instead of ~10 kernel launches plus the slicing of `run_clips`.  The forward inside the graph is
the same C entry point on the same operands as the eager driver, so the results are bit-identical to `run_clips`
(tests/test_gpu_stream.py).

Failure contract (include/tepose_amd.h, "failure channel"): a replayed graph is not status-checked by `Engine._run`, so
`push` reads the handle's fault word (one host-memory read) after its wait; on a give-up the model is switched to the
step-per-launch kernels, the graph is re-captured and the frame is recomputed from the saved window -- never a NaN result.
"""

import torch

from . import _lib
from .engine import on_device


class StreamSession:
    """One live clip.  `theta_init` [seqlen-1, 85] and `feature_init` [seqlen-1, 2048] are the history a stream starts from
    (demo.py:229-237 takes both from the VIBE bootstrap over the first frames).  `push(feature)` returns a dict of pinned host
    tensors for the newest frame (valid until the next push): keys `keep`, e.g. theta[85], kp_3d[J,3], verts[6890,3]."""

    def __init__(self, model, seqlen, feature_init, theta_init, J_regressor=None, keep=('theta', 'kp_3d', 'verts'), graph=True):
        self.model, self.T, self.J, self.keep = model, int(seqlen), J_regressor, tuple(keep)
        T = self.T
        dev = next(model.parameters()).device
        self.dev = dev
        if T < 2 or tuple(feature_init.shape) != (T - 1, 2048) or tuple(theta_init.shape) != (T - 1, 85):
            raise ValueError('feature_init / theta_init must be [seqlen-1, 2048] / [seqlen-1, 85] with seqlen >= 2')
        self.stream = torch.cuda.Stream(device=dev)
        eng = model._engine
        with torch.no_grad():
            eng.pack_model(model, dev)          # the workspace size depends on what is packed
        # A workspace of the session's own: the captured graph bakes its address into every kernel argument (the status words
        # that push() reads live in it too), and the engine's shared workspace moves whenever another call on the model needs
        # more bytes or the weights are re-packed.  Two sessions on one model do not share scratch either.
        self.ws = torch.empty(eng.workspace_bytes(1, T), dtype=torch.uint8, device=dev)
        self._captured_for = None
        self._rewatch()
        # the window as the model sees it (slot T-1 = the newest frame) and a scratch copy for the one-frame shift
        self.win = torch.zeros(1, T, 2133, device=dev)
        self.win[0, 1:, :2048] = feature_init.to(dev, torch.float32)      # after the first push's shift they sit in slots 0 .. T-2
        self.win[0, 1:, 2048:] = theta_init.to(dev, torch.float32)
        self.tmp = torch.empty_like(self.win)
        self.saved = torch.empty_like(self.win)                           # the window before a push (recompute after a fault)
        self.feat_host = torch.zeros(2048, dtype=torch.float32).pin_memory()
        self.out_host = {}
        self.graph = None
        self.use_graph = bool(graph)
        self.done = torch.cuda.Event()
        self.frames = 0
        # the buffers above were filled on the caller's stream; the session's stream is non-blocking (no implicit ordering)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(self.stream), eng.use_workspace(self.ws):
            # warm-up (its window is restored afterwards): packs the blob, sizes the workspace, creates the pinned result rows
            for attempt in (0, 1):
                with model._engine.lazy_status():
                    self._step()
                self.stream.synchronize()
                try:
                    model._engine.check_status()             # a give-up here has switched the model to the step kernels (warned)
                    break
                except _lib.TeposeTimeout:
                    if attempt:
                        raise
                finally:
                    self.win.copy_(self.saved)
            if self.use_graph:
                self._capture()
            else:
                self._captured_for = self._signature()
        self.stream.synchronize()

    # one step, queued on the current stream: what the graph captures
    def _step(self):
        T = self.T
        self.saved.copy_(self.win)                                   # the recompute point, should this step give up
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

    def _rewatch(self):
        eng = self.model._engine
        self._watch = eng._enc_tensors(self.model.encoder) + eng._reg_tensors(self.model.regressor)
        self._watch_sig = (tuple([t._version for t in self._watch]), self._watch[0].data_ptr(), self._watch[-1].data_ptr())

    def _signature(self):
        eng = self.model._engine
        return (eng.packed_generation, eng.blob.data_ptr() if eng.blob is not None else 0, self.ws.data_ptr())

    def _refresh(self):
        """Before a step: re-pack if the model's parameters changed in place since the last pack (outside any capture -- a replay would go on
        using the old packed blob without a sign), grow the session's workspace if the packed model now needs more, and re-capture a graph
        whose blob / workspace are no longer the ones it was captured against.  Same for the eager (graph=False) session."""
        eng = self.model._engine
        # Per push, on the frame's critical path: the in-place version counters of the watched parameter / buffer objects and two addresses (~5 us on the
        # host).  The engine's full signature walk (every tensor re-fetched from its module by name, ~35 us) runs when those moved, and every 32nd push as a
        # backstop for what the cheap check cannot see (a parameter OBJECT replaced by assignment).
        self._pushes_since_full = getattr(self, '_pushes_since_full', 0) + 1
        cheap = (tuple([t._version for t in self._watch]), self._watch[0].data_ptr(), self._watch[-1].data_ptr())
        if cheap != self._watch_sig or self._pushes_since_full >= 32:
            self._pushes_since_full = 0
            with torch.cuda.stream(self.stream):
                eng.pack_model(self.model, self.dev)                   # no-op while the parameter signatures stand
            self._rewatch()
        if self._signature() == self._captured_for:
            return
        need = eng.workspace_bytes(1, self.T)
        if self.ws.numel() < need:
            self.stream.synchronize()
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        if self.graph is not None:
            with torch.cuda.stream(self.stream):
                self._capture()
        else:
            self._captured_for = self._signature()

    def _capture(self):
        """Queue-free capture of one step with the session's own workspace; remembers which packed blob it was captured
        against (a re-pack or an adopted blob invalidates the graph: push() re-captures)."""
        eng = self.model._engine
        self.graph = torch.cuda.CUDAGraph()
        with eng.use_workspace(self.ws), torch.cuda.graph(self.graph, stream=self.stream):
            self._step()
        self._captured_for = self._signature()

    @torch.no_grad()
    def push(self, feature):
        """feature: [2048] (host tensor / numpy / device tensor).  Blocks until the newest frame's outputs are in the pinned
        result tensors and returns them."""
        eng = self.model._engine
        if torch.is_tensor(feature) and feature.is_cuda:
            feature = feature.cpu()
        self.feat_host.copy_(torch.as_tensor(feature, dtype=torch.float32).reshape(2048))
        # the blob the graph was captured against may have been re-packed (a weight change, here or by another caller: kernel selection may
        # differ, e.g. the fp16-range fallback) or replaced (adopt_blob, device move)
        self._refresh()
        for attempt in (0, 1):
            with torch.cuda.stream(self.stream), eng.use_workspace(self.ws):
                if self.graph is not None:
                    self.graph.replay()
                else:
                    with eng.lazy_status():
                        self._step()
                self.done.record(self.stream)
            self.done.synchronize()
            if eng.lib.tepose_status_peek(eng.handle) != _lib.E_TIMEOUT:
                break
            if attempt:
                _lib.check(_lib.E_TIMEOUT, 'StreamSession.push')
            # a persistent kernel gave up inside the replayed graph: clear, switch kernels, re-capture, recompute this frame
            eng.lib.tepose_status(eng.handle, self.stream.cuda_stream)
            eng._raise_if_kernel_fault('StreamSession.push')             # code 4: not a residency problem -- no switch, no re-run
            eng._degrade('StreamSession recomputes this frame and re-captures its graph')
            with torch.cuda.stream(self.stream):
                self.win.copy_(self.saved)
                if self.use_graph:
                    self._capture()
            self.stream.synchronize()
        self.frames += 1
        return self.out_host


_OUT_TAILS = {'theta': (85,), 'verts': (6890, 3), 'kp_2d': (None, 2), 'kp_3d': (None, 3), 'rotmat': (24, 3, 3)}


class MultiStreamSession:
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

    The failure contract is `StreamSession.push`'s: a give-up of a persistent kernel inside a tick switches the model to the step-per-launch
    kernels, restores every window, re-captures and runs the same tick again -- never a NaN result."""

    def __init__(self, model, seqlen, slots, J_regressor=None, keep=('theta', 'kp_3d', 'verts'), graph=True):
        self.model, self.T, self.S, self.J, self.keep = model, int(seqlen), int(slots), J_regressor, tuple(keep)
        T, S = self.T, self.S
        if not 1 <= S <= 64:
            raise ValueError('slots must be in [1, 64] (the range of the persistent small-batch kernels), got %d' % S)
        if T < 2:
            raise ValueError('seqlen must be >= 2')
        if not self.keep or any(k not in _OUT_TAILS for k in self.keep):
            raise ValueError('keep must name outputs among %s' % (tuple(_OUT_TAILS),))
        dev = next(model.parameters()).device
        self.dev = dev
        self.stream = torch.cuda.Stream(device=dev)
        eng = model._engine
        with torch.no_grad():
            eng.pack_model(model, dev)          # the workspace size depends on what is packed
        # a workspace of the session's own, for the reasons StreamSession has one: the graph bakes its address in
        self.ws = torch.empty(eng.workspace_bytes(S, T), dtype=torch.uint8, device=dev)
        self._captured_for = None
        self._pushes_since_full = 0
        self._rewatch()
        nj = 14 if J_regressor is not None else 49
        self.win = torch.zeros(S, T, 2133, device=dev)                    # idle windows are all zero
        self.saved = torch.zeros_like(self.win)                           # every window before a tick (recompute after a give-up)
        self.hist = torch.zeros(S, T - 1, 2133, device=dev)               # what a join loads
        self.hist_host = torch.zeros(S, T - 1, 2133).pin_memory()
        # what a tick uploads, as ONE pinned block and one device block: S op codes (int32), then S feature rows -- one H2D copy in the graph
        self.stage = torch.zeros(S * (1 + 2048), dtype=torch.float32, device=dev)
        self.stage_host = torch.zeros(S * (1 + 2048), dtype=torch.float32).pin_memory()
        self.ops, self.feat = self.stage[:S].view(torch.int32), self.stage[S:].view(S, 2048)
        self.ops_host, self.feat_host = self.stage_host[:S].view(torch.int32), self.stage_host[S:].view(S, 2048)
        self._ops_np = self.ops_host.numpy()                              # the same memory
        self.out_dev = {k: torch.empty((S,) + tuple(nj if d is None else d for d in tail), device=dev) for k, tail in _OUT_TAILS.items()}
        self.out_host = {k: torch.empty(self.out_dev[k].shape).pin_memory() for k in self.keep}
        self._rows = [{k: self.out_host[k][s] for k in self.keep} for s in range(S)]      # what push returns: views, made once
        self.occupied = [False] * S
        self._join = [False] * S            # staged: the slot's next push with a feature is op 2
        self._clear = [False] * S           # staged: the window still holds a person who left
        self.graphs = {}                    # variant ('host' / 'device' features) -> captured tick
        self.use_graph = bool(graph)
        self.done = torch.cuda.Event()
        self.ticks = 0
        self.stream.wait_stream(torch.cuda.current_stream(dev))           # the buffers above were filled on the caller's stream
        with torch.no_grad(), torch.cuda.stream(self.stream), eng.use_workspace(self.ws):
            # warm-up on all-zero windows with every op 0: sizes and caches settle; no window changes
            for attempt in (0, 1):
                with eng.lazy_status():
                    self._tick('host')
                self.stream.synchronize()
                try:
                    eng.check_status()           # a give-up here has switched the model to the step kernels (warned)
                    break
                except _lib.TeposeTimeout:
                    if attempt:
                        raise
            if self.use_graph:
                self._capture('host')
            else:
                self._captured_for = self._signature()
        self.stream.synchronize()

    # one tick, queued on the current stream: what a graph captures.  A single chain: no forked branches.
    def _tick(self, variant):
        eng, S, T = self.model._engine, self.S, self.T
        st = torch.cuda.current_stream(self.dev).cuda_stream
        if variant == 'host':
            self.stage.copy_(self.stage_host, non_blocking=True)         # op codes and features
        else:
            self.ops.copy_(self.ops_host, non_blocking=True)             # the features are on the device already
        # hist is always given: the library cannot see on the host whether an op is 2, and a join without hist would act as a hold
        _lib.check(eng.lib.tepose_session_advance(self.win.data_ptr(), self.saved.data_ptr(), S, T, self.ops.data_ptr(), self.feat.data_ptr(),
                                                  self.hist.data_ptr(), st), 'tepose_session_advance')
        with on_device(self.dev):
            eng.forward(self.win, self.J, out=self.out_dev)           # B = S, the forward run_clips and StreamSession call
        _lib.check(eng.lib.tepose_session_commit(self.win.data_ptr(), S, T, self.ops.data_ptr(), self.out_dev['theta'].data_ptr(), st),
                   'tepose_session_commit')
        for k in self.keep:
            self.out_host[k].copy_(self.out_dev[k], non_blocking=True)

    def _cheap_sig(self):
        return (tuple([t._version for t in self._watch]), tuple([t.data_ptr() for t in self._watch]))

    def _rewatch(self):
        eng = self.model._engine
        self._watch = eng._enc_tensors(self.model.encoder) + eng._reg_tensors(self.model.regressor)
        self._watch_sig = self._cheap_sig()

    def _signature(self):
        eng = self.model._engine
        return (eng.packed_generation, eng.blob.data_ptr() if eng.blob is not None else 0, self.ws.data_ptr())

    def _refresh(self, variant):
        """Before a tick, as StreamSession._refresh: re-pack after an in-place weight change (outside any capture), grow the workspace if the packed
        model needs more, drop graphs captured against another blob or workspace.  The cheap check carries the version counter AND the address of
        every watched tensor; a re-pack waits for the caller's current stream first (the weight change was queued there)."""
        eng = self.model._engine
        self._pushes_since_full += 1
        if self._cheap_sig() != self._watch_sig or self._pushes_since_full >= 32:
            self._pushes_since_full = 0
            self.stream.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(self.stream):
                eng.pack_model(self.model, self.dev)                   # no-op while the parameter signatures stand
            self._rewatch()
        if self._signature() != self._captured_for:
            need = eng.workspace_bytes(self.S, self.T)
            if self.ws.numel() < need:
                self.stream.synchronize()
                self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            self.graphs = {}
            self._captured_for = self._signature()
        if self.use_graph and variant not in self.graphs:
            with torch.cuda.stream(self.stream):
                self._capture(variant)

    def _capture(self, variant):
        eng = self.model._engine
        g = torch.cuda.CUDAGraph()
        with eng.use_workspace(self.ws), torch.cuda.graph(g, stream=self.stream):
            self._tick(variant)
        self.graphs[variant] = g
        self._captured_for = self._signature()

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
        eng, S = self.model._engine, self.S
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
        got = set(active)
        ops = [(2 if self._join[s] else 1) if s in got else (3 if self._clear[s] else 0) for s in range(S)]
        self._ops_np[:] = ops
        if rows is not None:
            for s in active:
                self.feat_host[s].copy_(torch.as_tensor(rows[s], dtype=torch.float32).reshape(2048))
        elif variant == 'host':
            self.feat_host.copy_(features)
        self._refresh(variant)
        if variant == 'device' or 2 in ops:
            if variant == 'device':
                # the caller's stream, taken BEFORE the session's becomes current: whatever is still writing `features` there finishes first
                self.stream.wait_stream(torch.cuda.current_stream(features.device))
            with torch.cuda.stream(self.stream):
                if variant == 'device':
                    self.feat.copy_(features, non_blocking=True)
                for s in active:
                    if ops[s] == 2:          # outside the graph, before the replay: the graph itself never changes
                        self.hist[s].copy_(self.hist_host[s], non_blocking=True)
        for attempt in (0, 1):
            with torch.cuda.stream(self.stream), eng.use_workspace(self.ws):
                if self.use_graph:
                    self.graphs[variant].replay()
                else:
                    with eng.lazy_status():
                        self._tick(variant)
                self.done.record(self.stream)
            self.done.synchronize()
            if eng.lib.tepose_status_peek(eng.handle) != _lib.E_TIMEOUT:
                break
            if attempt:
                _lib.check(_lib.E_TIMEOUT, 'MultiStreamSession.push')
            # a persistent kernel gave up inside the tick: clear, switch kernels, put every window back, re-capture, run the same ops again
            # (joins reload from hist, which the tick does not write)
            eng.lib.tepose_status(eng.handle, self.stream.cuda_stream)
            eng._raise_if_kernel_fault('MultiStreamSession.push')        # code 4: not a residency problem -- no switch, no re-run
            eng._degrade('MultiStreamSession recomputes this tick and re-captures its graph')
            with torch.cuda.stream(self.stream):
                self.win.copy_(self.saved)
                if self.use_graph:
                    self.graphs = {}
                    self._capture(variant)
            self.stream.synchronize()
        for s in range(S):
            if ops[s] == 2:
                self._join[s] = False
            if ops[s] >= 2:
                self._clear[s] = False       # a join overwrites the whole window, as a clear does
        self.ticks += 1
        return {s: self._rows[s] for s in active}
