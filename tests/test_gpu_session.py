"""GPU: the multi-person live session (tepose_amd.stream.MultiStreamSession over csrc/session.hip).  The two window
kernels alone, bit for bit against their numpy restatement (tests/_session_ref.py), between guard rows; one slot against StreamSession and
the reference-loop goldens; all slots present against the clip driver, bit for bit; people who join, miss frames and leave at different
ticks against each person's own run; graph against eager, device-fed against host-fed; a give-up inside a replayed tick; the errors."""
import os

import numpy as np
import pytest
import torch

import _buffers as BUF
import _session_ref as R
from tepose_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
KEEP = ('theta', 'kp_3d', 'verts')
# the persistent small-batch kernels at the smallest hidden size they take, and the step-per-launch kernels at the smallest window
ARCH = [(2, 256, 6), (1, 64, 2)]


@pytest.fixture(scope='module')
def smpl_np():
    return synth.synthetic_smpl(0)


def _clip(N, T, seed):
    """features [N,2048] and the theta history of the first T - 1 frames."""
    w = synth.synthetic_windows(1, max(N, T), seed)[0]
    return torch.from_numpy(w[:N, :2048].copy()), torch.from_numpy(w[:T - 1, 2048:].copy())


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize('S,T', [(1, 2), (3, 2), (3, 6), (64, 6), (5, 32)])
@pytest.mark.parametrize('with_saved', [True, False])
def test_the_window_kernels_equal_their_numpy_restatement_bit_for_bit(S, T, with_saved):
    from tepose_amd import _lib
    lib = _lib.load()
    dev = 'cuda'
    st = torch.cuda.current_stream().cuda_stream
    # a thread block serves one slot: an index off by one reaches at most one slot's window past the owned ones -- two slots of guard on each side
    for shift in (range(8) if S < 8 else (0,)):
        win_np, ops_np, feat_np, hist_np, theta_np = R.random_case(S, T, 1000 * S + T, shift)
        win = BUF.guarded_like((S, T, 2133), S, dev, name='win', guard_rows=2)
        saved = BUF.guarded_like((S, T, 2133), S, dev, name='saved', guard_rows=2)
        win.own.copy_(torch.from_numpy(win_np))
        ops, feat, hist, theta = (torch.from_numpy(a).to(dev) for a in (ops_np, feat_np, hist_np, theta_np))
        frozen = BUF.Frozen(ops=ops, feat=feat, hist=hist, theta=theta)
        rc = lib.tepose_session_advance(win.data_ptr(), saved.data_ptr() if with_saved else None, S, T, ops.data_ptr(), feat.data_ptr(),
                                        hist.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        want, want_saved = R.advance(win_np, ops_np, feat_np, hist_np)
        got = win.own.cpu().numpy()
        what = 'advance S=%d T=%d ops=%s' % (S, T, ops_np.tolist())
        assert R.same_bits(got, want), what
        for s in range(S):
            if int(ops_np[s]) not in (1, 2, 3):
                assert R.same_bits(got[s], win_np[s]), (what, s)                 # held: not one bit moved
        if with_saved:
            assert R.same_bits(saved.own.cpu().numpy(), want_saved), what         # every slot, whatever its op
        else:
            assert bool((saved.own.view(torch.int32) == -1).all()), what          # still the 0xFF fill: never written
        BUF.assert_guards_intact(win, saved, what=what)
        rc = lib.tepose_session_commit(win.data_ptr(), S, T, ops.data_ptr(), theta.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert R.same_bits(win.own.cpu().numpy(), R.commit(want, ops_np, theta_np)), 'commit ' + what
        BUF.assert_guards_intact(win, saved, what='commit ' + what)
        frozen.assert_unchanged(what)
    # a join without history holds (nothing is read through the null pointer)
    win_np, _, feat_np, _, _ = R.random_case(S, T, 5)
    win = torch.from_numpy(win_np).to(dev)
    ops = torch.full((S,), 2, dtype=torch.int32, device=dev)
    feat = torch.from_numpy(feat_np).to(dev)
    assert lib.tepose_session_advance(win.data_ptr(), None, S, T, ops.data_ptr(), feat.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert R.same_bits(win.cpu().numpy(), win_np)


# ------------------------------------------------------------------ 2. one slot = StreamSession
@pytest.mark.parametrize('name', ['driver_L2H128_N40T6', 'driver_L1H64_N9T4'])
def test_one_slot_equals_stream_session_and_the_reference_golden(name, smpl_np):
    from tepose_amd.stream import MultiStreamSession, StreamSession
    from tepose_amd.testing import build_model
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    L, H, N, T, seed_w, seed_x = [int(v) for v in g['meta']]
    model, _, _ = build_model(L, H, seed=seed_w, device='cuda', smpl_np=smpl_np)
    w = synth.synthetic_windows(1, N, seed_x)[0]
    feats = torch.from_numpy(w[:, :2048].copy())
    th0 = torch.from_numpy(g['theta_init'])
    J = torch.from_numpy(smpl_np['J_regressor_h36m'])
    one = StreamSession(model, T, feats[:T - 1], th0, J_regressor=J, keep=KEEP)
    ses = MultiStreamSession(model, T, 1, J_regressor=J, keep=KEEP)
    assert ses.graphs
    ses.join(0, feats[:T - 1], th0)
    got = {k: [] for k in KEEP}
    for f in feats[T - 1:]:
        ref = one.push(f)
        out = ses.push({0: f})
        assert list(out) == [0]
        for k in KEEP:
            assert torch.equal(out[0][k], ref[k]), k                           # every frame, bit for bit
            got[k].append(out[0][k].clone())
    got = {k: torch.stack(v).numpy() for k, v in got.items()}
    assert ses.ticks == N - T + 1
    assert np.abs(got['kp_3d'] - g['kp_3d']).max() < 1e-4
    assert np.abs(got['verts'][:, ::53] - g['verts_sub']).max() < 1e-4
    assert np.abs(got['theta'][:, :3] - g['theta'][:, :3]).max() < 1e-4
    assert np.abs(got['theta'][:, 75:] - g['theta'][:, 75:]).max() < 1e-4


# ------------------------------------------------------------------ 3. all slots present = the clip driver
@pytest.mark.parametrize('L,H,T', ARCH)
def test_all_slots_present_equal_the_clip_driver_bit_for_bit(L, H, T, smpl_np):
    from tepose_amd.driver import run_clips
    from tepose_amd.stream import MultiStreamSession
    from tepose_amd.testing import build_model
    N, S = 12, 3
    model, _, _ = build_model(L, H, seed=51, device='cuda', smpl_np=smpl_np, seqlen=T)
    clips = [_clip(N, T, 700 + i) for i in range(S)]
    J = torch.from_numpy(smpl_np['J_regressor_h36m'])
    ref = run_clips(model, [f for f, _ in clips], [t for _, t in clips], T, J_regressor=J, keep=KEEP, cache_projections=False)
    ses = MultiStreamSession(model, T, S, J_regressor=J, keep=KEEP)
    for s, (f, th) in enumerate(clips):
        ses.join(s, f[:T - 1], th)
    for j in range(N - T + 1):
        out = ses.push({s: clips[s][0][T - 1 + j] for s in range(S)})
        assert sorted(out) == [0, 1, 2]
        for s in range(S):
            for k in KEEP:
                assert torch.equal(out[s][k], ref[s][k][j].cpu()), (k, s, j)


# ------------------------------------------------------------------ 4 - 6. staggered lives
TICKS, NCLIP = 13, 16


def _script(tick):
    """What happens before and in tick `tick`: (joins, leaves, who gets a frame).  Person A lives in slot 0 from tick 0 and misses ticks 5 and 6;
    B lives in slot 2 from tick 3 and leaves before tick 9, where C takes the same slot; slots 1 and 3 are never used."""
    joins = {0: [('A', 0)], 3: [('B', 2)], 9: [('C', 2)]}.get(tick, [])
    leaves = [2] if tick == 9 else []
    fed = ([('A', 0)] if tick not in (5, 6) else []) + ([('B', 2)] if 3 <= tick < 9 else []) + ([('C', 2)] if tick >= 9 else [])
    return joins, leaves, fed


def _run_script(model, T, clips, graph=True, device_features=False):
    from tepose_amd.stream import MultiStreamSession
    S = 4
    ses = MultiStreamSession(model, T, S, keep=KEEP, graph=graph)
    nxt = {p: T - 1 for p in clips}                                  # the next frame of each person
    if device_features:
        busy0 = torch.softmax(torch.randn(4096, 4096, device='cuda'), dim=1)      # row-stochastic: its powers stay finite
    got = {p: {k: [] for k in KEEP} for p in clips}
    for tick in range(TICKS):
        joins, leaves, fed = _script(tick)
        for s in leaves:
            ses.leave(s)
        for p, s in joins:
            ses.join(s, clips[p][0][:T - 1], clips[p][1])
        if device_features:
            x = torch.full((S, 2048), float('nan'))                  # rows that are not named must not matter
            for p, s in fed:
                x[s] = clips[p][0][nxt[p]]
            # The features are WRITTEN by work still queued on the caller's stream when push is called: behind a chain of products (some
            # milliseconds of device time), a device-to-device copy fills the tensor, which holds NaN until then.  A push that does not
            # order itself after the caller's stream reads the NaN rows.
            src, busy = x.cuda(), busy0
            x_dev = torch.full((S, 2048), float('nan'), device='cuda')
            torch.cuda.synchronize()
            for _ in range(8):
                busy = busy @ busy0                                  # 8 products of 4096^3: ~1.1 TFLOP, several milliseconds
            x_dev.copy_(src)                                         # same stream: runs when the chain is through
            assert not torch.cuda.current_stream().query()           # ... which it is not yet: the case this test is about
            out = ses.push(x_dev, slots=[s for _, s in fed])
        else:
            out = ses.push({s: clips[p][0][nxt[p]] for p, s in fed})
        assert sorted(out) == sorted(s for _, s in fed), tick       # a held or idle slot is not reported
        for p, s in fed:
            nxt[p] += 1
            for k in KEEP:
                got[p][k].append(out[s][k].clone())
    assert not ses.win[1].any() and not ses.win[3].any()            # idle windows stay all zero
    return {p: {k: torch.stack(v) for k, v in d.items()} for p, d in got.items()}, ses


@pytest.fixture(scope='module', params=ARCH, ids=lambda a: 'L%dH%dT%d' % a)
def staggered(request, smpl_np):
    """Model, clips, each person's own run_clips result and the session's results for the script, shared by the tests below."""
    from tepose_amd.driver import run_clips
    from tepose_amd.testing import build_model
    L, H, T = request.param
    model, _, _ = build_model(L, H, seed=61, device='cuda', smpl_np=smpl_np, seqlen=T)
    clips = {p: _clip(NCLIP, T, 800 + i) for i, p in enumerate('ABC')}
    alone = {p: run_clips(model, [f], [th], T, keep=KEEP)[0] for p, (f, th) in clips.items()}
    got, ses = _run_script(model, T, clips)
    return model, T, clips, alone, got, ses


def test_staggered_lives_equal_each_persons_own_run(staggered):
    model, T, clips, alone, got, ses = staggered
    assert ses.graphs and ses.ticks == TICKS
    worst = 0.0
    for p, n in (('A', TICKS - 2), ('B', 6), ('C', TICKS - 9)):
        for k in KEEP:
            assert got[p][k].shape[0] == n and n <= NCLIP - T + 1
            assert torch.isfinite(got[p][k]).all(), (p, k)
            d = float((got[p][k] - alone[p][k][:n].cpu()).abs().max())
            worst = max(worst, d)
            print('person %s %-6s max|session - own run| = %.3e' % (p, k, d))
            assert d < 1e-4, (p, k, d)                               # B = 4 against B = 1 may select other kernels: the parity budget
    print('max over all = %.3e' % worst)
    again, _ = _run_script(model, T, clips)                          # a second session, the same script: the same bits
    for p in got:
        for k in KEEP:
            assert torch.equal(again[p][k], got[p][k]), (p, k)


def test_graph_and_eager_ticks_give_the_same_bits(staggered):
    model, T, clips, _, got, _ = staggered
    eager, ses = _run_script(model, T, clips, graph=False)
    assert not ses.graphs
    for p in got:
        for k in KEEP:
            assert torch.equal(eager[p][k], got[p][k]), (p, k)


def test_device_features_equal_host_features(staggered):
    model, T, clips, _, got, _ = staggered
    fed, ses = _run_script(model, T, clips, device_features=True)
    assert sorted(ses.graphs) == ['device', 'host']                  # the second variant was captured on first use
    for p in got:
        for k in KEEP:
            assert torch.equal(fed[p][k], got[p][k]), (p, k)


# ------------------------------------------------------------------ 7. a give-up inside a replayed tick
def test_a_give_up_inside_a_replayed_tick_is_repaired(smpl_np, monkeypatch):
    """As test_gpu_stream.py's test for one person: the hook is set between the healthy warm-up and the capture, so the first replay gives up.  The
    tick that gives up carries both joins."""
    from tepose_amd.stream import MultiStreamSession
    from tepose_amd.testing import build_model
    L, H, T, N, S = 2, 256, 6, 12, 2
    good, _, _ = build_model(L, H, seed=21, device='cuda', smpl_np=smpl_np)
    monkeypatch.setenv('TEPOSE_SEQ_SPIN_LIMIT', '20000')         # ~20 ms instead of ~2 s per give-up
    bad, _, _ = build_model(L, H, seed=21, device='cuda', smpl_np=smpl_np)
    monkeypatch.delenv('TEPOSE_SEQ_SPIN_LIMIT')
    clips = [_clip(N, T, 900 + i) for i in range(S)]
    keep = ('theta', 'verts')
    healthy = MultiStreamSession(good, T, S, keep=keep)
    ses = MultiStreamSession(bad, T, S, keep=keep, graph=False)   # healthy warm-up
    eng = bad._engine
    assert eng.uses_persistent(S) and not eng.degraded
    assert eng.lib.tepose_debug_set_test_fault(eng.handle, 1) == 0
    ses.use_graph = True
    with torch.no_grad(), torch.cuda.stream(ses.stream):
        ses._capture('host')                                      # kernel arguments (the unmeetable wait) are baked in here
    ses.stream.synchronize()
    assert eng.lib.tepose_debug_set_test_fault(eng.handle, 0) == 0
    for x in (healthy, ses):
        for s, (f, th) in enumerate(clips):
            x.join(s, f[:T - 1], th)
    for j in range(N - T + 1):
        feed = {s: clips[s][0][T - 1 + j] for s in range(S)}
        ref = {s: {k: v.clone() for k, v in r.items()} for s, r in healthy.push(feed).items()}
        if j == 0:
            with pytest.warns(RuntimeWarning, match='gave up') as rec:
                out = ses.push(feed)
            assert len([w for w in rec if 'gave up' in str(w.message)]) == 1
            assert eng.degraded
            for s, (f, th) in enumerate(clips):                   # what the join loaded is still there
                assert torch.equal(ses.hist[s, :, :2048].cpu(), f[:T - 1]) and torch.equal(ses.hist[s, :, 2048:].cpu(), th)
        else:
            out = ses.push(feed)
        for s in range(S):
            for k in keep:
                assert torch.isfinite(out[s][k]).all(), (k, s, j)
                assert (out[s][k] - ref[s][k]).abs().max() < 2e-5, (k, s, j)      # step kernels vs persistent kernels: rounding
    assert not good._engine.degraded


# ------------------------------------------------------------------ staleness
@pytest.mark.parametrize('graph', [True, False])
def test_an_in_place_weight_change_is_seen_by_the_next_tick(graph, smpl_np):
    """Parameters changed in place on the caller's stream, no eager forward in between: the next push re-packs (after waiting for that stream) and
    re-captures; its results are those of an eager forward on the same windows with the new weights."""
    from tepose_amd.stream import MultiStreamSession
    from tepose_amd.testing import build_model
    T, S = 2, 2
    model, _, _ = build_model(1, 64, seed=41, device='cuda', smpl_np=smpl_np, seqlen=T)
    clips = [_clip(8, T, 950 + s) for s in range(S)]
    ses = MultiStreamSession(model, T, S, keep=('theta', 'kp_3d'), graph=graph)
    for s, (f, th) in enumerate(clips):
        ses.join(s, f[:1], th)
    for j in range(3):
        ses.push({s: clips[s][0][1 + j] for s in range(S)})
    gen0 = model._engine.packed_generation
    with torch.no_grad():
        model.regressor.deccam.bias.add_(0.05)
        model.encoder.gru_fwd.weight_hh_l0.mul_(0.9)
    x = ses.win.clone()
    x[:, 0] = ses.win[:, 1]
    x[:, 1, :2048] = torch.stack([clips[s][0][4] for s in range(S)]).cuda()
    x[:, 1, 2048:] = 0
    stale = {k: v.clone() for k, v in ses.out_host.items()}
    out = ses.push({s: clips[s][0][4] for s in range(S)})
    got = {s: {k: v.clone() for k, v in out[s].items()} for s in range(S)}
    assert model._engine.packed_generation > gen0                    # re-packed by the push that followed the change
    with torch.no_grad():
        want = model(x)[0]
    for s in range(S):
        for k in ('theta', 'kp_3d'):
            assert torch.equal(got[s][k], want[k][s].cpu()), (k, s)
            assert not torch.equal(got[s][k], stale[k][s])


# ------------------------------------------------------------------ 8. errors
def test_slot_errors(smpl_np):
    from tepose_amd.stream import MultiStreamSession
    from tepose_amd.testing import build_model
    T = 2
    model, _, _ = build_model(1, 64, seed=71, device='cuda', smpl_np=smpl_np, seqlen=T)
    for slots in (0, 65):
        with pytest.raises(ValueError):
            MultiStreamSession(model, T, slots)
    f, th = _clip(4, T, 5)
    ses = MultiStreamSession(model, T, 2, keep=('theta',))
    ses.join(0, f[:1], th)
    with pytest.raises(ValueError, match='occupied'):
        ses.join(0, f[:1], th)
    with pytest.raises(ValueError, match='idle'):
        ses.leave(1)
    with pytest.raises(ValueError, match='idle'):
        ses.push({0: f[1], 1: f[1]})
    for bad in (-1, 2):
        with pytest.raises(ValueError, match='range'):
            ses.join(bad, f[:1], th)
        with pytest.raises(ValueError, match='range'):
            ses.leave(bad)
        with pytest.raises(ValueError, match='range'):
            ses.push({bad: f[1]})
    with pytest.raises(ValueError):
        ses.join(1, f[:2], th)                                    # history of the wrong length
    with pytest.raises(ValueError):
        ses.push(torch.zeros(3, 2048), slots=[0])                 # not [slots, 2048]
    # none of the refused calls changed the session: slot 0 still joins with its first frame, slot 1 is idle
    out = ses.push({0: f[1]})
    assert list(out) == [0] and torch.isfinite(out[0]['theta']).all()
    assert ses.push({}) == {}                                     # a tick in which nobody got a frame
    ses.leave(0)
    ses.join(0, f[:1], th)                                        # leave + join before a push: one join
    assert list(ses.push({0: f[1]})) == [0]
    ses.leave(0)
    assert ses.push({}) == {} and not ses.win.any()               # cleared
