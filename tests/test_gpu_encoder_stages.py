"""GPU: every stage of the temporal encoder that survives a forward -- gate pre-activations, the state of every cell step below the top layer and of the
top layer's last steps, the tail operand, the feature -- copied out of the forward's own workspace by tepose_encoder_tap and judged against the fp64
restatement of THAT stage (tests/_encoder_stages.py: bounds, exact facts and report are described and derived there; tests/test_encoder_stages_helper.py
checks them, and that CASES reaches every kernel family of the plan, without a GPU).  The feature comparisons of the other tests see the same kernels only
through GRUs that forget and a 3 Hp -> 2048 linear map.

The workspace is the test's own, filled with 0xFF bytes before the forward (NaN as fp32 and as fp16): a place no kernel wrote scores infinity.  CASES are
the smallest shapes that reach each family and edge, not the workload's."""
import ctypes

import pytest
import torch

import _encoder_stages as ES
from tepose_amd import _lib, synth

pytestmark = pytest.mark.gpu
E_SHAPE, E_WORKSPACE = -2, -3
NAN = float('nan')
STAGE = {'gi': 0, 'h': 1, 'tail': 2}

# (L, H, B, T, knobs)
CASES = [
    # granules / counters of the persistent kernel
    (2, 256, 3, 5, {}), (2, 256, 17, 5, {}), (3, 256, 64, 3, {}), (2, 1024, 37, 6, {}), (2, 256, 4, 36, {}),
    # width-first steps; Hp = 128 > H = 100: pad columns; T = 1: first steps only
    (2, 128, 100, 3, {}), (2, 100, 70, 3, {}), (2, 128, 96, 1, {}),
    # gemm_h3_kernel<GRU>
    (2, 192, 130, 3, {}),
    # 128 x 288-tile layer-0 projection
    (2, 1024, 129, 6, {}),
    # gru_step16_kernel<false>: B % 16 != 0 (row-major layer 0 under blocked layer 1); a ragged last tile of 16
    (2, 64, 641, 2, {}), (2, 64, 656, 3, {}),
    # gru_step16_kernel<true>: layer 1 only; a 3-direction plane-fed middle layer; B T = 8192: frame-major blocked layer-0 gi, barrier-free projection, gru_first16_kernel
    (2, 64, 640, 3, {}), (3, 64, 640, 3, {}), (2, 128, 1024, 8, {}),
    # one layer
    (1, 128, 40, 3, {}), (1, 320, 656, 2, {}),
    # knobs
    (2, 128, 200, 3, {'TEPOSE_EXACT_FP32': '1'}), (2, 128, 20, 3, {'TEPOSE_EXACT_FP32': '1'}),
    (2, 64, 770, 2, {'TEPOSE_EXACT_FP32': '1'}),                        # more than 768 rows: the tiled exact kernels (gemm_f32_kernel, gru_step_kernel)
    (2, 64, 640, 3, {'TEPOSE_GRU_STATE': 'fp32'}), (2, 64, 640, 3, {'TEPOSE_LARGE_BATCH_KERNELS': 'twoacc'}),
]
KNOBS = ('TEPOSE_EXACT_FP32', 'TEPOSE_LARGE_BATCH_KERNELS', 'TEPOSE_GRU_STATE', 'TEPOSE_S_MIN_B', 'TEPOSE_GI_BLK', 'TEPOSE_PERSISTENT')


def _id(c):
    return 'L%d-H%d-B%d-T%d%s' % (c[0], c[1], c[2], c[3], ''.join('-%s=%s' % (k[7:].lower(), v) for k, v in sorted(c[4].items())))


def _build(L, H, env, monkeypatch):
    from tepose_amd.testing import build_model
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model, state, _ = build_model(L, H, seed=11, device='cuda')
    model._engine.pack_encoder(model.encoder, torch.device('cuda', torch.cuda.current_device()))
    return model, state


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward(eng, x, ws):
    B, T = int(x.shape[0]), int(x.shape[1])
    feat = torch.full((B, 2048), NAN, dtype=torch.float32, device=x.device)
    _lib.check(eng.lib.tepose_encoder_fwd(eng.handle, x.data_ptr(), B, T, 0, feat.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'tepose_encoder_fwd')
    _lib.check(eng.lib.tepose_forward_status(eng.handle, ws.data_ptr(), _stream()), 'tepose_forward_status')
    return feat


def _tap(eng, B, T, stage, l, d, st, out, n, ws, ws_bytes=None):
    form = ctypes.c_int(-1)
    rc = eng.lib.tepose_encoder_tap(eng.handle, B, T, STAGE[stage], l or 0, d or 0, st or 0, out.data_ptr(), n, ctypes.byref(form), ws.data_ptr(),
                                    ws.numel() if ws_bytes is None else ws_bytes, _stream())
    return rc, form.value


def tap_all(eng, L, H, B, T, ws, feat):
    """every surviving stage, each into a NaN-filled tensor of the size the RESTATEMENT gives it (the entry refuses any other)"""
    Hp = ES.hp_of(H)
    gi, h, tail = {}, {}, None
    for stage, l, d, st in ES.surviving(L, T):
        shape = (ES.gi_slabs(L, T, l, d), B, 3 * Hp) if stage == 'gi' else (B, Hp) if stage == 'h' else (B, 3 * Hp)
        out = torch.full(shape, NAN, dtype=torch.float32, device=ws.device)
        rc, form = _tap(eng, B, T, stage, l, d, st, out, out.numel(), ws)
        _lib.check(rc, 'tepose_encoder_tap%r' % ((stage, l, d, st),))
        if stage == 'gi':
            gi[(l, d)] = (out.cpu(), form)
        elif stage == 'h':
            h[(l, d, st)] = (out.cpu(), form)
        else:
            tail = (out.cpu(), form)
    return ES.Taps(gi, h, tail, feat.cpu())


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_every_stage_against_fp64(case, monkeypatch):
    L, H, B, T, env = case
    model, state = _build(L, H, env, monkeypatch)
    eng = model._engine
    x = synth.synthetic_windows(B, T, 42)
    xg = torch.from_numpy(x).cuda()
    errs0 = int(eng.lib.tepose_debug_kernel_errors())
    ws = torch.full((int(eng.lib.tepose_workspace_bytes(eng.handle, B, T)),), 0xFF, dtype=torch.uint8, device='cuda')
    feat = _forward(eng, xg, ws)
    taps = tap_all(eng, L, H, B, T, ws, feat)
    again = _forward(eng, xg, ws)                                      # the taps left nothing behind that the next forward would see
    torch.cuda.synchronize()
    assert torch.equal(again, feat)
    plan = eng.select_kernels(B, T)
    records, failures = ES.check_stages(taps, state, x, L, H, plan, raise_on_fail=False)
    print('\n' + '\n'.join(ES.format_records(records, _id(case) + '  ')))
    if failures:
        raise ES.StageMismatch(failures)
    assert all(r['ratio'] <= 1.0 for r in records) and len(records) == len(ES.surviving(L, T)) + 1
    assert int(eng.lib.tepose_debug_kernel_errors()) == errs0          # no wave of the barrier-free kernels gave up a poll


def test_what_did_not_survive_and_wrong_sizes_are_refused_before_any_launch(monkeypatch):
    """TEPOSE_E_SHAPE for a top-layer step the ping-pong overwrote, for a layer whose projections the next layer overwrote and for a float count other
    than the stage's; TEPOSE_E_WORKSPACE for a workspace shorter than the forward's carve: nothing is written into NaN-filled buffers."""
    L, H, B, T = 3, 64, 5, 4
    model, _ = _build(L, H, {}, monkeypatch)
    eng = model._engine
    Hp = ES.hp_of(H)
    ws = torch.full((int(eng.lib.tepose_workspace_bytes(eng.handle, B, T)),), 0xFF, dtype=torch.uint8, device='cuda')
    _forward(eng, torch.from_numpy(synth.synthetic_windows(B, T, 42)).cuda(), ws)
    out = torch.full((T * B * 3 * Hp + 1,), NAN, dtype=torch.float32, device='cuda')
    nh, ng = B * Hp, T * B * 3 * Hp
    refused = [('h', 2, 0, T - 3, nh), ('h', 2, 1, 0, nh), ('h', 2, 2, 1, nh), ('h', 3, 0, 0, nh), ('h', 1, 0, T, nh),       # steps and layers that are not there
               ('gi', 1, 0, None, ng), ('gi', 1, 2, None, ng), ('gi', 3, 0, None, ng),                                        # layer 1's projections: overwritten by layer 2's
               ('h', 0, 0, 0, nh + 1), ('h', 0, 0, 0, nh - 1), ('gi', 0, 1, None, ng + 1), ('gi', 2, 2, None, ng),             # wrong counts (the top layer's d = 2 is one slab)
               ('tail', None, None, None, nh), ('tail', None, None, None, 3 * nh + 1)]
    for stage, l, d, st, n in refused:
        assert _tap(eng, B, T, stage, l, d, st, out, n, ws)[0] == E_SHAPE, (stage, l, d, st, n)
    for stage, l, d, st, n in [('h', 0, 0, 0, nh), ('gi', 0, 0, None, ng), ('gi', 2, 2, None, B * 3 * Hp), ('tail', None, None, None, 3 * nh)]:
        assert _tap(eng, B, T, stage, l, d, st, out, n, ws, ws_bytes=65536)[0] == E_WORKSPACE, (stage, l, d, st)
        assert _tap(eng, B, T, stage, l, d, st, out, n, ws, ws_bytes=1024)[0] == E_WORKSPACE, (stage, l, d, st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    rc, form = _tap(eng, B, T, 'h', 1, 2, T - 1, out, nh, ws)           # a middle layer's states all survive
    torch.cuda.synchronize()
    assert rc == 0 and form in range(5) and bool(torch.isfinite(out[:nh]).all()) and bool(torch.isnan(out[nh:]).all())
