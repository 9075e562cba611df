"""CPU: the host side of LsMultiStreamSession -- the per-slot frame counts of an LS stream under the shared slot bookkeeping,
the argument checks of the three per-slot C entries (EEND_EINVAL before any launch) and of their tensor wrappers, and the
refusal of a model that is not on the GPU.  No kernel runs here."""
import ctypes

import pytest
import torch

from fs_eend_amd.multistream import DONE, FLUSHING, OPEN, SlotTable

KEEP, PUSH, FLUSH = 0, 1, 2
EEND_EINVAL = -1


def test_slot_opened_mid_session_emits_every_frame_once():
    """LS conv_delay 9: a slot opened at step 5 beside a running one, fed 30 frames with pauses, then flushed, emits exactly 30
    frames -- the first with its 10th push, the last with its 9th zero embedding -- and steps its encoder 30 times."""
    center, T = 9, 30
    tab = SlotTable(2, center)
    a = tab.open()
    emitted, first_emit, pushed, steps = 0, None, 0, 0
    b = None
    pauses = {8, 9, 20}
    while b is None or tab.state[b] != DONE:
        if steps == 5:
            b = tab.open()
        push, flush = [a], []
        if b is not None and tab.state[b] == OPEN and steps not in pauses:
            if pushed < T:
                push.append(b)
            else:
                flush.append(b)
        plan = tab.plan(push, flush)
        if b is not None and b in push:
            assert plan.enc[b] == 1 and plan.win[b] == PUSH
            pushed += 1
        elif b is not None and tab.state[b] in (OPEN, FLUSHING) and plan.win[b] == KEEP:
            assert plan.dec[b] == 0 and plan.enc[b] == 0                       # a pause changes nothing
        if b is not None and plan.dec[b]:
            emitted += 1
            if first_emit is None:
                first_emit = pushed
        tab.commit(plan)
        steps += 1
    assert emitted == T and first_emit == center + 1
    assert tab.n_enc[b] == T and tab.n_dec[b] == T and tab.t[b] == T + center
    tab.close(b)
    assert tab.open() == b and tab.n_enc[b] == tab.n_dec[b] == tab.t[b] == 0


def test_new_entries_reject_bad_arguments(hip_lib):
    """Every per-slot entry returns EEND_EINVAL on a bad argument without launching (callable without a GPU)."""
    L = hip_lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value                   # a host address: only ever checked, never dereferenced
    st = None
    # eend_retention_step_ragged_f32(qkvg, kv, len, mask, rows_per_seq, out16, out32, N, H, eps, stream)
    assert L.eend_retention_step_ragged_f32(None, p, p, p, 1, None, p, 4, 4, 1e-6, st) == EEND_EINVAL
    assert L.eend_retention_step_ragged_f32(p, p, None, p, 1, None, p, 4, 4, 1e-6, st) == EEND_EINVAL
    assert L.eend_retention_step_ragged_f32(p, p, p, p, 1, None, None, 4, 4, 1e-6, st) == EEND_EINVAL     # no output
    assert L.eend_retention_step_ragged_f32(p, p, p, p, 3, None, p, 4, 4, 1e-6, st) == EEND_EINVAL        # N % rows_per_seq
    assert L.eend_retention_step_ragged_f32(p, p, p, p, 0, None, p, 4, 4, 1e-6, st) == EEND_EINVAL
    assert L.eend_retention_step_ragged_f32(p, p, p, p, 1, None, p, 0, 4, 1e-6, st) == EEND_EINVAL
    assert L.eend_retention_step_ragged_f32(p, p, p, p, 1, None, p, 4, 0, 1e-6, st) == EEND_EINVAL
    # eend_dwconv_step_ragged_f16(x, cache, len, mask, w, bn_w, bn_b, bn_m, bn_v, eps, out16, B, D, k, stream)
    assert L.eend_dwconv_step_ragged_f16(p, p, p, None, p, p, p, p, p, 1e-5, p, 2, 256, 16, st) == EEND_EINVAL
    assert L.eend_dwconv_step_ragged_f16(p, p, p, p, p, p, p, p, None, 1e-5, p, 2, 256, 16, st) == EEND_EINVAL
    assert L.eend_dwconv_step_ragged_f16(p, p, p, p, p, p, p, p, p, 1e-5, p, 2, 256, 1, st) == EEND_EINVAL    # k < 2
    assert L.eend_dwconv_step_ragged_f16(p, p, p, p, p, p, p, p, p, 1e-5, p, 0, 256, 16, st) == EEND_EINVAL
    # eend_window_push_f32(win, x, mode, S, k, D, stream)
    assert L.eend_window_push_f32(None, p, p, 2, 19, 256, st) == EEND_EINVAL
    assert L.eend_window_push_f32(p, p, p, 2, 0, 256, st) == EEND_EINVAL
    assert L.eend_window_push_f32(p, p, p, 0, 19, 256, st) == EEND_EINVAL
    assert L.eend_window_push_f32(p, p, p, 1 << 20, 19, 1 << 12, st) == EEND_EINVAL                   # S * D past int32


def test_wrappers_refuse_cpu_tensors(hip_lib):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(EendHipError):
        ops.retention_step_ragged(torch.zeros(2, 1024), torch.zeros(2, 4, 64, 64), i32, i32, 1, 2, 4, out32=torch.zeros(2, 256))
    bn = tuple(torch.zeros(256) for _ in range(4))
    with pytest.raises(EendHipError):
        ops.dwconv_step_ragged(torch.zeros(2, 256, dtype=torch.float16), torch.zeros(2, 256, 15), i32, i32, torch.zeros(256, 16), bn,
                               torch.zeros(2, 256, dtype=torch.float16))
    with pytest.raises(EendHipError):
        ops.window_push_f32(torch.zeros(2, 19 * 256), torch.zeros(2, 256), i32)


def test_session_refuses_a_cpu_model(hip_lib):
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.ls_model import OnlineConformerRetentionDADiarization
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    m = OnlineConformerRetentionDADiarization(n_speakers=None, in_size=345, n_units=256, n_heads=4, enc_n_layers=1, dec_n_layers=1,
                                              dropout=0.1, max_seqlen=1000, recurrent_chunk_size=50, conv_delay=9).eval()
    with pytest.raises(EendHipError):
        LsMultiStreamSession(m, slots=2, max_nspks=4)
