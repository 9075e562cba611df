"""GPU: prefill of an LS-EEND stream slot (LsMultiStreamSession.prefill) -- the chunk-parallel f32 retention against the float64
recurrence frame by frame (next to the serial chunk kernel it stands in for), its state hygiene and argument checks, the
frame-parallel conv cache bit for bit against the chunk kernel, and the session: against the reference's streaming logits and
the per-frame session, the neighbours' bits, the prefilled stream's own bits, one hour, the audio / segment wrappers, errors."""
import functools

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests.helpers import max_abs
from tests.ls_prefill_ref import ret_per_frame64
from tests.test_fs_prefill import _finish
from tests.test_ls_multistream import _Driver, _have, _model, _poison
from tests.test_ls_multistream_frames import _ret_inputs, _same

pytestmark = pytest.mark.gpu
F16, F32, I32 = torch.float16, torch.float32, torch.int32
H, D = 4, 256
NAN = float("nan")
BAR_OUT, BAR_STATE = 5e-5, 2e-6                    # the per-frame kernel's own bars (test_ls_multistream.py)

T0S = [0, 1, 63, 1000, 35999, 65537]
TS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


# ---------------------------------------------------------------------------------------------- the retention prefill
def _prefill(ops, qkvg, kv, t0, T, Nseq, dev, seq0=None, Ncache=None, tail=0, want16=True):
    """The call under test on sequences seq0 .. seq0 + Nseq - 1 of a state of Ncache sequences whose other sequences are NaN
    (as is the slot's own state at t0 == 0); qkvg and the outputs are the leading rows of buffers with `tail` NaN rows behind.
    -> out32, out16, the sequences' final state, and whether everything around them kept its bits."""
    seq0 = Nseq if seq0 is None else seq0
    Ncache = 2 * Nseq + 1 if Ncache is None else Ncache
    R = Nseq * T
    big = torch.full((Ncache, H, 64, 64), NAN)
    if t0 > 0:
        big[seq0:seq0 + Nseq] = kv
    kd = big.to(dev)
    qb = torch.full((R + tail, 4 * D), NAN)
    qb[:R] = qkvg
    qb = qb.to(dev)
    o32 = torch.full((R + tail, D), NAN, device=dev)
    o16 = torch.full((R + tail, D), NAN, dtype=F16, device=dev) if want16 else None
    ws = torch.full((ops.retention_prefill_ws(Nseq, H, T),), NAN, device=dev)
    ops.retention_prefill(qb[:R], kd, ws, seq0, Nseq, H, t0, T, 1e-6, out16=None if o16 is None else o16[:R], out32=o32[:R])
    torch.cuda.synchronize()
    kd = kd.cpu()
    around = bool(kd[:seq0].isnan().all()) and bool(kd[seq0 + Nseq:].isnan().all()) and bool(o32[R:].isnan().all())
    if o16 is not None:
        around = around and bool(o16[R:].isnan().all())
    return o32[:R].cpu(), None if o16 is None else o16[:R].cpu(), kd[seq0:seq0 + Nseq], around


def _parent(ops, qkvg, kv, t0, T, Nseq, dev):
    """The path this kernel stands in for: ops.retention_chunk_ragged chained at nmax = 64 over the same frames."""
    kd = (torch.full_like(kv, NAN) if t0 == 0 else kv).to(dev)
    q = qkvg.to(dev).view(Nseq, T, 4 * D)
    out = torch.empty(Nseq, T, D, device=dev)
    for a in range(0, T, 64):
        c = min(64, T - a)
        buf = torch.zeros(Nseq, 64, 4 * D, device=dev)
        buf[:, :c] = q[:, a:a + c]
        o = torch.empty(Nseq * 64, D, device=dev)
        ln = torch.full((Nseq,), t0 + a, dtype=I32, device=dev)
        ct = torch.full((Nseq,), c, dtype=I32, device=dev)
        ops.retention_chunk_ragged(buf.view(-1, 4 * D), kd, ln, ct, 1, Nseq, H, 64, 1e-6, out32=o)
        out[:, a:a + c] = o.view(Nseq, 64, D)[:, :c]
    torch.cuda.synchronize()
    return out.view(Nseq * T, D).cpu(), kd.cpu()


def _check_against_float64(ops, dev, Nseq, t0, T, seed):
    qkvg, kv = _ret_inputs(Nseq, T, seed)
    want_o, want_s = ret_per_frame64(qkvg.view(Nseq, T, 4 * D).numpy(), kv.numpy(), t0)
    want_o, want_s = torch.from_numpy(want_o).view(Nseq * T, D), torch.from_numpy(want_s)
    o32, o16, st, around = _prefill(ops, qkvg, kv, t0, T, Nseq, dev)
    po, ps = _parent(ops, qkvg, kv, t0, T, Nseq, dev)
    eo, es = float((o32.double() - want_o).abs().max()), float((st.double() - want_s).abs().max())
    peo, pes = float((po.double() - want_o).abs().max()), float((ps.double() - want_s).abs().max())
    bar_o = BAR_OUT if peo < BAR_OUT else 2 * peo              # the serial path's own error, where it exceeds the bar itself
    bar_s = BAR_STATE if pes < BAR_STATE else 2 * pes
    print(f"retention prefill Nseq {Nseq} t0 {t0} T {T}: outputs {eo:.2e} (serial chunks {peo:.2e}, bar {bar_o:.1e}), "
          f"state {es:.2e} (serial chunks {pes:.2e}, bar {bar_s:.1e})")
    assert torch.isfinite(o32).all() and torch.isfinite(st).all()
    assert around, "a neighbouring state sequence or a row behind the call's was written"
    assert torch.equal(o16, o32.clamp(-65504.0, 65504.0).to(F16))
    assert eo < bar_o and es < bar_s, (Nseq, t0, T, eo, es)


@pytest.mark.parametrize("t0", T0S)
@pytest.mark.parametrize("Nseq", [1, 3, 10])
def test_retention_prefill_matches_float64_recurrence(hip_lib, dev, Nseq, t0):
    """Frame by frame against the float64 recurrence at the chunk edges, with the per-frame kernel's bars (outputs 5e-5, state
    2e-6; where the serial chunk kernel itself exceeds one on a case, twice its error), NaN all around the call's state
    sequences and, at t0 == 0, in them."""
    from fs_eend_amd import ops
    for T in TS:
        _check_against_float64(ops, dev, Nseq, t0, T, seed=1000 * Nseq + T + t0 % 89)


@pytest.mark.parametrize("t0", [0, 35999])
def test_retention_prefill_1000_frames(hip_lib, dev, t0):
    from fs_eend_amd import ops
    _check_against_float64(ops, dev, 3, t0, 1000, seed=t0 + 5)


def test_retention_prefill_hygiene(hip_lib, dev):
    """Rows behind the call's (NaN) are not read: the bits are those of a run without them, with sequence i's tail chunk next
    to sequence i + 1's rows (Nseq 3, T 65); two calls give the same bits, and so does any placement in any state size."""
    from fs_eend_amd import ops
    for Nseq, t0, T in [(3, 7, 65), (1, 0, 130), (3, 0, 1), (10, 900, 63)]:
        qkvg, kv = _ret_inputs(Nseq, T, seed=Nseq + T)
        a32, a16, ast, around = _prefill(ops, qkvg, kv, t0, T, Nseq, dev, tail=70)
        assert around and torch.isfinite(a32).all() and torch.isfinite(ast).all()
        b32, b16, bst, _ = _prefill(ops, qkvg, kv, t0, T, Nseq, dev)
        assert torch.equal(a32, b32) and torch.equal(a16, b16) and torch.equal(ast, bst), (Nseq, t0, T)
        c32, _, cst, around = _prefill(ops, qkvg, kv, t0, T, Nseq, dev, seq0=0, Ncache=Nseq, want16=False)
        assert around and torch.equal(a32, c32) and torch.equal(ast, cst), (Nseq, t0, T)
        d32, d16, dst, around = _prefill(ops, qkvg, kv, t0, T, Nseq, dev, seq0=2, Ncache=Nseq + 40)
        assert around and torch.equal(a32, d32) and torch.equal(a16, d16) and torch.equal(ast, dst), (Nseq, t0, T)
    # a sequence's result does not depend on the sequences beside it in the call
    qkvg, kv = _ret_inputs(3, 65, seed=9)
    a32, _, ast, _ = _prefill(ops, qkvg, kv, 7, 65, 3, dev)
    one32, _, onest, _ = _prefill(ops, qkvg[65:130], kv[1:2], 7, 65, 1, dev)
    assert torch.equal(one32, a32[65:130]) and torch.equal(onest, ast[1:2])
    # saturation of the f16 output
    big = qkvg.clone()
    big[:, 3 * D:] = 1e6
    s32, s16, _, _ = _prefill(ops, big, kv, 7, 65, 3, dev)
    assert float(s32.abs().max()) > 65504 and torch.equal(s16, s32.clamp(-65504.0, 65504.0).to(F16)) and torch.isfinite(s16).all()


def test_prefill_entries_reject_bad_arguments(hip_lib, dev):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError, load
    L = load()
    Nseq, T, Ncache = 2, 70, 5
    q = torch.randn(Nseq * T + 1, 4 * D, device=dev)
    kv = torch.randn(Ncache, H, 64, 64, device=dev)
    o32 = torch.full((Nseq * T + 1, D), NAN, device=dev)
    o16 = torch.full((Nseq * T + 1, D), NAN, dtype=F16, device=dev)
    need = ops.retention_prefill_ws(Nseq, H, T)
    ws = torch.zeros(need, device=dev)
    kv0 = kv.clone()
    p = lambda t_: t_.data_ptr()
    call = lambda q_=p(q), kv_=p(kv), o16_=p(o16), o32_=p(o32), ws_=p(ws), wsn=need, nc=Ncache, s0=1, n=Nseq, t0=5, T_=T: \
        L.eend_retention_prefill_f32(q_, kv_, o16_, o32_, ws_, wsn, nc, s0, n, H, t0, T_, 1e-6, None)
    EINVAL = -1
    for bad in (dict(q_=None), dict(kv_=None), dict(ws_=None), dict(o16_=None, o32_=None), dict(q_=p(q) + 4), dict(kv_=p(kv) + 8),
                dict(o32_=p(o32) + 4), dict(o16_=p(o16) + 2), dict(ws_=p(ws) + 4), dict(T_=0), dict(T_=-3), dict(t0=-1),
                dict(s0=-1), dict(s0=4), dict(s0=Ncache), dict(n=0), dict(n=Ncache + 1, s0=0), dict(wsn=need - 1), dict(wsn=0)):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert torch.equal(kv, kv0) and bool(o32.isnan().all()) and bool(o16.isnan().all()) and not ws.any()
    assert call(o16_=None) == 0 and call(o32_=None) == 0                # one output is enough
    torch.cuda.synchronize()
    with pytest.raises(EendHipError):
        ops.retention_prefill(q[:Nseq * T], kv, ws, 1, Nseq, H, 5, T)                        # no output
    with pytest.raises(EendHipError):
        ops.retention_prefill(q[:Nseq * T], kv, ws, 4, Nseq, H, 5, T, out32=o32[:Nseq * T])  # sequences 4..5 of 5
    with pytest.raises(EendHipError):
        ops.retention_prefill(q[:Nseq * T], kv, ws[:need - 1], 1, Nseq, H, 5, T, out32=o32[:Nseq * T])
    with pytest.raises(EendHipError):
        ops.retention_prefill(q[:Nseq * T], kv, ws, 1, Nseq, H, -1, T, out32=o32[:Nseq * T])
    with pytest.raises(EendHipError):
        ops.retention_prefill(q[:Nseq * T - 1], kv, ws, 1, Nseq, H, 5, T, out32=o32[:Nseq * T])
    k = 16
    x16, c, w, y16 = torch.zeros(8, D, dtype=F16, device=dev), torch.zeros(3, D, k - 1, device=dev), torch.zeros(D, k, device=dev), \
        torch.zeros(8, D, dtype=F16, device=dev)
    bn = [torch.ones(D, device=dev) for _ in range(4)]
    dw = lambda x_=p(x16), c_=p(c), b=1, t0=0, T_=8: L.eend_dwconv_prefill_f16(x_, c_, b, t0, p(w), p(bn[0]), p(bn[1]), p(bn[2]), p(bn[3]),
                                                                              1e-5, p(y16), T_, 3, D, k, None)
    for bad in (dict(x_=None), dict(c_=None), dict(b=-1), dict(b=3), dict(t0=-1), dict(T_=0)):
        assert dw(**bad) == EINVAL, bad
    with pytest.raises(EendHipError):
        ops.dwconv_prefill(x16, c, 3, 0, w, bn, y16)
    with pytest.raises(EendHipError):
        ops.dwconv_prefill(x16, c, 1, 0, w, bn, y16[:7])


# ---------------------------------------------------------------------------------------------- the conv prefill
@pytest.mark.parametrize("t0", [0, 5])
def test_dwconv_prefill_bit_equal_to_chunk_chains(hip_lib, dev, t0):
    """Outputs and final cache of slot 1 of 3 equal ops.dwconv_chunk_ragged chained at nmax = 64, bit for bit, around the
    cache length k - 1 = 15 (T < k - 1: part of the old cache stays); a fresh slot's cache is NaN, the neighbours' rows are."""
    from fs_eend_amd import ops
    k, B, b = 16, 3, 1
    g = torch.Generator().manual_seed(t0 + 1)
    w = (torch.randn(D, k, generator=g) * 0.3).to(dev)
    bn = [t_.to(dev) for t_ in (torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1,
                                torch.rand(D, generator=g) + 0.5)]
    for T in [1, 2, 14, 15, 16, 17, 64, 65, 200]:
        x = (torch.randn(T, D, generator=g) * 2).to(F16).to(dev)
        cache = torch.full((B, D, k - 1), NAN)
        if t0:
            cache[b] = torch.randn(D, k - 1, generator=g)
        # reference: the chunk kernel, slot b alone advancing
        rc = cache.to(dev)
        want = torch.empty(T, D, dtype=F16, device=dev)
        for a in range(0, T, 64):
            c = min(64, T - a)
            buf = torch.zeros(B, 64, D, dtype=F16, device=dev)
            buf[b, :c] = x[a:a + c]
            o = torch.empty(B * 64, D, dtype=F16, device=dev)
            ln = torch.tensor([0, t0 + a, 0], dtype=I32, device=dev)
            ct = torch.tensor([0, c, 0], dtype=I32, device=dev)
            ops.dwconv_chunk_ragged(buf.view(-1, D), rc, ln, ct, w, bn, o, 64, 1e-5)
            want[a:a + c] = o.view(B, 64, D)[b, :c]
        cd = cache.to(dev)
        out = torch.full((T + 3, D), NAN, dtype=F16, device=dev)
        ops.dwconv_prefill(x, cd, b, t0, w, bn, out[:T], 1e-5)
        torch.cuda.synchronize()
        assert torch.equal(out[:T], want), (T, float((out[:T].float() - want.float()).abs().max()))
        assert bool(out[T:].isnan().all())
        assert torch.equal(cd[b], rc[b]) and torch.isfinite(cd[b]).all(), T
        assert bool(cd[0].isnan().all()) and bool(cd[2].isnan().all()), T


# ---------------------------------------------------------------------------------------------- the session
@functools.lru_cache(maxsize=None)
def _t120(dev):
    """The T120 case, its model and the per-frame session's logits of it (computed once, never changed)."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    ref = _Driver(LsMultiStreamSession(m, 4, meta["C"])).run({"x": (src, 0)})["x"]
    return meta, arr, m, src, ref


@pytest.mark.parametrize("P,rows", [(0, 1024), (1, 1024), (9, 1024), (10, 1024), (37, 1024), (63, 1024), (64, 1024), (65, 1024),
                                    (120, 1024), (120, 16)])
def test_session_prefill_then_step_vs_reference_and_per_frame(hip_lib, dev, P, rows):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src, ref = _t120(dev)
    T, C = meta["T"], meta["C"]
    ses = LsMultiStreamSession(m, 2, C, prefill_rows=rows)
    s = ses.open()
    y = ses.prefill(s, src[:P])
    n = max(0, P - ses.center)
    assert y.shape == (1, n, C) and y.dtype == F32
    assert (ses.table.t[s], ses.table.n_enc[s], ses.table.n_dec[s]) == (P, P, n)
    assert int(ses.len_enc[s]) == P and int(ses.len_dec[s]) == n
    out = [y]
    _finish(ses, s, src[P:], out)
    got = torch.cat(out, dim=1)
    assert got.shape == (1, T, C)
    err, gap = max_abs(got[0], arr["stream_logits"]), float((got - ref).abs().max())
    print(f"LS prefill {P} of {T} (pieces of {rows}): vs reference streaming {err:.2e}, vs per-frame session {gap:.2e}")
    assert err < 1e-3 and gap < 1e-4


def test_session_prefill_at_a_position(hip_lib, dev):
    """30 frames through step, 70 through prefill (at encoder position 30, decoder position 21), the rest through step."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src, ref = _t120(dev)
    T, C = meta["T"], meta["C"]
    ses = LsMultiStreamSession(m, 3, C)
    ses.open()
    s = ses.open()
    out = []
    for t in range(30):
        y = ses.step(push={s: src[t]})
        if s in y:
            out.append(y[s])
    y = ses.prefill(s, src[30:100].unsqueeze(0))
    assert y.shape == (1, 70, C) and ses.table.n_enc[s] == 100 and ses.table.n_dec[s] == 100 - ses.center
    out.append(y)
    _finish(ses, s, src[100:], out)
    got = torch.cat(out, dim=1)
    assert got.shape == (1, T, C)
    err, gap = max_abs(got[0], arr["stream_logits"]), float((got - ref).abs().max())
    print(f"LS step 30, prefill 70, step on: vs reference streaming {err:.2e}, vs per-frame session {gap:.2e}")
    assert err < 1e-3 and gap < 1e-4


def _state_of(ses, s):
    C = ses.C
    return ([kv[s].clone() for kv in ses.enc_kv] + [kv[s * C:(s + 1) * C].clone() for kv in ses.dec_kv] +
            [c[s].clone() for c in ses.caches] + [ses.win32[s].clone(), ses.len_enc[s].clone(), ses.len_dec[s].clone()])


def _schedule(ses, src, others, x_slot=None, P=70):
    """Three streams: `a` pushes every step, `b` pauses on some, `c` is short and is flushing when, with x_slot, a fourth stream
    is prefilled with P frames before step 47 and then pushed beside them.  -> {name: logits (1, m, C)}, the three's states"""
    slots = [ses.open() for _ in others]
    pos = [0] * len(others)
    out = {n: [] for n in ("a", "b", "c", "x")}
    px, x = P, None
    step = 0
    busy = lambda: any(ses.state(s) != "done" for s in slots) or (x is not None and ses.state(x) != "done")
    while busy():
        if step == 47 and x_slot is not None:
            assert ses.state(slots[2]) == "flushing"
            while True:                                                  # take slots until the wanted one comes up
                x = ses.open()
                if x == x_slot:
                    break
            out["x"].append(ses.prefill(x, src[:P]))
        push, flush = {}, []
        for i, s in enumerate(slots):
            if ses.state(s) != "open" or (i == 1 and step % 5 == 2):
                continue
            if pos[i] < others[i].shape[0]:
                push[s] = others[i][pos[i]]
                pos[i] += 1
            else:
                flush.append(s)
        if x is not None and ses.state(x) == "open":
            if px < src.shape[0]:
                push[x] = src[px]
                px += 1
            else:
                flush.append(x)
        y = ses.step(push=push, flush=flush)
        for name, s in zip(("a", "b", "c", "x"), slots + [x]):
            if s is not None and s in y:
                out[name].append(y[s])
        step += 1
    torch.cuda.synchronize()
    return {k: torch.cat(v, dim=1) for k, v in out.items() if v}, [_state_of(ses, s) for s in slots]


def test_prefill_leaves_the_neighbours_untouched_bit_exact(hip_lib, dev):
    """Three other slots stream, pause and flush across a prefill of a fourth: their logits and their final states keep their
    bits.  The prefilled stream gives the same bits in any slot, after a NaN-leaving occupant, graph on or off, max_frames 1 or 8."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src, ref = _t120(dev)
    T, C = meta["T"], meta["C"]
    g = torch.Generator().manual_seed(31)
    others = [(src + 0.3 * torch.randn(src.shape, generator=g).to(dev)).contiguous(), (src * 1.2).contiguous(),
              (torch.randn(45, src.shape[1], generator=g) * 2 - 3).to(dev)]
    mk = lambda **kw: LsMultiStreamSession(m, 6, C, **kw)
    plain, st_plain = _schedule(mk(), src, others)
    amid, st_amid = _schedule(mk(), src, others, x_slot=4)
    for name in ("a", "b", "c"):
        assert torch.equal(plain[name], amid[name]), f"{name}: max diff {float((plain[name] - amid[name]).abs().max()):.3e}"
    for i, (p, a) in enumerate(zip(st_plain, st_amid)):
        assert all(_same(u, v) for u, v in zip(p, a)), f"final state of neighbour {i}"

    def alone(ses, slot=0):
        while True:
            s = ses.open()
            if s == slot:
                break
        out = [ses.prefill(s, src[:70])]
        _finish(ses, s, src[70:], out)
        return torch.cat(out, dim=1)

    x0 = alone(mk())
    assert x0.shape == (1, T, C) and float((x0 - ref).abs().max()) < 1e-4
    assert torch.equal(amid["x"], x0), f"slot 4 amid traffic: max diff {float((amid['x'] - x0).abs().max()):.3e}"
    ses = mk()
    for s in range(6):
        _poison(ses, s)
    again = alone(ses, slot=3)
    assert torch.equal(again, x0), f"slot 3 after NaN occupants: max diff {float((again - x0).abs().max()):.3e}"
    eager = alone(mk(use_graph=False))
    assert torch.equal(eager, x0), f"graph off: max diff {float((eager - x0).abs().max()):.3e}"
    wide = alone(mk(max_frames=8))
    assert torch.equal(wide, x0), f"max_frames 8: max diff {float((wide - x0).abs().max()):.3e}"


def test_session_without_prefill_allocates_no_prefill_rows(hip_lib, dev):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src, ref = _t120(dev)
    ses = LsMultiStreamSession(m, 2, meta["C"])
    s = ses.open()
    ses.step(push={s: src[0]})
    assert ses._pre is None and ses.prefill_rows == 1024
    ses.prefill(s, src[1:3])
    assert ses._pre is not None


def test_one_hour_prefilled_to_frame_30000(hip_lib, dev):
    """ls_hour_stream_c10: 30 000 frames through prefill in pieces of 1024, the rest through step_frames at max_frames = 16,
    then the flush.  Reported next to the per-frame session's distance to the float64 recurrence (6.2e-5)."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    assert _have("ls_hour_stream_c10")
    meta, arr, m, src = _model("ls_hour_stream_c10", dev)
    T, C, n, P = meta["lengths"][0], meta["C"], 16, 30000
    ses = LsMultiStreamSession(m, 2, C, max_frames=n, prefill_rows=1024)
    ses.open()
    s = ses.open()
    out = [ses.prefill(s, src[:P])]
    assert out[0].shape == (1, P - ses.center, C) and int(ses.len_enc[s]) == P and int(ses.len_dec[s]) == P - ses.center
    for p in range(P, T, n):
        y = ses.step_frames(push={s: src[p:min(p + n, T)]}, flush=[s] if p + n >= T else ())
        if s in y:
            out.append(y[s])
    while ses.state(s) == "flushing":
        y = ses.step_frames()
        if s in y:
            out.append(y[s])
    got = torch.cat(out, dim=1)[0]
    assert got.shape == (T, C)
    rows = torch.as_tensor(arr["rows"], device=dev).long()
    d = (got[rows] - torch.as_tensor(arr["stream_logits"], device=dev)).abs()
    print(f"LS one hour, prefill to frame {P} in pieces of 1024: vs reference streaming max |d logit| {float(d.max()):.2e}")
    if _have("ls_hour_stream64_c10"):
        _, a64 = FX.load_case("ls_hour_stream64_c10")
        eo = (got[rows].double() - torch.as_tensor(a64["stream_logits64"], device=dev, dtype=torch.float64)).abs().flatten()
        print(f"   against the float64 recurrence: max {float(eo.max()):.2e}, mean {float(eo.mean()):.2e} (per-frame session: 6.2e-5)")
    assert float(d.max()) < 1e-3


def test_prefill_errors_and_empty_backlog(hip_lib, dev):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from fs_eend_amd.multistream import SlotError
    meta, arr, m, src, ref = _t120(dev)
    C = meta["C"]
    ses = LsMultiStreamSession(m, 3, C)
    s = ses.open()
    with pytest.raises(SlotError, match="free"):
        ses.prefill(1, src[:4])
    with pytest.raises(SlotError):
        ses.prefill(3, src[:4])
    with pytest.raises(SlotError, match="tensor"):
        ses.prefill(s, [[0.0] * src.shape[1]])
    for t in range(12):
        ses.step(push={s: src[t]})
    before = (ses.table.t[s], ses.table.n_enc[s], ses.table.n_dec[s]), _state_of(ses, s)
    for empty in (src[:0], src[:0].unsqueeze(0)):
        y = ses.prefill(s, empty)
        assert y.shape == (1, 0, C) and y.dtype == F32 and y.device == src.device
    assert ses._pre is None
    assert before[0] == (ses.table.t[s], ses.table.n_enc[s], ses.table.n_dec[s])
    assert all(torch.equal(a, b) for a, b in zip(before[1], _state_of(ses, s)))
    ses.step(flush=[s])
    assert ses.state(s) == "flushing"
    with pytest.raises(SlotError, match="flushing"):
        ses.prefill(s, src[:4])
    while ses.state(s) != "done":
        ses.step()
    with pytest.raises(SlotError, match="done"):
        ses.prefill(s, src[:4])


# ---------------------------------------------------------------------------------------------- the layers above
def test_segment_session_prefill(hip_lib, dev):
    """SegmentSession.prefill then stepping to the end gives the rttm lines of the per-frame run of the same stream.  The model
    has random weights, so 0.5 cuts no segment; the threshold is taken from the per-frame session's own probabilities (the
    middle of their widest gap between the 30th and 70th percentile), so that segments exist and no frame sits on the cut."""
    from fs_eend_amd import postproc
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src, ref = _t120(dev)
    C = meta["C"]
    stream = torch.cat([src, src.flip(0), src * 1.1]).contiguous()
    per = _Driver(LsMultiStreamSession(m, 2, C)).run({"x": (stream, 0)})["x"][0]
    pr = torch.sigmoid(per[:, 1:]).flatten().sort().values.cpu()
    mid = pr[int(0.3 * pr.numel()):int(0.7 * pr.numel())]
    gaps = mid[1:] - mid[:-1]
    at = int(gaps.argmax())
    threshold = float((mid[at] + mid[at + 1]) / 2)
    print(f"LS segment prefill: threshold {threshold:.6f} in a gap of {float(gaps[at]):.2e}")

    def run(P):
        ses = SegmentSession(LsMultiStreamSession(m, 3, C, max_frames=8), threshold=threshold, median=5)
        ses.open()
        s = ses.open()
        logits = [ses.prefill(s, stream[:P])[0]] if P else []
        polled = list(ses.poll().get(s, []))
        out = []
        _finish(ses, s, stream[P:], out)
        logits += [y[0] for y in out]
        polled += ses.poll().get(s, [])
        return ses.rttm(s, "rec"), torch.cat(logits), polled

    want, Lw, _ = run(0)
    got, Lg, polled = run(200)
    assert Lg.shape == Lw.shape == (stream.shape[0], C)
    assert want, "the stream closed no segment: the test shows nothing"
    assert got == want
    assert got == postproc.make_rttm("rec", torch.sigmoid(Lg[:, 1:]), threshold=threshold, median=5)
    tracks = [[] for _ in range(C - 1)]
    for spk, a, b in polled:
        tracks[spk].append((a, b))
    assert postproc.rttm_lines("rec", tracks) == want


def test_audio_session_prefill(hip_lib, dev):
    """AudioStreamSession.prefill of the first seconds, then push / end, against the same audio through push alone."""
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from tests.test_audio_stream import _ls_model
    from tests.test_feature_gpu import wave
    m, C = _ls_model(dev)
    y = torch.from_numpy(wave(8000 * 8 + 123, 2))
    cuts = [0, 41234, 47000, 47001, 60000, y.numel()]

    def run(first):
        ases = AudioStreamSession(LsMultiStreamSession(m, 2, C, max_frames=8))
        s = ases.open()
        out = []
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            out.append(first(ases, s, y[a:b]) if i == 0 else ases.push({s: y[a:b]})[s])
        out.append(ases.end([s])[s])
        assert ases.state(s) == "done"
        return out

    want = run(lambda ases, s, w: ases.push({s: w})[s])
    got = run(lambda ases, s, w: ases.prefill(s, w))
    assert got[0].shape == want[0].shape and got[0].shape[0] > 30 and got[0].shape[1] == C
    a, b = torch.cat(got), torch.cat(want)
    assert a.shape == b.shape
    gap = float((a - b).abs().max())
    print(f"LS audio prefill vs push: {a.shape[0]} frames, max |d logit| {gap:.2e}")
    assert gap < 1e-4
