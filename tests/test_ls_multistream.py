"""GPU: many LS-EEND streams in one session (LsMultiStreamSession) -- the per-slot state kernels against exact references, the
session against the reference's own streaming logits and against LsStreamSession, the slot invariance the design promises
(a stream's logits do not depend on its slot, its neighbours, its pauses, graph on or off, or what the slot held before) and
one slot carried through the one-hour stream while other slots come and go."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests.helpers import build_ls_mirror, max_abs

pytestmark = pytest.mark.gpu
F16, F32, I32 = torch.float16, torch.float32, torch.int32
H, D = 4, 256
NAN = float("nan")


# ---------------------------------------------------------------------------------------------- the kernels
def _ret_ref64(qkvg, kv, t):
    """One recurrent retention step of one row in float64 from a state at position t (decay 1; t == 0: empty state).
    qkvg (4D,), kv (H, 64, 64) -> new state (H, 64, 64), output (D,)."""
    x = qkvg.double()
    q, k, v, g = (x[i * D:(i + 1) * D].view(H, 64) for i in range(4))
    old = torch.zeros(H, 64, 64, dtype=torch.float64) if t == 0 else kv.double()
    new = old * np.sqrt(t / (t + 1.0)) + v[:, :, None] * k[:, None, :] / np.sqrt(t + 1.0)
    o = (new * q[:, None, :]).sum(-1)                                                # o[h][a] = sum_b q[b] kv[a][b]
    y = (o - o.mean(-1, keepdim=True)) / torch.sqrt(o.var(-1, unbiased=False, keepdim=True) + 1e-6)
    return new, (g * torch.sigmoid(g) * y).reshape(D)


def _ret_inputs(N, seed, poison_rows=()):
    g = torch.Generator().manual_seed(seed)
    qkvg = torch.randn(N, 4 * D, generator=g)
    qkvg[:, D:2 * D] *= 0.125                                                        # k arrives scaled by dk^-0.5
    kv = torch.randn(N, H, 64, 64, generator=g) * 0.3
    for n in poison_rows:
        kv[n] = NAN
    return qkvg, kv


@pytest.mark.parametrize("rps", [1, 10])
def test_ragged_retention_matches_float64_recurrence(hip_lib, dev, rps):
    from fs_eend_amd import ops
    lens = [0, 1, 2, 63, 1000, 35999, 0, 1000, 2]
    mask = [1, 1, 1, 1, 1, 1, 0, 0, 1]
    S = len(lens)
    N = S * rps
    poison = [n for n in range(N) if lens[n // rps] == 0]                            # empty states: never read
    qkvg, kv = _ret_inputs(N, seed=rps, poison_rows=poison)
    kd, qd = kv.to(dev), qkvg.to(dev)
    ln, mk = torch.tensor(lens, dtype=I32, device=dev), torch.tensor(mask, dtype=I32, device=dev)
    o32 = torch.full((N, D), NAN, device=dev)
    o16 = torch.full((N, D), NAN, dtype=F16, device=dev)
    ops.retention_step_ragged(qd, kd, ln, mk, rps, N, H, 1e-6, out16=o16, out32=o32)
    torch.cuda.synchronize()
    assert torch.equal(ln.cpu(), torch.tensor(lens, dtype=I32))                      # the lengths are not advanced here
    kd, o32, o16 = kd.cpu(), o32.cpu(), o16.cpu()
    for n in range(N):
        s = n // rps
        if not mask[s]:
            assert bool((kd[n].isnan() == kv[n].isnan()).all()) and torch.equal(kd[n].nan_to_num(), kv[n].nan_to_num()), (s, "state")
            assert torch.equal(o32[n], torch.zeros(D)) and torch.equal(o16[n], torch.zeros(D, dtype=F16)), (s, "output")
            continue
        new, out = _ret_ref64(qkvg[n], kv[n], lens[s])
        es = float((kd[n].double() - new).abs().max())
        eo = float((o32[n].double() - out).abs().max())
        assert es < 2e-6 and eo < 5e-5, (s, lens[s], es, eo)
        assert torch.equal(o16[n], o32[n].to(F16)), s
    assert torch.isfinite(o32).all()


@pytest.mark.parametrize("t", [0, 1, 7, 999, 35999])
def test_ragged_retention_bit_equal_to_uniform_step(hip_lib, dev, t):
    """All masks on, every slot at position t: bit for bit eend_retention_step_f32 with scale_in = t, for the state and both
    outputs -- at t = 0 with the ragged kernel's state NaN-poisoned and the uniform kernel's zeroed."""
    from fs_eend_amd import ops
    S, rps = 6, 10
    N = S * rps
    qkvg, kv = _ret_inputs(N, seed=100 + t)
    if t == 0:
        kv.zero_()
    qd = qkvg.to(dev)
    k_uni = kv.to(dev)
    k_rag = torch.full_like(k_uni, NAN) if t == 0 else k_uni.clone()
    s_in, s_out = torch.full((H,), float(t), device=dev), torch.empty(H, device=dev)
    u16, u32 = torch.empty(N, D, dtype=F16, device=dev), torch.empty(N, D, device=dev)
    ops.retention_step_f32(qd, k_uni, s_in, s_out, u16, N, H, 1e-6, out32=u32)
    r16, r32 = torch.empty_like(u16), torch.empty_like(u32)
    ln, mk = torch.full((S,), t, dtype=I32, device=dev), torch.ones(S, dtype=I32, device=dev)
    ops.retention_step_ragged(qd, k_rag, ln, mk, rps, N, H, 1e-6, out16=r16, out32=r32)
    torch.cuda.synchronize()
    assert float(s_out[0]) == t + 1
    assert torch.equal(k_rag, k_uni)
    assert torch.equal(r32, u32) and torch.equal(r16, u16)


def test_ragged_retention_paused_states_untouched(hip_lib, dev):
    from fs_eend_amd import ops
    S, rps = 12, 10
    N = S * rps
    qkvg, kv = _ret_inputs(N, seed=7)
    kv[5 * rps:6 * rps] = NAN                                                        # a NaN-holding paused slot stays as it is
    kd = kv.to(dev)
    mask = torch.tensor([1, 0] * (S // 2), dtype=I32, device=dev)
    ln = torch.tensor([3 * s + 1 for s in range(S)], dtype=I32, device=dev)
    o32 = torch.full((N, D), NAN, device=dev)
    ops.retention_step_ragged(qkvg.to(dev), kd, ln, mask, rps, N, H, 1e-6, out32=o32)
    torch.cuda.synchronize()
    kd, o32 = kd.cpu(), o32.cpu()
    for s in range(1, S, 2):
        r = slice(s * rps, (s + 1) * rps)
        assert torch.equal(kd[r].nan_to_num(), kv[r].nan_to_num()) and torch.equal(kd[r].isnan(), kv[r].isnan()), s
        assert torch.equal(o32[r], torch.zeros(rps, D)), s
    assert torch.isfinite(o32).all()


def test_ragged_retention_rejects_bad_arguments(hip_lib, dev):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError
    q = torch.zeros(20, 4 * D, device=dev)
    kv = torch.zeros(20, H, 64, 64, device=dev)
    o = torch.zeros(20, D, device=dev)
    ln = mk = torch.zeros(2, dtype=I32, device=dev)
    with pytest.raises(EendHipError):
        ops.retention_step_ragged(q, kv, ln, mk, 3, 20, H, out32=o)                 # 20 rows are not whole sequences of 3
    with pytest.raises(EendHipError):
        ops.retention_step_ragged(q, kv, ln, mk, 5, 20, H, out32=o)                 # 4 sequences, 2 lengths
    with pytest.raises(EendHipError):
        ops.retention_step_ragged(q, kv, ln, mk, 10, 20, H)                          # no output
    with pytest.raises(EendHipError):
        ops.retention_step_ragged(q, kv, ln.float(), mk, 10, 20, H, out32=o)         # lengths must be int32


def test_ragged_dwconv_bit_equal_to_uniform_step(hip_lib, dev):
    """Active slots: bit for bit eend_dwconv_step_f16 on the same cache (len 0: on a zero cache while the ragged kernel's holds
    NaN); paused slots: cache untouched, output row zero."""
    from fs_eend_amd import ops
    B, k = 9, 16
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(D, k, generator=g) * 0.3).to(dev)
    bn = tuple(t.to(dev) for t in (torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1,
                                   torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) + 0.5))
    lens = [0, 1, 5, 40000, 0, 3, 2, 0, 17]
    mask = [1, 1, 1, 1, 0, 0, 1, 1, 0]
    x = torch.randn(B, D, generator=g).to(F16).to(dev)
    cache = torch.randn(B, D, k - 1, generator=g)
    for b in range(B):
        if lens[b] == 0:
            cache[b] = NAN
    cd = cache.to(dev)
    out = torch.full((B, D), NAN, dtype=F16, device=dev)
    ops.dwconv_step_ragged(x, cd, torch.tensor(lens, dtype=I32, device=dev), torch.tensor(mask, dtype=I32, device=dev), w, bn, out,
                           1e-5)
    for b in range(B):
        if mask[b]:
            c1 = torch.zeros(1, D, k - 1, device=dev) if lens[b] == 0 else cache[b:b + 1].to(dev)
            o1 = torch.empty(1, D, dtype=F16, device=dev)
            ops.dwconv_step(x[b:b + 1].contiguous(), c1, w, bn, o1, 1e-5)
            assert torch.equal(out[b:b + 1], o1), b
            assert torch.equal(cd[b:b + 1], c1), b
        else:
            assert torch.equal(out[b], torch.zeros(D, dtype=F16, device=dev)), b
            got = cd[b].cpu()
            assert torch.equal(got.nan_to_num(), cache[b].nan_to_num()) and torch.equal(got.isnan(), cache[b].isnan()), b


def test_window_push_f32_exact(hip_lib, dev):
    from fs_eend_amd import ops
    S, k = 70, 19
    g = torch.Generator().manual_seed(3)
    win = torch.randn(S, k * D, generator=g)
    x = torch.randn(S, D, generator=g) * 3
    mode = torch.randint(0, 4, (S,), generator=g, dtype=I32)                         # 3: not a mode, leaves the slot alone
    mode[:3] = torch.tensor([0, 1, 2], dtype=I32)
    wd = win.to(dev)
    ops.window_push_f32(wd, x.to(dev), mode.to(dev))
    want = win.clone()
    for s in range(S):
        if mode[s] in (1, 2):
            want[s, :(k - 1) * D] = win[s, D:]
            want[s, (k - 1) * D:] = x[s] if mode[s] == 1 else 0
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu(), want)


# ---------------------------------------------------------------------------------------------- the session
def _model(case, dev):
    meta, arr = FX.load_case(case)
    m = build_ls_mirror(meta).to(dev)
    T = meta["lengths"][0] if "lengths" in meta else meta["T"]
    src = FX.make_src([T], meta["in_size"], meta["xseed"])[0].to(dev)
    return meta, arr, m, src


class _Driver:
    """Feeds scripted streams through a session: streams[name] = (frames, start step); a stream takes a slot at its start
    step, pushes its frames (skipping the steps in `pauses[name]`), flushes and closes when done."""

    def __init__(self, ses):
        self.ses, self.out, self.slot = ses, {}, {}

    def run(self, streams, pauses=None, closes=None, want_slot=None):
        pauses, closes, want_slot = pauses or {}, closes or {}, want_slot or {}
        pos = {n: 0 for n in streams}
        step = 0
        while True:
            for n, (_, start) in streams.items():
                if start == step:
                    self.slot[n] = self.ses.open()
                    self.out[n] = []
                    if n in want_slot:
                        assert self.slot[n] == want_slot[n], (n, self.slot[n])
            for n, at in closes.items():
                if at == step and n in self.slot:
                    self.ses.close(self.slot.pop(n))
            push, flush = {}, []
            for n, s in self.slot.items():
                fr = streams[n][0]
                if self.ses.state(s) != "open" or step in pauses.get(n, ()):
                    continue
                if pos[n] < len(fr):
                    push[s] = fr[pos[n]]
                    pos[n] += 1
                else:
                    flush.append(s)
            y = self.ses.step(push=push, flush=flush)
            by_slot = {s: n for n, s in self.slot.items()}
            for s, v in y.items():
                self.out[by_slot[s]].append(v)
            for n, s in list(self.slot.items()):
                if self.ses.state(s) == "done":
                    self.ses.close(s)
                    del self.slot[n]
            step += 1
            if not self.slot and all(start < step for _, start in streams.values()):
                return {n: torch.cat(v, dim=1) for n, v in self.out.items() if v}


def _single(m, src, C):
    from fs_eend_amd.ls_stream import LsStreamSession
    one = LsStreamSession(m, C, batch=1)
    ys = [one.push(src[t:t + 1]) for t in range(src.shape[0])]
    return torch.cat([y for y in ys if y is not None] + one.flush(), dim=1)


def test_session_vs_reference_and_single_stream(hip_lib, dev):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    T, C = meta["T"], meta["C"]
    g = torch.Generator().manual_seed(21)
    pert = lambda n: (src[:n] + 0.3 * torch.randn(n, src.shape[1], generator=g).to(dev)).contiguous()
    ses = LsMultiStreamSession(m, 4, C)
    streams = {"gold0": (src, 0), "p1": (pert(T), 0), "hold2": ([], 0), "p3": (pert(45), 3),
               "gold2": (src, 17), "p1b": (pert(25), 52)}
    out = _Driver(ses).run(streams, pauses={"p3": range(20, 26), "gold2": [40, 41, 90]}, closes={"hold2": 1, "p1": 50},
                           want_slot={"gold0": 0, "p1": 1, "hold2": 2, "p3": 2, "gold2": 3, "p1b": 1})
    a, b = out["gold0"], out["gold2"]
    assert a.shape == (1, T, C) and b.shape == (1, T, C)
    assert torch.equal(a, b), f"slot 0 vs slot 3 (late, paused): {float((a - b).abs().max()):.3e}"
    assert out["p3"].shape == (1, 45, C) and out["p1b"].shape == (1, 25, C)
    err = max_abs(a[0], arr["stream_logits"])
    gap = float((a - _single(m, src, C)).abs().max())
    print(f"LS multi-stream session: vs reference streaming {err:.2e}, vs LsStreamSession(batch=1) {gap:.2e}")
    assert err < 1e-3 and gap < 1e-4


def _poison(ses, s):
    """What a misbehaving previous occupant could leave in slot s: NaN in every piece of its state."""
    C = ses.C
    for kv in ses.enc_kv:
        kv[s] = NAN
    for kv in ses.dec_kv:
        kv[s * C:(s + 1) * C] = NAN
    for c in ses.caches:
        c[s] = NAN
    ses.win32[s] = NAN


@pytest.mark.parametrize("use_graph", [True, False])
def test_slot_invariance_bit_exact(hip_lib, dev, use_graph):
    """One stream's logits, bit for bit: alone in slot 0; in slot 7 amid other streams that join and leave (one of them fed
    NaN features, the free slots NaN-poisoned); paused for some frames; in a slot whose previous occupant left NaN state."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    C = meta["C"]
    src = src[:70].contiguous()
    g = torch.Generator().manual_seed(5)
    other = lambda n: (torch.randn(n, src.shape[1], generator=g) * 2 - 3).to(dev)
    mk = lambda: LsMultiStreamSession(m, 8, C, use_graph=use_graph)

    alone = _Driver(mk()).run({"x": (src, 0)})["x"]
    ses = mk()
    for s in range(8):
        _poison(ses, s)
    nan_stream = other(40)
    nan_stream[10:] = NAN
    crowd = {f"o{i}": (other(20 + 9 * i), 0) for i in range(6)}
    crowd.update({"nan": (nan_stream, 0), "x": (src, 3), "o7": (other(30), 40), "o8": (other(12), 60)})
    amid = _Driver(ses).run(crowd, closes={"o3": 50}, want_slot={"nan": 6, "x": 7, "o7": 0, "o8": 1})["x"]
    paused = _Driver(mk()).run({"x": (src, 0), "o": (other(50), 0)}, pauses={"x": [5, 6, 7, 30, 41, 42]})["x"]
    ses = mk()
    dr = _Driver(ses)
    bad = other(50)
    bad[20:] = NAN
    dr.run({"bad": (bad, 0)})
    assert bool(ses.enc_kv[0][0].isnan().any()) and bool(ses.dec_kv[0][:C].isnan().any())   # the slot does hold NaN now
    _poison(ses, 0)
    reopened = dr.run({"x": (src, 0)}, want_slot={"x": 0})["x"]
    for name, got in (("amid traffic in slot 7", amid), ("paused", paused), ("reopened after NaN", reopened)):
        assert got.shape == alone.shape, name
        assert torch.equal(got, alone), f"{name}: max diff {float((got - alone).abs().max()):.3e}"
    full = alone.shape[1] - m.delay                  # the last conv_delay frames of the cut stream see zero look-ahead frames
    assert max_abs(alone[0, :full], arr["stream_logits"][:full]) < 1e-3
    if use_graph:
        eager = _Driver(LsMultiStreamSession(m, 8, C, use_graph=False)).run({"x": (src, 0)})["x"]
        assert torch.equal(eager, alone)


def test_session_survives_a_weight_refresh(hip_lib, dev):
    """The captured graph points into the model's operand copies: after load_state_dict mid-stream (same values, new copies,
    the old ones freed and scribbled over) the session captures again and keeps every slot's state -- not a bit changes."""
    import gc
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    C = meta["C"]
    src = src[:60].contiguous()

    def run(refresh):
        ses = LsMultiStreamSession(m, 2, C)
        a, b = ses.open(), ses.open()
        ys = []
        for t in range(src.shape[0]):
            if refresh and t == 30:
                g0 = ses._graph
                m.load_state_dict({k_: v.clone() for k_, v in m.state_dict().items()})
                gc.collect()
                torch.cuda.empty_cache()
                junk = torch.full((64 * 1024 * 1024,), NAN, device=dev)
                del junk
            y = ses.step(push={a: src[t], b: src[-1 - t]})
            if refresh and t == 30:
                assert ses._graph is not g0
            if a in y:
                ys.append(y[a])
        return torch.cat(ys, dim=1)

    y0, y1 = run(False), run(True)
    assert torch.equal(y0, y1)
    assert max_abs(y0[0], arr["stream_logits"][:y0.shape[1]]) < 1e-3


def _have(name):
    return os.path.exists(os.path.join(FX.GOLDEN_DIR, name + ".npz"))


def test_one_hour_in_one_slot_among_other_streams(hip_lib, dev):
    """ls_hour_stream_c10 in slot 0 of a 4-slot session for the whole hour, paused at a few frames, while the other slots open,
    pause, flush and close on a fixed schedule: the per-slot scale stays exact to t = 36 000."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    assert _have("ls_hour_stream_c10")
    meta, arr, m, src = _model("ls_hour_stream_c10", dev)
    T, C = meta["lengths"][0], meta["C"]
    ses = LsMultiStreamSession(m, 4, C)
    s0 = ses.open()
    pauses = {7, 1000, 1001, 20000, 35990}
    keep = {int(r): i for i, r in enumerate(arr["rows"])}
    got = torch.zeros(len(keep), C, device=dev)
    n = pos = step = opened = 0
    life = {}                                       # other slot -> [first frame index into src, frames left]
    while ses.state(s0) != "done":
        if step % 997 == 0 and len(life) < 3:
            s = ses.open()
            life[s] = [(step * 31) % (T - 4000), 500 + (step * 13) % 3000]
            opened += 1
        push, flush = {}, []
        if pos < T:
            if step not in pauses:
                push[s0] = src[pos]
                pos += 1
        elif ses.state(s0) == "open":
            flush.append(s0)
        for s, (i0, left) in life.items():
            if ses.state(s) != "open" or (step + s) % 11 == 0:
                continue
            if left > 0:
                push[s] = src[i0]
                life[s] = [i0 + 1, left - 1]
            else:
                flush.append(s)
        y = ses.step(push=push, flush=flush)
        if s0 in y:
            if n in keep:
                got[keep[n]] = y[s0][0, 0]
            n += 1
        for s in [s for s in life if ses.state(s) == "done"]:
            ses.close(s)
            del life[s]
        step += 1
    torch.cuda.synchronize()
    assert n == T and opened > 20
    assert int(ses.len_enc[s0]) == T and int(ses.len_dec[s0]) == T
    want = torch.as_tensor(arr["stream_logits"], device=dev)
    d = (got - want).abs()
    print(f"LS one hour in slot 0 of a 4-slot session: vs reference streaming max |d logit| {float(d.max()):.2e} "
          f"(first 600 {float(d[:600].max()):.2e}, last 600 {float(d[-600:].max()):.2e}); {opened} other streams")
    assert float(d.max()) < 1e-3
    if _have("ls_hour_stream64_c10"):
        _, a64 = FX.load_case("ls_hour_stream64_c10")
        truth = torch.as_tensor(a64["stream_logits64"], device=dev, dtype=torch.float64)
        eo = (got.double() - truth).abs().flatten()
        print(f"   against the float64 recurrence: max {float(eo.max()):.2e}, mean {float(eo.mean()):.2e}")
        assert float(eo.max()) < 3e-4 and float(eo.mean()) < 3e-5
