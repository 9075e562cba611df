"""GPU: many frames per slot and step in the LS-EEND multi-stream session (LsMultiStreamSession with max_frames = n) -- the
chunk kernels bit for bit against the per-frame kernels they replace, their state hygiene and argument checks, the n-frame
session against the reference's streaming logits and against the per-frame session, the slot invariance of the n-frame step,
step() mixed with step_frames(), one hour in chunks of 16, and the audio / segment wrappers on top."""
import random

import pytest
import torch

from oracle import fixtures as FX
from tests.helpers import max_abs
from tests.test_fs_multistream_frames import _ChunkDriver, _sizes
from tests.test_ls_multistream import _Driver, _have, _model, _poison, _ret_ref64

pytestmark = pytest.mark.gpu
F16, F32, I32 = torch.float16, torch.float32, torch.int32
H, D = 4, 256
NAN = float("nan")

# positions: empty, 1, 2^k +- 1, beyond an hour (36 000 frames)
LENS = [0, 1, 2, 3, 63, 65, 1023, 1025, 35999, 40001, 65535, 65537, 0, 7]


def _counts(nmax, S, seed):
    g = torch.Generator().manual_seed(seed)
    c = [int(v) for v in torch.randint(0, nmax + 1, (S,), generator=g)]
    c[0], c[1], c[2] = nmax, 0, 1                      # a full chunk from an empty state, an idle slot, a single frame
    c[-2] = min(nmax, 2)                               # the second empty state
    return c


def _ret_inputs(Nseq, nmax, seed):
    g = torch.Generator().manual_seed(seed)
    qkvg = torch.randn(Nseq * nmax, 4 * D, generator=g)
    qkvg[:, D:2 * D] *= 0.125                                                        # k arrives scaled by dk^-0.5
    return qkvg, torch.randn(Nseq, H, 64, 64, generator=g) * 0.3


def _per_frame_retention(ops, qkvg, kv, lens, cnts, sps, nmax, dev):
    """c successive ops.retention_step_ragged calls per slot: -> state, out16, out32 in the chunk layout."""
    S = len(lens)
    Nseq = S * sps
    kd = kv.to(dev)
    ln = torch.tensor(lens, dtype=I32, device=dev)
    o16 = torch.zeros(Nseq * nmax, D, dtype=F16, device=dev)
    o32 = torch.zeros(Nseq * nmax, D, device=dev)
    q = qkvg.to(dev).view(Nseq, nmax, 4 * D)
    for j in range(nmax):
        mk = torch.tensor([1 if j < c else 0 for c in cnts], dtype=I32, device=dev)
        a16 = torch.empty(Nseq, D, dtype=F16, device=dev)
        a32 = torch.empty(Nseq, D, device=dev)
        ops.retention_step_ragged(q[:, j].contiguous(), kd, ln, mk, sps, Nseq, H, 1e-6, out16=a16, out32=a32)
        ops.counter_add_masked(ln, mk)
        o16.view(Nseq, nmax, D)[:, j] = a16
        o32.view(Nseq, nmax, D)[:, j] = a32
    return kd, o16, o32


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("nmax", [1, 4, 16, 64])
@pytest.mark.parametrize("sps", [3, 10, 1])
def test_chunk_retention_bit_equal_to_per_frame_steps(hip_lib, dev, sps, nmax):
    """Outputs (f16, f32) and final state of one chunk launch equal c successive one-frame launches bit for bit."""
    from fs_eend_amd import ops
    S = len(LENS)
    Nseq = S * sps
    cnts = _counts(nmax, S, seed=nmax + sps)
    poison = [q for q in range(Nseq) if LENS[q // sps] == 0]                         # empty states: never read
    qkvg, kv = _ret_inputs(Nseq, nmax, seed=100 * sps + nmax)
    for q in poison:
        kv[q] = NAN
    want_kv, w16, w32 = _per_frame_retention(ops, qkvg, kv, LENS, cnts, sps, nmax, dev)
    kd = kv.to(dev)
    ln, ct = torch.tensor(LENS, dtype=I32, device=dev), torch.tensor(cnts, dtype=I32, device=dev)
    o16 = torch.full((Nseq * nmax, D), NAN, dtype=F16, device=dev)
    o32 = torch.full((Nseq * nmax, D), NAN, device=dev)
    ops.retention_chunk_ragged(qkvg.to(dev), kd, ln, ct, sps, Nseq, H, nmax, 1e-6, out16=o16, out32=o32)
    torch.cuda.synchronize()
    assert torch.equal(ln.cpu(), torch.tensor(LENS, dtype=I32))                      # the lengths are not advanced here
    assert torch.equal(o32, w32), float((o32 - w32).abs().max())
    assert torch.equal(o16, w16)
    assert _same(kd, want_kv)
    for s, c in enumerate(cnts):                                                     # rows beyond the count are zero
        rows = o32.view(S, sps, nmax, D)[s, :, c:]
        assert torch.equal(rows, torch.zeros_like(rows)), s


@pytest.mark.parametrize("sps", [1, 10])
def test_chunk_retention_matches_float64_recurrence(hip_lib, dev, sps):
    """Against the float64 recurrence frame by frame, with the tolerances of the per-frame kernel's test (state 2e-6, outputs
    5e-5; a chunk here has at most 4 frames and keep <= 1, so the state error stays within a few roundings of one step's)."""
    from fs_eend_amd import ops
    nmax = 4
    lens = [0, 1, 63, 1000, 35999, 40001]
    cnts = [4, 3, 0, 2, 4, 1]
    S = len(lens)
    Nseq = S * sps
    qkvg, kv = _ret_inputs(Nseq, nmax, seed=sps)
    for q in range(Nseq):
        if lens[q // sps] == 0:
            kv[q] = NAN
    kd = kv.to(dev)
    o32 = torch.full((Nseq * nmax, D), NAN, device=dev)
    t = lambda v: torch.tensor(v, dtype=I32, device=dev)
    ops.retention_chunk_ragged(qkvg.to(dev), kd, t(lens), t(cnts), sps, Nseq, H, nmax, 1e-6, out32=o32)
    torch.cuda.synchronize()
    kd, o32 = kd.cpu(), o32.cpu()
    worst_o = worst_s = 0.0
    for q in range(Nseq):
        s = q // sps
        st = kv[q]
        for j in range(cnts[s]):
            st, want = _ret_ref64(qkvg[q * nmax + j], st, lens[s] + j)
            worst_o = max(worst_o, float((o32[q * nmax + j].double() - want).abs().max()))
        if cnts[s]:
            worst_s = max(worst_s, float((kd[q].double() - st).abs().max()))
    print(f"chunk retention vs float64 recurrence (sps {sps}): outputs {worst_o:.2e}, state {worst_s:.2e}")
    assert worst_s < 2e-6 and worst_o < 5e-5


def test_chunk_retention_state_hygiene(hip_lib, dev):
    """c = 0 leaves the state alone bit for bit beside NaN rows; t = 0 over a NaN state is the fresh-slot result; a slot's
    result depends neither on its neighbours nor on nmax."""
    from fs_eend_amd import ops
    sps, nmax = 3, 8
    lens, cnts = [5, 0, 900, 17], [0, 8, 3, 0]
    S = len(lens)
    Nseq = S * sps
    qkvg, kv = _ret_inputs(Nseq, nmax, seed=5)
    kv[3 * sps:] = NAN                                                               # slot 3 (c = 0): a NaN state stays as it is
    q = qkvg.view(Nseq, nmax, 4 * D).clone()
    q[:sps] = NAN                                                                    # slot 0 (c = 0): NaN rows are never read
    q[2 * sps:3 * sps, 3:] = NAN                                                     # slot 2: rows beyond its count
    t = lambda v: torch.tensor(v, dtype=I32, device=dev)

    def run(kv0, qq, ln, ct, n):
        kd = kv0.to(dev)
        o = torch.full((qq.shape[0] * n, D), NAN, device=dev)
        ops.retention_chunk_ragged(qq.reshape(-1, 4 * D).to(dev), kd, t(ln), t(ct), sps, qq.shape[0], H, n, 1e-6, out32=o)
        torch.cuda.synchronize()
        return kd.cpu(), o.cpu().view(qq.shape[0], n, D)

    kv_nan = kv.clone()
    kv_nan[sps:2 * sps] = NAN                                                        # slot 1 starts at t = 0 over NaN leftovers
    kd, o = run(kv_nan, q, lens, cnts, nmax)
    assert not o.isnan().any()
    for s in (0, 3):
        assert _same(kd[s * sps:(s + 1) * sps], kv_nan[s * sps:(s + 1) * sps]), s
        assert torch.equal(o[s * sps:(s + 1) * sps], torch.zeros(sps, nmax, D)), s
    assert torch.equal(o[2 * sps:3 * sps, 3:], torch.zeros(sps, nmax - 3, D))
    # slot 1 alone, on a zero state, and slot 2 alone at nmax = 3: the same bits
    kz = torch.zeros(sps, H, 64, 64)
    k1, o1 = run(kz, q[sps:2 * sps], [0], [8], nmax)
    assert torch.equal(o1, o[sps:2 * sps]) and torch.equal(k1, kd[sps:2 * sps])
    k2, o2 = run(kv[2 * sps:3 * sps], q[2 * sps:3 * sps, :3].contiguous(), [900], [3], 3)
    assert torch.equal(o2, o[2 * sps:3 * sps, :3]) and torch.equal(k2, kd[2 * sps:3 * sps])


@pytest.mark.parametrize("nmax", [1, 4, 16, 64])
def test_chunk_dwconv_bit_equal_to_per_frame_steps(hip_lib, dev, nmax):
    from fs_eend_amd import ops
    k = 15
    lens = [0, 1, 2, 13, 14, 15, 40001, 0, 7]
    B = len(lens)
    cnts = _counts(nmax, B, seed=nmax)
    g = torch.Generator().manual_seed(nmax)
    x = (torch.randn(B * nmax, D, generator=g) * 2).to(F16)
    cache = torch.randn(B, D, k - 1, generator=g)
    for b, t_ in enumerate(lens):
        if t_ == 0:
            cache[b] = NAN                                                           # read as zeros
    w = torch.randn(D, k, generator=g) * 0.3
    bn = [torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1,
          torch.rand(D, generator=g) + 0.5]
    wd, bnd = w.to(dev), [b.to(dev) for b in bn]
    t = lambda v: torch.tensor(v, dtype=I32, device=dev)
    # reference: one-frame calls
    rc, ln = cache.to(dev), t(lens)
    want = torch.zeros(B * nmax, D, dtype=F16, device=dev)
    xd = x.to(dev)
    for j in range(nmax):
        mk = t([1 if j < c else 0 for c in cnts])
        o = torch.empty(B, D, dtype=F16, device=dev)
        ops.dwconv_step_ragged(xd.view(B, nmax, D)[:, j].contiguous(), rc, ln, mk, wd, bnd, o, 1e-5)
        ops.counter_add_masked(ln, mk)
        want.view(B, nmax, D)[:, j] = o
    cd = cache.to(dev)
    out = torch.full((B * nmax, D), NAN, dtype=F16, device=dev)
    ops.dwconv_chunk_ragged(xd, cd, t(lens), t(cnts), wd, bnd, out, nmax, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert _same(cd, rc)
    for b, c in enumerate(cnts):
        assert torch.equal(out.view(B, nmax, D)[b, c:], torch.zeros(nmax - c, D, dtype=F16, device=dev)), b
        if c == 0:
            assert _same(cd[b].cpu(), cache[b]), b


def test_window_chunk_f32_exact(hip_lib, dev):
    """The stored window against a sequence of ops.window_push_f32 calls and the compacted im2col rows computed in torch:
    random pushes / dummies / emissions, a full chunk, an idle slot, flush only, push + flush in one step, and a flush
    spread over two steps."""
    from fs_eend_amd import ops
    S, k, nmax = 23, 19, 8
    g = torch.Generator().manual_seed(4)
    t = lambda v: torch.tensor(v, dtype=I32, device=dev)
    win0 = torch.randn(S, k * D, generator=g)
    wd, ref_win = win0.to(dev), win0.to(dev)
    for step in range(2):
        x = torch.randn(S * nmax, D, generator=g) * 3
        npush, ndummy, ndec = [], [], []
        for s in range(S):
            p = int(torch.randint(0, nmax + 1, (1,), generator=g))
            d = int(torch.randint(0, nmax - p + 1, (1,), generator=g))
            e = int(torch.randint(0, p + d + 1, (1,), generator=g))
            npush.append(p), ndummy.append(d), ndec.append(e)
        npush[0], ndummy[0], ndec[0] = nmax, 0, nmax                       # a full chunk that emits every window
        npush[1], ndummy[1], ndec[1] = 0, 0, 0                             # an idle slot
        npush[2], ndummy[2], ndec[2] = 0, nmax, 3                          # flushing only
        npush[3], ndummy[3], ndec[3] = 3, 5, 8                             # push + flush in one step ...
        if step == 1:
            npush[3], ndummy[3], ndec[3] = 0, 4, 4                         # ... and the rest of the flush in the next
        cols = torch.full((S * nmax, k * D), NAN, device=dev)
        ops.window_chunk_f32(wd, x.to(dev), cols, t(npush), t(ndummy), t(ndec), nmax)
        hist = [[] for _ in range(S)]
        for f in range(nmax):
            mode = [1 if f < npush[s] else 2 if f < npush[s] + ndummy[s] else 0 for s in range(S)]
            xf = torch.stack([x[s * nmax + f] for s in range(S)]).to(dev)
            ops.window_push_f32(ref_win, xf, t(mode))
            for s in range(S):
                if mode[s]:
                    hist[s].append(ref_win[s].clone())
        want = torch.zeros(S * nmax, k * D, device=dev)
        for s in range(S):
            P = npush[s] + ndummy[s]
            for i in range(ndec[s]):
                want[s * nmax + i] = hist[s][P - ndec[s] + i]
        torch.cuda.synchronize()
        assert torch.equal(wd, ref_win), step
        assert torch.equal(cols, want), step
        # the same im2col rows from the frames themselves: z = stored taps, pushed frames, zero frames
        if step == 0:
            z = torch.cat([win0[0].view(k, D), x[:nmax]])
            for i in range(nmax):
                assert torch.equal(cols[i].cpu().view(k, D), z[i + 1:i + 1 + k])


def test_spk_attn_rows_matches_per_frame_layout(hip_lib, dev):
    """The slab-layout speaker attention: frame (b, t) gives the bits the one-frame kernel gives on that frame's C rows."""
    from fs_eend_amd import ops
    B, C, Tp = 5, 10, 4
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(B, C, Tp, 768, generator=g).to(dev)
    out = torch.full((B * C * Tp, 256), NAN, device=dev)
    ops.spk_attn_rows_f32(qkv.view(-1, 768), out, B, C, Tp)
    for t_ in range(Tp):
        one = torch.empty(B * C, 256, device=dev)
        ops.spk_attn_step_f32(qkv[:, :, t_].contiguous().view(-1, 768), one, B, C)
        assert torch.equal(out.view(B, C, Tp, 256)[:, :, t_].reshape(B * C, 256), one), t_


def test_chunk_entries_reject_bad_arguments(hip_lib, dev):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError, load
    L = load()
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev)
    q, kv, o = z(20 * 4, 4 * D), z(20, H, 64, 64), z(20 * 4, D)
    ln, ct = z(4, dt=I32), z(4, dt=I32)
    with pytest.raises(EendHipError):
        ops.retention_chunk_ragged(q, kv, ln, ct, 3, 20, H, 4, out32=o)              # 20 sequences are not whole slots of 3
    with pytest.raises(EendHipError):
        ops.retention_chunk_ragged(q, kv, ln, ct, 5, 20, H, 65, out32=o)             # nmax beyond 64
    with pytest.raises(EendHipError):
        ops.retention_chunk_ragged(q, kv, ln, ct, 5, 20, H, 0, out32=o)
    with pytest.raises(EendHipError):
        ops.retention_chunk_ragged(q, kv, ln, ct, 5, 20, H, 4)                       # no output
    with pytest.raises(EendHipError):
        ops.retention_chunk_ragged(q, kv, ln, ct.float(), 5, 20, H, 4, out32=o)      # counts must be int32
    p = lambda t_: t_.data_ptr()
    EINVAL = -1
    assert L.eend_retention_chunk_ragged_f32(None, p(kv), p(ln), p(ct), 5, 4, None, p(o), 20, H, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(p(q), p(kv), p(ln), p(ct), 3, 4, None, p(o), 20, H, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(p(q), p(kv), p(ln), p(ct), 5, 65, None, p(o), 20, H, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(p(q), p(kv), p(ln), p(ct), 1, 64, None, p(o), 1 << 21, H, 1e-6, None) == EINVAL   # offsets
    x16, c, w, o16 = z(4 * 4, D, dt=F16), z(4, D, 14), z(D, 15), z(4 * 4, D, dt=F16)
    bn = [z(D) + 1 for _ in range(4)]
    with pytest.raises(EendHipError):
        ops.dwconv_chunk_ragged(x16, c, ln, ct, w, bn, o16, 65)
    with pytest.raises(EendHipError):
        ops.dwconv_chunk_ragged(x16, c, ln, ct, w, bn, o16, 8)                       # rows do not match nmax
    assert L.eend_dwconv_chunk_ragged_f16(p(x16), None, p(ln), p(ct), 4, p(w), p(bn[0]), p(bn[1]), p(bn[2]), p(bn[3]), 1e-5, p(o16),
                                          4, D, 15, None) == EINVAL
    assert L.eend_dwconv_chunk_ragged_f16(p(x16), p(c), p(ln), p(ct), 0, p(w), p(bn[0]), p(bn[1]), p(bn[2]), p(bn[3]), 1e-5, p(o16),
                                          4, D, 15, None) == EINVAL
    win, x, cols = z(4, 19 * D), z(4 * 4, D), z(4 * 4, 19 * D)
    with pytest.raises(EendHipError):
        ops.window_chunk_f32(win, x, cols, ct, ct, ct, 8)
    with pytest.raises(EendHipError):
        ops.window_chunk_f32(win, x, cols.half(), ct, ct, ct, 4)
    assert L.eend_window_chunk_f32(p(win), p(x), None, p(ct), p(ct), p(ct), 4, 4, 19, D, None) == EINVAL
    assert L.eend_window_chunk_f32(p(win), p(x), p(cols), p(ct), p(ct), p(ct), 4, 65, 19, D, None) == EINVAL
    assert L.eend_window_chunk_f32(p(win), p(x), p(cols), p(ct), p(ct), p(ct), 1 << 20, 64, 19, D, None) == EINVAL
    with pytest.raises(EendHipError):
        ops.spk_attn_rows_f32(z(40, 768), z(40, 256), 1, 17, 1)
    assert L.eend_spk_attn_rows_f32(None, p(o), 1, 10, 4, 0.125, None) == EINVAL
    assert L.eend_spk_attn_rows_f32(p(q), p(o), 1, 17, 4, 0.125, None) == EINVAL
    assert L.eend_spk_attn_rows_f32(p(q), p(o), 1, 10, 0, 0.125, None) == EINVAL


# ---------------------------------------------------------------------------------------------- the session
def _streams4(src, T, dev, seed=21):
    g = torch.Generator().manual_seed(seed)
    pert = lambda n: (src[:n] + 0.3 * torch.randn(n, src.shape[1], generator=g).to(dev)).contiguous()
    return {"gold0": src, "p1": pert(T), "p2": pert(45), "gold3": src}


@pytest.mark.parametrize("nmax", [4, 16])
def test_session_frames_vs_reference_and_per_frame(hip_lib, dev, nmax):
    """Four streams cut from ls_stream_T120 in random chunks of 0..n frames: < 1e-3 from the reference's streaming logits and
    < 1e-4 from the per-frame session on the same streams."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    T, C = meta["T"], meta["C"]
    st = _streams4(src, T, dev)
    starts = {"gold0": 0, "p1": 0, "p2": 2, "gold3": 5}
    per = _Driver(LsMultiStreamSession(m, 4, C)).run({n: (x, starts[n]) for n, x in st.items()})
    ses = LsMultiStreamSession(m, 4, C, max_frames=nmax)
    assert ses.max_frames == nmax and sorted(ses._rows) == sorted({1, nmax})
    got = _ChunkDriver(ses).run({n: (x, starts[n], _sizes(i + nmax, nmax)) for i, (n, x) in enumerate(st.items())})
    err = gap = 0.0
    for n, x in st.items():
        assert got[n].shape == per[n].shape == (1, x.shape[0], C), (n, got[n].shape)
        gap = max(gap, float((got[n] - per[n]).abs().max()))
    for n in ("gold0", "gold3"):
        err = max(err, max_abs(got[n][0], arr["stream_logits"]))
    print(f"LS n-frame session (max_frames {nmax}): vs reference streaming {err:.2e}, vs per-frame session {gap:.2e}")
    assert err < 1e-3
    assert gap < 1e-4


@pytest.mark.parametrize("use_graph", [True, False])
def test_session_frames_slot_invariance_bit_exact(hip_lib, dev, use_graph):
    """One stream fed in the same chunks: alone in slot 0; in slot 3 beside NaN-fed neighbours after a NaN-leaving occupant,
    with pauses (0-frame chunks sit at the same places); graph on or off -- the same bits."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    T, C, nmax = meta["T"], meta["C"], 8
    sizes = _sizes(3, nmax)
    mk = lambda g=use_graph: LsMultiStreamSession(m, 4, C, use_graph=g, max_frames=nmax)
    alone = _ChunkDriver(mk()).run({"x": (src, 0, sizes)})["x"]
    assert alone.shape == (1, T, C) and not alone.isnan().any()
    ses = mk()
    for s in range(4):
        _poison(ses, s)
    nan_feed = torch.full((60, src.shape[1]), NAN, device=dev)
    other = (src[:70] * 1.3).contiguous()
    out = _ChunkDriver(ses).run({"nan": (nan_feed, 0, [5, 0, 8]), "o1": (other, 0, _sizes(5, nmax)), "hold": (other[:3], 0, [1]),
                                 "x": (src, 0, sizes)}, want_slot={"nan": 0, "o1": 1, "hold": 2, "x": 3})
    assert torch.equal(out["x"], alone), f"slot 3 amid others: {float((out['x'] - alone).abs().max()):.3e}"
    # a reopened slot after a NaN stream, neighbours changed
    ses2 = mk()
    first = _ChunkDriver(ses2).run({"nan": (nan_feed, 0, [8])})
    again = _ChunkDriver(ses2).run({"x": (src, 0, sizes), "o": (other, 0, [3, 8, 0])}, want_slot={"x": 0})
    assert torch.equal(again["x"], alone)
    if use_graph:
        eager = _ChunkDriver(mk(False)).run({"x": (src, 0, sizes)})["x"]
        assert torch.equal(eager, alone)


def test_session_mixes_step_and_step_frames(hip_lib, dev):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    T, C = meta["T"], meta["C"]
    ses = LsMultiStreamSession(m, 4, C, max_frames=8)
    out = _ChunkDriver(ses).run({"a": (src, 0, _sizes(11, 8)), "b": (src, 4, _sizes(12, 8))}, per_frame=("a", "b"))
    err = max(max_abs(out[n][0], arr["stream_logits"]) for n in ("a", "b"))
    print(f"LS session, step() mixed with step_frames(): vs reference streaming {err:.2e}")
    assert out["a"].shape == (1, T, C) and err < 1e-3
    # the default session: one row set, step_frames takes one frame per slot
    from fs_eend_amd.multistream import SlotError
    one = LsMultiStreamSession(m, 2, C)
    assert one.max_frames == 1 and list(one._rows) == [1]
    s = one.open()
    with pytest.raises(SlotError):
        one.step_frames(push={s: src[:2]})
    ys = []
    for t_ in range(T):
        ys += list(one.step_frames(push={s: src[t_:t_ + 1]}).values())
    one.step_frames(flush=[s])
    assert len(ys) == T - ses.center and ys[0].shape == (1, 1, C)


def test_one_hour_in_chunks_of_16_among_other_streams(hip_lib, dev):
    """ls_hour_stream_c10 in slot 0 in chunks of 16 while other streams come and go.  Reported next to the per-frame
    session's distance to the float64 recurrence (6.2e-5)."""
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    assert _have("ls_hour_stream_c10")
    meta, arr, m, src = _model("ls_hour_stream_c10", dev)
    T, C, nmax = meta["lengths"][0], meta["C"], 16
    ses = LsMultiStreamSession(m, 4, C, max_frames=nmax)
    s0 = ses.open()
    keep = {int(r): i for i, r in enumerate(arr["rows"])}
    got = torch.zeros(len(keep), C, device=dev)
    n = pos = step = opened = 0
    life = {}
    rng = random.Random(5)
    while ses.state(s0) != "done":
        if step % 61 == 0 and len(life) < 3:
            s = ses.open()
            life[s] = [(step * 31) % (T - 4000), 500 + (step * 13) % 3000]
            opened += 1
        push, flush = {}, []
        if ses.state(s0) == "open":
            if step % 97 != 5:                                         # a pause now and then
                push[s0] = src[pos:pos + nmax]
                pos += push[s0].shape[0]
            if pos >= T:
                flush.append(s0)
        for s, (i0, left) in life.items():
            if ses.state(s) != "open" or (step + s) % 11 == 0:
                continue
            c = min(rng.randrange(0, nmax + 1), left)
            if c:
                push[s] = src[i0:i0 + c]
                life[s] = [i0 + c, left - c]
            if life[s][1] <= 0:
                flush.append(s)
        y = ses.step_frames(push=push, flush=flush)
        if s0 in y:
            for row in y[s0][0]:
                if n in keep:
                    got[keep[n]] = row
                n += 1
        for s in [s for s in life if ses.state(s) == "done"]:
            ses.close(s)
            del life[s]
        step += 1
    torch.cuda.synchronize()
    assert n == T and opened > 20
    assert int(ses.len_enc[s0]) == T and int(ses.len_dec[s0]) == T
    d = (got - torch.as_tensor(arr["stream_logits"], device=dev)).abs()
    print(f"LS one hour in chunks of 16 in slot 0: vs reference streaming max |d logit| {float(d.max()):.2e}; {opened} other streams")
    if _have("ls_hour_stream64_c10"):
        _, a64 = FX.load_case("ls_hour_stream64_c10")
        eo = (got.double() - torch.as_tensor(a64["stream_logits64"], device=dev, dtype=torch.float64)).abs().flatten()
        print(f"   against the float64 recurrence: max {float(eo.max()):.2e}, mean {float(eo.mean()):.2e} (per-frame session: 6.2e-5)")
    assert float(d.max()) < 1e-3


# ---------------------------------------------------------------------------------------------- the layers above
def test_audio_session_over_frames_session(hip_lib, dev):
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    from tests.test_audio_stream import _ls_model, audio_path, wave
    m, C = _ls_model(dev)
    waves = [wave(8000 * 3 + 4321, 1), wave(8000 * 8, 2), wave(8000 * 5 + 79, 3)]
    want = audio_path(AudioStreamSession(LsMultiStreamSession(m, 3, C)), waves, seed=7, max_chunk=20000)
    got = audio_path(AudioStreamSession(LsMultiStreamSession(m, 3, C, max_frames=8)), waves, seed=7, max_chunk=20000)
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (i, g.shape, w.shape)
        worst = max(worst, float((g - w).abs().max()))
    print(f"LS audio session, max_frames 8 vs per frame: {worst:.2e}")
    assert worst < 1e-3


def test_segment_session_over_frames_session(hip_lib, dev):
    """SegmentSession over a max_frames = 8 LS session: each slot's rttm lines are make_rttm over its whole stream of logits."""
    from fs_eend_amd import postproc
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    meta, arr, m, src = _model("ls_stream_T120", dev)
    C, nmax = meta["C"], 8
    g = torch.Generator().manual_seed(9)
    streams = [src, (src + 0.5 * torch.randn(src.shape, generator=g).to(dev)).contiguous(), src.flip(0).contiguous()]
    ses = SegmentSession(LsMultiStreamSession(m, 4, C, max_frames=nmax), threshold=0.5, median=5)
    assert ses.max_frames == nmax
    slots = [ses.open() for _ in streams]
    pos, logits = [0] * len(streams), [[] for _ in streams]
    polled = {s: [] for s in slots}
    rng = random.Random(3)
    while any(ses.state(s) != "done" for s in slots):
        push, flush = {}, []
        for i, s in enumerate(slots):
            if ses.state(s) != "open" or rng.random() < 0.2:
                continue
            c = min(rng.randrange(0, nmax + 1), streams[i].shape[0] - pos[i])
            if c:
                push[s] = streams[i][pos[i]:pos[i] + c]
                pos[i] += c
            if pos[i] >= streams[i].shape[0]:
                flush.append(s)
        for s, v in ses.step_frames(push=push, flush=flush).items():
            logits[slots.index(s)].append(v[0])
        if rng.random() < 0.3:
            for s, segs in ses.poll().items():
                polled[s] += segs
    for s, segs in ses.poll().items():
        polled[s] += segs
    for i, s in enumerate(slots):
        Lg = torch.cat(logits[i])
        assert Lg.shape == (streams[i].shape[0], C)
        want = postproc.make_rttm("rec", torch.sigmoid(Lg[:, 1:]), threshold=0.5, median=5)
        assert ses.rttm(s, "rec") == want, i
        per = [[] for _ in range(C - 1)]
        for spk, a, b in polled[s]:
            per[spk].append((a, b))
        assert postproc.rttm_lines("rec", per) == want, i
