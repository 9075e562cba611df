"""GPU: a stream slot of FsMultiStreamSession suspended to a StreamSnapshot and resumed -- in another slot, another session
(other slot count, cache capacity, max_frames, graph setting), through the host and through a file -- goes on bit for bit as the
uninterrupted stream; so do a flushing slot, a fork, the neighbours, and the wrappers' own state (SegmentSession here).

An FS stream's logits depend on how its frames were cut into steps (the chunk attention sums in another order than the
per-frame decode), so every comparison is against an uninterrupted stream that took the same frames in the same steps.
Sessions here have 3 or 4 slots on purpose.  A session's linears take the skinny kernels up to 16 rows and the tiled GEMM above,
and the two sum in different orders: a stream's logits are bit-equal between sessions whose row counts fall on the same side
(slots * C <= 16 decoder rows, or more; slots * max_frames <= 16 encoder rows, or more), and differ by ~3e-5 across it.  Moving a
stream across that line keeps its state exactly but not the bits of the logits that follow."""
import pytest
import torch

from tests.helpers import max_abs

pytestmark = pytest.mark.gpu
DELAY = 9                                                         # the look-ahead: frame u is emitted with frame u + 9


@pytest.fixture(scope="module")
def fs(hip_lib, dev):
    from tests.test_fs_multistream import _models
    meta, arr, sm, src = _models("fs_stream_T60", dev)
    assert sm.cnn.center == DELAY
    return meta, arr, sm, src


def _ses(fs, slots, C=None, **kw):
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    kw.setdefault("cap", 64)
    return FsMultiStreamSession(fs[2], slots, fs[0]["C"] if C is None else C, **kw)


def _play(ses, s, src, a, b, n, out, flush=False):
    """Frames a .. b - 1 of src to slot s, one per step() when n == 1 and in step_frames() chunks of n otherwise; with `flush`
    the stream then ends and is stepped to done the same way.  Emitted logits are appended to out."""
    step = ses.step if n == 1 else ses.step_frames
    take = lambda y: out.append(y[s].reshape(-1, y[s].shape[-1])) if s in y else None
    for i in range(a, b, n):
        take(step({s: src[i] if n == 1 else src[i:min(i + n, b)]}))
    if flush:
        take(step(flush=[s]))
        while ses.state(s) == "flushing":
            take(step())
        assert ses.state(s) == "done"


_REF = {}


def _uninterrupted(fs, t, na, nb):
    """The golden stream through one slot of one session: frames [0, t) in steps of na frames, the rest in steps of nb."""
    key = (t if (na, nb) != (1, 1) else 0, na, nb)              # one frame per step throughout: the cut does not show
    if key not in _REF:
        src = fs[3]
        ses = _ses(fs, 3, max_frames=max(na, nb), use_graph=False)
        s, out = ses.open(), []
        _play(ses, s, src, 0, t, na, out)
        _play(ses, s, src, t, src.shape[0], nb, out, flush=True)
        _REF[key] = torch.cat(out)
    return _REF[key]


def test_uninterrupted_stream_matches_the_fixture(fs):
    meta, arr, _, _ = fs
    for na, nb in ((1, 1), (1, 4), (4, 1)):
        ref = _uninterrupted(fs, 17, na, nb)
        assert ref.shape == (meta["T"], meta["C"])
        assert max_abs(ref, arr["stream_logits"]) < 1e-3


def _host(snap, tmp_path):
    return snap.to("cpu")


def _file(snap, tmp_path):
    from fs_eend_amd.multistream import StreamSnapshot
    path = str(tmp_path / "slot.snap")
    snap.save(path)
    return StreamSnapshot.load(path)


# how the stream travels: (frames per step before, after, first session, second session (None: the same one), the snapshot's way)
ROUTES = {
    "same-session": (1, 1, dict(slots=3), None, None),
    "other-1to4": (1, 4, dict(slots=3), dict(slots=4, cap=16, max_frames=4, use_graph=False), None),
    "other-4to1": (4, 1, dict(slots=3, cap=16, max_frames=4, use_graph=False), dict(slots=4, cap=16), None),
    "host": (1, 1, dict(slots=3, use_graph=False), dict(slots=4, cap=16), _host),
    "file": (1, 1, dict(slots=4), dict(slots=3, cap=32, use_graph=False), _file),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("t", [0, 1, 8, 9, 10, 17, -1, None], ids=lambda t: {-1: "T-1", None: "T"}.get(t, str(t)))
def test_cut_and_resume_bit_equal(fs, tmp_path, t, route):
    meta, _, _, src = fs
    T = meta["T"]
    t = T if t is None else T + t if t < 0 else t
    na, nb, kw_a, kw_b, via = ROUTES[route]
    want = _uninterrupted(fs, t, na, nb)
    A = _ses(fs, **kw_a)
    hold = A.open()                                               # slot 0, idle; the stream runs in slot 1
    sa, out = A.open(), []
    _play(A, sa, src, 0, t, na, out)
    snap = A.suspend(sa)
    assert A.state(sa) == "free" and snap.kind == "fs" and snap.table["t"] == t and snap.device == A.dev
    assert snap.nbytes == snap.parts["model"]["blob"].numel() > 0
    if via is not None:
        snap = via(snap, tmp_path)
        assert snap.device.type == "cpu" and snap.table["n_enc"] == t
    if kw_b is None:
        B = A
        A.close(hold)                                             # the lowest free slot is now another one than the stream left
        sb = B.resume(snap)
        assert sb == hold != sa
    else:
        B = _ses(fs, **kw_b)
        assert B.open() == 0
        cap0 = B.cap
        sb = B.resume(snap)
        assert sb == 1 and B.cap == (cap0 if t < cap0 else 2 * cap0 if t < 2 * cap0 else 4 * cap0)    # grown by resume itself
    assert B.state(sb) == "open" and (B.table.t[sb], B.table.n_enc[sb], B.table.n_dec[sb]) == (t, t, max(0, t - DELAY))
    _play(B, sb, src, t, T, nb, out, flush=True)
    got = torch.cat(out)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"max diff {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("left", [9, 4, 1])
def test_flushing_slot_resumes_to_a_bit_equal_tail(fs, left):
    """Suspended while flushing with `left` dummy frames to go (9: flushed with a full chunk of pushes, none taken yet)."""
    meta, _, _, src = fs
    T, C = meta["T"], meta["C"]
    n = 4 if left == DELAY else 1

    def run(cut):
        ses = _ses(fs, 3, max_frames=n)
        step = lambda: ses.step if n == 1 else ses.step_frames
        s, out = ses.open(), []
        take = lambda y: out.append(y[s].reshape(-1, C)) if s in y else None
        if n == 4:
            _play(ses, s, src, 0, T - 4, 4, out)
            take(ses.step_frames({s: src[T - 4:]}, flush=[s]))    # a full chunk and the flush: its dummies all follow later
        else:
            _play(ses, s, src, 0, T, 1, out)
            take(ses.step(flush=[s]))                             # the first dummy frame goes with the flush
            for _ in range(DELAY - left - 1):
                take(ses.step())
        assert ses.state(s) == "flushing" and ses.table.flush_left[s] == left
        if cut:
            snap = ses.suspend(s)
            assert snap.table["state"] == "flushing" and snap.table["flush_left"] == left
            ses = _ses(fs, 4, cap=16, max_frames=n, use_graph=False)
            ses.open()
            s = ses.resume(snap)
            assert s == 1 and ses.state(s) == "flushing"
        while ses.state(s) == "flushing":
            take(step()())
        assert ses.state(s) == "done"
        return torch.cat(out)

    whole, resumed = run(False), run(True)
    assert whole.shape == (T, C) and torch.equal(whole, resumed)
    if n == 1:
        assert torch.equal(whole, _uninterrupted(fs, 0, 1, 1))


def test_snapshot_forks_a_stream(fs):
    meta, _, _, src = fs
    T = meta["T"]
    ses = _ses(fs, 3, cap=32)
    a, out_a, out_b = ses.open(), [], []
    _play(ses, a, src, 0, 20, 1, out_a)
    snap = ses.snapshot(a)
    assert ses.state(a) == "open" and ses.table.t[a] == 20        # the slot is untouched and goes on
    b = ses.resume(snap)
    assert b == 1
    out_b += out_a
    for i in range(20, T):                                        # the same frames to both, in the same steps
        y = ses.step({a: src[i], b: src[i]})
        out_a.append(y[a].reshape(1, -1)), out_b.append(y[b].reshape(1, -1))
    y = ses.step(flush=[a, b])
    while True:
        out_a.append(y[a].reshape(1, -1)), out_b.append(y[b].reshape(1, -1))
        if ses.state(a) == "done":
            break
        y = ses.step()
    assert ses.state(b) == "done"
    ga, gb = torch.cat(out_a), torch.cat(out_b)
    assert torch.equal(ga, gb) and torch.equal(ga, _uninterrupted(fs, 0, 1, 1))
    c = ses.resume(snap)                                          # a snapshot can be resumed more than once
    assert c == 2 and ses.table.t[c] == 20


def test_neighbour_is_undisturbed_and_the_freed_slot_is_reused(fs):
    """A neighbour streams through suspends, resumes (one growing the caches), a fork and closes around it."""
    meta, _, _, src = fs
    T, C = meta["T"], meta["C"]
    g = torch.Generator().manual_seed(31)
    nsrc = (src + 0.3 * torch.randn(src.shape, generator=g).to(src.device)).contiguous()
    solo = _ses(fs, 3, cap=16)
    s, want = solo.open(), []
    _play(solo, s, nsrc, 0, T, 1, want, flush=True)
    ses = _ses(fs, 4, cap=16)
    first = ses.open()                                            # slot 0: leaves early
    nb, got = ses.open(), []                                      # slot 1: the neighbour
    x, snaps = ses.open(), {}                                     # slot 2: the stream that comes and goes
    for i in range(T):
        push = {nb: nsrc[i]}
        if ses.state(x) == "open":
            push[x] = src[i]
        y = ses.step(push)
        got.append(y[nb].reshape(1, -1)) if nb in y else None
        if i == 5:
            ses.close(first)
        if i == 12:
            snaps[12] = ses.suspend(x)
            assert ses.state(x) == "free" and ses.open() == first and ses.open() == x     # the freed slots are handed out again
            ses.close(first), ses.close(x)
            x = ses.resume(snaps[12])
            assert x == first
        if i == 30:                                               # a fork: the original goes on in its slot
            snaps[30] = ses.snapshot(x)
            assert ses.resume(snaps[30]) == 2
        if i == 40:
            ses.close(x)
    _play(ses, nb, nsrc, T, T, 1, got, flush=True)
    assert torch.equal(torch.cat(got), torch.cat(want))
    small = _ses(fs, 3, cap=16)                                   # ... and here resume itself grows the caches, beside a neighbour
    nb, got = small.open(), []
    _play(small, nb, nsrc, 0, 10, 1, got)
    assert small.cap == 16 and small.resume(snaps[30]) == 1 and small.cap == 32
    _play(small, nb, nsrc, 10, T, 1, got, flush=True)
    assert torch.equal(torch.cat(got), torch.cat(want))


def test_resume_over_the_stale_rows_of_a_longer_stream(fs):
    meta, _, _, src = fs
    T = meta["T"]
    A = _ses(fs, 3)
    s, out = A.open(), []
    _play(A, s, src, 0, 17, 1, out)
    snap = A.suspend(s)
    B = _ses(fs, 4, cap=16)
    g = torch.Generator().manual_seed(8)
    junk = (torch.randn(45, src.shape[1], generator=g) * 2 - 3).to(src.device)
    junk[30:] = float("nan")
    s = B.open()
    _play(B, s, junk, 0, 45, 1, [], flush=True)                   # slot 0 held 45 rows, NaN among them
    B.close(s)
    assert B.resume(snap) == s
    _play(B, s, src, 17, T, 1, out, flush=True)
    assert torch.equal(torch.cat(out), _uninterrupted(fs, 0, 1, 1))


def test_errors_leave_the_session_untouched(fs):
    from fs_eend_amd.multistream import SlotError, StreamSnapshot
    meta, _, _, src = fs
    T, C = meta["T"], meta["C"]
    donor = _ses(fs, 1)
    s = donor.open()
    _play(donor, s, src, 0, 30, 1, [])
    snap = donor.snapshot(s)
    other_c = _ses(fs, 2, C=C + 1)
    other_c.open()
    X, Y = _ses(fs, 3, cap=16), _ses(fs, 3, cap=16)               # X is disturbed, Y is not
    out = {X: [], Y: []}
    for ses in (X, Y):
        assert ses.open() == 0
        _play(ses, 0, src, 0, 12, 1, out[ses])
    with pytest.raises(SlotError, match="not open"):
        X.suspend(1)                                              # a free slot
    with pytest.raises(SlotError):
        X.snapshot(2)                                             # no such slot
    with pytest.raises(SlotError, match="C "):
        other_c.resume(snap)                                      # another C
    with pytest.raises(SlotError, match="C "):
        X.resume(other_c.snapshot(0))
    ls_like = StreamSnapshot("ls", dict(snap.signature, kind="ls"), snap.table, snap.parts)
    with pytest.raises(SlotError, match="kind"):
        X.resume(ls_like)
    with pytest.raises(SlotError, match="parts"):
        X.resume(StreamSnapshot("fs", snap.signature, snap.table, dict(snap.parts, tracker={})))
    with pytest.raises(SlotError, match="StreamSnapshot"):
        X.resume(snap.parts)
    assert X.open() == 1 and X.open() == 2
    with pytest.raises(SlotError, match="in use"):
        X.resume(snap)                                            # no free slot
    X.close(1), X.close(2)
    assert X.cap == Y.cap == 16 and X.table.state == Y.table.state        # a refused 30-frame snapshot grew nothing
    for ses in (X, Y):
        _play(ses, 0, src, 12, T, 1, out[ses], flush=True)
    assert torch.equal(torch.cat(out[X]), torch.cat(out[Y]))
    assert torch.equal(torch.cat(out[X]), _uninterrupted(fs, 0, 1, 1))


def test_segment_session_across_the_cut(fs):
    """A SegmentSession suspended while a segment is open, resumed (from the host) in a second one: the rttm lines and the
    concatenated polls are the uninterrupted run's; segments drained by rttm() but not yet polled travel too."""
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.multistream import SlotError
    meta, _, _, src = fs
    T = meta["T"]
    ref = _uninterrupted(fs, 0, 1, 1)
    thr = float(torch.sigmoid(ref[:, 1:]).median())               # both decisions occur whatever the random weights give
    mk = lambda slots, **kw: SegmentSession(_ses(fs, slots, **kw), threshold=thr, median=5)

    def run(cut):
        A = mk(3)
        s, out, polled, open_at, snap = A.open(), [], [], [], None
        for i in range(T):
            y = A.step({s: src[i]})
            out.append(y[s].reshape(1, -1)) if s in y else None
            if i in (15, 25, 44):
                polled += A.poll().get(s, [])
            if i == 33:
                A.rttm(s, "rec")                                  # drains the device ring: segments now pending on the host
            if cut is None and A.active(s):
                open_at.append(i)
            if i == cut:
                assert A.active(s)
                snap = A.suspend(s)
                assert sorted(snap.parts) == ["model", "tracker"] and A.state(s) == "free"
                A = mk(4, cap=16, use_graph=False)
                A.open()
                s = A.resume(snap.to("cpu"))
                assert s == 1
        y = A.step(flush=[s])
        while True:
            out.append(y[s].reshape(1, -1)) if s in y else None
            if A.state(s) == "done":
                break
            y = A.step()
        polled += A.poll().get(s, [])
        return torch.cat(out), A.rttm(s, "rec"), polled, open_at, snap

    whole = run(None)
    assert torch.equal(whole[0], ref) and sum(len(v) for v in whole[1].values()) > 2
    cuts = [i for i in whole[3] if 34 <= i < 44][:2]              # a segment is open, and rttm() has left segments pending
    assert cuts, f"no frame in 34..43 with an open segment (open at {whole[3]})"
    for cut in cuts:
        got = run(cut)
        assert torch.equal(got[0], whole[0]) and got[1] == whole[1] and got[2] == whole[2], cut
    snap = got[4]
    with pytest.raises(SlotError, match="parts"):
        _ses(fs, 1).resume(snap)                                  # the bare session refuses a snapshot with the tracker's part
    bare = _ses(fs, 1)
    with pytest.raises(SlotError, match="parts"):
        mk(1).resume(bare.snapshot(bare.open()))                  # ... and the wrapper one without it
    other = SegmentSession(_ses(fs, 1), threshold=thr, median=7)
    with pytest.raises(SlotError, match="tracker"):
        other.resume(snap)                                        # another tracker configuration
    assert other.state(0) == "free" and other.ses.cap == 64
