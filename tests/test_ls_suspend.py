"""GPU: a stream slot of LsMultiStreamSession suspended to a StreamSnapshot and resumed -- in another slot, another session
(other slot count, max_frames, graph setting), through the host and through a file, into a slot full of NaN -- goes on bit for
bit as the uninterrupted stream; so do a flushing slot, a fork, the neighbours, and an AudioStreamSession cut in mid-frame.

Every comparison is against an uninterrupted stream that took the same frames in the same steps.
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
def ls(hip_lib, dev):
    from tests.test_ls_multistream import _model
    meta, arr, m, src = _model("ls_stream_T120", dev)
    return meta, arr, m, src


def _ses(ls, slots, C=None, **kw):
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    ses = LsMultiStreamSession(ls[2], slots, ls[0]["C"] if C is None else C, **kw)
    assert ses.center == DELAY
    return ses


def _poison_free(ses):
    from tests.test_ls_multistream import _poison
    for s in range(ses.S):
        if ses.state(s) == "free":
            _poison(ses, s)


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


def _uninterrupted(ls, t, na, nb):
    """The golden stream through one slot of one session: frames [0, t) in steps of na frames, the rest in steps of nb."""
    key = (t if (na, nb) != (1, 1) else 0, na, nb)              # one frame per step throughout: the cut does not show
    if key not in _REF:
        src = ls[3]
        ses = _ses(ls, 3, max_frames=max(na, nb), use_graph=False)
        s, out = ses.open(), []
        _play(ses, s, src, 0, t, na, out)
        _play(ses, s, src, t, src.shape[0], nb, out, flush=True)
        _REF[key] = torch.cat(out)
    return _REF[key]


def test_uninterrupted_stream_matches_the_fixture(ls):
    meta, arr, _, _ = ls
    for na, nb in ((1, 1), (1, 4), (4, 1)):
        ref = _uninterrupted(ls, 65, na, nb)
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
    "other-1to4": (1, 4, dict(slots=3), dict(slots=4, max_frames=4, use_graph=False), None),
    "other-4to1": (4, 1, dict(slots=3, max_frames=4, use_graph=False), dict(slots=4), None),
    "host": (1, 1, dict(slots=3, use_graph=False), dict(slots=4), _host),
    "file": (1, 1, dict(slots=4), dict(slots=3, use_graph=False), _file),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("t", [0, 1, 8, 9, 10, 17, 63, 64, 65, -1, None], ids=lambda t: {-1: "T-1", None: "T"}.get(t, str(t)))
def test_cut_and_resume_bit_equal(ls, tmp_path, t, route):
    meta, _, _, src = ls
    T = meta["T"]
    t = T if t is None else T + t if t < 0 else t
    na, nb, kw_a, kw_b, via = ROUTES[route]
    want = _uninterrupted(ls, t, na, nb)
    A = _ses(ls, **kw_a)
    hold = A.open()                                               # slot 0, idle; the stream runs in slot 1
    sa, out = A.open(), []
    _play(A, sa, src, 0, t, na, out)
    snap = A.suspend(sa)
    assert A.state(sa) == "free" and snap.kind == "ls" and snap.table["t"] == t and snap.device == A.dev
    assert snap.nbytes == snap.parts["model"]["blob"].numel() > 0
    if via is not None:
        snap = via(snap, tmp_path)
        assert snap.device.type == "cpu" and snap.table["n_enc"] == t
    if kw_b is None:
        B = A
        A.close(hold)                                             # the lowest free slot is now another one than the stream left
        _poison_free(B)                                           # ... and holds NaN in every piece of its state
        sb = B.resume(snap)
        assert sb == hold != sa
    else:
        B = _ses(ls, **kw_b)
        assert B.open() == 0
        _poison_free(B)
        sb = B.resume(snap)
        assert sb == 1
    assert B.state(sb) == "open" and (B.table.t[sb], B.table.n_enc[sb], B.table.n_dec[sb]) == (t, t, max(0, t - DELAY))
    _play(B, sb, src, t, T, nb, out, flush=True)
    got = torch.cat(out)
    assert got.shape == want.shape
    assert torch.equal(got, want), f"max diff {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("left", [9, 4, 1])
def test_flushing_slot_resumes_to_a_bit_equal_tail(ls, left):
    """Suspended while flushing with `left` dummy frames to go (9: flushed with a full chunk of pushes, none taken yet)."""
    meta, _, _, src = ls
    T, C = meta["T"], meta["C"]
    n = 4 if left == DELAY else 1

    def run(cut):
        ses = _ses(ls, 3, max_frames=n)
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
            ses = _ses(ls, 4, max_frames=n, use_graph=False)
            ses.open()
            _poison_free(ses)
            s = ses.resume(snap)
            assert s == 1 and ses.state(s) == "flushing"
        while ses.state(s) == "flushing":
            take(step()())
        assert ses.state(s) == "done"
        return torch.cat(out)

    whole, resumed = run(False), run(True)
    assert whole.shape == (T, C) and torch.equal(whole, resumed)
    if n == 1:
        assert torch.equal(whole, _uninterrupted(ls, 0, 1, 1))


def test_snapshot_forks_a_stream(ls):
    meta, _, _, src = ls
    T = meta["T"]
    ses = _ses(ls, 3)
    a, out_a, out_b = ses.open(), [], []
    _play(ses, a, src, 0, 70, 1, out_a)
    snap = ses.snapshot(a)
    assert ses.state(a) == "open" and ses.table.t[a] == 70        # the slot is untouched and goes on
    _poison_free(ses)
    b = ses.resume(snap)
    assert b == 1
    out_b += out_a
    for i in range(70, T):                                        # the same frames to both, in the same steps
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
    assert torch.equal(ga, gb) and torch.equal(ga, _uninterrupted(ls, 0, 1, 1))
    c = ses.resume(snap)                                          # a snapshot can be resumed more than once
    assert c == 2 and ses.table.t[c] == 70


def test_neighbour_is_undisturbed_and_the_freed_slot_is_reused(ls):
    """A neighbour streams through suspends, resumes, a fork and closes around it."""
    meta, _, _, src = ls
    T = meta["T"]
    g = torch.Generator().manual_seed(31)
    nsrc = (src + 0.3 * torch.randn(src.shape, generator=g).to(src.device)).contiguous()
    solo = _ses(ls, 3)
    s, want = solo.open(), []
    _play(solo, s, nsrc, 0, T, 1, want, flush=True)
    ses = _ses(ls, 4)
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
            _poison_free(ses)
            x = ses.resume(snaps[12])
            assert x == first
        if i == 70:                                               # a fork: the original goes on in its slot
            snaps[70] = ses.snapshot(x)
            assert ses.resume(snaps[70]) == 2
        if i == 90:
            ses.close(x)
    _play(ses, nb, nsrc, T, T, 1, got, flush=True)
    assert torch.equal(torch.cat(got), torch.cat(want))


def test_errors_leave_the_session_untouched(ls, dev):
    from fs_eend_amd.fs_multistream import FsMultiStreamSession
    from fs_eend_amd.multistream import SlotError, StreamSnapshot
    from tests.test_fs_multistream import _models
    meta, _, _, src = ls
    T, C = meta["T"], meta["C"]
    donor = _ses(ls, 1)
    s = donor.open()
    _play(donor, s, src, 0, 30, 1, [])
    snap = donor.snapshot(s)
    fmeta, _, sm, fsrc = _models("fs_stream_T60", dev)
    fs_ses = FsMultiStreamSession(sm, 2, fmeta["C"], cap=16)
    f = fs_ses.open()
    fs_ses.step({f: fsrc[0]})
    fs_snap = fs_ses.snapshot(f)
    other_c = _ses(ls, 2, C=C - 1)
    other_c.open()
    X, Y = _ses(ls, 3), _ses(ls, 3)                               # X is disturbed, Y is not
    out = {X: [], Y: []}
    for ses in (X, Y):
        assert ses.open() == 0
        _play(ses, 0, src, 0, 12, 1, out[ses])
    with pytest.raises(SlotError, match="not open"):
        X.suspend(1)                                              # a free slot
    with pytest.raises(SlotError, match="kind"):
        X.resume(fs_snap)                                         # an FS snapshot into an LS session
    with pytest.raises(SlotError, match="kind"):
        fs_ses.resume(snap)                                       # ... and the other way round
    with pytest.raises(SlotError, match="C "):
        other_c.resume(snap)                                      # another C
    with pytest.raises(SlotError, match="C "):
        X.resume(other_c.snapshot(0))
    with pytest.raises(SlotError, match="parts"):
        X.resume(StreamSnapshot("ls", snap.signature, snap.table, dict(snap.parts, frontend={})))
    assert X.open() == 1 and X.open() == 2
    with pytest.raises(SlotError, match="in use"):
        X.resume(snap)                                            # no free slot
    X.close(1), X.close(2)
    assert X.table.state == Y.table.state and fs_ses.cap == 16 and fs_ses.state(1) == "free"
    for ses in (X, Y):
        _play(ses, 0, src, 12, T, 1, out[ses], flush=True)
    assert torch.equal(torch.cat(out[X]), torch.cat(out[Y]))
    assert torch.equal(torch.cat(out[X]), _uninterrupted(ls, 0, 1, 1))


def test_audio_session_cut_in_mid_frame(ls, tmp_path):
    """About 3 s of 8 kHz audio through AudioStreamSession(SegmentSession(LsMultiStreamSession)), suspended after 12345 samples
    (neither a multiple of the 80-sample hop nor of the 800-sample model frame, and inside an STFT tile) and resumed from a
    file in a second stack: logits bit-equal, the same lines."""
    from fs_eend_amd.audio_stream import AudioStreamSession
    from fs_eend_amd.live_rttm import SegmentSession
    from fs_eend_amd.multistream import SlotError, StreamSnapshot
    from tests.test_feature_gpu import wave
    y = torch.from_numpy(wave(8000 * 3 + 777, 12))
    cuts = [0, 4000, 4100, 12345, 12346, 20000, y.numel()]        # the chunks of both runs; the stream leaves after 12345 samples
    mk = lambda slots, **kw: AudioStreamSession(SegmentSession(_ses(ls, slots, **kw), threshold=0.5, median=3))

    def run(cut, tmp=None):
        A = mk(3)
        s, out = A.open(), []
        for a, b in zip(cuts, cuts[1:]):
            out.append(A.push({s: y[a:b]})[s])
            if b == cut:
                snap = A.suspend(s)
                assert sorted(snap.parts) == ["frontend", "model", "tracker"] and A.state(s) == "free"
                assert snap.parts["frontend"]["recv"] == cut and snap.nbytes > snap.parts["model"]["blob"].numel()
                with pytest.raises(SlotError, match="parts"):
                    A.ses.resume(snap)                            # the stack without the front-end refuses its part
                snap.save(tmp)
                A = mk(4, use_graph=False)
                A.open()
                _poison_free(A.ses.ses)
                s = A.resume(StreamSnapshot.load(tmp))
                assert s == 1 and A.fe.table.recv[s] == cut
        out.append(A.end([s])[s])
        return torch.cat(out), A.ses.rttm(s, "rec")

    whole = run(None)
    got = run(12345, str(tmp_path / "call.snap"))
    assert whole[0].shape == (31, ls[0]["C"])                     # 24777 samples: 310 log-mel frames, 31 model frames
    assert torch.equal(got[0], whole[0]), f"max diff {float((got[0] - whole[0]).abs().max()):.3e}"
    assert got[1] == whole[1]
