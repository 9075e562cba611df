"""CPU: the host side of the speech-activity mask in live_rttm.py -- the flag queue of a SegmentSession against a fake session
(the real SlotTable, so rows are emitted conv_delay pushes late) and a fake tracker that records what it is fed, every
validation error leaving the state unchanged, the snapshot part (a plain tracker's keeps its keys), and the parameter domain of
the two C-ABI entries."""
import random
import types

import pytest
import torch

from fs_eend_amd.multistream import SlotError, SlotTable, StreamSnapshot

EINVAL = -1
C, IN = 4, 5


class FakeModel:
    _in_size = IN


class FakeSession:
    """The slot bookkeeping of a multi-stream session (the real SlotTable and its plans) with zero logits."""
    input_transform = None
    parts = ("model",)

    def __init__(self, slots, center, max_frames=1):
        self.S, self.C, self.dev, self.m, self.max_frames = slots, C, torch.device("cpu"), FakeModel(), max_frames
        self.table = SlotTable(slots, center)
        self._emitted = None

    def open(self):
        return self.table.open()

    def close(self, s):
        self.table.close(s)

    def state(self, s):
        return self.table.state[s]

    def _run(self, plan, n):
        if plan.idle:
            self.table.commit(plan)
            return {}
        self.table.commit(plan)
        self._emitted = (torch.zeros(self.S, n, C), torch.tensor(plan.dec, dtype=torch.int32), n)
        return {s: torch.zeros(1, plan.dec[s], C) for s in plan.emit}

    def step(self, push=None, flush=()):
        return self._run(self.table.plan(dict(push or {}).keys(), flush), 1)

    def step_frames(self, push=None, flush=()):
        feats = {s: x.reshape(-1, IN) for s, x in dict(push or {}).items()}
        return self._run(self.table.plan_frames({s: int(x.shape[0]) for s, x in feats.items()}, flush, self.max_frames), self.max_frames)

    def prefill(self, s, feats):
        plan = self.table.plan_prefill(s, int(feats.reshape(-1, IN).shape[0]))
        self.table.commit(plan)
        return torch.zeros(1, plan.dec[s], C)

    def emitted(self):
        return self._emitted

    def seek(self, s, t):
        pass


class FakeTracker:
    """Stands in for SegmentTracker: keeps the real FlagFifo and records, per slot, the flags of the rows it was fed."""

    def __init__(self, slots, device=None, sad=False, **kw):
        from fs_eend_amd import live_rttm as LR
        self.S, self.sad, self.kw = slots, sad, kw
        self.fifo = LR.FlagFifo(slots) if sad else None
        self.fed = {s: [] for s in range(slots)}
        self.ended, self.launches = [], 0

    def reset(self, s):
        self.fed[s] = []
        if self.sad:
            self.fifo.clear(s)

    close = reset

    def feed_rows(self, x, counts, rows_per_slot=1, sad=None):
        assert (sad is not None) == self.sad and x.shape[:2] == (self.S, rows_per_slot)
        self.launches += 1
        if self.sad:
            assert sad.shape == (self.S, rows_per_slot) and sad.dtype == torch.uint8
            for s, n in enumerate(counts.tolist()):
                self.fed[s] += sad[s, :n].tolist()

    def feed(self, rows=None, end=(), sad=None):
        self.launches += 1
        for s, x in dict(rows or {}).items():
            assert len(sad[s]) == x.shape[0]
            self.fed[s] += list(sad[s])
        self.ended += list(end)

    def end(self, slots):
        self.ended += list(slots)


@pytest.fixture
def LR(monkeypatch):
    from fs_eend_amd import live_rttm
    monkeypatch.setattr(live_rttm, "SegmentTracker", FakeTracker)
    return live_rttm


def frames(n):
    return torch.zeros(n, IN)


def fifo_state(ses):
    return [list(q) for q in ses.tracker.fifo.q], {s: list(v) for s, v in ses.tracker.fed.items()}, list(ses.ses.table.t)


def test_step_late_emission_pauses_and_flush(LR):
    """conv_delay = 3: a row leaves 3 pushes after its frame came in, so its flag waits; paused slots keep theirs; the flush
    drains the queue, and a finished stream has none left."""
    rng = random.Random(1)
    ses = LR.SegmentSession(FakeSession(4, center=3), sad=True)
    want = {}
    slots = [ses.open() for _ in range(3)]
    lens = {slots[0]: 20, slots[1]: 2, slots[2]: 9}                    # one stream shorter than the delay
    pos = {s: 0 for s in slots}
    for s in slots:
        want[s] = [rng.randrange(2) for _ in range(lens[s])]
    step = 0
    while any(ses.state(s) != "done" for s in slots):
        push, flush, sad = {}, [], {}
        for s in slots:
            if ses.state(s) != "open" or (s == slots[0] and step in (4, 5, 11)):   # slot 0 pauses now and then
                continue
            if pos[s] < lens[s]:
                push[s] = frames(1)
                sad[s] = want[s][pos[s]] if step % 2 else [want[s][pos[s]]]     # a scalar or a sequence of one
                pos[s] += 1
            else:
                flush.append(s)
        out = ses.step(push=push, flush=flush, sad=sad)
        for s in slots:                                               # flags waiting = frames pushed - rows emitted so far
            assert len(ses.tracker.fifo.q[s]) == pos[s] - len(ses.tracker.fed[s])
            if ses.state(s) == "open" and pos[s] >= 3:
                assert len(ses.tracker.fifo.q[s]) == 3
        step += 1
    for s in slots:
        assert ses.tracker.fed[s] == want[s] and ses.tracker.fifo.q[s] == []
    assert sorted(ses.tracker.ended) == sorted(slots)
    ses.close(slots[0])
    s = ses.open()                                                    # a reopened slot starts with an empty queue
    assert s == slots[0] and ses.tracker.fifo.q[s] == [] and ses.tracker.fed[s] == []


def test_step_frames_ragged_counts_and_prefill_pieces(LR):
    rng = random.Random(2)
    ses = LR.SegmentSession(FakeSession(3, center=4, max_frames=8), sad=True)
    a, b = ses.open(), ses.open()
    T = {a: 45, b: 13}
    want = {s: [rng.randrange(2) for _ in range(T[s])] for s in T}
    pos = {a: 0, b: 0}
    out = ses.prefill(a, frames(2), sad=want[a][:2])                  # shorter than the delay: nothing emitted, two flags wait
    assert out.shape[1] == 0 and ses.tracker.fifo.q[a] == want[a][:2] and ses.tracker.launches == 0
    out = ses.prefill(a, frames(9), sad=torch.tensor(want[a][2:11]))  # a second piece, flags as a tensor
    assert out.shape[1] == 7 and ses.tracker.fed[a] == want[a][:7] and ses.tracker.fifo.q[a] == want[a][7:11]
    pos[a] = 11
    while any(ses.state(s) != "done" for s in T):
        push, flush, sad = {}, [], {}
        for s in T:
            if ses.state(s) != "open":
                continue
            n = min(rng.choice([0, 1, 3, 8]), T[s] - pos[s])
            push[s] = frames(n)
            if n or rng.random() < 0.5:                               # a slot that pushes no frame may leave its flags out
                sad[s] = want[s][pos[s]:pos[s] + n]
            pos[s] += n
            if pos[s] == T[s]:
                flush.append(s)                                       # pushed and flushed in one call
        ses.step_frames(push=push, flush=flush, sad=sad)
        for s in T:
            assert ses.tracker.fed[s] + ses.tracker.fifo.q[s] == want[s][:pos[s]]
    assert all(ses.tracker.fed[s] == want[s] for s in T)


def test_validation_errors_change_nothing(LR):
    ses = LR.SegmentSession(FakeSession(4, center=2, max_frames=4), sad=True)
    a, b = ses.open(), ses.open()
    for _ in range(3):
        ses.step(push={a: frames(1), b: frames(1)}, sad={a: 1, b: 0})
    before = fifo_state(ses)
    bad_steps = [dict(push={a: frames(1)}),                                        # no flags at all
                 dict(push={a: frames(1), b: frames(1)}, sad={a: 1}),              # one slot's missing
                 dict(push={a: frames(1)}, sad={a: 1, b: 0}),                      # flags for a slot that is not pushed
                 dict(push={a: frames(1)}, sad={a: [1, 0]}),                       # two flags for one frame
                 dict(push={a: frames(1)}, sad={a: []}),
                 dict(push={a: frames(1)}, sad={a: 1, 3: 1}),                      # flags for a free slot
                 dict(push={a: frames(1)}, sad={a: object()}),
                 dict(push={a: frames(1), 3: frames(1)}, sad={a: 1, 3: 1})]        # the wrapped session's own refusal
    for kw in bad_steps:
        with pytest.raises(SlotError):
            ses.step(**kw)
        assert fifo_state(ses) == before, kw
    bad_frames = [dict(push={a: frames(3)}, sad={a: [1, 0]}),
                  dict(push={a: frames(3)}, sad={a: [1, 0, 1, 1]}),
                  dict(push={a: frames(3)}),
                  dict(push={a: frames(0)}, sad={a: [1]}),
                  dict(push={a: frames(2)}, sad={a: [1, 0], b: [1]}),
                  dict(push={a: [[0.0] * IN]}, sad={a: [1]}),                      # not a tensor
                  dict(push={a: frames(5)}, sad={a: [1] * 5})]                     # more than max_frames: the session refuses
    for kw in bad_frames:
        with pytest.raises(SlotError):
            ses.step_frames(**kw)
        assert fifo_state(ses) == before, kw
    for kw in (dict(feats=frames(3)), dict(feats=frames(3), sad=[1, 0]), dict(feats=frames(3), sad=[1] * 4),
               dict(feats=[[0.0] * IN], sad=[1])):
        with pytest.raises(SlotError):
            ses.prefill(a, **kw)
        assert fifo_state(ses) == before, kw
    with pytest.raises(SlotError):
        ses.prefill(3, frames(2), sad=[1, 1])                         # a free slot: the session refuses, nothing queued
    assert fifo_state(ses) == before
    with pytest.raises(SlotError, match="misalign"):
        ses.seek(a, 10)
    ses.step(push={a: frames(1)}, sad={a: 1})                         # and the session goes on
    assert ses.tracker.fed[a] == [1, 1] and ses.tracker.fifo.q[a] == [1, 1]


def test_plain_session_takes_no_flags(LR):
    ses = LR.SegmentSession(FakeSession(2, center=1))
    a = ses.open()
    assert ses.tracker.sad is False and ses.tracker.fifo is None
    with pytest.raises(SlotError):
        ses.step(push={a: frames(1)}, sad={a: 1})
    with pytest.raises(SlotError):
        ses.step_frames(push={a: frames(1)}, sad={a: [1]})
    with pytest.raises(SlotError):
        ses.prefill(a, frames(1), sad=[1])
    assert ses.ses.table.t[a] == 0
    ses.step(push={a: frames(1)})
    ses.step(push={a: frames(1)})
    ses.seek(a, 5)
    assert ses.tracker.launches == 1


def test_flag_fifo_rules():
    from fs_eend_amd import live_rttm as LR
    q = LR.FlagFifo(3)
    got = q.check({0: 2, 1: 1, 2: 0}, {0: (True, 0.0), 1: torch.tensor([7])})     # non-zero is speech
    assert got == {0: [1, 0], 1: [1]} and q.q == [[], [], []]                      # check changes nothing
    q.push(got)
    q.push({0: [1]})
    assert q.pop({0: 2, 1: 0}) == {0: [1, 0], 1: []} and q.q == [[1], [1], []]
    with pytest.raises(AssertionError):
        q.pop({0: 1, 1: 2})                                           # more rows than flags: a bug, and nothing was popped
    assert q.q == [[1], [1], []]
    assert q.export(0) == [1] and LR.FlagFifo.fits(q.export(0)) and LR.FlagFifo.fits([])
    for v in (None, [2], [0.5], "01", [None]):
        assert not LR.FlagFifo.fits(v)
    q.adopt(2, (1, 0, 1))
    assert q.q[2] == [1, 0, 1]
    q.clear(2)
    assert q.q[2] == []
    assert LR.host_flags(1, 1, "x") == [1] and LR.host_flags(torch.tensor([[0], [3]]), 2, "x") == [0, 1]
    with pytest.raises(SlotError):
        LR.host_flags([1, 0], 3, "x")


PLAIN_KEYS = {"ntracks", "col0", "threshold", "median", "is_prob", "capacity"}


def test_snapshot_part_and_config(tmp_path):
    from fs_eend_amd import live_rttm as LR
    plain = LR.tracker_config(3, 1, 0.5, 11, False, 8)
    assert set(plain) == PLAIN_KEYS and plain == LR.tracker_config(3, 1, 0.5, 11, False, 8, sad=False)
    masked = LR.tracker_config(3, 1, 0.5, 11, False, 8, sad=True)
    assert set(masked) == PLAIN_KEYS | {"sad"} and masked["sad"] is True and masked != plain
    log = LR.SegmentLog(2, 3, 8)
    assert set(log.export(0)) == {"state", "segs", "pending", "overflowed", "unreported"}      # today's host fields

    # the tracker's own export / check_part / adopt on a stand-in that has the fields they read (the device rows on the CPU)
    def stand_in(sad):
        tr = types.SimpleNamespace(ntracks=3, col0=1, threshold=0.5, median=11, is_prob=False, cap=8, sad=sad, S=2,
                                   log=LR.SegmentLog(2, 3, 8), fifo=LR.FlagFifo(2) if sad else None,
                                   hist=torch.zeros(2, 64, dtype=torch.int64), open_=torch.full((2, 64), -1, dtype=torch.int32),
                                   box=torch.zeros(2, LR.HDR + 24, dtype=torch.int32))
        for name in ("_config", "export", "check_part", "adopt"):
            setattr(tr, name, types.MethodType(getattr(LR.SegmentTracker, name), tr))
        return tr

    p, m = stand_in(False), stand_in(True)
    assert set(p.export(0)) == {"state", "segs", "pending", "overflowed", "unreported", "config", "hist", "open", "box"}
    assert set(p.export(0)["config"]) == PLAIN_KEYS
    m.fifo.push({1: [1, 0, 0, 1]})
    m.hist[1, 2] = 77
    part = m.export(1)
    assert part["fifo"] == [1, 0, 0, 1] and part["config"]["sad"] is True
    snap = StreamSnapshot("fs", {"kind": "fs"}, {"state": "open", "t": 4, "n_enc": 4, "n_dec": 0, "flush_left": 0},
                          {"model": {"blob": torch.zeros(4, dtype=torch.uint8), "sections": [("x", 0, 4)]}, "tracker": part})
    path = str(tmp_path / "s.pt")
    snap.to("cpu").save(path)
    back = StreamSnapshot.load(path).parts["tracker"]
    assert back["fifo"] == [1, 0, 0, 1] and back["config"] == part["config"] and torch.equal(back["hist"], part["hist"])
    m2 = stand_in(True)
    m2.check_part(back)
    m2.adopt(0, back)
    assert m2.fifo.q == [[1, 0, 0, 1], []] and int(m2.hist[0, 2]) == 77
    for tr, other in ((p, back), (m2, p.export(0))):                  # neither kind resumes the other's part
        was = (tr.fifo.q if tr.fifo else None, tr.hist.clone())
        with pytest.raises(SlotError):
            tr.check_part(other)
        assert (tr.fifo.q if tr.fifo else None) == was[0] and torch.equal(tr.hist, was[1])
    for bad in (dict(back, fifo=[2]), {k: v for k, v in back.items() if k != "fifo"}, dict(back, fifo="10")):
        with pytest.raises(SlotError):
            m2.check_part(bad)


def test_tracker_refuses_bad_flags_on_the_host():
    """SegmentTracker._check_sad runs before any launch; it needs no device."""
    from fs_eend_amd import live_rttm as LR
    rows = {0: torch.zeros(3, 4), 2: torch.zeros(0, 4)}
    plain = types.SimpleNamespace(sad=False, fifo=None)
    assert LR.SegmentTracker._check_sad(plain, rows, None) is None
    with pytest.raises(SlotError):
        LR.SegmentTracker._check_sad(plain, rows, {0: [1, 1, 1]})
    masked = types.SimpleNamespace(sad=True, fifo=LR.FlagFifo(4))
    assert LR.SegmentTracker._check_sad(masked, rows, {0: [1, 0, 5]}) == {0: [1, 0, 1]}
    assert LR.SegmentTracker._check_sad(masked, rows, {0: torch.tensor([1, 0, 1]), 2: []}) == {0: [1, 0, 1], 2: []}
    for sad in (None, {}, {0: [1, 1]}, {0: [1, 1, 1], 1: [1]}, {0: [1, 1, 1], 2: [1]}):
        with pytest.raises(SlotError):
            LR.SegmentTracker._check_sad(masked, rows, sad)


def test_no_cpu_fallback():
    """Without a GPU the drop-in entry points raise; nothing is computed on the host."""
    from fs_eend_amd import postproc
    from fs_eend_amd.lib import EendHipError
    p = torch.rand(6, 3)
    if not torch.cuda.is_available():
        with pytest.raises(EendHipError):
            postproc.sad_func(torch.where(p > 0.5, 1, 0), torch.ones(6, 1), p)
        with pytest.raises(EendHipError):
            postproc.make_rttm("r", p, sad=torch.ones(6))
    with pytest.raises(EendHipError):
        postproc.sad_fuse(p, torch.ones(6))                           # the device entry takes GPU tensors only
    with pytest.raises(EendHipError):
        postproc.activity(p, sad=torch.ones(6))


def test_cabi_domain(hip_lib):
    """Arguments outside the domain return EEND_EINVAL before any launch (the pointers are never touched)."""
    from fs_eend_amd import lib as L
    lib = L.load()
    p = 64                                                          # never dereferenced: every call below is rejected or empty
    ok = dict(desc=p, counts=p, ends=None, sad=p, n=2, ld=11, col0=1, ntracks=10, thr=0.5, k=11, is_prob=0, hist=p, open=p, box=p,
              S=4, cap=16)

    def feed(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.eend_segtrack_feed_sad_f32(a["desc"], a["counts"], a["ends"], a["sad"], a["n"], a["ld"], a["col0"], a["ntracks"],
                                              a["thr"], a["k"], a["is_prob"], a["hist"], a["open"], a["box"], a["S"], a["cap"], None)

    for kw in (dict(k=0), dict(k=2), dict(k=63 + 2), dict(k=-1), dict(ntracks=0), dict(ntracks=65, ld=80), dict(ld=10),
               dict(col0=-1), dict(n=-1), dict(n=5), dict(S=0), dict(cap=0), dict(desc=None), dict(counts=None), dict(sad=None),
               dict(hist=None), dict(open=None), dict(box=None), dict(S=1 << 20, cap=1 << 12, n=0), dict(sad=None, n=0)):
        assert feed(**kw) == EINVAL, kw
    assert feed(n=0) == 0                                           # nothing to do: no launch

    def fuse(pred=p, ld=4, T=8, S=3, thr=0.5, sad=p, out=p):
        return lib.eend_sad_fuse_f32(pred, ld, T, S, thr, sad, out, None)

    for kw in (dict(pred=None), dict(sad=None), dict(out=None), dict(T=0), dict(T=-1), dict(S=0), dict(ld=2)):
        assert fuse(**kw) == EINVAL, kw
    assert lib.eend_abi_version() == 5                                # the entries are additive
