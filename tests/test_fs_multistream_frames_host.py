"""Host-only: SlotTable.plan_frames, the bookkeeping of the multi-frame step (FsMultiStreamSession.step_frames) -- emission counts,
flushing in one or several steps, push plus flush in one call, its errors, and that committing a plan of n frames leaves the
table exactly as n frames through the one-frame rules do (`_OneFrameSlot`, an independent model of them)."""
import random

import pytest

from fs_eend_amd.multistream import DONE, FLUSHING, FREE, OPEN, SlotError, SlotTable


KEEP, PUSH, FLUSH = 0, 1, 2


def _state(tb, s):
    return (tb.state[s], tb.t[s], tb.n_enc[s], tb.n_dec[s], tb.flush_left[s])


class _OneFrameSlot:
    """One slot under the one-frame rules, written out apart from SlotTable: a frame pushes, starts a flush (its first dummy
    frame) or, while flushing, takes a dummy frame; it emits logits once the look-ahead of `center` frames is full."""

    def __init__(self, center):
        self.center = center
        self.state, self.t, self.n_enc, self.n_dec, self.flush_left = FREE, 0, 0, 0, 0

    def open(self):
        self.state, self.t, self.n_enc, self.n_dec, self.flush_left = OPEN, 0, 0, 0, 0

    def frame(self, push=False, flush=False):
        """-> 1 when the frame emitted logits."""
        if push:
            win = PUSH
        elif (flush and self.center > 0) or (self.state == FLUSHING and self.flush_left > 0):
            win = FLUSH
        else:
            win = KEEP
        dec = 1 if win != KEEP and self.t + 1 >= self.center + 1 else 0
        if flush:
            self.state, self.flush_left = FLUSHING, self.center
        self.n_enc += 1 if push else 0
        self.n_dec += dec
        if win != KEEP:
            self.t += 1
        if win == FLUSH:
            self.flush_left -= 1
        if self.state == FLUSHING and self.flush_left <= 0:
            self.state = DONE
        return dec


def test_warm_up_emission_counts():
    tb = SlotTable(2, center=5)
    a = tb.open()
    p = tb.plan_frames({a: 4}, nmax=8)
    assert (p.enc[a], p.npush[a], p.ndummy[a], p.dec[a]) == (4, 4, 0, 0)     # the look-ahead is not full yet
    tb.commit(p)
    p = tb.plan_frames({a: 8}, nmax=8)
    assert p.dec[a] == 7                                                    # windows after pushes 5..12: frames 0..6
    assert p.emit == [a] and p.counts()[3] == [7, 0]
    tb.commit(p)
    assert _state(tb, a) == (OPEN, 12, 12, 7, 0)
    p = tb.plan_frames({}, nmax=8)                                         # a pause: nothing to run
    assert p.idle and p.emit == []
    tb.commit(p)
    assert _state(tb, a) == (OPEN, 12, 12, 7, 0)


def test_flush_in_one_step():
    tb = SlotTable(1, center=5)
    a = tb.open()
    tb.commit(tb.plan_frames({a: 8}, nmax=8))
    p = tb.plan_frames(flush=[a], nmax=8)
    assert (p.npush[a], p.ndummy[a], p.dec[a]) == (0, 5, 5)
    tb.commit(p)
    assert _state(tb, a) == (DONE, 13, 8, 8, 0)


def test_flush_spread_over_steps():
    tb = SlotTable(1, center=5)
    a = tb.open()
    tb.commit(tb.plan_frames({a: 2}, nmax=2))
    p = tb.plan_frames(flush=[a], nmax=2)
    assert (p.ndummy[a], p.dec[a]) == (2, 0)
    tb.commit(p)
    assert tb.state[a] == FLUSHING and tb.flush_left[a] == 3
    with pytest.raises(SlotError):
        tb.plan_frames({a: 1}, nmax=2)                                      # a push to a flushing slot
    decs = []
    while tb.state[a] == FLUSHING:
        p = tb.plan_frames(nmax=2)
        decs.append(p.dec[a])
        tb.commit(p)
    assert decs == [1, 1] and _state(tb, a) == (DONE, 7, 2, 2, 0)


def test_push_and_flush_in_one_call():
    tb = SlotTable(2, center=3)
    a, b = tb.open(), tb.open()
    p = tb.plan_frames({a: 5, b: 8}, flush=[a, b], nmax=8)
    assert (p.npush[a], p.ndummy[a], p.dec[a]) == (5, 3, 5)
    assert (p.npush[b], p.ndummy[b], p.dec[b]) == (8, 0, 5)                 # no room left: the dummies follow later
    tb.commit(p)
    assert tb.state[a] == DONE and tb.state[b] == FLUSHING
    p = tb.plan_frames(nmax=8)
    assert (p.ndummy[b], p.dec[b]) == (3, 3)
    tb.commit(p)
    assert _state(tb, b) == (DONE, 11, 8, 8, 0)


def test_errors():
    tb = SlotTable(3, center=2)
    a, b = tb.open(), tb.open()
    with pytest.raises(SlotError):
        tb.plan_frames({a: 5}, nmax=4)                                      # more than max_frames
    with pytest.raises(SlotError):
        tb.plan_frames({a: -1}, nmax=4)
    with pytest.raises(SlotError):
        tb.plan_frames(flush=[a, a], nmax=4)                                # a slot named twice
    with pytest.raises(SlotError):
        tb.plan_frames({2: 1}, nmax=4)                                      # a free slot
    with pytest.raises(SlotError):
        tb.plan_frames({7: 1}, nmax=4)
    tb.commit(tb.plan_frames(flush=[b], nmax=1))
    assert tb.state[b] == FLUSHING
    with pytest.raises(SlotError):
        tb.plan_frames({b: 1}, nmax=4)                                      # a push to a flushing slot
    with pytest.raises(SlotError):
        tb.plan_frames(flush=[b], nmax=4)


@pytest.mark.parametrize("center", [0, 1, 3, 9])
@pytest.mark.parametrize("nmax", [1, 2, 4, 16])
def test_frames_commit_like_one_frame_plans(center, nmax):
    """Random traffic: after every call, each slot's state equals that of a `_OneFrameSlot` driven through the same frames, one
    frame at a time."""
    rng = random.Random(center * 100 + nmax)
    S = 5
    tb = SlotTable(S, center)
    ref = [_OneFrameSlot(center) for _ in range(S)]
    for _ in range(400):
        if rng.random() < 0.2 and FREE in tb.state:
            s = tb.open()
            ref[s].open()
        push, flush = {}, []
        for s in range(S):
            if tb.state[s] == OPEN:
                r = rng.random()
                if r < 0.6:
                    push[s] = rng.randrange(0, nmax + 1)
                if r < 0.1 or 0.6 <= r < 0.65:
                    flush.append(s)
            elif tb.state[s] == DONE and rng.random() < 0.5:
                tb.close(s)
                ref[s].state = FREE
        p = tb.plan_frames(push, flush, nmax)
        emitted = list(p.dec)
        tb.commit(p)
        for s in range(S):
            r = ref[s]
            if r.state == FREE:
                continue
            n = push.get(s, 0)
            dec = 0
            for _ in range(n):                                              # the pushed frames
                dec += r.frame(push=True)
            budget = nmax - n
            if s in flush:                                                  # the flush: its first dummy, if there is room
                if budget == 0:
                    r.state, r.flush_left = FLUSHING, center                # started, dummies in later steps
                    if center <= 0:
                        r.state = DONE
                else:
                    dec += r.frame(flush=True)
                    budget -= 1 if center > 0 else 0
            while r.state == FLUSHING and budget > 0:                      # dummies while there is room
                dec += r.frame()
                budget -= 1
            ref_state = (r.state, r.t, r.n_enc, r.n_dec, r.flush_left)
            assert emitted[s] == dec, (s, emitted[s], dec)
            assert _state(tb, s) == ref_state, (s, _state(tb, s), ref_state)
