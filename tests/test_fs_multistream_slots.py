"""CPU: the slot bookkeeping of the multi-stream sessions (multistream.SlotTable) -- slot lifetimes, the errors on misuse and
the per-slot mode rows the device reads for a frame step.  No GPU, no library calls."""
import pytest

from fs_eend_amd.multistream import DONE, FLUSHING, FREE, OPEN, SlotError, SlotTable

KEEP, PUSH, FLUSH = 0, 1, 2


def _run(tab, push=(), flush=()):
    plan = tab.plan(push, flush)
    tab.commit(plan)
    return plan


def test_open_takes_the_lowest_free_slot_and_errors_past_S():
    tab = SlotTable(3, center=2)
    assert [tab.open() for _ in range(3)] == [0, 1, 2]
    assert tab.state == [OPEN] * 3
    with pytest.raises(SlotError):
        tab.open()
    tab.close(1)
    assert tab.state[1] == FREE
    assert tab.open() == 1


def test_push_to_free_or_unknown_slot_errors():
    tab = SlotTable(2, center=2)
    with pytest.raises(SlotError):
        tab.plan(push=[0])
    tab.open()
    with pytest.raises(SlotError):
        tab.plan(push=[2])
    with pytest.raises(SlotError):
        tab.plan(push=[-1])
    with pytest.raises(SlotError):
        tab.plan(flush=[1])
    with pytest.raises(SlotError):
        tab.plan(push=[0], flush=[0])
    with pytest.raises(SlotError):
        tab.close(1)


def test_one_stream_lifetime_matches_the_single_stream_session():
    """T pushes + conv_delay dummy frames emit T frames of logits, the first once the look-ahead is full (FsStreamSession)."""
    center, T = 3, 5
    tab = SlotTable(1, center)
    s = tab.open()
    emitted = []
    for i in range(T):
        p = _run(tab, push=[s])
        assert p.enc == [1] and p.win == [PUSH]
        assert p.dec == [1 if i >= center else 0]
        emitted += p.emit
    assert tab.n_enc[s] == T and tab.n_dec[s] == T - center and tab.t[s] == T
    p = _run(tab, flush=[s])
    assert p.enc == [0] and p.win == [FLUSH] and p.dec == [1]
    assert tab.state[s] == FLUSHING
    emitted += p.emit
    for _ in range(center - 1):
        p = _run(tab)                                    # a flushing slot advances without being named again
        assert p.win == [FLUSH] and p.dec == [1]
        emitted += p.emit
    assert tab.state[s] == DONE and len(emitted) == T
    assert tab.n_enc[s] == T and tab.n_dec[s] == T and tab.t[s] == T + center
    p = _run(tab)
    assert p.idle and p.emit == []
    with pytest.raises(SlotError):
        tab.plan(push=[s])                               # done: only close() is left
    tab.close(s)
    assert tab.state[s] == FREE


def test_short_stream_flush_emits_only_what_it_pushed():
    tab = SlotTable(1, center=4)
    s = tab.open()
    _run(tab, push=[s])
    _run(tab, push=[s])
    n = len(_run(tab, flush=[s]).emit)
    while tab.state[s] == FLUSHING:
        n += len(_run(tab).emit)
    assert n == 2 and tab.n_dec[s] == 2


def test_mode_rows_for_a_mixed_frame():
    """Slot 0 pushes past the look-ahead, slot 1 pauses, slot 2 flushes, slot 3 is free, slot 4 pushes its first frame."""
    center = 2
    tab = SlotTable(5, center)
    for _ in range(5):
        tab.open()
    tab.close(3)
    for _ in range(3):
        _run(tab, push=[0, 1, 2])
    _run(tab, push=[4])
    p = tab.plan(push=[0, 4], flush=[2])
    assert p.modes() == [[1, 0, 0, 0, 1],
                         [PUSH, KEEP, FLUSH, KEEP, PUSH],
                         [1, 0, 1, 0, 0]]
    assert p.emit == [0, 2] and not p.idle
    tab.commit(p)
    assert tab.state == [OPEN, OPEN, FLUSHING, FREE, OPEN]
    assert tab.n_enc == [4, 3, 3, 0, 2] and tab.n_dec == [2, 1, 2, 0, 0] and tab.t == [4, 3, 4, 0, 2]
    assert tab.max_len() == 4


def test_reopen_starts_from_zero():
    tab = SlotTable(1, center=1)
    s = tab.open()
    for _ in range(4):
        _run(tab, push=[s])
    tab.close(s)
    assert tab.max_len() == 0                            # free slots do not count towards the cache capacity
    assert tab.open() == s
    assert (tab.t[s], tab.n_enc[s], tab.n_dec[s]) == (0, 0, 0)
    assert _run(tab, push=[s]).dec == [0]


def test_close_while_flushing_frees_the_slot():
    tab = SlotTable(2, center=3)
    a, b = tab.open(), tab.open()
    _run(tab, push=[a, b])
    _run(tab, flush=[a])
    tab.close(a)
    p = _run(tab, push=[b])
    assert p.win == [KEEP, PUSH] and tab.state == [FREE, OPEN]
