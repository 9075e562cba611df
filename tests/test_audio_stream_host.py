"""CPU: the frame bookkeeping of the incremental audio front-end (audio_stream.FrontEndTable) -- per-call frame counts add up to
the batch front-end's, emitted ranges are contiguous, nothing is emitted before its samples are in, and the errors of misuse."""
import random

import pytest

from fs_eend_amd import audio_stream as A
from fs_eend_amd.multistream import SlotError

LENGTHS = [0, 1, 79, 80, 81, 99, 100, 659, 660, 661, 800, 801, 1600, 8000, 12345]
SHAPES = [(7, 10), (0, 1), (2, 4), (15, 16)]


def batch_counts(n, ctx, sub):
    """feature.logmel / splice_subsample: n_frames = 1 + n // 80 - (n % 80 == 0), ceil(n_frames / sub) model frames"""
    T = 1 + n // 80 - (1 if n % 80 == 0 else 0)
    return T, (T + sub - 1) // sub


def chunkings(n, rng):
    yield "whole", [n]
    yield "ones", [1] * min(n, 900) + ([n - 900] if n > 900 else [])
    for k in (79, 80, 81, 800):
        yield str(k), [k] * (n // k) + ([n % k] if n % k else [])
    cuts = sorted(rng.randrange(n + 1) for _ in range(rng.randrange(1, 12)))
    yield "random", [b - a for a, b in zip([0] + cuts, cuts + [n])]


def run(n, sizes, ctx, sub, slot=2, S=4):
    t = A.FrontEndTable(S, ctx, sub)
    t.reset(slot)
    f = j = recv = 0
    for k, m in enumerate(sizes + [None]):
        end = m is None
        plan = t.plan({} if end else {slot: m}, end=[slot] if end else ())
        assert [p.slot for p in plan] == [slot]
        p = plan[0]
        assert (p.recv0, p.f0, p.j0) == (recv, f, j)                        # contiguous ranges
        assert p.f1 >= p.f0 and p.j1 >= p.j0
        if not end:
            assert p.recv1 == recv + m
            for jj in range(p.j0, p.j1):
                assert p.recv1 >= 80 * (sub * jj + ctx) + 100, (jj, p.recv1)  # at (7, 10): samples up to 800 j + 659
            assert 80 * (p.f1 - 1) + 100 <= p.recv1 or p.f1 == 0             # log-mel frame f needs samples up to 80 f + 99
        assert 0 <= p.f1 - p.rb1 <= 2 * ctx < A.RING                       # the ring holds what later splices read
        assert p.rb0 <= p.rb1 and p.rb0 <= p.f0
        for jj in range(p.j0, p.j1):                                        # every frame a splice reads is in the ring or new
            for c in range(2 * ctx + 1):
                fr = jj * sub + c - ctx
                assert fr < 0 or fr >= p.f1 or fr >= p.rb0
        if p.f0 < p.f1:
            assert p.recv1 - (80 * p.f1 - 100) < A.TAIL or end              # the tail that stays behind fits
        assert recv - (80 * p.f0 - 100) < A.TAIL
        t.commit(plan)
        recv, f, j = p.recv1, p.f1, p.j1
    assert t.state[slot] == A.ENDED
    return recv, f, j


@pytest.mark.parametrize("ctx,sub", SHAPES)
def test_counts_add_up_to_batch(ctx, sub):
    rng = random.Random(ctx * 31 + sub)
    for n in LENGTHS:
        for name, sizes in chunkings(n, rng):
            assert sum(sizes) == n
            recv, T, J = run(n, sizes, ctx, sub)
            assert (T, J) == batch_counts(n, ctx, sub), (n, name)


def test_readiness_edges():
    t = A.FrontEndTable(1)
    assert [A.logmel_frames(n, False) for n in (0, 99, 100, 179, 180)] == [0, 0, 1, 1, 2]
    assert [A.logmel_frames(n, True) for n in (0, 1, 79, 80, 81, 160)] == [0, 1, 1, 1, 2, 2]
    assert [A.model_frames(T, False, 7, 10) for T in (0, 7, 8, 17, 18)] == [0, 0, 1, 1, 2]
    assert [A.model_frames(T, True, 7, 10) for T in (0, 1, 10, 11)] == [0, 1, 1, 2]
    t.reset(0)
    p = t.plan({0: 659})[0]
    assert p.j1 == 0 and p.f1 == 7
    t.commit([p])
    p = t.plan({0: 1})[0]
    assert p.j1 == 1 and p.f1 == 8


def test_many_slots_in_one_call():
    t = A.FrontEndTable(5, 7, 10)
    for s in (0, 1, 3):
        t.reset(s)
    plan = t.plan({3: 800, 0: 1000}, end=[1])
    assert [p.slot for p in plan] == [0, 1, 3]
    assert [(p.f1, p.j1) for p in plan] == [(12, 1), (0, 0), (9, 1)]
    t.commit(plan)
    assert t.recv == [1000, 0, 0, 800, 0] and t.state[1] == A.ENDED and t.state[2] == A.FREE


def test_errors():
    t = A.FrontEndTable(3)
    with pytest.raises(SlotError):
        t.plan({0: 10})                                                     # never reset: free
    t.reset(0)
    with pytest.raises(SlotError):
        t.plan({3: 10})                                                     # unknown slot
    with pytest.raises(SlotError):
        t.plan({}, end=[0, 0])
    with pytest.raises(ValueError):
        t.plan({0: -1})
    t.commit(t.plan({0: 500}, end=[0]))
    with pytest.raises(SlotError):
        t.plan({0: 10})                                                     # feed after end
    with pytest.raises(SlotError):
        t.plan({}, end=[0])
    t.reset(0)
    assert t.plan({0: 10})[0].recv0 == 0                                    # reset starts over
    t.close(0)
    with pytest.raises(SlotError):
        t.plan({0: 10})
    for bad in [dict(context_size=16), dict(context_size=-1), dict(subsampling=0), dict(subsampling=17)]:
        with pytest.raises(ValueError):
            A.FrontEndTable(2, **bad)


def test_feed_descriptor_and_tile_tables():
    """The words of one feed, written out by hand from the rules of audio_stream's module text (ctx 2, sub 4: log-mel frame f
    needs 80 f + 100 samples, model frame j needs log-mel frame 4 j + 2, the ring starts at frame max(0, min(T, 4 j - 2))).

    Slots 1 and 2 each hold 500 samples from an earlier call: frames 0..5, model frame 0 emitted, ring = frames 2..5.
    slot 0: 0 -> 5700 = 100 + 80 * 70 samples: frames 0..70 (two STFT tiles, 64 + 7), model frames 0..17 since 4 * 17 + 2 = 70
            (two splice tiles, 16 + 2), ring afterwards from frame 4 * 18 - 2 = 70; its 71 rows of Y start at row 0.
    slot 1: 500 -> 501 samples: frame 6 needs 580, so nothing new and no tile, but its 4 ring rows still take Y rows 71..74.
    slot 2: ends at 500 samples: 1 + 500 // 80 = 7 frames in all, so frame 6 is new (one STFT tile), ceil(7 / 4) = 2 model
            frames, so model frame 1 is new (one splice tile, output row 18), ring afterwards from frame 6; Y rows 75..79 hold
            ring frames 2..5 and frame 6."""
    t = A.FrontEndTable(3, 2, 4)
    for s in range(3):
        t.reset(s)
    t.commit(t.plan({1: 500, 2: 500}))
    assert (t.frames, t.mframes) == ([0, 6, 6], [0, 1, 1])
    desc, stft, splice, rows, y_rows, o_rows = A.feed_words(t.plan({0: 5700, 1: 1}, end=[2]), [0x1000, 0x2000, 0])
    #                chunk  recv0 recv1 f0 f1 rb0 rb1 ybase slot
    assert desc == [[0x1000, 0, 5700, 0, 71, 0, 70, 0, 0],
                    [0x2000, 500, 501, 6, 6, 2, 2, 71, 1],
                    [0, 500, 500, 6, 7, 2, 6, 75, 2]]
    assert stft == [[0, 0, 64], [0, 64, 7], [2, 6, 1]]                      # {descriptor, first frame, frames}
    assert splice == [[0, 0, 16, 0], [0, 16, 2, 16], [2, 1, 1, 18]]         # {descriptor, first model frame, rows, output row}
    assert (y_rows, o_rows) == (80, 19)
    assert rows == {0: (0, 18), 1: (18, 0), 2: (18, 1)}


def test_front_end_rejects_batch_only_options():
    for kw in [dict(input_transform="logmel23_mn"), dict(input_transform="logmel23", pad_mode="reflect"),
               dict(input_transform="mfcc")]:
        with pytest.raises(ValueError, match="logmel23_mn|reflect|unsupported"):
            A.AudioFrontEnd(2, device="cpu", **kw)
