"""Host-only: the batched block copy entry (eend_copy_blocks) is declared in the public header, exported by the library and bound
in lib.py, and refuses every bad entry with EEND_EINVAL before any launch; a StreamSnapshot survives save / load; a slot's table
fields exported from one SlotTable and adopted into another plan and commit as the uninterrupted slot's."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER = 9
OK, EINVAL = 0, -1
A, B = 1 << 20, 1 << 24                                           # non-null, 16-byte aligned addresses that are never dereferenced


def test_entry_in_header_library_and_bindings(hip_lib):
    from fs_eend_amd import build, lib
    hdr = open(os.path.join(ROOT, "include", "eend_hip.h")).read()
    assert re.search(r"\bint eend_copy_blocks\(const eend_block_copy\* entries, int n, void\* stream\);", hdr)
    assert re.search(r"\blong eend_copy_blocks_tile_bytes\(void\);", hdr)
    assert re.search(r"typedef struct eend_block_copy \{\s*const void\* src;\s*void\* dst;\s*long nblocks, block_bytes, src_stride, "
                     r"dst_stride;\s*\} eend_block_copy;", hdr)
    assert "eend_copy_blocks" in lib.PROTOTYPES and len(lib.PROTOTYPES["eend_copy_blocks"]) == 3
    L = lib.load()
    assert L.eend_copy_blocks is not None and L.eend_copy_blocks_tile_bytes is not None
    assert L.eend_abi_version() == 5 and lib.ABI_VERSION == 5
    assert "copy_blocks.hip" in build.SOURCES


def _call(L, entries, n=None):
    from fs_eend_amd.lib import BlockCopy
    arr = (BlockCopy * max(len(entries), 1))(*[BlockCopy(*e) for e in entries])
    return L.eend_copy_blocks(arr, len(entries) if n is None else n, None)


def test_tile_bytes(hip_lib):
    tile = hip_lib.eend_copy_blocks_tile_bytes()
    assert tile > 0 and tile % 16 == 0


def test_entry_rejects_bad_arguments_without_launch(hip_lib):
    L = hip_lib
    good = dict(src=A, dst=B, nblocks=4, block_bytes=1024, src_stride=4096, dst_stride=1024)
    E = lambda **kw: tuple(dict(good, **kw)[k] for k in ("src", "dst", "nblocks", "block_bytes", "src_stride", "dst_stride"))
    empty = (None, None, 0, 0, 0, 0)
    assert L.eend_copy_blocks(None, 1, None) == EINVAL            # null entries with n > 0
    assert _call(L, [empty], n=-1) == EINVAL
    assert _call(L, [empty] * 65) == EINVAL                       # n > 64
    bad = [dict(src=None), dict(dst=None),                        # null pointer in an entry that moves bytes
           dict(nblocks=-1), dict(block_bytes=-16), dict(src_stride=-4096), dict(dst_stride=-1024),
           dict(src=A + 8), dict(dst=B + 4), dict(block_bytes=1000), dict(src_stride=4100), dict(dst_stride=1032),
           dict(src_stride=1008), dict(dst_stride=512),          # a stride below block_bytes with nblocks > 1
           dict(dst=A), dict(dst=A + 3 * 4096 + 1008), dict(src=B + 4 * 1024 - 16),    # first / last byte ranges overlap
           dict(dst=A + 1024, dst_stride=4096)]                  # interleaved blocks: the two ranges still overlap
    for kw in bad:
        assert _call(L, [E(**kw)]) == EINVAL, kw
        assert _call(L, [empty, E(), E(**kw)]) == EINVAL, kw      # wherever it stands in the table
    # misaligned or negative fields are refused in an entry that moves nothing too
    assert _call(L, [(None, None, 0, 8, 0, 0)]) == EINVAL and _call(L, [(None, None, -1, 0, 0, 0)]) == EINVAL


def test_calls_that_move_nothing_succeed_without_launch(hip_lib):
    L = hip_lib
    assert L.eend_copy_blocks(None, 0, None) == OK
    assert _call(L, [(None, None, 0, 0, 0, 0)], n=0) == OK
    # empty entries: no blocks, or blocks of no bytes (a fresh slot: len = 0); null pointers allowed, strides free
    assert _call(L, [(None, None, 0, 1024, 0, 0), (A, B, 24, 0, 128 * 1024, 0), (None, B, 5, 0, 0, 0)] + [(A, A, 0, 0, 0, 0)] * 61) == OK


def _snap():
    from fs_eend_amd.multistream import StreamSnapshot
    g = torch.Generator().manual_seed(4)
    blob = torch.randint(0, 256, (3 * 256,), generator=g, dtype=torch.uint8)
    sig = {"kind": "fs", "D": 256, "H": 4, "C": 3, "k": 19, "enc_layers": 1, "dec_layers": 1, "in_size": 345,
           "dtypes": "kv float16, window float16"}
    table = {"state": "flushing", "t": 31, "n_enc": 27, "n_dec": 22, "flush_left": 5}
    parts = {"model": {"blob": blob, "sections": [("enc0.k", 0, 256), ("enc0.v", 256, 16), ("win", 512, 256)]},
             "tracker": {"hist": torch.arange(64), "segs": [(0, 3, 9), (1, 4, 30)], "pending": [], "overflowed": False,
                         "state": "open", "config": {"threshold": 0.5, "median": 11}}}
    return StreamSnapshot("fs", sig, table, parts)


def test_snapshot_survives_save_and_load(tmp_path):
    from fs_eend_amd.multistream import SlotError, StreamSnapshot
    a = _snap()
    assert a.nbytes == 3 * 256 + 64 * 8
    path = str(tmp_path / "slot.snap")
    a.save(path)
    b = StreamSnapshot.load(path)
    assert (b.kind, b.signature, b.table) == (a.kind, a.signature, a.table) and b.nbytes == a.nbytes
    assert sorted(b.parts) == sorted(a.parts)
    assert b.parts["model"]["sections"] == a.parts["model"]["sections"]
    assert b.parts["model"]["blob"].dtype == torch.uint8 and torch.equal(b.parts["model"]["blob"], a.parts["model"]["blob"])
    ta, tb = a.parts["tracker"], b.parts["tracker"]
    assert torch.equal(tb.pop("hist"), ta["hist"]) and tb == {k: v for k, v in ta.items() if k != "hist"}
    assert not b.mismatch(a.signature)
    torch.save({"format": 99}, path)
    with pytest.raises(SlotError, match="format"):
        StreamSnapshot.load(path)


def test_signature_mismatch_is_reported():
    from fs_eend_amd.multistream import SlotError, StreamSnapshot, check_parts
    a = _snap()
    assert a.mismatch(dict(a.signature)) == {}
    assert a.mismatch(dict(a.signature, C=6, kind="ls")) == {"C": (3, 6), "kind": ("fs", "ls")}
    check_parts(a, ("model", "tracker"))
    for parts in (("model",), ("model", "tracker", "frontend"), ("model", "frontend")):
        with pytest.raises(SlotError, match="parts"):
            check_parts(a, parts)
    with pytest.raises(SlotError):
        check_parts({"model": None}, ("model",))
    assert isinstance(a, StreamSnapshot)


def _pushed(table, s, n):
    """n committed one-frame plans of slot s -> [frames of logits emitted per step]"""
    out = []
    for _ in range(n):
        plan = table.plan([s])
        out.append(plan.dec[s])
        table.commit(plan)
    return out


def _fields(tab, s):
    return (tab.state[s], tab.t[s], tab.n_enc[s], tab.n_dec[s], tab.flush_left[s])


@pytest.mark.parametrize("t", [0, 8, 9, 10, 40])
def test_adopted_slot_plans_and_commits_as_the_uninterrupted_one(t):
    from fs_eend_amd.multistream import SlotTable
    a, b = SlotTable(2, CENTER), SlotTable(5, CENTER)
    sa = a.open()
    for _ in range(3):
        b.open()                                                  # the stream lands at another index: slot 3
    _pushed(a, sa, t)
    f = a.export(sa)
    assert f == {"state": "open", "t": t, "n_enc": t, "n_dec": max(0, t - CENTER), "flush_left": 0}
    sb = b.adopt(dict(f))
    assert sb == 3 and _fields(b, sb) == _fields(a, sa)
    assert _pushed(a, sa, 12) == _pushed(b, sb, 12)               # the same frames emit at the same steps
    pa, pb = a.plan_frames({sa: 3}, [sa], 4), b.plan_frames({sb: 3}, [sb], 4)
    assert (pa.npush[sa], pa.ndummy[sa], pa.dec[sa]) == (pb.npush[sb], pb.ndummy[sb], pb.dec[sb])
    a.commit(pa), b.commit(pb)
    while a.state[sa] != "done":
        pa, pb = a.plan(), b.plan()
        assert (pa.ndummy[sa], pa.dec[sa]) == (pb.ndummy[sb], pb.dec[sb])
        a.commit(pa), b.commit(pb)
        assert _fields(b, sb) == _fields(a, sa)
    assert b.state[sb] == "done" and a.n_dec[sa] == t + 12 + 3


@pytest.mark.parametrize("left", [9, 4, 1])
def test_adopted_flushing_slot_finishes_as_the_uninterrupted_one(left):
    from fs_eend_amd.multistream import SlotTable
    a, b = SlotTable(3, CENTER), SlotTable(2, CENTER)
    a.open()
    sa = a.open()
    _pushed(a, sa, 25)
    if left == CENTER:                                            # flushed with a full step of pushes: no dummy frame taken yet
        a.commit(a.plan_frames({sa: 4}, [sa], 4))
    else:                                                         # flushed alone: CENTER - left dummy frames taken with it
        a.commit(a.plan_frames({}, [sa], CENTER - left))
    pushed = a.n_enc[sa]
    assert (a.state[sa], a.flush_left[sa]) == ("flushing", left)
    sb = b.adopt(a.export(sa))
    assert sb == 0 and _fields(b, sb) == _fields(a, sa)
    steps = 0
    while a.state[sa] != "done":
        pa, pb = a.plan(), b.plan()
        assert (pa.ndummy[sa], pa.dec[sa]) == (pb.ndummy[sb], pb.dec[sb]) == (1, 1)
        a.commit(pa), b.commit(pb)
        steps += 1
    assert steps == left and _fields(b, sb) == _fields(a, sa) and b.n_dec[sb] == pushed


def test_export_and_adopt_check_their_arguments():
    from fs_eend_amd.multistream import SlotError, SlotTable
    tab = SlotTable(1, CENTER)
    with pytest.raises(SlotError):
        tab.export(0)                                             # a free slot has nothing to export
    s = tab.open()
    f = tab.export(s)
    with pytest.raises(SlotError, match="in use"):
        tab.adopt(f)                                              # no free slot
    tab.close(s)
    for bad in (dict(f, state="free"), dict(f, t=-1), dict(f, n_enc="3"), {k: v for k, v in f.items() if k != "n_dec"}, None):
        with pytest.raises(SlotError):
            tab.adopt(bad)
        assert tab.state == ["free"]
    assert tab.adopt(f) == 0
