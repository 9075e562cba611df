"""CPU: the host side of the device data path (fs_eend_amd/device_data.py, eend_chunk_batch_f32): the entry is exported and bound
at ABI 5, every refusal is raised before anything touches a device, the descriptor and tile tables are what the kernels index
with, and ChunkDataset yields the rows of data.on_the_fly_chunk under data.MyDistributedSampler.  No launches here."""
import ctypes
import os
import re

import numpy as np
import pytest

from fs_eend_amd import data as D
from fs_eend_amd import device_data as DD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_exported_and_bound(hip_lib):
    from fs_eend_amd import lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eend_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+eend_chunk_batch_f32\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m and len(m.group(1).split(",")) == len(L.PROTOTYPES["eend_chunk_batch_f32"]) == 20
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "eend_chunk_batch_f32")
    assert hip_lib.eend_abi_version() == 5 == L.ABI_VERSION
    # argument checks of the entry itself come before any launch: no chunks is a no-op, bad arguments are EEND_EINVAL (-1)
    z = [None] * 3
    call = lambda storage=0, B=0, n_stft=0, S=4, mode=1, ctx=7, sub=10: hip_lib.eend_chunk_batch_f32(
        None, storage, None, None, B, None, n_stft, None, 0, None, None, None, None, S, mode, ctx, sub, *z)
    assert call() == 0
    assert call(n_stft=1) == -1 and call(storage=2) == -1 and call(mode=3) == -1 and call(ctx=-1) == -1 and call(sub=0) == -1
    assert call(S=0) == -1 and call(S=65) == -1 and call(B=65536) == -1 and call(B=1) == -1        # B = 1 with no descriptors


def corpus(storage="f32"):
    c = DD.DeviceCorpus("cuda:0", storage=storage)
    dt = np.float32 if storage == "f32" else np.int16
    c.add("r0", np.zeros(10400, dtype=dt), [("a", 0.1, 0.5), ("b", 0.3, 1.0), ("c", 0.9, 1.2)], {"a": "s1", "b": "s0", "c": "s1"})
    c.add("r1", np.zeros(20013, dtype=dt), [("d", 0.0, 2.0)], {"d": "x"})
    c.add("r2", np.zeros(5120, dtype=dt), [], {})
    return c


def test_corpus_bookkeeping():
    c = corpus()
    assert c.reco2dur == {"r0": 1.3, "r1": 20013 / 8000, "r2": 0.64} and c.recordings()[0] == ("r0", 1.3)
    assert c.speakers == {"r0": ["s0", "s1"], "r1": ["x"], "r2": []}
    assert c._off == {"r0": 0, "r1": 10400, "r2": 30413} and c._seg == {"r0": (0, 3), "r1": (3, 4), "r2": (4, 4)}
    assert c._segrows == [(10, 50, 1), (30, 100, 0), (90, 120, 1), (0, 200, 0)]
    # reco2dur feeds data.chunk_table as it is
    rows = D.chunk_table(c.recordings(), chunk_size=5, chunk_step=5, frame_shift=80, rate=8000, subsampling=10)
    assert rows[:2] == [("r0", 0, 50), ("r0", 50, 100)] and [r[0] for r in rows].count("r1") == 5 and rows[-1] == ("r2", 0, 50)
    with pytest.raises(ValueError):
        c.add("r0", np.zeros(8, dtype=np.float32), [], {})
    with pytest.raises(TypeError):
        c.add("r3", np.zeros(8, dtype=np.int16), [], {})
    with pytest.raises(TypeError):
        corpus("s16").add("r3", np.zeros(8, dtype=np.float32), [], {})


def test_refusals_come_before_any_device_work():
    with pytest.raises(NotImplementedError):
        DD.DeviceCorpus("cuda:0", frame_shift=64)
    with pytest.raises(NotImplementedError):
        DD.DeviceCorpus("cuda:0", frame_size=256)
    with pytest.raises(ValueError):
        DD.DeviceCorpus("cuda:0", rate=16000)
    with pytest.raises(ValueError):
        DD.DeviceCorpus("cuda:0", storage="mulaw")
    c = corpus()                                            # never finalized: nothing below may get as far as the device
    ok = [("r0", 0, 50)]
    for transform in ("logmel", "logmel23_mvn", "", None):
        with pytest.raises(ValueError):
            c.batch(ok, input_transform=transform)
    with pytest.raises(IndexError):
        c.batch(ok, n_speakers=1)                           # r0 has two speakers
    with pytest.raises(KeyError):
        c.batch([("nope", 0, 50)])
    with pytest.raises(ValueError):
        c.batch([("r0", -1, 50)])
    with pytest.raises(ValueError):
        c.batch([("r0", 60, 50)])
    with pytest.raises(ValueError):
        c.batch(ok, context_size=-1)
    with pytest.raises(ValueError):
        c.batch(ok, subsampling=0)
    with pytest.raises(RuntimeError, match="finalize"):
        c.batch(ok)                                         # a good call gets as far as this, and no further
    # more than 2^31 - 1 frames or rows, and more chunks than one launch grid takes
    big = (2 ** 31) * 80
    z = [0]
    with pytest.raises(ValueError, match="2\\^31"):
        DD.plan_batch(z, [big], z, [2 ** 31], z, z, 10)
    half = (2 ** 30) * 80
    with pytest.raises(ValueError, match="2\\^31"):
        DD.plan_batch(z * 2, [half] * 2, z * 2, [2 ** 30] * 2, z * 2, z * 2, 1)
    n = 65536
    with pytest.raises(ValueError, match="65535"):
        DD.plan_batch([0] * n, [0] * n, [0] * n, [0] * n, [0] * n, [0] * n, 10)


def test_descriptor_and_tile_tables():
    """Chunks of 0, 1, 64, 65 and 129 frames: one STFT tile per 64 frames, one splice tile per 16 model frames."""
    c = corpus()
    rows = [("r1", 251, 300), ("r1", 250, 251), ("r0", 10, 74), ("r1", 100, 165), ("r0", 1, 200)]       # the last is clipped: 129 frames
    p, S, S_max, recs = c.plan(rows, subsampling=10)
    assert p["frames"].tolist() == [0, 1, 64, 65, 129] and p["rows"].tolist() == [0, 1, 7, 7, 13]
    assert (S, S_max, recs) == ([1, 1, 2, 1, 2], 2, ["r1", "r1", "r0", "r1", "r0"])
    assert (p["y_rows"], p["o_rows"]) == (259, 28)
    assert p["desc"].dtype == np.int64 and p["desc"].tolist() == [
        # first sample, samples, frames, Y row, start, end, segment rows
        [10400 + 20013, 0, 0, 0, 251, 300, 3, 4],
        [10400 + 20000, 13, 1, 0, 250, 251, 3, 4],
        [800, 5120, 64, 1, 10, 74, 0, 3],
        [10400 + 8000, 5200, 65, 65, 100, 165, 3, 4],
        [80, 10320, 129, 130, 1, 200, 0, 3]]
    assert p["stft"].tolist() == [[1, 0, 1], [2, 0, 64], [3, 0, 64], [3, 64, 1], [4, 0, 64], [4, 64, 64], [4, 128, 1]]
    assert p["splice"].tolist() == [[1, 0, 1, 0], [2, 0, 7, 1], [3, 0, 7, 8], [4, 0, 13, 15]]
    # subsampling 1: 129 model frames are 9 splice tiles, the last of one row
    p1 = c.plan(rows, subsampling=1, context_size=0)[0]
    assert p1["rows"].tolist() == [0, 1, 64, 65, 129]
    assert p1["splice"][-2:].tolist() == [[4, 112, 16, 130 + 112], [4, 128, 1, 130 + 128]]
    assert len(p1["splice"]) == 1 + 4 + 5 + 9
    # every chunk stays inside the corpus, every tile inside its chunk
    d = p["desc"]
    assert (d[:, 0] + d[:, 1] <= 10400 + 20013 + 5120).all()
    for ci, first, cnt in p["stft"].tolist():
        assert 0 < cnt <= 64 and first + cnt <= d[ci, 2]
    for ci, first, cnt, orow in p["splice"].tolist():
        assert 0 < cnt <= 16 and first + cnt <= p["rows"][ci] and orow == p["obase"][ci] + first
    # an empty batch
    e = c.plan([])[0]
    assert e["desc"].shape == (0, 8) and e["stft"].shape == (0, 3) and e["splice"].shape == (0, 4) and e["o_rows"] == 0


def test_chunk_dataset_follows_the_sampler():
    c = corpus()
    table = D.chunk_table(c.recordings(), chunk_size=5, chunk_step=5, frame_shift=80, rate=8000, subsampling=10, on_the_fly=True)
    assert len(table) >= 4 and len(table[0]) == 4
    ds = DD.ChunkDataset(c, table, chunk_size=5, subsampling=10, data_type="train")
    assert len(ds) == len(table)
    sampler = D.MyDistributedSampler(ds, num_replicas=1, rank=0, shuffle=True, seed=3)
    pairs = list(sampler)
    assert len(pairs) == len(table)
    for index, seed in pairs:
        got = ds[(index, seed)]
        assert got == D.on_the_fly_chunk(table[index], seed, 5, 10, "train")
        rec, st, ed = got
        assert rec == table[index][0] and 0 <= st <= ed <= table[index][1]
    # evaluation keeps the grid; a plain index returns the row itself, with or without the recorded length
    ev = DD.ChunkDataset(c, table, chunk_size=5, subsampling=10, data_type="dev")
    assert ev[(1, 99)] == (table[1][0], table[1][2], table[1][3]) == ev[1]
    grid = D.chunk_table(c.recordings(), chunk_size=5, chunk_step=5, frame_shift=80, rate=8000, subsampling=10)
    assert DD.ChunkDataset(c, grid)[0] == grid[0]
    with pytest.raises(ValueError):
        DD.ChunkDataset(c, grid)[(0, 1)]
    with pytest.raises(KeyError):
        DD.ChunkDataset(c, [("nope", 0, 10)])
    # the collate function of a DataLoader over the dataset receives exactly these descriptors
    from torch.utils.data import DataLoader
    seen = []
    loader = DataLoader(ds, batch_size=3, sampler=D.MyDistributedSampler(ds, num_replicas=1, rank=0, shuffle=True, seed=3),
                        num_workers=0, collate_fn=lambda rows: seen.append(list(rows)) or rows)
    list(loader)
    assert [r for b in seen for r in b] == [ds[p] for p in pairs]
