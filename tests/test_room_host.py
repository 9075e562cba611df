"""CPU: the host side of room impulse responses (fs_eend_amd/rooms.py, eend_room_rir_f32): the entry is exported and bound at
ABI 5, `draw_rooms` is deterministic and keeps its distances, every refusal of `plan_rooms` is raised without a device, the
word and tile tables are what the kernel indexes with, `draw_recipes(rir_groups=)` keeps a mixture in one room, and
`SourcePool.from_device` refuses what it cannot adopt.  No launches here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fs_eend_amd import rooms as RM
from fs_eend_amd import simulate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row(**kw):
    r = {"name": "h", "size": (3.0, 4.0, 2.5), "source": (1.0, 1.5, 1.2), "receiver": (2.0, 3.0, 1.0), "beta": 0.8, "c": 343.0}
    r.update(kw)
    return r


def test_entry_is_exported_and_bound(hip_lib):
    from fs_eend_amd import lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eend_hip.h")).read(), flags=re.S)
    for name, nargs in (("eend_room_rir_f32", 6), ("eend_room_limits", 4)):
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(L.PROTOTYPES[name]) == nargs
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert hip_lib.eend_abi_version() == 5 == L.ABI_VERSION
    lim = RM.limits()
    hdr = open(os.path.join(ROOT, "fs-eend_amd", "csrc", "kernels.h")).read()
    for name, val in (("ROOM_TILE", lim["tile"]), ("ROOM_WINDOW", lim["window"]), ("ROOM_MAX_ROWS", lim["max_rows"]),
                      ("ROOM_MAX_AXIS", lim["max_axis"]), ("ROOM_WORDS", RM.ROOM_WORDS)):
        assert re.search(rf"#define {name} {val}\b", hdr)
    assert lim["window"] == 64 and lim["tile"] >= 1 and lim["max_axis"] >= 750
    assert hip_lib.eend_room_limits(None, None, None, None) == -1
    # argument checks come before any launch: no row is a no-op, bad arguments are EEND_EINVAL (-1)
    call = lambda R=0, tiles=0: hip_lib.eend_room_rir_f32(None, R, None, tiles, None, None)
    assert call() == 0
    assert call(tiles=1) == -1 and call(R=-1) == -1 and call(R=lim["max_rows"] + 1, tiles=lim["max_rows"] + 1) == -1
    assert call(R=1, tiles=1) == -1                         # a row with no tables


def test_draw_rooms_is_deterministic_and_keeps_its_distances():
    rows, groups = RM.draw_rooms(7, n_rooms=40, n_sources=3, min_distance=1.0, margin=0.4)
    again, groups2 = RM.draw_rooms(7, n_rooms=40, n_sources=3, min_distance=1.0, margin=0.4)
    assert rows == again and groups == groups2 and rows != RM.draw_rooms(8, n_rooms=40, n_sources=3, min_distance=1.0, margin=0.4)[0]
    assert len(rows) == 120 and rows[4]["name"] == "room_00001_01" and rows[4]["room"] == "room_00001"
    assert list(groups) == [f"room_{i:05d}" for i in range(40)] and groups["room_00001"] == [f"room_00001_{j:02d}" for j in range(3)]
    for r in rows:
        L, s, m = np.array(r["size"]), np.array(r["source"]), np.array(r["receiver"])
        assert (L >= [3.0, 3.0, 2.5]).all() and (L <= [10.0, 10.0, 4.0]).all() and 0.2 <= r["rt60"] <= 0.8
        assert (s >= 0.4).all() and (s <= L - 0.4).all() and (m >= 0.4).all() and (m <= L - 0.4).all()
        assert np.linalg.norm(s - m) >= 1.0
        assert r["beta"] == RM.eyring_beta(L, r["rt60"], 343.0) and r["c"] == 343.0
    # the sources of a room share its receiver, size and walls
    assert len({(r["size"], r["receiver"], r["beta"]) for r in rows[3:6]}) == 1
    with pytest.raises(ValueError, match="margin"):
        RM.draw_rooms(1, 1, 1, margin=1.3)
    RM.plan_rooms(rows, 100)                                # what it draws is what plan_rooms takes


def test_plan_refusals_need_no_device(hip_lib):
    lim = RM.limits()
    RM.plan_rooms([row()], 100)                             # the good case passes
    with pytest.raises(ValueError, match="below 1"):
        RM.plan_rooms([row(size=(3.0, 0.99, 2.5), source=(1.0, 0.5, 1.2), receiver=(2.0, 0.7, 1.0))], 100)
    for s in ((0.0, 1.5, 1.2), (3.0, 1.5, 1.2), (1.0, 4.5, 1.2), (1.0, 1.5, -0.1)):
        with pytest.raises(ValueError, match="source .* not strictly inside"):
            RM.plan_rooms([row(source=s)], 100)
        with pytest.raises(ValueError, match="receiver .* not strictly inside"):
            RM.plan_rooms([row(receiver=s)], 100)
    for b in (-0.01, 1.01, (0.5, 0.5, 0.5, 0.5, 0.5, 1.5)):
        with pytest.raises(ValueError, match="outside \\[0, 1\\]"):
            RM.plan_rooms([row(beta=b)], 100)
    RM.plan_rooms([row(beta=0.0), row(name="g", beta=1.0)], 100)                            # both ends are taken
    for c in (0.0, -343.0):
        with pytest.raises(ValueError, match="speed of sound"):
            RM.plan_rooms([row(c=c)], 100)
    for K in (0, -3, S.MAX_TAPS + 1):
        with pytest.raises(ValueError, match="taps"):
            RM.plan_rooms([row()], K)
    RM.plan_rooms([row()], S.MAX_TAPS)
    with pytest.raises(ValueError, match="1 cm"):
        RM.plan_rooms([row(receiver=(1.0, 1.5, 1.205))], 100)
    RM.plan_rooms([row(receiver=(1.0, 1.5, 1.22))], 100)
    with pytest.raises(ValueError, match="twice"):
        RM.plan_rooms([row(), row()], 100)
    with pytest.raises(ValueError, match=f"at most {lim['max_rows']} rows"):
        RM.plan_rooms([row(name=i) for i in range(lim["max_rows"] + 1)], 1)
    with pytest.raises(ValueError, match="finite"):
        RM.plan_rooms([row(source=(1.0, float("nan"), 1.2))], 100)
    with pytest.raises(ValueError, match="taps names"):
        RM.plan_rooms([row(), row(name="g")], (100, 200, 300))
    with pytest.raises(ValueError, match="normalize"):
        RM.plan_rooms([row()], 100, normalize="peak")
    # a sound so fast that the image tables of a 1 m room outgrow the kernel's
    small = row(size=(1.0, 1.0, 1.0), source=(0.3, 0.4, 0.5), receiver=(0.6, 0.7, 0.5))
    RM.plan_rooms([small], S.MAX_TAPS)
    with pytest.raises(ValueError, match="image-table entries"):
        RM.plan_rooms([dict(small, c=600.0)], S.MAX_TAPS)
    from fs_eend_amd import lib as L
    with pytest.raises(L.EendHipError):
        RM.room_responses([row()], 100, device="cpu")


def test_word_and_tile_tables(hip_lib):
    T = RM.limits()["tile"]
    rows = [row(name=f"h{i}") for i in range(4)]
    p = RM.plan_rooms(rows, (1, T - 1, T, T + 1))
    assert p["rooms"].dtype == np.int64 and p["rooms"].shape == (4, RM.ROOM_WORDS) and p["tiles"].dtype == np.int64
    v = p["rooms"][:, :17].view(np.float64)
    assert v[0].tolist() == [3.0, 4.0, 2.5, 1.0, 1.5, 1.2, 2.0, 3.0, 1.0] + [0.8] * 6 + [8000.0 / 343.0, 1.0 / (4.0 * np.pi)]
    assert p["rooms"][:, 17:].tolist() == [[1, 0, 1], [T - 1, 1, 1], [T, T, 1], [T + 1, 2 * T, 2]]      # K, first sample, tiles
    assert p["table"] == {"h0": (0, 1), "h1": (1, T - 1), "h2": (T, T), "h3": (2 * T, T + 1)} and p["total"] == 3 * T + 1
    # every tile once, the one with the most images (the latest taps; the rooms are the same) first
    assert sorted(p["tiles"].tolist()) == [[0, 0], [1, 0], [2, 0], [3, 0], [3, T]] and p["tiles"][0].tolist() == [3, T]
    # ragged taps over rooms of different sizes: late tiles of the small room lead, every (row, tile) is there once
    rows = [row(name="big", size=(9.0, 8.0, 4.0)), row(name="small", size=(3.0, 3.2, 2.5), receiver=(2.0, 3.0, 1.0)), row(name="one")]
    p = RM.plan_rooms(rows, (5 * T, 3 * T + 5, 1), normalize="direct")
    want = [[0, k] for k in range(0, 5 * T, T)] + [[1, k] for k in range(0, 3 * T + 5, T)] + [[2, 0]]
    assert sorted(p["tiles"].tolist()) == want and p["tiles"][0].tolist() == [1, 3 * T]
    assert p["rooms"][:, 19].tolist() == [5, 4, 1] and p["offsets"].tolist() == [0, 5 * T, 8 * T + 5]
    for r, k in p["tiles"].tolist():
        assert k % T == 0 and k < p["taps"][r]
    d0 = np.sqrt(1.0 + (1.5 * 1.5 + 0.2 * 0.2))
    assert abs(p["rooms"][:, :17].view(np.float64)[0, 16] - d0) < 1e-15                      # "direct": g = |s - r|
    assert RM.plan_rooms(rows, 10, normalize=2.5)["rooms"][:, :17].view(np.float64)[:, 16].tolist() == [2.5] * 3
    e = RM.plan_rooms([], 10)
    assert e["rooms"].shape == (0, RM.ROOM_WORDS) and e["tiles"].shape == (0, 2) and e["total"] == 0


UTTS = {f"s{s}_u{i}": (1000 * (3 * s + i), 1000) for s in range(4) for i in range(3)}
SPK2UTT = {f"s{s}": [f"s{s}_u{i}" for i in range(3)] for s in range(4)}


def test_draw_recipes_keeps_a_mixture_in_one_room():
    groups = {f"room{r}": [f"room{r}_{j}" for j in range(4)] for r in range(5)}
    rirs = {h: (100 * i, 100) for i, h in enumerate(sum(groups.values(), []))}
    recipes = S.draw_recipes(3, SPK2UTT, UTTS, rirs=rirs, n_mixtures=60, n_speakers=(2, 4), rir_groups=groups)
    assert recipes == S.draw_recipes(3, SPK2UTT, UTTS, rirs=rirs, n_mixtures=60, n_speakers=(2, 4), rir_groups=groups)
    seen = set()
    for r in recipes:
        hs = [t["rir"] for t in r["tracks"]]
        assert len(set(hs)) == len(hs) >= 2                                                # no response twice
        assert len({h.rsplit("_", 1)[0] for h in hs}) == 1 and all(h in rirs for h in hs)   # one room
        seen.add(hs[0].rsplit("_", 1)[0])
    assert seen == set(groups)
    groups["room2"] = groups["room2"][:2]
    with pytest.raises(ValueError, match="room 'room2' has 2 responses"):
        S.draw_recipes(3, SPK2UTT, UTTS, rirs=rirs, n_mixtures=60, n_speakers=(3, 4), rir_groups=groups)
    with pytest.raises(KeyError, match="unknown impulse response"):
        S.draw_recipes(3, SPK2UTT, UTTS, rirs=rirs, n_mixtures=1, rir_groups={"r": ["nope"]})
    with pytest.raises(ValueError, match="no room"):
        S.draw_recipes(3, SPK2UTT, UTTS, rirs=rirs, n_mixtures=1, rir_groups={})


def test_draw_recipes_without_groups_is_unchanged():
    rirs = {f"h{i}": (100 * i, 100) for i in range(7)}
    noises = {"n0": (0, 5000), "n1": (5000, 300)}
    for seed in (0, 5):
        a = S.draw_recipes(seed, SPK2UTT, UTTS, rirs=rirs, noises=noises, n_mixtures=20)
        b = S.draw_recipes(seed, SPK2UTT, UTTS, rirs=rirs, noises=noises, n_mixtures=20, rir_groups=None)
        assert a == b
    # pinned: the first draws of seed 5 (numpy's PCG64 stream is stable), so a change of the draw order cannot hide
    r = S.draw_recipes(5, SPK2UTT, UTTS, rirs=rirs, noises=noises, n_mixtures=1)[0]
    rng = np.random.Generator(np.random.PCG64(5))
    chosen = rng.choice(4, size=int(rng.integers(1, 5)), replace=False)
    assert [t["speaker"] for t in r["tracks"]] == [f"s{i}" for i in chosen.tolist()]


def test_source_pool_from_device_refusals():
    from fs_eend_amd import lib as L
    with pytest.raises(TypeError):
        S.SourcePool.from_device(torch.zeros(10, dtype=torch.float64), {"a": (0, 10)})
    with pytest.raises(TypeError):
        S.SourcePool.from_device(torch.zeros(10, dtype=torch.float32), {"a": (0, 10)}, storage="s16")
    with pytest.raises(TypeError):
        S.SourcePool.from_device(torch.zeros(2, 5), {"a": (0, 10)})
    with pytest.raises(ValueError, match="storage"):
        S.SourcePool.from_device(torch.zeros(10), {}, storage="mulaw")
    with pytest.raises(ValueError, match="outside"):
        S.SourcePool.from_device(torch.zeros(10), {"a": (0, 6), "b": (6, 5)})
    with pytest.raises(ValueError, match="outside"):
        S.SourcePool.from_device(torch.zeros(10), {"a": (-1, 6)})
    with pytest.raises(L.EendHipError):                     # a host tensor: the pool lives on the GPU
        S.SourcePool.from_device(torch.zeros(10), {"a": (0, 6), "b": (6, 4)})
