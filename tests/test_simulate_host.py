"""CPU: the host side of simulated mixtures (fs_eend_amd/simulate.py, eend_sim_mix_f32): the entry is exported and bound at ABI 5,
every refusal of `plan` is raised without a device, and the tables of a hand-worked two-mixture case are what the kernels index
with.  No launches here."""
import ctypes
import os
import re

import numpy as np
import pytest

from fs_eend_amd import simulate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_exported_and_bound(hip_lib):
    from fs_eend_amd import lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eend_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+eend_sim_mix_f32\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m and len(m.group(1).split(",")) == len(L.PROTOTYPES["eend_sim_mix_f32"]) == 20
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "eend_sim_mix_f32")
    assert hip_lib.eend_abi_version() == 5 == L.ABI_VERSION
    # the layout constants the host plans with are the kernels'
    v = [ctypes.c_int() for _ in range(3)]
    assert hip_lib.eend_sim_limits(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [S.TILE, S.SLICE, S.MAX_TAPS] == [2048, 1024, 8192]
    hdr = open(os.path.join(ROOT, "fs-eend_amd", "csrc", "kernels.h")).read()
    for name, val in (("SIM_MIX_WORDS", S.MIX_WORDS), ("SIM_TRACK_WORDS", S.TRACK_WORDS), ("SIM_PLACE_WORDS", S.PLACE_WORDS)):
        assert re.search(rf"#define {name} {val}\b", hdr)
    # argument checks come before any launch: no mixture is a no-op, bad arguments are EEND_EINVAL (-1)
    call = lambda us=0, ns=0, os_=0, M=0, tiles=0: hip_lib.eend_sim_mix_f32(None, us, None, None, ns, None, M, None, None, None, tiles,
                                                                             None, None, None, os_, None, None, None, None, None)
    assert call() == 0
    assert call(tiles=1) == -1 and call(us=2) == -1 and call(ns=-1) == -1 and call(os_=2) == -1 and call(M=65536) == -1
    assert call(M=1, tiles=1) == -1                         # a mixture with no tables


UTTS = {"u0": (0, 100), "u1": (100, 50), "u2": (150, 3000)}
RIRS = {"h0": (0, 4), "h1": (4, 8192), "long": (8196, 8193)}
NOISES = {"n0": (0, 7), "n1": (7, 1000)}


def recipe(**kw):
    r = {"name": "m", "length": 400, "tracks": [{"speaker": "A", "rir": "h0", "gain": 0.5, "placements": [("u0", 10), ("u1", 200)]}],
         "noise": "n0", "noise_offset": 3, "snr_db": 10.0}
    r.update(kw)
    return r


def track(placements, rir=None, speaker="A", gain=1.0):
    return {"speaker": speaker, "rir": rir, "gain": gain, "placements": placements}


def test_plan_refusals_need_no_device():
    S.plan([recipe()], UTTS, RIRS, NOISES)                                          # the good case passes
    with pytest.raises(KeyError, match="utterance"):
        S.plan([recipe(tracks=[track([("nope", 0)])])], UTTS, RIRS, NOISES)
    with pytest.raises(KeyError, match="impulse"):
        S.plan([recipe(tracks=[track([("u0", 0)], rir="nope")])], UTTS, RIRS, NOISES)
    with pytest.raises(KeyError, match="noise"):
        S.plan([recipe(noise="nope")], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="sorted"):
        S.plan([recipe(tracks=[track([("u1", 200), ("u0", 10)])])], UTTS, RIRS, NOISES)        # unsorted
    with pytest.raises(ValueError, match="overlap"):
        S.plan([recipe(tracks=[track([("u0", 10), ("u1", 109)])])], UTTS, RIRS, NOISES)        # u0 covers 10 .. 109
    S.plan([recipe(tracks=[track([("u0", 10), ("u1", 110)])])], UTTS, RIRS, NOISES)            # touching is not overlapping
    with pytest.raises(ValueError, match="before the mixture"):
        S.plan([recipe(tracks=[track([("u0", -1)])])], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="8192"):
        S.plan([recipe(tracks=[track([("u0", 0)], rir="long")])], UTTS, RIRS, NOISES)
    S.plan([recipe(tracks=[track([("u0", 0)], rir="h1")])], UTTS, RIRS, NOISES)                # 8192 taps are taken
    with pytest.raises(ValueError, match="at most 64"):
        S.plan([recipe(tracks=[track([("u0", 0)], speaker=i) for i in range(65)])], UTTS, RIRS, NOISES)
    S.plan([recipe(tracks=[track([("u0", 0)], speaker=i) for i in range(64)])], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="65535"):
        S.plan([recipe(name=i, tracks=[]) for i in range(65536)], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="2\\^31"):
        S.plan([recipe(name=i, length=2 ** 30, tracks=[]) for i in range(2)], UTTS, RIRS, NOISES)
    for n in (0, -5):
        with pytest.raises(ValueError, match="at least one sample"):
            S.plan([recipe(length=n, tracks=[])], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="twice"):
        S.plan([recipe(), recipe()], UTTS, RIRS, NOISES)
    with pytest.raises(ValueError, match="noise_offset"):
        S.plan([recipe(noise_offset=-1)], UTTS, RIRS, NOISES)
    # the device side refuses to exist on a CPU, and simulate wants finalized pools
    from fs_eend_amd import lib as L
    with pytest.raises(L.EendHipError):
        S.SourcePool("cpu")
    with pytest.raises(ValueError):
        S.SourcePool("cuda:0", storage="mulaw")
    pool = S.SourcePool("cuda:0", "s16")                    # nothing touches the device before finalize()
    pool.add("a", np.zeros(5, dtype=np.int16))
    pool.add("b", np.zeros(3, dtype=np.int16))
    assert pool.table == {"a": (0, 5), "b": (5, 3)}
    with pytest.raises(ValueError):
        pool.add("a", np.zeros(5, dtype=np.int16))
    with pytest.raises(TypeError):
        pool.add("c", np.zeros(5, dtype=np.float32))
    with pytest.raises(RuntimeError, match="finalized"):
        S.simulate(pool, None, None, [])


def test_tables_of_a_hand_worked_case():
    """Two mixtures: 5000 samples (three tiles) with two tracks, one of them dry and clipped at the end, and noise; 2048 samples
    (one tile) with one track without a placement and no noise."""
    r0 = {"name": "m0", "length": 5000, "noise": "n1", "noise_offset": 1234, "snr_db": 20.0, "tracks": [
        {"speaker": "B", "rir": "h0", "gain": 0.5, "placements": [("u0", 0), ("u1", 100), ("u0", 4900)]},
        {"speaker": "A", "rir": None, "gain": 2.0, "placements": [("u2", 2500)]}]}
    r1 = {"name": "m1", "length": 2048, "noise": "n0", "noise_offset": 5, "snr_db": None,
          "tracks": [{"speaker": "C", "rir": "h1", "gain": 1.0, "placements": []}]}
    p = S.plan([r0, r1], UTTS, RIRS, NOISES)
    bits = lambda g: int(np.float32(g).view(np.uint32))
    c = int(np.float64(10.0 ** -2.0).view(np.int64))
    assert all(p[k].dtype == np.int64 for k in ("mix", "tracks", "places", "tiles"))
    assert p["mix"].tolist() == [
        # N, first sample, first track, tracks, noise, L, o, bits of c, first tile, tiles
        [5000, 0, 0, 2, 7, 1000, 1234, c, 0, 3],
        [2048, 5000, 2, 1, 0, 0, 0, 0, 3, 1]]
    assert p["tracks"].tolist() == [
        # response (-1: none), K, bits of the gain, first placement, placements
        [0, 4, bits(0.5), 0, 3],
        [-1, 1, bits(2.0), 3, 1],
        [4, 8192, bits(1.0), 4, 0]]
    assert p["places"].tolist() == [[0, 0, 100], [100, 100, 50], [4900, 0, 100], [2500, 150, 2500]]     # start, source, clipped length
    assert p["tiles"].tolist() == [[0, 0], [0, 2048], [0, 4096], [1, 0]]
    assert (p["names"], p["lengths"].tolist(), p["offsets"].tolist(), p["total"]) == (["m0", "m1"], [5000, 2048], [0, 5000], 7048)
    assert p["segments"][0] == [("m0_0_0", 0.0, 100 / 8000), ("m0_0_1", 100 / 8000, 150 / 8000), ("m0_0_2", 4900 / 8000, 5000 / 8000),
                                ("m0_1_0", 2500 / 8000, 5000 / 8000)]
    assert p["utt2spk"][0] == {"m0_0_0": "B", "m0_0_1": "B", "m0_0_2": "B", "m0_1_0": "A"}
    assert p["segments"][1] == [] and p["utt2spk"][1] == {}
    # every placement stays inside its utterance pool and its mixture, every tile inside its mixture
    for (start, src, n), N in zip(p["places"].tolist(), [5000] * 4):
        assert 0 <= start and start + n <= N and 0 <= src and src + n <= 3150
    for m, t0 in p["tiles"].tolist():
        assert t0 % S.TILE == 0 and t0 < p["lengths"][m]
    # an empty call
    e = S.plan([], UTTS)
    assert e["mix"].shape == (0, 10) and e["tracks"].shape == (0, 5) and e["places"].shape == (0, 3) and e["tiles"].shape == (0, 2)
    assert e["total"] == 0
