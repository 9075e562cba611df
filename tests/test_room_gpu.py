"""GPU: room impulse responses on the device (fs_eend_amd/rooms.py, eend_room_rir_f32) against the float64 restatement of the
contract (tests/room_ref.py): every tap within (n_k + 16) 2^-24 S_k, bit for bit where the contract says so, and end to end
through simulate() and DeviceCorpus.batch.  Shapes are a few tiles (T taps each, as eend_room_limits reports) of small rooms; the
one MAX_TAPS row is compared on a strided subset of its tiles."""
import numpy as np
import pytest
import torch

import room_ref as R

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
G = 1.0 / (4.0 * np.pi)
ROOM, SRC, RCV = (3.0, 4.0, 2.5), (1.84, 1.47, 1.36), (0.35, 2.21, 1.93)
NEAR = (1.9, 1.2, 1.3)                                      # 0.28 m from SRC: the direct path's window is clipped at k < 0
BETA = (0.9, 0.8, 0.7, 0.85, 0.6, 0.75)


def mk(name, size=ROOM, source=SRC, receiver=RCV, beta=BETA, c=343.0):
    return {"name": name, "size": size, "source": source, "receiver": receiver, "beta": beta, "c": c}


def tile():
    from fs_eend_amd import rooms
    return rooms.limits()["tile"]


def generate(dev, rows, taps, normalize=None):
    """-> [response of every row] as numpy float32, from one room_responses call."""
    from fs_eend_amd import rooms
    pool = rooms.room_responses(rows, taps, device=dev, normalize=normalize)
    torch.cuda.synchronize()
    h = pool.samples.cpu().numpy()
    assert list(pool.table) == [r["name"] for r in rows] and pool.storage == "f32"
    return [h[a:a + n] for a, n in pool.table.values()]


def scale_of(r, normalize):
    p = np.subtract(r["source"], r["receiver"]).astype(np.float64)
    return G if normalize is None else float(np.sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2])))


def check_bound(rows, taps, hs, what, normalize=None, ranges=None):
    """Every tap (or the taps of `ranges` {row index: [(k_lo, k_hi)]}) against float64: |h - ref| <= (n_k + 16) 2^-24 S_k, and
    exactly zero where no image has a term.  -> the worst observed fraction of the bound."""
    worst, terms = 0.0, 0
    taps = [taps] * len(rows) if np.isscalar(taps) else list(taps)
    for i, (r, K, h) in enumerate(zip(rows, taps, hs)):
        assert h.shape == (K,) and np.isfinite(h).all(), (what, i)
        args = (r["size"], r["source"], r["receiver"], r["beta"], r["c"], scale_of(r, normalize), K)
        imgs = R.row_images(*args)
        for lo, hi in (ranges or {}).get(i, [(0, K)]):
            ref, n, S = R.response(*args, lo, hi, imgs=imgs)
            bound = (n + 16) * U24 * S
            err = np.abs(h[lo:hi].astype(np.float64) - ref)
            bad = np.nonzero(err > bound)[0]
            assert bad.size == 0, (what, i, K, (lo + bad[:8]).tolist(), err[bad[:8]].tolist(), bound[bad[:8]].tolist(), n[bad[:8]].tolist())
            nz = bound > 0
            terms += int(n.sum())
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
    print(f"{what}: worst |h - ref| / bound = {worst:.3e} over {terms} terms")
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_tap_counts_around_the_tile(hip_lib, dev):
    """K = 1, T - 1, T, T + 1, 3 T + 5 with six different walls, for a receiver whose direct path lies past the first taps and
    for one 0.28 m from the source, whose window is clipped at k < 0 (tau < W / 2)."""
    T = tile()
    Ks = [1, T - 1, T, T + 1, 3 * T + 5]
    rows = [mk(f"far{K}") for K in Ks] + [mk(f"near{K}", receiver=NEAR) for K in Ks]
    hs = generate(dev, rows, Ks + Ks)
    assert check_bound(rows, Ks + Ks, hs, "K sweep") > 0
    assert hs[0][0] == 0 and hs[5][0] != 0                   # K = 1: nothing has arrived at 1.76 m; the near one's sidelobe has
    assert np.abs(hs[9]).argmax() == int(round(8000.0 / 343.0 * np.linalg.norm(np.subtract(SRC, NEAR))))


def test_integer_and_near_integer_delays(hip_lib, dev):
    """Anechoic, c = 320, |s - r| = 0.4 m: tau = 10 exactly (f = 0, j = 0), every other tap exactly zero; then one coordinate
    moved by 1e-9 m: f = 2.5e-8, the neighbours are the sinc's zero crossings missed by that much, tap 42 the window's last."""
    rows = [mk("exact", source=(0.5, 1.0, 1.0), receiver=(0.9, 1.0, 1.0), beta=0.0, c=320.0),
            mk("near", source=(0.5, 1.0, 1.0), receiver=(0.9 + 1e-9, 1.0, 1.0), beta=0.0, c=320.0),
            mk("below", source=(0.5, 1.0, 1.0), receiver=(0.9 - 1e-9, 1.0, 1.0), beta=0.0, c=320.0)]
    hs = generate(dev, rows, 64)
    check_bound(rows, 64, hs, "integer delays")
    assert abs(float(hs[0][10]) - G / 0.4) <= 17 * U24 * G / 0.4 and not np.delete(hs[0], 10).any()
    assert hs[1][42] != 0 and hs[1][43] == 0 and (hs[1][:43] != 0).all()
    assert hs[2][42] == 0 and (hs[2][:42] != 0).all()


def test_symmetric_and_absorbing_and_rigid_rooms(hip_lib, dev):
    """The source at the exact centre of a cube with equal walls (many images at one distance), two walls with beta = 0, and
    beta = 1 everywhere at K = 2 T."""
    T = tile()
    rows = [mk("cube", size=(2.0, 2.0, 2.0), source=(1.0, 1.0, 1.0), receiver=(0.6, 1.3, 0.8), beta=0.7),
            mk("centre", size=(2.0, 2.0, 2.0), source=(1.0, 1.0, 1.0), receiver=(1.0, 1.0, 1.5), beta=0.7),
            mk("absorbing", beta=(0.0, 0.9, 0.8, 0.0, 0.7, 0.6)),
            mk("rigid", beta=1.0)]
    taps = [256, 256, 256, 2 * T]
    hs = generate(dev, rows, taps)
    assert check_bound(rows, taps, hs, "cube / absorbing / rigid") > 0


def test_smallest_and_largest_rooms(hip_lib, dev):
    """A 1 x 1 x 1 m room at K = 512 (the most images per tap, the deepest axis tables); a 12 x 9 x 4 m room at K = T + 1 whose
    source is 9 m away (no image reaches the response: both tiles empty) and one with the direct path alone."""
    T = tile()
    rows = [mk("small", size=(1.0, 1.0, 1.0), source=(0.3, 0.4, 0.55), receiver=(0.7, 0.2, 0.5), beta=0.9),
            mk("large_far", size=(12.0, 9.0, 4.0), source=(2.0, 3.0, 1.5), receiver=(10.0, 7.0, 2.5), beta=0.8),
            mk("large_near", size=(12.0, 9.0, 4.0), source=(6.0, 4.0, 2.0), receiver=(6.5, 4.5, 2.0), beta=0.8)]
    taps = [512, T + 1, T + 1]
    hs = generate(dev, rows, taps)
    assert check_bound(rows, taps, hs, "1 m and 12 m rooms") > 0
    assert not hs[1].any() and hs[2].any()


def test_ragged_call_up_to_max_taps(hip_lib, dev):
    """One call over rows of different rooms with taps (1, T, 700, MAX_TAPS).  The MAX_TAPS row (an 8 x 7 x 4 m room) is compared
    on every 17th tile, the first and the last; T divides MAX_TAPS, so the last partial tile of the call is the 700-tap row's."""
    from fs_eend_amd import simulate as S
    T = tile()
    rows = [mk("one", receiver=NEAR), mk("tile", size=(2.0, 2.0, 2.0), source=(1.0, 1.0, 1.0), receiver=(0.6, 1.3, 0.8), beta=0.7),
            mk("mid"), mk("long", size=(8.0, 7.0, 4.0), source=(2.5, 3.0, 1.5), receiver=(5.0, 4.5, 1.2), beta=0.85)]
    taps = [1, T, 700, S.MAX_TAPS]
    hs = generate(dev, rows, taps)
    last = (S.MAX_TAPS - 1) // T * T
    picked = sorted(set(range(0, S.MAX_TAPS, 17 * T)) | {last})
    assert 700 % T != 0
    assert check_bound(rows, taps, hs, "ragged", ranges={3: [(k, min(k + T, S.MAX_TAPS)) for k in picked]}) > 0
    assert np.abs(hs[3]).max() > 0 and hs[3][last:].any()


def test_bits_depend_on_the_row_only(hip_lib, dev):
    """The same rows alone, in a batch among others, in reversed order and in a second run are identical, and normalize="direct"
    is the scale it is defined by."""
    T = tile()
    mine = [mk("a"), mk("b", size=(2.0, 2.0, 2.0), source=(1.0, 1.0, 1.0), receiver=(0.6, 1.3, 0.8), beta=0.7)]
    taps = [5 * T + 9, 3 * T]
    others = [mk("o1", receiver=NEAR), mk("o2", beta=0.3), mk("o3", size=(5.0, 4.0, 3.0))]
    alone = [generate(dev, [r], K)[0] for r, K in zip(mine, taps)]
    batch = generate(dev, [others[0], mine[0], others[1], mine[1], others[2]], [T, taps[0], 700, taps[1], 2 * T + 1])
    rev = generate(dev, mine[::-1], taps[::-1])
    again = generate(dev, mine, taps)
    for i in range(2):
        assert np.abs(alone[i]).max() > 0
        assert np.array_equal(bits(alone[i]), bits(batch[1 + 2 * i])) and np.array_equal(bits(alone[i]), bits(rev[1 - i]))
        assert np.array_equal(bits(alone[i]), bits(again[i]))
    direct = generate(dev, mine, taps, normalize="direct")
    explicit = generate(dev, mine, taps, normalize=[scale_of(r, "direct") for r in mine])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(direct, explicit))
    check_bound(mine, taps, direct, "normalize=direct", normalize="direct")
    k = int(round(8000.0 / 343.0 * scale_of(mine[0], "direct")))
    assert 0.5 < direct[0][k] < 1.5 and abs(alone[0][k]) < 0.1                             # the direct path has amplitude 1


def test_simulate_takes_the_generated_pool(hip_lib, dev):
    """simulate() with the pool from room_responses gives the bits of simulate() with the same responses downloaded and added
    one by one with SourcePool.add."""
    from fs_eend_amd import rooms, simulate as S
    rng = np.random.default_rng(31)
    rows, groups = rooms.draw_rooms(4, n_rooms=2, n_sources=2)
    made = rooms.room_responses(rows, (300, 450, 64, 1000), device=dev, normalize="direct")
    assert isinstance(made, S.SourcePool) and made.samples.is_cuda and made.samples.dtype == torch.float32
    copied = S.SourcePool(dev)
    host = made.samples.cpu().numpy()
    for name, (a, n) in made.table.items():
        copied.add(name, host[a:a + n].copy())
    copied.finalize()
    utts = S.SourcePool(dev, "f32")
    for i in range(4):
        utts.add(f"u{i}", (rng.standard_normal(3000 + 500 * i) * 0.1).astype(np.float32))
    utts.finalize()
    recipes = [{"name": "m", "length": 9000, "noise": None, "noise_offset": 0, "snr_db": None, "tracks": [
        {"speaker": f"s{i}", "rir": rows[i]["name"], "gain": 1.0 - 0.1 * i, "placements": [(f"u{i}", 400 * i)]} for i in range(4)]}]
    c1, _ = S.simulate(utts, made, None, recipes)
    c2, _ = S.simulate(utts, copied, None, recipes)
    torch.cuda.synchronize()
    assert c1.samples.abs().max() > 0 and torch.equal(c1.samples, c2.samples)


def test_rooms_to_batches(hip_lib, dev):
    """draw_rooms -> room_responses -> draw_recipes(rir_groups=) -> simulate -> corpus.batch runs: finite features, as many
    label columns as the mixture has speakers, every mixture in one room."""
    from fs_eend_amd import rooms, simulate as S
    rng = np.random.default_rng(32)
    rows, groups = rooms.draw_rooms(9, n_rooms=3, n_sources=3)
    rirs = rooms.room_responses(rows, 800, device=dev, normalize="direct")
    utts, spk2utt = S.SourcePool(dev, "s16"), {}
    for s in range(4):
        for i in range(2):
            utts.add(f"s{s}_u{i}", rng.integers(-8000, 8000, int(rng.integers(2000, 5000))).astype(np.int16))
            spk2utt.setdefault(f"s{s}", []).append(f"s{s}_u{i}")
    utts.finalize()
    recipes = S.draw_recipes(6, spk2utt, utts, rirs=rirs, n_mixtures=4, n_speakers=(2, 3), n_utts=(1, 2), beta=0.2, rir_groups=groups)
    corpus, stats = S.simulate(utts, rirs, None, recipes)
    batch_rows = [(r["name"], 0, min(r["length"] // 80, 100)) for r in recipes]
    feats, labels, recs = corpus.batch(batch_rows, context_size=7, subsampling=10, input_transform="logmel23_mn")
    torch.cuda.synchronize()
    assert recs == [r["name"] for r in recipes]
    for r, f, l in zip(recipes, feats, labels):
        assert len({t["rir"].rsplit("_", 1)[0] for t in r["tracks"]}) == 1
        assert torch.isfinite(f).all() and f.abs().max() > 0 and l.shape[1] == len(r["tracks"]) and l.shape[0] == f.shape[0]
    assert torch.isfinite(stats["y"]).all() and stats["y"].abs().max() > 0
