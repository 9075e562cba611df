"""CPU: the float64 restatement of the room impulse response contract (tests/room_ref.py) pinned by properties of the image
method itself, so that the GPU tests compare against something that has been checked: a single image in an anechoic room,
reciprocity, a brute-force lattice walk with the window evaluated as written, 0^0 = 1, image counts under the rule "window
meets [0, K)", and Eyring's formula."""
import math

import numpy as np

import room_ref as R

G = 1.0 / (4.0 * np.pi)
ROOM, SRC, RCV = (3.0, 4.0, 2.5), (1.84, 1.47, 1.36), (0.35, 2.21, 1.93)
BETA = (0.9, 0.8, 0.7, 0.85, 0.6, 0.75)


def test_anechoic_room_is_one_windowed_sinc():
    # c = 320: q = 25 samples per metre; |s - r| = 0.4 m puts the one image at tau = 10 exactly (0.9 - 0.5 is the double 0.4)
    h, n, S = R.response(ROOM, (0.5, 1.0, 1.0), (0.9, 1.0, 1.0), 0.0, 320.0, G, 64)
    assert abs(h[10] - 1.0 / (4.0 * np.pi * 0.4)) <= 1e-16
    assert np.abs(np.delete(h, 10)).max() < 1e-15 and n.sum() == 1 and n[10] == 1
    # off the grid: h[k] = g / d w(k - tau) with the window as it is written
    s, r = np.array([0.5, 1.0, 1.0]), np.array([0.83, 1.2, 0.9])
    d = float(np.linalg.norm(s - r))
    h, n, S = R.response(ROOM, s, r, 0.0, 343.0, G, 64)
    want = G / d * R.window(np.arange(64) - 8000.0 / 343.0 * d)
    assert np.abs(h - want).max() < 1e-15 and np.array_equal(n, (want != 0).astype(np.int64)) and np.allclose(S, np.abs(want), atol=1e-15)
    # a direct path closer than the window's half width is clipped at k < 0, and taps past K are dropped
    assert (n[:40] == 1).all() and n[50:].sum() == 0
    assert np.array_equal(R.response(ROOM, s, r, 0.0, 343.0, G, 20)[0], h[:20])


def test_reciprocity():
    a = R.response(ROOM, SRC, RCV, BETA, 343.0, G, 512)[0]
    b = R.response(ROOM, RCV, SRC, BETA, 343.0, G, 512)[0]
    assert np.abs(a).max() > 0.03 and np.abs(a - b).max() < 1e-14


def test_brute_force_lattice_walk_agrees():
    K = 200
    a, n, S = R.response(ROOM, SRC, RCV, BETA, 343.0, G, K)
    b = R.brute_force(ROOM, SRC, RCV, BETA, 343.0, G, K)
    assert n.max() > 50 and np.abs(a - b).max() < 1e-15
    # a range of taps is the same taps
    h2, n2, S2 = R.response(ROOM, SRC, RCV, BETA, 343.0, G, K, 64, 130)
    assert np.array_equal(h2, a[64:130]) and np.array_equal(n2, n[64:130]) and np.array_equal(S2, S[64:130])


def test_zero_to_the_zero_is_one():
    assert R.power(0.0, np.array([0, 1, 2])).tolist() == [1.0, 0.0, 0.0]
    # the walls at x = 0 and y = Ly absorb everything: the direct path (all exponents 0) and the images that never touch them stay
    beta = (0.0, 0.9, 0.8, 0.0, 0.7, 0.6)
    a, n, _ = R.response(ROOM, SRC, RCV, beta, 343.0, G, 256)
    b = R.brute_force(ROOM, SRC, RCV, beta, 343.0, G, 256)
    d = float(np.linalg.norm(np.subtract(SRC, RCV)))
    k = int(round(8000.0 / 343.0 * d))
    assert np.abs(a - b).max() < 1e-15 and abs(a[k]) > 0.5 * G / d and 0 < n.max() < R.response(ROOM, SRC, RCV, BETA, 343.0, G, 256)[1].max()


def test_image_counts_by_time():
    assert R.image_count(ROOM, SRC, RCV, 343.0, 256) == 259
    assert R.image_count(ROOM, SRC, RCV, 343.0, 1024) == 12911


def test_eyring_beta_is_its_formula():
    from fs_eend_amd import rooms
    L, rt60, c = (6.0, 5.0, 3.0), 0.3, 343.0
    V, S = 90.0, 2.0 * (30.0 + 15.0 + 18.0)
    alpha = 1.0 - math.exp(-24.0 * math.log(10.0) * V / (c * S * rt60))
    assert rooms.eyring_beta(L, rt60, c) == math.sqrt(1.0 - alpha)
    assert 0.0 < rooms.eyring_beta(L, 0.2) < rooms.eyring_beta(L, 0.8) < 1.0
    assert "no decay" in rooms.eyring_beta.__doc__
