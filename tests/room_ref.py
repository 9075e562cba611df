"""Float64 numpy restatement of the arithmetic contract of room impulse responses (include/eend_hip.h at eend_room_rir_f32, DESIGN
10e): the image method in a shoebox room with a 64-tap Hann-windowed sinc placed at every image's delay.  Checker only.

`response` is the yardstick: it enumerates the images from per-axis tables (coordinate offset and coefficient product per
(n, u)), forms p, d, tau = kc + f operation by operation as the contract writes them, and evaluates every term in the split form
(sin(pi x) = -(-1)^j sin(pi f), Hann = sin^2(pi y / W) with y = W / 2 - |j - f| taken as (W / 2 - |j|) +- f).  It returns the sum
h, the number n_k of non-zero terms per tap and the sum S_k of their magnitudes, which the value contract's bound is made of.
`brute_force` walks the lattice image by image and evaluates w(k - tau) as it is written, for the tests of this file."""
import numpy as np

W = 64
RATE = 8000.0


def window(x):
    """w(x) = sinc(x) (1 + cos(2 pi x / W)) / 2 for |x| < W / 2, else 0, as written."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) < W / 2, np.sinc(x) * 0.5 * (1.0 + np.cos(2.0 * np.pi * x / W)), 0.0)


def power(b, e):
    """b^e elementwise with 0^0 = 1 (e a non-negative integer array)."""
    return np.where(e == 0, 1.0, np.power(float(b), e.astype(np.float64)))


def axis_table(s, L, r, b0, b1, N):
    """Entries (n, u), |n| <= N, u in {0, 1}: offset ((1 - 2u) s + 2n L) - r and coefficient b0^|n - u| b1^|n|."""
    n = np.repeat(np.arange(-N, N + 1), 2)
    u = np.tile(np.array([0, 1]), 2 * N + 1)
    off = (np.where(u == 1, -float(s), float(s)) + (2 * n).astype(np.float64) * float(L)) - float(r)
    return off, power(b0, np.abs(n - u)) * power(b1, np.abs(n))


def images(L, s, r, beta, q, g, K):
    """Every image whose window meets [0, K) and whose amplitude is not zero: -> (kc int64, f, A) with tau = kc + f."""
    dmax = (K - 1 + W // 2) / q
    tabs = []
    for a in range(3):
        N = int(np.floor(dmax / (2.0 * L[a]))) + 1
        tabs.append(axis_table(s[a], L[a], r[a], beta[2 * a], beta[2 * a + 1], N))
    (px, cx), (py, cy), (pz, cz) = tabs
    kcs, fs, As = [], [], []
    r2 = (py * py)[:, None] + (pz * pz)[None, :]                    # px px + (py py + pz pz)
    cyz = cy[:, None] * cz[None, :]
    for i in range(len(px)):
        d = np.sqrt(px[i] * px[i] + r2)
        tau = q * d
        kc = np.rint(tau)
        f = tau - kc
        A = ((g * cx[i]) * cyz) / d
        keep = (A != 0) & (kc + np.where(f < 0, -32, -31) <= K - 1)
        kcs.append(kc[keep].astype(np.int64))
        fs.append(f[keep])
        As.append(A[keep])
    return np.concatenate(kcs), np.concatenate(fs), np.concatenate(As)


def terms(kc, f, A, k_lo, k_hi):
    """The terms of the given images at taps k_lo <= k < k_hi: -> (k, value) flat arrays of the live (image, tap) pairs."""
    sel = (kc + 32 >= k_lo) & (kc - 32 < k_hi)
    kc, f, A = kc[sel], f[sel], A[sel]
    j = np.arange(-32, 33)[None, :]
    k = kc[:, None] + j
    ff, AA = f[:, None], A[:, None]
    y = (32 - np.abs(j)) + np.where(j > 0, ff, np.where(j < 0, -ff, -np.abs(ff)))
    live = (y > 0) & (k >= k_lo) & (k < k_hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        sn = np.where(j == 0, np.sinc(ff), -np.where(j % 2 == 0, 1.0, -1.0) * np.sin(np.pi * ff) / (np.pi * (j - ff)))
    val = AA * sn * np.sin(np.pi * y / W) ** 2
    return k[live], val[live]


def row_images(L, s, r, beta, c, g, K):
    """`images` of a row given as the host gives it (beta one value or six, c in m/s)."""
    beta = np.repeat(np.asarray(beta, dtype=np.float64).reshape(-1), 6) if np.size(beta) == 1 else np.asarray(beta, dtype=np.float64)
    return images(np.asarray(L, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(r, dtype=np.float64), beta,
                  RATE / float(c), float(g), K)


def response(L, s, r, beta, c, g, K, k_lo=0, k_hi=None, chunk=200000, imgs=None):
    """-> (h, n_k, S_k) over the taps k_lo <= k < k_hi (all K by default), float64 / int64 / float64.  imgs: row_images of the
    same row, to share them among several tap ranges."""
    k_hi = K if k_hi is None else k_hi
    kc, f, A = row_images(L, s, r, beta, c, g, K) if imgs is None else imgs
    n = k_hi - k_lo
    h, S, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    for a in range(0, len(kc), chunk):
        k, v = terms(kc[a:a + chunk], f[a:a + chunk], A[a:a + chunk], k_lo, k_hi)
        h += np.bincount(k - k_lo, weights=v, minlength=n)
        S += np.bincount(k - k_lo, weights=np.abs(v), minlength=n)
        cnt += np.bincount((k - k_lo)[v != 0], minlength=n)
    return h, cnt, S


def image_count(L, s, r, c, K):
    """Images (of any amplitude) whose window meets [0, K)."""
    return len(images(np.asarray(L, float), np.asarray(s, float), np.asarray(r, float), np.ones(6), RATE / float(c), 1.0, K)[0])


def brute_force(L, s, r, beta, c, g, K):
    """The lattice walk: every (n, l, m, u, v, w) within reach, w(k - tau) evaluated as written.  -> h float64 [K]."""
    q = RATE / float(c)
    dmax = (K - 1 + W // 2) / q
    h = np.zeros(K)
    k = np.arange(K, dtype=np.float64)
    N = [int(np.floor(dmax / (2.0 * L[a]))) + 1 for a in range(3)]
    pw = lambda b, e: 1.0 if e == 0 else float(b) ** e
    for n in range(-N[0], N[0] + 1):
        for l in range(-N[1], N[1] + 1):
            for m in range(-N[2], N[2] + 1):
                for u in (0, 1):
                    for v in (0, 1):
                        for w in (0, 1):
                            p = ((1 - 2 * u) * s[0] + 2 * n * L[0] - r[0], (1 - 2 * v) * s[1] + 2 * l * L[1] - r[1],
                                 (1 - 2 * w) * s[2] + 2 * m * L[2] - r[2])
                            d = float(np.sqrt(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2])))
                            if d >= dmax + 1.0 / q:
                                continue
                            A = (g * pw(beta[0], abs(n - u)) * pw(beta[1], abs(n)) * pw(beta[2], abs(l - v)) * pw(beta[3], abs(l))
                                 * pw(beta[4], abs(m - w)) * pw(beta[5], abs(m)) / d)
                            h += A * window(k - q * d)
    return h
