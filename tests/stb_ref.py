"""Float64 restatement of block-online EEND-EDA with a speaker-tracing buffer (reference FS-EEND/train/tfm_STB.py:147-204 with
find_best_perm, cal_cor, upd_buf, upd_buf_FIFO of train/utils/utils.py), written from the definitions, for the tests of
fs_eend_amd.stb and of csrc/stb.hip.  numpy only; the assignment is scipy's.

  centre      xc = [x_buf; x_i] - column mean
  block 0     y = sigmoid(logits[:, :c]); emit y; the buffer takes the CENTRED rows and y; S = c
  block k     p = sigmoid(logits[:, :c]); S' = max(S, c); everything zero-padded to S' columns;
              corr[r][q] = cov / (sqrt(var_r) sqrt(var_q) + 1e-6) over the L buffer rows; perm maximises the total correlation;
              y_i[:, r] = p[L:, perm[r]]; T <= buf_size appends the RAW rows, otherwise buf_size rows are kept in time order
  fifo        the last buf_size rows
  kld         p_t = y_t / sum_c y_t (0 where the sum is 0), zeros -> 1e-6; w_t = sum_c p log(p S'), negative -> 0, then 0 -> 1e-6
              (w = 1 at S' = 0); keep the buf_size largest key_t = w_t / -ln u_t, u_t = (h + 0.5) 2^-32,
              h = mix(mix(mix(seed ^ 0x9E3779B9) + k) + t), on equal keys the lower t
  tie rule    tracked rows r < S are solved against all S' columns; only pairs with a predicted column q < c are kept, every other
              row takes the columns left over in ascending order (padding has correlation 0 with everything)

The buffers and the posteriors are f32 storage, as on the device: posteriors are the float64 sigmoid rounded to f32, block 0's
centred rows are rounded to f32; correlations, weights and keys are float64 from those f32 values.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

MAX_SPK = 15
M32 = 0xFFFFFFFF


def mix(x):
    """murmur3's 32-bit finaliser."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draw_hash(seed, k, t):
    return mix(mix(mix((seed & M32) ^ 0x9E3779B9) + k) + t)


def stream_seed(seed, key):
    """The 32-bit seed of a stream from the session's seed and the stream's key."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    return mix(mix(int(seed) & M32) + ((key & M32) ^ (key >> 32)))


def sigmoid32(x):
    return (1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))).astype(np.float32)


def center(x_buf, x_i):
    """-> float64 (L + n, F)"""
    x = np.asarray(x_i, dtype=np.float64)
    if x_buf is not None and len(x_buf):
        x = np.concatenate([np.asarray(x_buf, dtype=np.float64), x], axis=0)
    return x - x.mean(axis=0, keepdims=True)


def correlations(z_buf, z_pred):
    """cal_cor for every pair of columns: (S', S') float64."""
    a = np.asarray(z_buf, dtype=np.float64)
    b = np.asarray(z_pred, dtype=np.float64)
    a = a - a.mean(axis=0, keepdims=True)
    b = b - b.mean(axis=0, keepdims=True)
    cov = a.T @ b
    sa = np.sqrt((a * a).sum(axis=0))
    sb = np.sqrt((b * b).sum(axis=0))
    return cov / (sa[:, None] * sb[None, :] + 1e-6)


def _solve(m):
    r, q = linear_sum_assignment(m, True)
    return dict(zip(r.tolist(), q.tolist())), float(m[r, q].sum())


def assign(corr, S, c):
    """-> perm (S',), margin: the best total correlation minus the runner-up's (inf where there is no other assignment of the
    tracked rows).  Assignments that differ only in which padding column a row takes are one assignment."""
    Sn = corr.shape[0]
    perm = np.full(Sn, -1, dtype=np.int64)
    margin = float("inf")
    if S > 0 and Sn > 0:
        m = corr[:S].copy()
        best, total = _solve(m)
        for r, q in best.items():
            if q < c:
                perm[r] = q
            alt = m.copy()
            if q < c:
                alt[r, q] = -1e9
            else:
                alt[r, c:] = -1e9
            _, t2 = _solve(alt)
            if t2 > -1e8:
                margin = min(margin, total - t2)
    left = [q for q in range(Sn) if q not in set(perm[perm >= 0].tolist())]
    for r in range(Sn):
        if perm[r] < 0:
            perm[r] = left.pop(0)
    return perm, margin


def weights(y, Sn):
    """upd_buf's sampling weights of the rows y (T, S') in float64."""
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[0]
    if Sn == 0:
        return np.ones(T)
    s = y.sum(axis=1, keepdims=True)
    p = np.divide(y, s, out=np.zeros_like(y), where=s != 0)
    p[p == 0] = 1e-6
    w = (p * np.log(p * Sn)).sum(axis=1)
    w[w < 0] = 0.0
    w[w == 0] = 1e-6
    return w


def race_keys(w, seed, k):
    h = np.array([draw_hash(seed, k, t) for t in range(len(w))], dtype=np.float64)
    u = (h + 0.5) * 2.0 ** -32
    return np.asarray(w, dtype=np.float64) / -np.log(u)


def race_select(keys, m):
    """-> the indices of the m largest keys in ascending order (equal keys: the lower index wins), and the relative gap between
    the m-th and the next key."""
    order = sorted(range(len(keys)), key=lambda t: (-keys[t], t))
    gap = float("inf")
    if m < len(keys):
        a, b = keys[order[m - 1]], keys[order[m]]
        gap = (a - b) / abs(a) if a != 0 else 0.0
    return np.array(sorted(order[:m]), dtype=np.int64), gap


def select_rows(y, Sn, buf_size, policy, seed, k):
    """Which of the rows y (T, S') stay when T > buf_size -> (ascending indices, key gap)."""
    T = y.shape[0]
    if T <= buf_size:
        return np.arange(T), float("inf")
    if policy == "fifo":
        return np.arange(T - buf_size, T), float("inf")
    if policy == "kld":
        return race_select(race_keys(weights(y, Sn), seed, k), buf_size)
    raise ValueError(policy)


def keep_rows(x_buf, x_i, z_buf, y_i, sel):
    """Rows `sel` of [x_buf; x_i] and [z_buf; y_i]."""
    return np.concatenate([x_buf, x_i], axis=0)[sel], np.concatenate([z_buf, y_i], axis=0)[sel]


class State:
    """A stream: x_buf (L, F) f32, y_buf (L, 15) f32 zero beyond S, S, k."""

    def __init__(self, F):
        self.x_buf = np.zeros((0, F), dtype=np.float32)
        self.y_buf = np.zeros((0, MAX_SPK), dtype=np.float32)
        self.S = 0
        self.k = 0


def track(st, x_i, xc, logits, count, buf_size, policy, seed):
    """One block: updates `st`, -> dict(y (n, 15) f32 zero beyond width, width, perm (15,), sel, margin, gap)."""
    x_i = np.asarray(x_i, dtype=np.float32)
    n, L = x_i.shape[0], st.x_buf.shape[0]
    T = L + n
    c = min(max(int(count), 0), MAX_SPK)
    p = np.zeros((T, MAX_SPK), dtype=np.float32)
    p[:, :c] = sigmoid32(np.asarray(logits)[:T, :c])
    perm = np.arange(MAX_SPK)
    margin = gap = float("inf")
    if L == 0:
        Sn, y = c, p
        x_new = np.asarray(xc, dtype=np.float64).astype(np.float32)
    else:
        Sn = max(st.S, c)
        if Sn > 0:
            pm, margin = assign(correlations(st.y_buf[:, :Sn], p[:L, :Sn]), st.S, c)
            perm[:Sn] = pm
        y = np.zeros((n, MAX_SPK), dtype=np.float32)
        y[:, :Sn] = p[L:, perm[:Sn]]
        x_new = x_i
    sel, gap = select_rows(np.concatenate([st.y_buf, y], axis=0)[:, :Sn], Sn, buf_size, policy, seed, st.k)
    x_keep, y_keep = keep_rows(st.x_buf if L else x_new[:0], x_new, st.y_buf, y, sel)
    st.x_buf, st.y_buf, st.S, st.k = x_keep, y_keep, Sn, st.k + 1
    return dict(y=y, width=Sn, perm=perm, sel=sel, margin=margin, gap=gap, count=c)


def loop(model_test, x, blk_size, buf_size, policy, seed, orders):
    """The block loop of test_step over one recording x (frames, F).  model_test(xc float64 (T, F), order) -> logits (T, 15), count;
    orders(k, T) -> the frame order of block k.  -> (blocks [track's dict + xc, logits, order], result (frames, max width))."""
    x = np.asarray(x, dtype=np.float32)
    st = State(x.shape[1])
    blocks = []
    for s in range(0, x.shape[0], blk_size):
        x_i = x[s:s + blk_size]
        xc = center(st.x_buf, x_i)
        order = orders(st.k, xc.shape[0])
        logits, count = model_test(xc, order)
        out = track(st, x_i, xc, logits, count, buf_size, policy, seed)
        out.update(xc=xc, logits=np.asarray(logits), order=np.asarray(order))
        blocks.append(out)
    width = max(b["width"] for b in blocks)
    return blocks, np.concatenate([b["y"][:, :width] for b in blocks], axis=0), st
