"""Float64 numpy statements of the LS-EEND retention recurrence (decay 1) over a backlog, shared by the CPU and GPU tests of the
retention prefill: the per-frame recurrence as the frame step runs it, and the three-pass chunk form the prefill kernel
implements (chunk sums, their exclusive prefix in chunk order, the chunk outputs)."""
import numpy as np

H, D, CH = 4, 256, 64


def _split(qkvg):
    """qkvg (N, T, 4D) -> q, k, v, g (N, T, H, 64) float64"""
    x = np.asarray(qkvg, dtype=np.float64)
    return [x[..., i * D:(i + 1) * D].reshape(x.shape[0], x.shape[1], H, 64) for i in range(4)]


def _norm_gate(o, g, eps):
    """per-head LayerNorm (no affine) of o (..., 64), then the swish gate"""
    y = (o - o.mean(-1, keepdims=True)) / np.sqrt(o.var(-1, keepdims=True) + eps)
    return g / (1.0 + np.exp(-g)) * y


def ret_per_frame64(qkvg, kv, t0, eps=1e-6):
    """N sequences, T frames each from position t0, frame by frame:
        kv_t = kv_{t-1} sqrt(t / (t+1)) + v_t k_t^T / sqrt(t+1),  o_t[a] = sum_b q_t[b] kv_t[a][b],  r_t = LN_64(o_t) swish(g_t)
    qkvg (N, T, 4D), kv (N, H, 64, 64) (not read when t0 == 0) -> outputs (N, T, D), final state (N, H, 64, 64)."""
    q, k, v, g = _split(qkvg)
    N, T = q.shape[:2]
    st = np.zeros((N, H, 64, 64)) if t0 == 0 else np.asarray(kv, dtype=np.float64).copy()
    out = np.empty((N, T, H, 64))
    for j in range(T):
        t = t0 + j
        st = st * np.sqrt(t / (t + 1.0)) + v[:, j, :, :, None] * k[:, j, :, None, :] / np.sqrt(t + 1.0)
        out[:, j] = _norm_gate((st * q[:, j, :, None, :]).sum(-1), g[:, j], eps)
    return out.reshape(N, T, D), st


def ret_chunks64(qkvg, kv, t0, eps=1e-6):
    """The same in chunks of 64 frames, from kv_t = (sqrt(t0) kv_{t0-1} + sum_{i = t0..t} v_i k_i^T) / sqrt(t+1):
        sums    P_c = sum_{i in c} v_i k_i^T
        scan    S_c = sqrt(t0) kv_in + sum_{c' < c} P_c' in chunk order;  kv_out = (S_last + P_last) / sqrt(t0 + T)
        outputs o_i = ((Q K^T . [j <= i]) V + Q S_c^T)_i / sqrt(t0 + 64 c + i + 1), then LayerNorm and gate
    A tail chunk is padded with zero rows, as the kernel loads it."""
    q, k, v, g = _split(qkvg)
    N, T = q.shape[:2]
    nc = (T + CH - 1) // CH
    pad = lambda x: np.concatenate([x, np.zeros((N, nc * CH - T, H, 64))], axis=1).reshape(N, nc, CH, H, 64)
    Q, K, V = pad(q), pad(k), pad(v)
    P = np.einsum("ncjha,ncjhb->nchab", V, K)                                  # pass 1
    S = np.empty_like(P)                                                       # pass 2
    run = np.zeros((N, H, 64, 64)) if t0 == 0 else np.sqrt(float(t0)) * np.asarray(kv, dtype=np.float64)
    for c in range(nc):
        S[:, c] = run
        run = run + P[:, c]
    kv_out = run / np.sqrt(float(t0 + T))
    mask = np.tril(np.ones((CH, CH)))                                          # pass 3: [j <= i], the diagonal included
    A = np.einsum("ncihb,ncjhb->nchij", Q, K) * mask
    o = np.einsum("nchij,ncjha->nciha", A, V) + np.einsum("ncihb,nchab->nciha", Q, S)
    pos = t0 + np.arange(nc * CH).reshape(nc, CH) + 1.0
    o = (o / np.sqrt(pos)[None, :, :, None, None]).reshape(N, nc * CH, H, 64)[:, :T]
    return _norm_gate(o, g, eps).reshape(N, T, D), kv_out
