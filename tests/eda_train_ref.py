"""Float64 restatement of the differentiable attractor path of the offline EEND-EDA baseline (reference
FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py, `EncoderDecoderAttractor.forward` :109-127 and the bmm head of :47), written from the
definitions for the tests of eend_lstm_train_f32, eend_lstm_bwd_f32, eend_wgrad_f32, eend_eda_count_loss_f32, eend_eda_head_bwd_f32
and of fs_eend_amd.eda_model's autograd functions.  Everything is numpy float64.

  forward   z = G[order[t]] + W_hh h;  i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_g);  c = f c + i g;  h = o tanh(c)
  backward  (t = T-1 .. 0)  dh = dh_all[t] + W_hh^T dz(t+1);  dc += dh o (1 - tanh^2 c_t);  dz_o = dh tanh(c_t) o (1 - o);
            dz_i = dc g i (1 - i);  dz_g = dc i (1 - g^2);  dz_f = dc c_{t-1} f (1 - f);  dc <- dc f
            dG[order[t]] = dz(t);  dW_hh = sum_t dz(t) h_{t-1}^T;  dW_ih = dG^T xs;  db_ih = db_hh = sum rows of dG;  dxs = dG W_ih
  counter   z[b][c] = attractors[b][c] . w + bias for c <= n_b, labels [1] * n_b + [0], loss = mean BCE-with-logits over all of them
  head      logits = emb attractors^T;  d attractors = dlogits^T emb;  d emb = dlogits attractors
"""
import numpy as np

EDA_PARAMS = ("encoder.weight_ih_l0", "encoder.weight_hh_l0", "encoder.bias_ih_l0", "encoder.bias_hh_l0", "decoder.weight_ih_l0",
              "decoder.weight_hh_l0", "decoder.bias_ih_l0", "decoder.bias_hh_l0", "counter.weight", "counter.bias")


def mirror_of(meta, make, counter):
    """make() under the golden's seed (default initialisation), oracle.fixtures.perturb_, the counter gain on counter(module).weight;
    verified against the stored checksums.  The common part of this module's build_mirror and tests/eda_ref.py's."""
    import torch
    from oracle import fixtures as FX
    torch.manual_seed(meta["seed"])
    m = make()
    FX.perturb_(m, meta["pseed"])
    with torch.no_grad():
        counter(m).weight.mul_(meta["counter_gain"])
    FX.check_params(m.state_dict(), meta["checksums"])
    return m


def build_mirror(meta):
    """A training golden's parameters in the product's own EncoderDecoderAttractor, as tools/gen_golden_eda_train.py built them in the
    reference's (mirror_of)."""
    from fs_eend_amd.eda_model import EncoderDecoderAttractor
    return mirror_of(meta, lambda: EncoderDecoderAttractor(256), lambda m: m.counter)


def golden_inputs(meta):
    """xs (B, T, 256), Ra (B, C, 256) of the differentiated scalar loss + sum(attractors Ra), and the frame order or None."""
    import torch
    g = torch.Generator().manual_seed(meta["xseed"])
    xs = torch.randn(meta["B"], meta["T"], 256, generator=g)
    g = torch.Generator().manual_seed(meta["rseed"])
    Ra = meta["ra_scale"] * torch.randn(meta["B"], max(meta["n_speakers"]) + 1, 256, generator=g)
    order = None if meta["oseed"] is None else np.random.RandomState(meta["oseed"]).permutation(meta["T"])
    return xs, Ra, order


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def lstm_forward(W_hh, G=None, order=None, h0=None, c0=None, bias=None, T=None):
    """The one float64 recurrence of the tests (tests/eda_ref.lstm is a view of it).  G (B, rows, 4H) input pre-activations read at
    row order[t] (None: the bias (4H,) alone, for T steps) -> dict(hT, cT, h_all, c_all (B, T, H), gates (B, T, 4H) after their
    functions, h_prev (B, T, H) in step order, c0)."""
    W = _f64(W_hh)
    H = W.shape[1]
    if G is not None:
        G = _f64(G)
        B = G.shape[0]
        T = G.shape[1] if T is None else T
    else:
        B = 1 if h0 is None else _f64(h0).shape[0]
        bias = _f64(bias)
    h = np.zeros((B, H)) if h0 is None else _f64(h0).copy()
    c = np.zeros((B, H)) if c0 is None else _f64(c0).copy()
    out = dict(c0=c.copy(), h_all=np.zeros((B, T, H)), c_all=np.zeros((B, T, H)), gates=np.zeros((B, T, 4 * H)),
               h_prev=np.zeros((B, T, H)))
    for t in range(T):
        z = h @ W.T + (G[:, t if order is None else int(order[t])] if G is not None else bias[None])
        i, f, g, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
        out["h_prev"][:, t] = h
        c = f * c + i * g
        h = o * np.tanh(c)
        out["gates"][:, t] = np.concatenate([i, f, g, o], axis=1)
        out["h_all"][:, t], out["c_all"][:, t] = h, c
    out["hT"], out["cT"] = h, c
    return out


def lstm_backward(W_hh, fwd, order=None, dh_all=None, dhT=None, dcT=None, rows=None):
    """fwd: what lstm_forward returned.  -> dG (B, rows, 4H) with step t's gradients at row order[t] (zeros elsewhere), dh0, dc0."""
    W = _f64(W_hh)
    H = W.shape[1]
    B, T, _ = fwd["h_all"].shape
    rows = T if rows is None else rows
    dG = np.zeros((B, rows, 4 * H))
    dh = np.zeros((B, H)) if dhT is None else _f64(dhT).copy()
    dc = np.zeros((B, H)) if dcT is None else _f64(dcT).copy()
    for t in range(T - 1, -1, -1):
        if dh_all is not None:
            dh = dh + _f64(dh_all)[:, t]
        gt = fwd["gates"][:, t]
        i, f, g, o = gt[:, :H], gt[:, H:2 * H], gt[:, 2 * H:3 * H], gt[:, 3 * H:]
        c_t = fwd["c_all"][:, t]
        c_prev = fwd["c_all"][:, t - 1] if t > 0 else fwd["c0"]
        tc = np.tanh(c_t)
        dc = dc + dh * o * (1.0 - tc * tc)
        dz = np.concatenate([dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], axis=1)
        dc = dc * f
        dG[:, t if order is None else int(order[t])] = dz
        dh = dz @ W
    return dG, dh, dc


def h_prev_rows(fwd, order=None, rows=None):
    """h_prev in the row layout of G: the hidden state that entered step t at row order[t]."""
    B, T, H = fwd["h_prev"].shape
    out = np.zeros((B, T if rows is None else rows, H))
    for t in range(T):
        out[:, t if order is None else int(order[t])] = fwd["h_prev"][:, t]
    return out


def count_loss(attractors, w, bias, n_speakers):
    """-> loss, d attractors (B, C, H), dw (H,), dbias for a unit loss gradient."""
    A, w, bias = _f64(attractors), _f64(w).reshape(-1), float(_f64(bias).reshape(-1)[0])
    n_tot = sum(int(n) + 1 for n in n_speakers)
    loss, dA, dw, db = 0.0, np.zeros_like(A), np.zeros_like(w), 0.0
    for b, n in enumerate(n_speakers):
        for c in range(int(n) + 1):
            z = float(A[b, c] @ w + bias)
            y = 1.0 if c < n else 0.0
            loss += max(z, 0.0) - z * y + np.log1p(np.exp(-abs(z)))
            g = (_sigmoid(z) - y) / n_tot
            dA[b, c] = g * w
            dw += g * A[b, c]
            db += g
    return loss / n_tot, dA, dw, db


def head_backward(dlogits, emb, attractors):
    """logits = emb attractors^T -> d attractors (B, C, H), d emb (B, T, H)."""
    d, e, a = _f64(dlogits), _f64(emb), _f64(attractors)
    return np.einsum("btc,bth->bch", d, e), np.einsum("btc,bch->bth", d, a)


def attractor_path(p, xs, n_speakers, order=None, dloss=1.0, dattractors=None):
    """EncoderDecoderAttractor.forward and its backward.  p: the module's parameters by name (EDA_PARAMS; anything _f64 takes),
    xs (B, T, H) in storage order, read at order[t] in step t.  -> dict(loss, attractors, dxs, grads {name: array})."""
    p = {k: _f64(v) for k, v in p.items()}
    xs = _f64(xs)
    G = xs @ p["encoder.weight_ih_l0"].T + p["encoder.bias_ih_l0"] + p["encoder.bias_hh_l0"]
    enc = lstm_forward(p["encoder.weight_hh_l0"], G, order)
    C = max(int(n) for n in n_speakers) + 1
    dec = lstm_forward(p["decoder.weight_hh_l0"], None, None, enc["hT"], enc["cT"], p["decoder.bias_ih_l0"] + p["decoder.bias_hh_l0"], C)
    attractors = dec["h_all"]
    loss, dA, dw, db = count_loss(attractors, p["counter.weight"], p["counter.bias"], n_speakers)
    dA = dloss * dA + (0.0 if dattractors is None else _f64(dattractors))
    dGd, dh0, dc0 = lstm_backward(p["decoder.weight_hh_l0"], dec, None, dh_all=dA)
    dGe, _, _ = lstm_backward(p["encoder.weight_hh_l0"], enc, order, dhT=dh0, dcT=dc0)
    grads = {
        "encoder.weight_ih_l0": np.einsum("btn,btk->nk", dGe, xs),
        "encoder.weight_hh_l0": np.einsum("btn,btk->nk", dGe, h_prev_rows(enc, order)),
        "encoder.bias_ih_l0": dGe.sum((0, 1)), "encoder.bias_hh_l0": dGe.sum((0, 1)),
        "decoder.weight_ih_l0": np.zeros_like(p["decoder.weight_ih_l0"]),
        "decoder.weight_hh_l0": np.einsum("btn,btk->nk", dGd, dec["h_prev"]),
        "decoder.bias_ih_l0": dGd.sum((0, 1)), "decoder.bias_hh_l0": dGd.sum((0, 1)),
        "counter.weight": (dloss * dw).reshape(1, -1), "counter.bias": np.asarray([dloss * db]),
    }
    return dict(loss=loss, attractors=attractors, dxs=dGe @ p["encoder.weight_ih_l0"], grads=grads, dGe=dGe, dGd=dGd)
