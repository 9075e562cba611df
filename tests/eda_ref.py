"""Float64 restatement of the offline EEND-EDA baseline's inference (reference FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py:
`test` :54-76 and `estimate` :94-107), written from the definitions of the operators, for the tests of fs_eend_amd.eda_model and
of eend_lstm_f32.  Everything is computed in float64 from a state dict with the reference's keys.

  encoder     x = pad_sequence(src, -1);  x = LayerNorm(x W^T + b);  n_layers post-norm layers
              x = LN1(x + MHA(x)),  x = LN2(x + W2 relu(W1 x + b1) + b2), attention unmasked over all T rows of the padded batch
  LSTM        z = x_t W_ih^T + b_ih + W_hh h + b_hh, gates (i, f, g, o);  c = s(f) c + s(i) tanh(g);  h = s(o) tanh(c)
  attractors  encoder LSTM over emb[:, order], its final (h, c) start the decoder LSTM, which reads 15 zero vectors
  counter     p = sigmoid(attractor . w + b);   logits = emb attractors^T
  count rule  n_spk given: the first n_spk columns; th given: per sequence the columns before its own first p < th, all 15 if none
              (the reference's two quirks -- the first item's count reused for the batch, an exception when no p < th -- are not
              restated: fs_eend_amd.eda_model does not reproduce them).
"""
import numpy as np
import torch

from tests.eda_train_ref import _sigmoid, lstm_forward, mirror_of

MAX_N_SPEAKERS = 15


def build_mirror(meta):
    """The golden case's parameters in the product's own class, as tools/gen_golden_eda.py built them in the reference's
    (eda_train_ref.mirror_of)."""
    from fs_eend_amd.eda_model import TransformerEDADiarization
    return mirror_of(meta, lambda: TransformerEDADiarization(n_speakers=None, in_size=meta["in_size"], **meta["cfg"]).eval(),
                     lambda m: m.eda.counter)


def lstm(W_hh, G=None, order=None, h0=None, c0=None, bias=None, T=None):
    """The recurrence alone, as eend_lstm_f32 states it (eda_train_ref.lstm_forward) -> hT (B, H), cT (B, H), h_all (B, T, H)."""
    f = lstm_forward(W_hh, G, order, h0, c0, bias, T)
    return f["hT"], f["cT"], f["h_all"]


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def encoder(src, sd, n_heads, n_layers):
    """-> emb (B, T, D) float64 torch tensor; T the longest sequence."""
    p = {k: v.detach().cpu().double() for k, v in sd.items()}
    T = max(s.shape[0] for s in src)
    x = torch.full((len(src), T, src[0].shape[1]), -1.0, dtype=torch.float64)
    for b, s in enumerate(src):
        x[b, :s.shape[0]] = s.detach().cpu().double()
    x = _ln(x @ p["enc.encoder.weight"].T + p["enc.encoder.bias"], p["enc.encoder_norm.weight"], p["enc.encoder_norm.bias"])
    B, _, D = x.shape
    dh = D // n_heads
    for n in range(n_layers):
        q = f"enc.transformer_encoder.layers.{n}."
        qkv = x @ p[q + "self_attn.in_proj_weight"].T + p[q + "self_attn.in_proj_bias"]
        Q, K, V = (t.view(B, T, n_heads, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
        A = torch.softmax(Q @ K.transpose(-1, -2) / dh ** 0.5, dim=-1) @ V
        A = A.transpose(1, 2).reshape(B, T, D) @ p[q + "self_attn.out_proj.weight"].T + p[q + "self_attn.out_proj.bias"]
        x = _ln(x + A, p[q + "norm1.weight"], p[q + "norm1.bias"])
        F = torch.relu(x @ p[q + "linear1.weight"].T + p[q + "linear1.bias"]) @ p[q + "linear2.weight"].T + p[q + "linear2.bias"]
        x = _ln(x + F, p[q + "norm2.weight"], p[q + "norm2.bias"])
    return x


def estimate(xs, sd, max_n_speakers=MAX_N_SPEAKERS):
    """xs (B, T, D) in reading order -> attractors (B, C, D), probs (B, C), numpy float64."""
    p = {k: v.detach().cpu().double().numpy() for k, v in sd.items() if k.startswith("eda.")}
    xs = np.asarray(xs.detach().cpu().double().numpy() if isinstance(xs, torch.Tensor) else xs, dtype=np.float64)
    G = xs @ p["eda.encoder.weight_ih_l0"].T + p["eda.encoder.bias_ih_l0"] + p["eda.encoder.bias_hh_l0"]
    hT, cT, _ = lstm(p["eda.encoder.weight_hh_l0"], G)
    _, _, attractors = lstm(p["eda.decoder.weight_hh_l0"], None, None, hT, cT,
                            p["eda.decoder.bias_ih_l0"] + p["eda.decoder.bias_hh_l0"], max_n_speakers)
    probs = _sigmoid(attractors @ p["eda.counter.weight"][0] + p["eda.counter.bias"][0])
    return attractors, probs


def keep_counts(probs, n_spk=None, th=None):
    if n_spk is not None:
        return [int(n_spk)] * probs.shape[0]
    if th is None:
        raise ValueError("n_spk or th")
    out = []
    for p in probs:
        below = np.nonzero(p < th)[0]
        out.append(int(below[0]) if below.size else p.shape[0])
    return out


def test(src, ilens, sd, n_heads, n_layers, order, n_spk=None, th=None):
    """-> dict(emb (B, T, D), attractors (B, 15, D), probs (B, 15), logits (B, T, 15), counts [B], output_active [(ilen, n)])."""
    emb = encoder(src, sd, n_heads, n_layers).numpy()
    order = np.asarray(order)
    attractors, probs = estimate(emb[:, order], sd)
    logits = emb @ attractors.transpose(0, 2, 1)
    counts = keep_counts(probs, n_spk, th)
    active = [logits[b, :l, :counts[b]] for b, l in enumerate(ilens)]
    return dict(emb=emb, attractors=attractors, probs=probs, logits=logits, counts=counts, output_active=active)
