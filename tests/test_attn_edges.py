"""GPU: every causal time-axis attention entry at its mask, tile and padding edges, against the exact constructions and the float64
reference of tests/attn_edge_ref.py (the CPU checks of tests/test_attn_edges_ref.py show that a one-key mask error fails them).

  a) staircase / reverse staircase: every row's exact answer is one value row (V[min(i + delay, kv_len - 1)], or V[0]); bar
     STAIR_BAR (the f16 rounding of |V| <= 10), a mask error costs >= 0.5;
  b) poison: key / value / x rows at or beyond kv_len, cache rows beyond t and dO rows at or beyond q_len are finite values of about
     1e3 that would win the softmax; outputs are pre-filled with NaN, so a row the kernel should have written and did not fails too;
  c) random inputs against ref_attn, per-row error (max over the row / that row's reference RMS), so an early row's error is not
     hidden under a flat absolute bar; the existing absolute bar of each form is asserted as well.

Measured worst per-row errors on random inputs (MI355X) and the bars (<= 2x the measurement): ROW_BAR below, each entry's comment
holds the measured value.
"""
import ctypes

import pytest
import torch

from tests import attn_edge_ref as R

pytestmark = pytest.mark.gpu
F16, BF16, F32, I32 = torch.float16, torch.bfloat16, torch.float32, torch.int32

# worst per-row error on the random grids below, and the bar (<= 2x the measured value)
ROW_BAR = {
    "attn_causal": 2.5e-2,      # measured 1.36e-2 (eend_attn_causal_bf16, resident and tiled)
    "packed": 3.0e-2,           # measured 1.66e-2 (eend_inproj_attn_causal_packed_f16, nseq up to 301)
    "long": 1.8e-2,             # measured 9.3e-3 (eend_inproj_attn_causal_long_f16)
    "lse": 2.5e-2,              # measured 1.36e-2 (eend_attn_causal_lse_bf16, p_drop 0 and 0.2)
    "train": 2.5e-2,            # measured 1.40e-2 (eend_inproj_attn_train_bf16, p_drop 0 and 0.2)
    "bwd": 3.5e-1,              # measured 1.76e-1 (eend_attn_causal_bwd_bf16, dQ / dK / dV, rows normalised by max(row, tensor) RMS)
    "decode": 2.8e-3,           # measured 1.42e-3 (eend_attn_decode_f16 / _dev_f16)
    "split": 2.6e-3,            # measured 1.33e-3 (eend_attn_decode_split_f16)
}
# the absolute bars of the existing tests of each form (train: test_inproj_attn_train_fused; split: the single-wave form's bar, which the
# existing split test is held to through its 2e-3 agreement with it)
ABS_BAR = {"attn_causal": 2e-2, "packed": 2e-2, "long": 2e-2, "lse": 2e-2, "train": 3e-2, "decode": 4e-3, "split": 4e-3}

TP_PACKED = list(range(64, 513, 64))
TP_LONG = [576, 1024, 1536, 2048, 3072, 4096]
DELAYS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 511, 512, 513]
KVS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]
KVS_LONG = [1, 33, 64, 129, 511, 512, 513, 1023, 1024, 1025]


def _delays(Tp, extra=()):
    return sorted({d for d in DELAYS if d <= Tp} | {Tp - 1, Tp} | set(extra))


def _kvs(Tp, long=False):
    return sorted({k for k in (KVS_LONG if long else KVS) if k <= Tp} | {Tp - 1, Tp})


def _measured(name, val):
    print(f"[measured] {name} worst per-row error {val:.3e} (bar {ROW_BAR[name]:.1e})")


@pytest.fixture(scope="module")
def T(hip_lib, dev):
    from fs_eend_amd import train
    return train


def _keep_at(spec, nseq, H, Tp, rows, keys, dev):
    """keep bit of element ((n*H + h)*Tp + rows[i], keys[i]) -> bool (nseq, H, len(rows))"""
    from oracle import dropout_ref as DR
    a = (torch.arange(nseq, device=dev)[:, None, None] * H + torch.arange(H, device=dev)[None, :, None]) * Tp + rows[None, None, :]
    return DR.keep_mask(a.to(torch.int64), keys[None, None, :].to(torch.int64), spec[0], spec[1])


def _dspec(p_drop, Tp, site):
    from fs_eend_amd import lib as L
    if not p_drop:
        return None, None
    sp = R.drop_spec(p_drop, Tp, site)
    return sp, L.Dropout(sp[0], sp[1], sp[2])


# ------------------------------------------------------------------------------------------------ forward runners
class _HeadRows:
    """entries fed bf16 Q / K / V head rows: eend_attn_causal_bf16 (ops.attn_causal) and eend_attn_causal_lse_bf16"""

    def __init__(self, T, dev, nseq, Tp, lse=False):
        self.T, self.dev, self.nseq, self.Tp, self.lse = T, dev, nseq, Tp, lse
        self.O = torch.empty(nseq * Tp, 256, dtype=F16, device=dev)
        self.L = torch.empty(nseq * 4 * Tp, dtype=F32, device=dev)

    def set(self, Q, K, V):
        self.q, self.k = Q.to(self.dev, BF16).contiguous(), K.to(self.dev, BF16).contiguous()
        self.vt = V.to(self.dev, BF16).transpose(-1, -2).contiguous()

    def run(self, delay, kv_len, drop=None):
        from fs_eend_amd import ops
        self.O.fill_(float("nan"))
        if self.lse:
            self.L.fill_(float("nan"))
            self.T._call("eend_attn_causal_lse_bf16", self.q, self.k, self.vt, self.O, self.L, self.nseq, 4, self.Tp, 256, delay, kv_len,
                         ops.LN2, None if drop is None else ctypes.byref(drop))
        else:
            ops.attn_causal(self.q, self.k, self.vt, self.O, self.nseq, 4, self.Tp, delay, kv_len, scale=ops.LN2)
        return self.O.view(self.nseq, self.Tp, 256), self.L.view(self.nseq, 4, self.Tp)


class _Inproj:
    """entries fed f16 x and the packed in-projection: packed (Tp <= 512), long (> 512), train (<= 512, dropout, saved Q / K / V)"""

    def __init__(self, T, dev, nseq, Tp, form):
        self.T, self.dev, self.nseq, self.Tp, self.form = T, dev, nseq, Tp, form
        self.O = torch.empty(nseq * Tp, 256, dtype=F16, device=dev)
        n = nseq * Tp * 256
        self.L = torch.empty(nseq * 4 * Tp, dtype=F32, device=dev)
        self.qkv = [torch.empty(n, dtype=BF16, device=dev) for _ in range(3)]

    def set(self, x, W, b):
        from fs_eend_amd import ops
        self.x = x.to(self.dev, F16).contiguous()
        self.wp = ops.inproj_attn_pack(W.to(self.dev, F16).contiguous())
        self.b = b.to(self.dev, F32).contiguous()

    def run(self, delay, kv_len, drop=None):
        from fs_eend_amd import ops
        self.O.fill_(float("nan"))
        if self.form == "packed":
            ops.inproj_attn_causal_packed(self.x, self.wp, self.b, self.O, self.nseq, 4, self.Tp, delay, kv_len)
        elif self.form == "long":
            need = ops.inproj_attn_long_scratch(self.nseq, self.Tp, delay, kv_len)
            if need is None:
                return None, None
            part = torch.full((need[0],), float("nan"), dtype=F16, device=self.dev)
            lse = torch.full((need[1],), float("nan"), dtype=F32, device=self.dev)
            ops.inproj_attn_causal_long(self.x, self.wp, self.b, self.O, part, lse, self.nseq, 4, self.Tp, delay, kv_len)
        else:
            self.L.fill_(float("nan"))
            for t in self.qkv:
                t.fill_(float("nan"))
            self.T._call("eend_inproj_attn_train_bf16", self.x, 256, self.wp, self.b, self.O, 256, *self.qkv, self.L, self.nseq, 4, self.Tp,
                         delay, kv_len, None if drop is None else ctypes.byref(drop))
        return self.O.view(self.nseq, self.Tp, 256), self.L.view(self.nseq, 4, self.Tp)


def _stair_grid(run_form, nseq, Tp, delays, kvs, dev, spec=None, check_lse=False):
    """run one form over delays x kv_len on the staircase and the reverse staircase; returns the failing (reverse, delay, kv_len, err)"""
    bad = []
    H = 4
    for reverse in (False, True):
        for kv in kvs:
            Vd = run_form.load(reverse, kv).to(dev)             # (1, H, Tp, 64): the value rows the kernel sees
            errs, combos = [], []
            for d in delays:
                O, L = run_form.runner.run(d, kv, spec[1] if spec else None)
                if O is None:
                    continue
                last = torch.zeros(Tp, dtype=torch.long) if reverse else R.last_visible(Tp, d, kv)
                lastd = last.to(dev)
                want = Vd[:, :, lastd].expand(nseq, H, Tp, 64)
                if spec:
                    kb = _keep_at(spec[0], nseq, H, Tp, torch.arange(Tp, device=dev), lastd, dev)
                    want = want * (kb.double() * spec[0][2])[..., None]
                e = (R.rows_to_heads(O.double()) - want).abs().amax()
                if check_lse and not reverse:
                    e = torch.maximum(e, (L.double() - R.STAIR_S * lastd.double()).abs().amax() / 64)
                errs.append(e)
                combos.append(d)
            if errs:
                es = torch.stack(errs).cpu()
                for d, e in zip(combos, es.tolist()):
                    if not (e < R.STAIR_BAR):
                        bad.append((reverse, d, kv, e))
    return bad


class _StairHeads:
    def __init__(self, runner, nseq, Tp):
        self.runner, self.nseq, self.Tp = runner, nseq, Tp

    def load(self, reverse, kv):
        Q, K, V = R.stair_qkv(self.nseq, 4, self.Tp, kv, reverse=reverse)
        self.runner.set(Q, K, V)
        return V[:1]


class _StairX:
    def __init__(self, runner, nseq, Tp):
        self.runner, self.nseq, self.Tp = runner, nseq, Tp

    def load(self, reverse, kv):
        W, b = R.stair_inproj(reverse=reverse)
        x = R.stair_x(self.nseq, self.Tp, kv, reverse=reverse)
        self.runner.set(x, W, b)
        return R.inproj_heads(x[:self.Tp], W, b, 1, self.Tp)[2]


# ------------------------------------------------------------------------------------------------ a) + b): staircases
@pytest.mark.parametrize("Tp", TP_PACKED + TP_LONG)
def test_attn_causal_staircase(T, dev, Tp):
    """eend_attn_causal_bf16: resident kernel (attn_full.hip) up to 512, tiled (attn.hip) beyond"""
    nseq = 3 if Tp <= 512 else 1
    bad = _stair_grid(_StairHeads(_HeadRows(T, dev, nseq, Tp), nseq, Tp), nseq, Tp, _delays(Tp, [1 << 25]), _kvs(Tp, Tp > 512), dev)
    assert not bad, bad[:20]


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("Tp", [64, 128, 192, 256, 512, 576, 1024])
def test_attn_lse_staircase(T, dev, Tp, p_drop):
    """eend_attn_causal_lse_bf16 (training forward, two-launch form): context rows and the log2 lse (= s * last visible key), and with
    dropout every row's keep bit of its one (row, key) element"""
    nseq = 2
    spec = _dspec(p_drop, Tp, 3)
    bad = _stair_grid(_StairHeads(_HeadRows(T, dev, nseq, Tp, lse=True), nseq, Tp), nseq, Tp, _delays(Tp), _kvs(Tp, Tp > 512), dev,
                      spec if p_drop else None, check_lse=True)
    assert not bad, bad[:20]


@pytest.mark.parametrize("Tp", TP_PACKED)
def test_packed_staircase(T, dev, Tp):
    """eend_inproj_attn_causal_packed_f16 at every Tp = 64 m <= 512 (slots beyond Tp empty)"""
    nseq = 3
    bad = _stair_grid(_StairX(_Inproj(T, dev, nseq, Tp, "packed"), nseq, Tp), nseq, Tp, _delays(Tp), _kvs(Tp), dev)
    assert not bad, bad[:20]


@pytest.mark.parametrize("Tp", TP_LONG)
def test_long_staircase(T, dev, Tp):
    """eend_inproj_attn_causal_long_f16: (query group, key group) items + combine, key-group edges of kv_len, look-ahead into later
    groups cut by kv_len, the 2^24 delay clamp (delay 2^25)"""
    nseq = 1
    bad = _stair_grid(_StairX(_Inproj(T, dev, nseq, Tp, "long"), nseq, Tp), nseq, Tp, _delays(Tp, [1 << 25]), _kvs(Tp, True), dev)
    assert not bad, bad[:20]


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("Tp", TP_PACKED)
def test_train_fused_staircase(T, dev, Tp, p_drop):
    """eend_inproj_attn_train_bf16: context rows, lse, and (dropout) the keep bit of every row's one (row, key) element; the saved
    Q / K / V head rows are the exact projections, poison rows included"""
    nseq = 3
    spec = _dspec(p_drop, Tp, 2)
    st = _StairX(_Inproj(T, dev, nseq, Tp, "train"), nseq, Tp)
    bad = _stair_grid(st, nseq, Tp, _delays(Tp), _kvs(Tp), dev, spec if p_drop else None, check_lse=True)
    assert not bad, bad[:20]
    r = st.runner
    q, k, v = R.inproj_heads(r.x.double(), R.stair_inproj(reverse=True)[0].to(dev), r.b.double(), nseq, Tp)
    for got, want in zip(r.qkv, (q, k, v)):
        assert torch.equal(got.view(nseq, 4, Tp, 64).double(), want)


# ------------------------------------------------------------------------------------------------ c) random inputs
def _rand_heads(nseq, Tp, kv_len, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = (torch.randn(nseq, 4, Tp, 64, device=dev, generator=g) * R.QSCALE_LOG2).to(BF16)
    k = torch.randn(nseq, 4, Tp, 64, device=dev, generator=g).to(BF16)
    v = torch.randn(nseq, 4, Tp, 64, device=dev, generator=g).to(BF16)
    if kv_len < Tp:
        k[..., kv_len:, :] = R.POISON
        v[..., kv_len:, :] = R.poison_rows(Tp - kv_len, 64).to(dev, BF16)
    return q, k, v


def _rand_x(nseq, Tp, kv_len, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(nseq, Tp, 256, device=dev, generator=g)
    if kv_len < Tp:
        x[:, kv_len:] = R.poison_rows(Tp - kv_len, 256).to(dev, F32)
    w = torch.randn(768, 256, device=dev, generator=g) / 16
    b = torch.randn(768, device=dev, generator=g) * 0.1
    w[:256] *= R.QSCALE_LOG2
    b[:256] *= R.QSCALE_LOG2
    return x.reshape(nseq * Tp, 256).to(F16), w.to(F16), b


def _row_check(name, O, want, kv_len, worst):
    """rows < kv_len against the reference (per-row and absolute bars); every row finite"""
    got = R.rows_to_heads(O.double())
    assert torch.isfinite(got).all(), name + ": non-finite / unwritten rows"
    e = R.row_err(got[..., :kv_len, :], want[..., :kv_len, :]).max().item()
    a = (got[..., :kv_len, :] - want[..., :kv_len, :]).abs().max().item()
    worst[name] = max(worst.get(name, 0.0), e)
    assert e < ROW_BAR[name], (name, e)
    assert a < ABS_BAR[name], (name, a)


FWD_RANDOM = [(1, 64, 0, 1), (3, 128, 31, 100), (2, 192, 32, 192), (1, 320, 63, 257), (5, 448, 65, 447), (2, 512, 512, 511), (7, 512, 0, 500),
              (1, 576, 65, 576), (2, 1024, 511, 1000), (1, 2048, 0, 2047), (1, 4096, 513, 4095)]


@pytest.mark.parametrize("nseq,Tp,delay,kv_len", FWD_RANDOM)
def test_head_rows_random(T, dev, nseq, Tp, delay, kv_len):
    """eend_attn_causal_bf16 and eend_attn_causal_lse_bf16 (also with dropout) on random bf16 Q / K / V, poisoned padding keys"""
    q, k, v = _rand_heads(nseq, Tp, kv_len, Tp + delay, dev)
    worst = {}
    want, lse = R.ref_attn(q, k, v, delay, kv_len, R.LN2)
    hr = _HeadRows(T, dev, nseq, Tp)
    hr.set(q, k, v)
    O, _ = hr.run(delay, kv_len)
    _row_check("attn_causal", O, want, kv_len, worst)
    hr = _HeadRows(T, dev, nseq, Tp, lse=True)
    hr.set(q, k, v)
    for p_drop in (0.0, 0.2):
        spec = _dspec(p_drop, Tp, 3)
        keep = None if not p_drop else R.drop_keep(spec[0][0], spec[0][1], nseq, 4, Tp, device=dev)
        w = want if not p_drop else R.ref_attn(q, k, v, delay, kv_len, R.LN2, keep, spec[0][2])[0]
        O, L = hr.run(delay, kv_len, spec[1])
        _row_check("lse", O, w, kv_len, worst)
        assert (L[..., :kv_len].double() - lse[..., :kv_len]).abs().max().item() < 2e-2
    for n_, e in worst.items():
        _measured(n_, e)


@pytest.mark.parametrize("nseq,Tp,delay,kv_len", [c for c in FWD_RANDOM if c[1] <= 512] + [(300, 512, 0, 500), (301, 128, 33, 65)])
def test_packed_and_train_random(T, dev, nseq, Tp, delay, kv_len):
    """eend_inproj_attn_causal_packed_f16 and eend_inproj_attn_train_bf16 (also with dropout) against the float64 projection + attention
    of the same f16 x / W; padding x rows poisoned"""
    x, w, b = _rand_x(nseq, Tp, kv_len, nseq + Tp + delay, dev)
    worst = {}
    want, _ = R.ref_attn(*R.inproj_heads_bf16(x, w, b, nseq, Tp, key_bias=False), delay, kv_len, R.LN2)
    r = _Inproj(T, dev, nseq, Tp, "packed")
    r.set(x, w, b)
    O, _ = r.run(delay, kv_len)
    _row_check("packed", O, want, kv_len, worst)
    q, k, v = R.inproj_heads(x, w, b, nseq, Tp)
    qr, kr, vr = R.inproj_heads_bf16(x, w, b, nseq, Tp)
    want, lse = R.ref_attn(qr, kr, vr, delay, kv_len, R.LN2)
    r = _Inproj(T, dev, nseq, Tp, "train")
    r.set(x, w, b)
    for p_drop in (0.0, 0.2):
        spec = _dspec(p_drop, Tp, 2)
        keep = None if not p_drop else R.drop_keep(spec[0][0], spec[0][1], nseq, 4, Tp, device=dev)
        wnt = want if not p_drop else R.ref_attn(qr, kr, vr, delay, kv_len, R.LN2, keep, spec[0][2])[0]
        O, L = r.run(delay, kv_len, spec[1])
        _row_check("train", O, wnt, kv_len, worst)
        assert (L[..., :kv_len].double() - lse[..., :kv_len]).abs().max().item() < 3e-2
        for got, ref in zip(r.qkv, (q, k, v)):                                  # saved head rows: the bf16 rounding of the projection
            g_ = got.view(nseq, 4, Tp, 64).double()[..., :kv_len, :]
            ref = ref[..., :kv_len, :]
            assert ((g_ - ref).abs() <= ref.abs() * 2 ** -7 + 1e-2).all()
    for n_, e in worst.items():
        _measured(n_, e)


@pytest.mark.parametrize("nseq,Tp,delay,kv_len", [(2, 576, 65, 576), (2, 1024, 511, 1000), (1, 1024, 1 << 25, 513), (1, 2048, 0, 2047),
                                                  (3, 1536, 600, 700), (1, 4096, 513, 4095), (1, 3072, 1023, 1025)])
def test_long_random(T, dev, nseq, Tp, delay, kv_len):
    """eend_inproj_attn_causal_long_f16 against the float64 projection + attention"""
    x, w, b = _rand_x(nseq, Tp, kv_len, nseq + Tp + delay % 4096, dev)
    want, _ = R.ref_attn(*R.inproj_heads_bf16(x, w, b, nseq, Tp, key_bias=False), delay, kv_len, R.LN2)
    r = _Inproj(T, dev, nseq, Tp, "long")
    r.set(x, w, b)
    O, _ = r.run(delay, kv_len)
    assert O is not None
    worst = {}
    _row_check("long", O, want, kv_len, worst)
    _measured("long", worst["long"])


# ------------------------------------------------------------------------------------------------ backward
def _bwd(T, dev, q, k, v, dO, nseq, Tp, delay, kv_len, q_len, spec):
    """forward (lse entry) + eend_attn_causal_bwd_bf16, pre-scaled convention; returns (dq, dk, dv) (n, H, Tp, 64) float64"""
    from fs_eend_amd import ops
    hr = _HeadRows(T, dev, nseq, Tp, lse=True)
    hr.set(q, k, v)
    dr = None if spec is None else spec[1]
    O, L = hr.run(delay, kv_len, dr)
    qT, kT = (t.transpose(-1, -2).contiguous() for t in (hr.q, hr.k))
    dO16 = R.heads_to_rows(dO).to(BF16).contiguous().view(-1, 256)
    dot_ws = torch.empty(nseq * Tp * 256, dtype=BF16, device=dev)
    dh_ws = torch.empty(nseq * 4 * Tp, dtype=F32, device=dev)
    dqkv = torch.full((nseq * Tp, 768), float("nan"), dtype=BF16, device=dev)
    T._call("eend_attn_causal_bwd_bf16", hr.q, qT, hr.k, kT, v.to(BF16).contiguous(), dO16, 256, hr.O, 256, hr.L, dot_ws, dh_ws, dqkv, 768,
            nseq, 4, Tp, delay, kv_len, q_len, 1.0, 0.125, ops.LN2, None if dr is None else ctypes.byref(dr))
    d = dqkv.view(nseq, Tp, 3, 4, 64).double()
    return tuple(d[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _poison_dO(nseq, Tp, q_len, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    dO = torch.randn(nseq, 4, Tp, 64, device=dev, generator=g)
    if q_len < Tp:
        dO[..., q_len:, :] = R.POISON
    return dO.to(BF16).double()


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("Tp", TP_PACKED + [576, 1024, 2048])
def test_bwd_staircase(T, dev, Tp, p_drop):
    """eend_attn_causal_bwd_bf16 (fused <= 512 / two kernels beyond) on the staircase: dV_j = sum of (keep * scale *) dO_i over the rows
    i < q_len whose last visible key is j -- exactly the closed form; dQ / dK finite, padding rows of dQKV exactly zero; dO rows at or
    beyond q_len poisoned"""
    nseq = 3
    spec = _dspec(p_drop, Tp, 3)
    bad = []
    delays = sorted({d for d in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, Tp - 1, Tp) if d <= Tp})
    kvs = sorted({k for k in (1, 31, 33, 65, 129, Tp - 1, Tp) if k <= Tp})
    dO = _poison_dO(nseq, Tp, Tp, Tp, dev)
    for kv in kvs:
        Q, K, V = (t.to(dev) for t in R.stair_qkv(nseq, 4, Tp, kv))
        for q_len in sorted({kv, max(1, kv - 33), min(Tp, kv + 31)}):
            dOq = dO.clone()
            dOq[..., q_len:, :] = R.POISON
            for d in delays:
                dq, dk, dv = _bwd(T, dev, Q, K, V, dOq, nseq, Tp, d, kv, q_len, spec if p_drop else None)
                last = R.last_visible(Tp, d, kv).to(dev)
                w = dOq[..., :q_len, :]
                if p_drop:
                    kb = _keep_at(spec[0], nseq, 4, Tp, torch.arange(q_len, device=dev), last[:q_len], dev)
                    w = w * (kb.double() * spec[0][2])[..., None]
                want = torch.zeros_like(dv).index_add_(2, last[:q_len], w)
                e = ((dv - want).abs() / (want.abs() * 2 ** -7 + R.STAIR_BAR)).amax()
                fin = torch.isfinite(dq).all() & torch.isfinite(dk).all()
                z = (dq[..., q_len:, :] != 0).sum() + (dk[..., kv:, :] != 0).sum() + (dv[..., kv:, :] != 0).sum()
                bad.append((d, kv, q_len, e, fin, z))
    fails = [(d, kv, ql, e.item(), f.item(), z.item()) for d, kv, ql, e, f, z in bad if not (e.item() < 1 and f.item() and z.item() == 0)]
    assert not fails, fails[:20]


BWD_RANDOM = [(1, 64, 0, 64, 64), (3, 128, 31, 100, 90), (2, 192, 32, 192, 150), (64, 256, 0, 250, 250), (5, 320, 63, 257, 300),
              (2, 448, 64, 447, 447), (65, 512, 0, 500, 480), (2, 512, 512, 511, 511), (1, 576, 65, 576, 500), (2, 1024, 511, 1000, 1000)]


@pytest.mark.parametrize("p_drop", [0.0, 0.2])
@pytest.mark.parametrize("nseq,Tp,delay,kv_len,q_len", BWD_RANDOM)
def test_bwd_random(T, dev, nseq, Tp, delay, kv_len, q_len, p_drop):
    """dQ / dK / dV against float64 autograd with the q_len cut, dO rows at or beyond q_len poisoned, padding keys poisoned; per-row error
    relative to max(row RMS, tensor RMS): the gradient of a query with one or two visible keys is a near-cancellation (exactly 0 for one)
    with no scale of its own"""
    q, k, v = _rand_heads(nseq, Tp, kv_len, Tp * 3 + delay, dev)
    dO = _poison_dO(nseq, Tp, q_len, Tp + 1, dev)
    spec = _dspec(p_drop, Tp, 3)
    keep = None if not p_drop else R.drop_keep(spec[0][0], spec[0][1], nseq, 4, Tp, device=dev)
    qt = q.double() / R.QSCALE_LOG2                                              # the kernel's dQ is w.r.t. the un-scaled q
    ref = R.ref_attn_bwd(qt, k, v, dO, delay, kv_len, q_len, 0.125, keep, 1.0 if spec[0] is None else spec[0][2])
    got = _bwd(T, dev, q, k, v, dO, nseq, Tp, delay, kv_len, q_len, spec if p_drop else None)
    worst = 0.0
    for name, g_, r_ in zip(("dq", "dk", "dv"), got, ref):
        assert torch.isfinite(g_).all(), name
        n = q_len if name == "dq" else kv_len
        assert (g_[..., n:, :] == 0).all(), name + " pad rows"
        gv, rv = g_[..., :n, :], r_[..., :n, :]
        floor = rv.pow(2).mean().sqrt()
        e = ((gv - rv).abs().amax(-1) / rv.pow(2).mean(-1).sqrt().clamp_min(floor.item())).max().item()
        worst = max(worst, e)
        assert ((gv - rv).norm() / rv.norm()).item() < 1.5e-2, name
        assert ((gv - rv).abs().max() / rv.abs().max()).item() < 3e-2, name
        assert e < ROW_BAR["bwd"], (name, e)
    _measured("bwd", worst)


# ------------------------------------------------------------------------------------------------ decode entries
def _decode_case(N, cap, t, kind, dev, seed):
    """(qkv (N, 768) f16, K / V caches (N, 4, cap, 64) f16 with rows >= t poisoned, reference K / V rows 0..t float64)"""
    H = 4
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        kc = torch.randn(N, H, cap, 64, generator=g).double()
        vc = torch.randn(N, H, cap, 64, generator=g).double()
        qkv = torch.randn(N, 3, H, 64, generator=g).double()
        sign = 1.0
    else:
        sign = -1.0 if kind == "reverse" else 1.0
        j = torch.arange(cap)
        kc = torch.zeros(N, H, cap, 64, dtype=torch.float64)
        kc[..., 0] = (j >> 6).double()
        kc[..., 1] = (j & 63).double()
        vc = torch.stack([R.stair_values(cap, 64, 7 * h) for h in range(H)])[None].expand(N, H, cap, 64).clone()
        qkv = torch.zeros(N, 3, H, 64, dtype=torch.float64)
        qkv[:, 0, :, 0] = sign * 64 * 128.0                       # scale 1/8: 16 nats per key
        qkv[:, 0, :, 1] = sign * 128.0
        qkv[:, 1] = kc[:, :, t]
        qkv[:, 2] = vc[:, :, t]
    kref = kc[:, :, :t + 1].clone()
    vref = vc[:, :, :t + 1].clone()
    kref[:, :, t] = qkv[:, 1]
    vref[:, :, t] = qkv[:, 2]
    kc[:, :, t:, 0:2] = sign * R.POISON
    kc[:, :, t:, 2:] = R.POISON
    vc[:, :, t:] = R.poison_rows(cap - t, 64)
    return (qkv.reshape(N, 768).to(dev, F16), kc.to(dev, F16), vc.to(dev, F16), kref, vref)


@pytest.mark.parametrize("N", [1, 5])
def test_decode_edges(T, dev, N):
    """eend_attn_decode_f16 / _dev_f16 (single wave) and eend_attn_decode_split_f16 (cap 4096 / 8192) at t around 64-key chunks and
    512-key pieces: against ref_attn on the staircase (answer V[t]), the reverse staircase (V[0]) and random rows; rows beyond t of the
    cache poisoned and left untouched, row t the appended k / v; _dev bit-identical to the host-count form"""
    from fs_eend_amd import ops
    fails, worst = [], {"decode": 0.0, "split": 0.0}
    for cap in (1536, 4096, 8192):
        split = cap >= 4096
        ws = torch.empty(ops.attn_decode_split_ws(N, 4, cap), dtype=F32, device=dev) if split else None
        for t in sorted({0, 1, 31, 32, 63, 64, 511, 512, 513, 1024, cap - 1}):
            for kind in ("stair", "reverse", "random"):
                qkv, kc, vc, kref, vref = _decode_case(N, cap, t, kind, dev, cap + t)
                q = qkv.double().view(N, 3, 4, 1, 64)[:, 0]
                want, _ = R.ref_attn(q, kref.to(dev).to(F16), vref.to(dev).to(F16), t, t + 1, 0.125)
                want = want.view(N, 256)
                if kind == "stair":
                    want_x = vref[:, :, t].reshape(N, 256).to(dev)
                elif kind == "reverse":
                    want_x = vref[:, :, 0].reshape(N, 256).to(dev)
                td = torch.tensor([t], dtype=I32, device=dev)
                outs = []
                forms = ("split",) if split else ("decode", "dev")
                for form in forms:
                    k1, v1 = kc.clone(), vc.clone()
                    o = torch.full((N, 256), float("nan"), dtype=F16, device=dev)
                    if form == "decode":
                        ops.attn_decode(qkv, k1, v1, o, N, 4, cap, t)
                    elif form == "dev":
                        ops.attn_decode_dev(qkv, k1, v1, o, N, 4, cap, td)
                    else:
                        ops.attn_decode_split(qkv, k1, v1, o, ws, N, 4, cap, td)
                    outs.append(o)
                    # the append and nothing else: row t = the new k / v, every other row unchanged
                    kk, vv = kc.clone(), vc.clone()
                    kk[:, :, t] = qkv.view(N, 3, 4, 64)[:, 1]
                    vv[:, :, t] = qkv.view(N, 3, 4, 64)[:, 2]
                    if not (torch.equal(k1, kk) and torch.equal(v1, vv)):
                        fails.append((cap, t, kind, form, "cache"))
                    od = o.double()
                    if not torch.isfinite(od).all():
                        fails.append((cap, t, kind, form, "non-finite"))
                        continue
                    name = "split" if form == "split" else "decode"
                    if kind == "random":
                        e = R.row_err(od.view(N, 4, 64), want.view(N, 4, 64)).max().item()
                        a = (od - want).abs().max().item()
                        worst[name] = max(worst[name], e)
                        if not (e < ROW_BAR[name] and a < ABS_BAR[name]):
                            fails.append((cap, t, kind, form, e, a))
                    else:
                        e = (od - want_x).abs().max().item()
                        if not e < R.STAIR_BAR:
                            fails.append((cap, t, kind, form, e))
                if len(outs) == 2 and not torch.equal(outs[0], outs[1]):
                    fails.append((cap, t, kind, "dev != host"))
    for n_, e in worst.items():
        _measured(n_, e)
    assert not fails, fails[:20]


# ------------------------------------------------------------------------------------------------ rejections
def test_out_of_envelope_shapes_are_rejected(T, dev):
    """Tp not a multiple of 64, kv_len < 1, kv_len > Tp, q_len outside 1 .. Tp, Tp > 512 on the packed / fused entries, t outside the
    cache: EendHipError, never a silent answer"""
    from fs_eend_amd import ops, lib as L
    E = L.EendHipError
    nseq, Tp = 2, 128
    big = 640
    x = torch.zeros(nseq * big, 256, dtype=F16, device=dev)
    w = torch.zeros(768, 256, dtype=F16, device=dev)
    b = torch.zeros(768, dtype=F32, device=dev)
    wp = ops.inproj_attn_pack(w)
    o = torch.zeros(nseq * big, 256, dtype=F16, device=dev)
    qkv = [torch.zeros(nseq * 4 * big * 64, dtype=BF16, device=dev) for _ in range(5)]
    lse = torch.zeros(nseq * 4 * big, dtype=F32, device=dev)
    part = torch.zeros(4 * nseq * 512 * 256, dtype=F16, device=dev)
    lse_l = torch.zeros(64 * nseq * 4 * 512, dtype=F32, device=dev)
    bad = [(Tp, 0, 0), (Tp, 0, Tp + 1), (Tp, 0, -3), (96, 0, 96), (Tp - 32, 0, 64)]
    for tp, d, kv in bad + [(576, 0, 576)]:
        with pytest.raises(E):
            ops.inproj_attn_causal_packed(x, wp, b, o, nseq, 4, tp, d, kv)
        with pytest.raises(E):
            T._call("eend_inproj_attn_train_bf16", x, 256, wp, b, o, 256, qkv[0], qkv[1], qkv[2], lse, nseq, 4, tp, d, kv, None)
    for tp, d, kv in bad:
        with pytest.raises(E):
            ops.attn_causal(qkv[0], qkv[1], qkv[2], o, nseq, 4, tp, d, kv)
        with pytest.raises(E):
            T._call("eend_attn_causal_lse_bf16", qkv[0], qkv[1], qkv[2], o, lse, nseq, 4, tp, 256, d, kv, ops.LN2, None)
    for tp, d, kv in [(512, 0, 512), (1000, 0, 1000), (1024, 0, 0), (1024, 0, 1025), (1024, 0, -1)]:
        with pytest.raises(E):
            T._call("eend_inproj_attn_causal_long_f16", x, 256, wp, b, o, part, lse_l, nseq, 4, tp, 256, d, kv)
    dot_ws = torch.zeros(nseq * big * 256, dtype=BF16, device=dev)
    dh_ws = torch.zeros(nseq * 4 * big, dtype=F32, device=dev)
    dqkv = torch.zeros(nseq * big, 768, dtype=BF16, device=dev)
    for tp, kv, ql in [(Tp, 0, Tp), (Tp, Tp + 1, Tp), (Tp, Tp, 0), (Tp, Tp, Tp + 1), (96, 96, 96), (big, big, big + 1), (big, 0, big)]:
        with pytest.raises(E):
            T._call("eend_attn_causal_bwd_bf16", qkv[0], qkv[3], qkv[1], qkv[4], qkv[2], qkv[0], 256, o, 256, lse, dot_ws, dh_ws, dqkv, 768,
                    nseq, 4, tp, 0, kv, ql, 1.0, 0.125, ops.LN2, None)
    kc = torch.zeros(1, 4, 64, 64, dtype=F16, device=dev)
    for t in (-1, 64, 65):
        with pytest.raises(E):
            ops.attn_decode(torch.zeros(1, 768, dtype=F16, device=dev), kc, kc.clone(), torch.zeros(1, 256, dtype=F16, device=dev), 1, 4, 64, t)
    torch.cuda.synchronize()
    # nothing was written by a rejected call
    assert (o == 0).all() and (dqkv == 0).all() and (lse == 0).all() and (kc == 0).all()
