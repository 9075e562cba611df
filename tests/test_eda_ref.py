"""CPU: the float64 restatement of the offline EEND-EDA baseline (tests/eda_ref.py) against the golden vectors the reference itself
produced (tools/gen_golden_eda.py), and the host side of fs_eend_amd.eda_model: state-dict contract, `order` validation, the errors.

Bar of the restatement: every stored output within FACTOR = 4 times the reference's own fp32-vs-float64 gap for that output (stored
with the golden as max |x32 - x64| / rms(x64)).  The golden is the reference's fp32 result, the restatement is float64, so their
distance IS that gap up to the restatement's own rounding (1e-15): a factor of 1 would hold if the two float64 computations agreed to
the last bit; 4 leaves room for the gap being a maximum over a subsampled tensor here (every 16th emb row) and for libm differences.
"""
import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests import eda_ref as ER

FACTOR = 4.0
CASES = FX.list_cases("eda_")


def _rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.sqrt((want ** 2).mean()))


@pytest.fixture(scope="module")
def ref_runs():
    """eda_ref.test once per golden case, shared by the tests below."""
    out = {}
    for name in CASES:
        meta, arr = FX.load_case(name)
        m = ER.build_mirror(meta)
        src = FX.make_src(meta["lengths"], meta["in_size"], meta["xseed"])
        kw = dict(th=meta["th"]) if meta["rule"] == "th" else dict(n_spk=meta["n_spk"])
        out[name] = (meta, arr, m, ER.test(src, meta["lengths"], m.state_dict(), meta["cfg"]["n_heads"], meta["cfg"]["n_layers"],
                                           arr["order"], **kw))
    return out


def test_the_three_cases_exist():
    assert CASES == ["eda_T37", "eda_T700", "eda_ragged"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_vs_golden(ref_runs, name):
    meta, arr, _, r = ref_runs[name]
    rows = meta["rows"]
    for key, got in (("logits", r["logits"]), ("probs", r["probs"]), ("attractors", r["attractors"]), ("emb", r["emb"][:, ::rows])):
        assert got.shape == arr[key].shape
        err, bar = _rel_err(got, arr[key]), FACTOR * meta["gaps"][key]["rel"]
        print(f"{name} {key}: err {err:.2e} bar {bar:.2e}")
        assert err <= bar, f"{name} {key}: {err:.2e} > {bar:.2e}"
    assert r["counts"] == meta["counts"] == arr["counts"].tolist()
    for y, l, c in zip(r["output_active"], meta["lengths"], meta["counts"]):
        assert y.shape == (l, c)


@pytest.mark.parametrize("name", CASES)
def test_threshold_has_clearance(name):
    meta, arr = FX.load_case(name)
    assert all(1 <= c <= 14 for c in meta["counts"])
    if meta["rule"] == "th":
        assert np.abs(arr["probs"].astype(np.float64) - meta["th"]).min() > 1e-2
        assert ER.keep_counts(arr["probs"], th=meta["th"]) == meta["counts"]
    if meta["th_two"] is not None:
        assert np.abs(arr["probs"].astype(np.float64) - meta["th_two"]).min() > 1e-2
        assert ER.keep_counts(arr["probs"], th=meta["th_two"]) == meta["counts_two"] and len(set(meta["counts_two"])) > 1


def test_order_is_the_one_numpy_draws(ref_runs):
    for name, (meta, arr, _, _) in ref_runs.items():
        np.random.seed(meta["oseed"])
        order = np.arange(max(meta["lengths"]))
        np.random.shuffle(order)
        assert np.array_equal(order, arr["order"]), name


def test_count_rule():
    p = np.array([[0.9, 0.8, 0.3, 0.9], [0.9, 0.9, 0.9, 0.9], [0.1, 0.9, 0.9, 0.9]])
    assert ER.keep_counts(p, th=0.5) == [2, 4, 0]           # per sequence; all columns where no p < th
    assert ER.keep_counts(p, n_spk=3) == [3, 3, 3]
    with pytest.raises(ValueError):
        ER.keep_counts(p)


def test_state_dict_contract(ref_runs):
    """Key set = the golden's checksum keys (build_mirror has verified the checksums), shapes as the reference's modules have them."""
    meta, _, m, _ = ref_runs["eda_ragged"]
    sd = m.state_dict()
    assert set(sd) == set(meta["checksums"])
    want = {"enc.encoder.weight": (256, 345), "enc.encoder.bias": (256,), "enc.encoder_norm.weight": (256,),
            "enc.transformer_encoder.layers.1.self_attn.in_proj_weight": (768, 256),
            "enc.transformer_encoder.layers.1.linear1.weight": (2048, 256), "enc.transformer_encoder.layers.0.norm2.bias": (256,),
            "eda.encoder.weight_ih_l0": (1024, 256), "eda.encoder.weight_hh_l0": (1024, 256), "eda.encoder.bias_ih_l0": (1024,),
            "eda.encoder.bias_hh_l0": (1024,), "eda.decoder.weight_ih_l0": (1024, 256), "eda.decoder.weight_hh_l0": (1024, 256),
            "eda.decoder.bias_ih_l0": (1024,), "eda.decoder.bias_hh_l0": (1024,), "eda.counter.weight": (1, 256),
            "eda.counter.bias": (1,)}
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert len(sd) == 4 + 12 * 2 + 8 + 2
    sd2 = {k: v.clone() for k, v in sd.items()}
    m.load_state_dict(sd2)                                    # strict


def test_unsupported_sizes_raise_at_construction():
    from fs_eend_amd.eda_model import TransformerEDADiarization
    for kw in (dict(n_units=128, n_heads=4), dict(n_units=256, n_heads=8)):
        with pytest.raises(NotImplementedError):
            TransformerEDADiarization(n_speakers=None, in_size=345, n_layers=1, dropout=0.1, **kw)


def test_order_validation():
    from fs_eend_amd.eda_model import check_order
    assert check_order([2, 0, 1], 3).dtype == np.int32
    assert check_order(torch.tensor([1, 0]), 2).tolist() == [1, 0]
    for bad, T in (([0, 1], 3), ([0, 0, 1], 3), ([0, 1, 3], 3), ([-1, 0, 1], 3), ([0.0, 1.0, 2.0], 3), ([[0, 1, 2]], 3),
                   ([True, False], 2)):
        with pytest.raises(ValueError):
            check_order(bad, T)


def test_errors_before_any_device_work(ref_runs):
    from fs_eend_amd.lib import EendHipError
    meta, _, m, _ = ref_runs["eda_T37"]
    src = FX.make_src(meta["lengths"], meta["in_size"], meta["xseed"])
    with pytest.raises(ValueError):
        m.test(src, meta["lengths"])                          # neither n_spk nor th
    with pytest.raises(ValueError):
        m.test(src, meta["lengths"], n_spk=2, order=[0, 1, 2])  # not a permutation of the 37 frames
    with pytest.raises(EendHipError):
        m.test(src, meta["lengths"], n_spk=2)                 # CPU tensors, CPU parameters
    with pytest.raises(EendHipError):
        m.eda.estimate(torch.zeros(1, 5, 256))
    with pytest.raises(NotImplementedError):
        m(src, None, meta["lengths"])                         # training is out of scope


def test_lstm_entry_rejects_shapes_on_the_host(hip_lib):
    """EEND_EINVAL before any launch: hidden size != 256, T < 1, B < 1, and the pointer rules."""
    L = hip_lib
    assert L.eend_lstm_ok(1, 1, 256) == 1 and L.eend_lstm_ok(64, 5000, 256) == 1
    assert L.eend_lstm_ok(1, 1, 128) == 0 and L.eend_lstm_ok(1, 0, 256) == 0 and L.eend_lstm_ok(0, 1, 256) == 0
    p = 0x1000                                                # never dereferenced: every call below is refused
    call = lambda B=1, T=1, H=256, G=p, rows=1, bias=p, W=p, h0=None, c0=None, hT=p, cT=p: \
        L.eend_lstm_f32(G, rows, None, bias, W, h0, c0, hT, cT, None, B, T, H, None)
    for kw in (dict(H=128), dict(H=512), dict(T=0), dict(B=0), dict(T=3, rows=2), dict(W=None), dict(hT=None), dict(cT=None),
               dict(G=None, bias=None), dict(h0=p), dict(c0=p)):
        assert call(**kw) == -1, kw
    assert L.eend_eda_count_f32(p, p, p, 0.5, p, None, 1, 17, None) == -1 and L.eend_eda_count_f32(p, p, p, 0.5, p, None, 0, 15, None) == -1
    assert L.eend_eda_head_f32(p, 4, p, p, 1, 5, 15, None) == -1 and L.eend_eda_head_f32(p, 8, p, p, 1, 5, 17, None) == -1
