"""GPU: offline EEND-EDA inference (fs_eend_amd.eda_model) against the golden vectors the reference produced
(tools/gen_golden_eda.py; parameter checksums verified first by eda_ref.build_mirror).

Bar: every output's error, normalised by that output's RMS in the golden (max |got - golden| / rms(golden)), within 2^13 times the
golden's stored fp32-vs-float64 gap of the reference for that output -- 2^13 is the unit-roundoff ratio of the f16 operands of the
encoder's MFMA kernels to fp32, the project's conditioning rule.  The kept counts must be equal (the goldens' thresholds have 1e-2
of clearance from every probability).  (err, bar, err / bar) per case and output go to profiles/eda_parity_margins.json.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from tests import eda_ref as ER

pytestmark = pytest.mark.gpu

RATIO = 2.0 ** 13
CASES = FX.list_cases("eda_")
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eda_parity_margins.json")


def _rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got.detach().cpu().double().numpy() - want).max() / np.sqrt((want ** 2).mean()))


def _record(case, rows):
    data = {}
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            data = json.load(f)
    data[case] = rows
    with open(MARGINS, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def models(dev):
    out = {}
    for name in CASES:
        meta, arr = FX.load_case(name)
        m = ER.build_mirror(meta).to(dev)
        src = [s.to(dev) for s in FX.make_src(meta["lengths"], meta["in_size"], meta["xseed"])]
        out[name] = (meta, arr, m, src)
    return out


def _rule(meta):
    return dict(th=meta["th"]) if meta["rule"] == "th" else dict(n_spk=meta["n_spk"])


@pytest.mark.parametrize("name", CASES)
def test_test_and_estimate_vs_golden(hip_lib, dev, models, name):
    meta, arr, m, src = models[name]
    lengths, rows = meta["lengths"], meta["rows"]
    active, emb, attr14 = m.test(src, lengths, order=arr["order"], **_rule(meta))
    torch.cuda.synchronize()
    T = max(lengths)
    assert emb.shape == (len(src), T, 256) and attr14.shape == (len(src), 14, 256)
    order = torch.as_tensor(arr["order"].astype(np.int64), device=dev)
    est_attr, est_probs = m.eda.estimate(emb[:, order])
    got = dict(logits=m.last_logits, probs=m.last_probs, attractors=attr14, emb=emb[:, ::rows],
               estimate_attractors=est_attr, estimate_probs=est_probs)
    want = dict(logits=arr["logits"], probs=arr["probs"], attractors=arr["attractors"][:, :14], emb=arr["emb"],
                estimate_attractors=arr["attractors"], estimate_probs=arr["probs"])
    report, failed = {}, []
    for key in got:
        assert tuple(got[key].shape) == want[key].shape, key
        assert torch.isfinite(got[key]).all(), key
        err, bar = _rel_err(got[key], want[key]), RATIO * meta["gaps"][key.replace("estimate_", "")]["rel"]
        report[key] = dict(err=err, bar=bar, ratio=err / bar)
        print(f"{name} {key}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
        if err > bar:
            failed.append(f"{key}: {err:.3e} > {bar:.3e}")
    _record(name, report)
    assert not failed, f"{name}: " + "; ".join(failed)
    assert m.last_counts == meta["counts"]
    for b, (y, l, c) in enumerate(zip(active, lengths, meta["counts"])):
        assert y.shape == (l, c) and torch.equal(y, m.last_logits[b, :l, :c])


def test_n_spk_and_th_slicing(hip_lib, dev, models):
    meta, arr, m, src = models["eda_T37"]
    by_th = m.test(src, meta["lengths"], th=meta["th"], order=arr["order"])[0]
    logits = m.last_logits.clone()
    assert [tuple(y.shape) for y in by_th] == [(37, meta["counts"][0])]
    for n in (1, 2, 15):
        by_n = m.test(src, meta["lengths"], n_spk=n, order=arr["order"])[0]
        assert by_n[0].shape == (37, n) and torch.equal(by_n[0], logits[0, :, :n])
    # a threshold below every probability keeps all 15 columns (the reference raises there)
    assert m.test(src, meta["lengths"], th=0.0, order=arr["order"])[0][0].shape == (37, 15)
    assert m.test(src, meta["lengths"], th=1.1, order=arr["order"])[0][0].shape == (37, 0)


def test_counts_are_per_item(hip_lib, dev, models):
    """Two items whose counts differ at one threshold: each keeps the columns before its OWN first p < th (the reference would apply
    the first item's count to both)."""
    meta, arr, m, src = models["eda_ragged"]
    want = meta["counts_two"]
    assert len(set(want)) > 1
    active = m.test(src, meta["lengths"], th=meta["th_two"], order=arr["order"])[0]
    assert m.last_counts == want
    assert [tuple(y.shape) for y in active] == [(l, c) for l, c in zip(meta["lengths"], want)]
    assert ER.keep_counts(m.last_probs.cpu().numpy(), th=meta["th_two"]) == want


def test_default_order_is_numpy_s(hip_lib, dev, models):
    """order=None draws np.arange(T) + np.random.shuffle as the reference does: the golden's seed reproduces the golden's order."""
    meta, arr, m, src = models["eda_T37"]
    explicit = m.test(src, meta["lengths"], order=arr["order"], **_rule(meta))[0][0].clone()
    np.random.seed(meta["oseed"])
    a = m.test(src, meta["lengths"], **_rule(meta))[0][0].clone()
    np.random.seed(meta["oseed"])
    b = m.test(src, meta["lengths"], **_rule(meta))[0][0].clone()
    np.random.seed(meta["oseed"] + 1)
    c = m.test(src, meta["lengths"], **_rule(meta))[0][0].clone()
    assert torch.equal(a, explicit) and torch.equal(a, b) and not torch.equal(a, c)
