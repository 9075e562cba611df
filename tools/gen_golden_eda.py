"""Golden vectors of the offline EEND-EDA baseline (runs ONLY where the reference checkout exists, like oracle/gen_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_eda.py [case ...]

Imports the reference's model file by path, builds it under torch.manual_seed(seed) + oracle.fixtures.perturb_, runs `test` on
CPU fp32 and writes data only to tests/golden/eda_*.npz: the seeds and the config, the frame order the call drew, the parameter
checksums, logits for all 15 columns, probs, the 15 attractors, every 16th emb row, the kept counts, and per stored output the
reference's own fp32-vs-float64 gap (the same module after .double(), same inputs and order), as max |x32 - x64| / rms(x64).
For the `th` cases the threshold is picked here so that the kept count is between 1 and 14 and no probability lies within 1e-2
of it: a count that flips on rounding would let a test hide a wrong attractor.
"""
import copy
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import fixtures as FX

REF_MODEL = "/root/reference/FS-EEND/nnet/model/offl_tfm_enc_lstm_enc_dec.py"
ROWS = 16
IN_SIZE = 345
ONLY = set(sys.argv[1:])


def cfg(n_layers):
    return dict(n_units=256, n_heads=4, n_layers=n_layers, dropout=0.1)


CASES = [
    dict(name="eda_T37", cfg=cfg(1), lengths=[37], seed=20, pseed=33, xseed=801, oseed=901, rule="th"),
    # padding rows take part in both attention and LSTM; `th_two` is a threshold at which the two items keep different counts
    dict(name="eda_ragged", cfg=cfg(2), lengths=[130, 77], seed=21, pseed=43, xseed=802, oseed=902, rule="n_spk", n_spk=3),
    # a window of more than 512 frames: the grouped attention form
    dict(name="eda_T700", cfg=cfg(4), lengths=[700], seed=22, pseed=35, xseed=803, oseed=903, rule="th"),
]
# Under default initialisation + perturb_ the counter's 15 probabilities of a recording span about 0.01 (0.52 .. 0.53 in every one of
# 300 perturbation seeds tried), so NO threshold has 1e-2 of clearance on both sides.  The generator therefore multiplies
# eda.counter.weight by this gain after perturb_ (the tests rebuild the parameters the same way, the checksums cover the result),
# and the perturbation seeds above are ones for which a threshold with the clearance exists.
COUNTER_GAIN = 16.0


def _np(t):
    return t.detach().cpu().numpy()


def pick_th(probs, differ=False):
    """The threshold with the widest clearance from every probability among those that keep 1 .. 14 columns of every sequence
    (differ: and not the same count for all of them)."""
    best = None
    for th in np.arange(0.02, 0.981, 0.001):
        counts = []
        for p in probs:
            below = np.nonzero(p < th)[0]
            counts.append(int(below[0]) if below.size else len(p))
        if not all(1 <= c <= 14 for c in counts) or (differ and len(set(counts)) == 1):
            continue
        margin = float(np.abs(probs - th).min())
        if best is None or margin > best[1]:
            best = (float(round(th, 3)), margin, counts)
    assert best is not None and best[1] > 1e-2, f"no threshold keeps 1..14 columns with 1e-2 clearance: {best}, probs {probs}"
    return best


def draw_order(oseed, T):
    np.random.seed(oseed)
    order = np.arange(T)
    np.random.shuffle(order)
    return order


def full_outputs(m, src, order):
    """The tensors behind `test`: emb (B, T, E), attractors (B, 15, E), probs (B, 15), logits (B, T, 15)."""
    emb = m.enc(src)
    attractors, probs = m.eda.estimate(emb[:, order, :])
    logits = torch.bmm(emb, attractors.transpose(1, 2))
    return dict(emb=emb, attractors=attractors, probs=probs, logits=logits)


def main():
    spec = importlib.util.spec_from_file_location("ref_offl_eda", REF_MODEL)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for case in CASES:
        if ONLY and case["name"] not in ONLY:
            continue
        torch.manual_seed(case["seed"])
        m = ref.TransformerEDADiarization(n_speakers=None, in_size=IN_SIZE, **case["cfg"]).eval()
        FX.perturb_(m, case["pseed"])
        with torch.no_grad():
            m.eda.counter.weight.mul_(COUNTER_GAIN)
        src = FX.make_src(case["lengths"], IN_SIZE, case["xseed"])
        T = max(case["lengths"])
        order = draw_order(case["oseed"], T)
        with torch.no_grad():
            out32 = full_outputs(m, src, order)
            m64 = copy.deepcopy(m).double()
            out64 = full_outputs(m64, [s.double() for s in src], order)
        probs = _np(out32["probs"]).astype(np.float64)
        kw, th, margin = {}, None, None
        if case["rule"] == "th":
            th, margin, counts = pick_th(probs)
            kw = dict(th=th)
        else:
            counts = [case["n_spk"]] * len(src)
            kw = dict(n_spk=case["n_spk"])
        two = pick_th(probs, differ=True) if len(src) > 1 else None
        assert all(1 <= c <= 14 for c in counts)
        # the call itself, under the same numpy seed: it must draw `order` and return the slices of the tensors above
        np.random.seed(case["oseed"])
        with torch.no_grad():
            active, emb_call, attr_call = m.test(src, case["lengths"], **kw)
        assert torch.equal(emb_call, out32["emb"]) and torch.equal(attr_call, out32["attractors"][:, :-1, :])
        for b, (y, l) in enumerate(zip(active, case["lengths"])):
            assert torch.equal(y, out32["logits"][b, :l, :counts[b]]), f"{case['name']}: replaying the order does not reproduce test()"
        gaps = {}
        for k in out32:
            a, b = _np(out32[k]).astype(np.float64), _np(out64[k])
            gaps[k] = dict(max_abs=float(np.abs(a - b).max()), rms=float(np.sqrt((b ** 2).mean())),
                           rel=float(np.abs(a - b).max() / np.sqrt((b ** 2).mean())))
        arrays = dict(order=order.astype(np.int32), logits=_np(out32["logits"]), probs=_np(out32["probs"]),
                      attractors=_np(out32["attractors"]), emb=_np(out32["emb"][:, ::ROWS]), counts=np.asarray(counts, dtype=np.int32))
        meta = dict(kind="eda_test", cfg=case["cfg"], lengths=case["lengths"], seed=case["seed"], pseed=case["pseed"],
                    xseed=case["xseed"], oseed=case["oseed"], rows=ROWS, in_size=IN_SIZE, rule=case["rule"], th=th,
                    th_margin=margin, n_spk=case.get("n_spk"), counts=counts, gaps=gaps, counter_gain=COUNTER_GAIN,
                    th_two=two[0] if two else None, th_two_margin=two[1] if two else None, counts_two=two[2] if two else None,
                    checksums=FX.param_checksums(m.state_dict()), torch=torch.__version__)
        p = FX.save_case(case["name"], meta, arrays)
        print(f"{case['name']}: counts {counts} th {th} (clearance {margin}) gaps "
              + ", ".join(f"{k} {v['rel']:.2e}" for k, v in gaps.items())
              + f" -> {os.path.relpath(p)} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
