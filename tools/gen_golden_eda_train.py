"""Golden vectors of the differentiable EEND-EDA attractor path (runs ONLY where the reference checkout exists, like
tools/gen_golden_eda.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_eda_train.py [case ...]

Imports the reference's model file by path, builds its EncoderDecoderAttractor under torch.manual_seed(seed) + oracle.fixtures.perturb_
and the counter gain of the inference goldens, runs `forward(xs, n_speakers)` on CPU fp32 under autograd and writes data only to
tests/golden/edatrain_*.npz: the seeds, n_speakers, the parameter checksums, the loss, the attractors, d loss / d xs, the L2 norm
of every parameter's gradient, and for each of those the reference's own fp32-vs-float64 gap (the same module after .double(), same
inputs), as max |x32 - x64| / rms(x64).  (The names do not start with eda_: that prefix lists the inference goldens.)

The scalar that is differentiated is loss + sum(attractors * Ra) with a seeded Ra scaled by 1e-3, so that attractors beyond
n_b + 1, which the counter loss does not see, carry a gradient too, as they do through the head in training.  A case with `oseed`
feeds the reference xs[:, order] and stores d xs back in storage order, which is what `forward(xs, n_speakers, order=order)` of
fs_eend_amd.eda_model returns.
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
ONLY = set(sys.argv[1:])
COUNTER_GAIN = 16.0
RA_SCALE = 1e-3

CASES = [
    dict(name="edatrain_T37", B=1, T=37, n_speakers=[2], seed=30, pseed=53, xseed=811, rseed=821, oseed=None),
    # ragged counts, one of them zero, and a frame order
    dict(name="edatrain_B3", B=3, T=70, n_speakers=[2, 0, 3], seed=31, pseed=54, xseed=812, rseed=822, oseed=912),
]


def make_inputs(case):
    """xs (B, T, 256), Ra (B, C, 256) and the frame order (or None), from the case's seeds."""
    g = torch.Generator().manual_seed(case["xseed"])
    xs = torch.randn(case["B"], case["T"], 256, generator=g)
    g = torch.Generator().manual_seed(case["rseed"])
    Ra = RA_SCALE * torch.randn(case["B"], max(case["n_speakers"]) + 1, 256, generator=g)
    order = None
    if case["oseed"] is not None:
        order = np.random.RandomState(case["oseed"]).permutation(case["T"])
    return xs, Ra, order


def run(eda, xs, Ra, order, n_speakers):
    eda.zero_grad()
    xs = xs.clone().requires_grad_(True)
    xo = xs if order is None else xs[:, torch.as_tensor(order)]
    loss, attractors = eda(xo, n_speakers)
    (loss + (attractors * Ra).sum()).backward()
    out = dict(loss=loss.detach().reshape(1), attractors=attractors.detach(), dxs=xs.grad.detach())
    norms = {k: float(p.grad.double().norm()) for k, p in eda.named_parameters()}
    return {k: v.double().numpy() for k, v in out.items()}, norms


def main():
    spec = importlib.util.spec_from_file_location("ref_offl_eda", REF_MODEL)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for case in CASES:
        if ONLY and case["name"] not in ONLY:
            continue
        torch.manual_seed(case["seed"])
        eda = ref.EncoderDecoderAttractor(256)
        FX.perturb_(eda, case["pseed"])
        with torch.no_grad():
            eda.counter.weight.mul_(COUNTER_GAIN)
        xs, Ra, order = make_inputs(case)
        out32, norms32 = run(eda, xs, Ra, order, case["n_speakers"])
        eda64 = copy.deepcopy(eda).double()
        out64, norms64 = run(eda64, xs.double(), Ra.double(), order, case["n_speakers"])
        gaps = {}
        for k in out32:
            d, rms = np.abs(out32[k] - out64[k]).max(), np.sqrt((out64[k] ** 2).mean())
            gaps[k] = dict(max_abs=float(d), rms=float(rms), rel=float(d / rms))
        norm_gaps = {k: abs(norms32[k] - norms64[k]) / norms64[k] if norms64[k] > 0 else 0.0 for k in norms32}
        arrays = dict(loss=out32["loss"].astype(np.float32), attractors=out32["attractors"].astype(np.float32),
                      dxs=out32["dxs"].astype(np.float32))
        if order is not None:
            arrays["order"] = order.astype(np.int32)
        meta = dict(kind="eda_train", B=case["B"], T=case["T"], n_speakers=case["n_speakers"], seed=case["seed"], pseed=case["pseed"],
                    xseed=case["xseed"], rseed=case["rseed"], oseed=case["oseed"], counter_gain=COUNTER_GAIN, ra_scale=RA_SCALE,
                    gaps=gaps, grad_norms=norms32, grad_norm_gaps=norm_gaps, checksums=FX.param_checksums(eda.state_dict()),
                    torch=torch.__version__)
        p = FX.save_case(case["name"], meta, arrays)
        print(f"{case['name']}: loss {float(out32['loss'][0]):.6f} gaps " + ", ".join(f"{k} {v['rel']:.2e}" for k, v in gaps.items())
              + " norm gaps " + ", ".join(f"{k.split('.')[0][:3]}.{k.split('.')[1]} {v:.1e}" for k, v in norm_gaps.items())
              + f" -> {os.path.relpath(p)} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
