"""CPU: the host side of the collar DER sweep -- the two C-ABI entries are declared in include/eend_hip.h and bound in lib.py,
the ABI constant is what it was, the limits entry and the parameter domain of eend_collar_der_sweep_u64 answer without a
launch, and every argument error of the sweep's functions in fs_eend_amd.metrics is a ValueError raised before anything
touches the GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_header_declares_and_binding_carries_the_entries():
    from fs_eend_amd import lib as L
    txt = open(os.path.join(ROOT, "include", "eend_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("eend_collar_der_sweep_u64", 20), ("eend_der_sweep_limits", 4)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name])
    assert L.ABI_VERSION == 5 and re.search(r"#define\s+EEND_ABI_VERSION\s+5\b", txt)
    from fs_eend_amd import build as B
    assert "der_sweep.hip" in B.SOURCES


def test_limits_and_domain(hip_lib):
    from fs_eend_amd import metrics as M
    assert M.sweep_limits() == (16, 4, 32, 127) == (M.MAX_THRESHOLDS, M.MAX_MEDIANS, M.MAX_POINTS, M.MAX_MEDIAN)
    assert hip_lib.eend_der_sweep_limits(None, None, None, None) == EINVAL
    assert hip_lib.eend_abi_version() == 5                            # the entries are additive
    _, hmax = M.limits()
    p = 64                                                            # never dereferenced: every call below is rejected
    ok = dict(ref=p, roff=p, Cr=2, pred=p, poff=p, Ch=3, sad=None, B=1, th=p, nth=5, med=p, nmed=2, sub=10, h=25, skip=0, counters=p,
              cooc=p, mapping=p, totals=None)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return hip_lib.eend_collar_der_sweep_u64(a["ref"], a["roff"], a["Cr"], a["pred"], a["poff"], a["Ch"], a["sad"], a["B"], a["th"],
                                                 a["nth"], a["med"], a["nmed"], a["sub"], a["h"], a["skip"], a["counters"], a["cooc"],
                                                 a["mapping"], a["totals"], None)

    for kw in (dict(ref=None), dict(roff=None), dict(pred=None), dict(poff=None), dict(th=None), dict(med=None), dict(counters=None),
               dict(cooc=None), dict(mapping=None), dict(Cr=0), dict(Cr=17), dict(Ch=0), dict(Ch=17), dict(B=0), dict(B=65536),
               dict(sub=0), dict(h=-1), dict(h=hmax + 1), dict(nth=0), dict(nth=17), dict(nmed=0), dict(nmed=5), dict(nth=16, nmed=3),
               dict(nth=9, nmed=4), dict(pred=66)):
        assert call(**kw) == EINVAL, kw


def act(T, C, dtype=torch.uint8):
    return torch.zeros(T, C, dtype=dtype)


GOOD = dict(ref=act(50, 2), pred=torch.rand(5, 3), thresholds=(0.4, 0.5), medians=(1, 11), sads=None, collar=50, subsampling=10)
BAD = [dict(medians=(1, 4)), dict(medians=(0,)), dict(medians=(-3,)), dict(medians=(129,)), dict(medians=(3.0,)), dict(medians=(True,)),
       dict(medians=()), dict(thresholds=()), dict(thresholds=[0.1 * i for i in range(17)]), dict(medians=(1, 3, 5, 7, 9)),
       dict(thresholds=[0.1 * i for i in range(9)], medians=(1, 3, 5, 7)), dict(thresholds=(0.5, float("nan"))),
       dict(thresholds=(float("inf"),)), dict(thresholds=(-float("inf"), 0.5)), dict(thresholds=(1e39,)), dict(thresholds=("0.5",)),
       dict(sads=[torch.ones(4)]), dict(sads=[torch.ones(5, 2)]), dict(sads=[torch.ones(5, 1, 1)]),
       dict(ref=[act(50, 2), act(50, 2)], pred=[torch.rand(5, 3), torch.rand(5, 3)], sads=[torch.ones(5)]),
       dict(ref=[act(50, 2), act(50, 2)], pred=[torch.rand(5, 3), torch.rand(5, 3)], sads=[torch.ones(5), None]),
       dict(collar=3), dict(collar=10 ** 6), dict(subsampling=0), dict(ref=act(5, 17)), dict(pred=torch.rand(5, 17)),
       dict(pred=torch.rand(5)), dict(ref=[act(5, 2), act(6, 2)], pred=[torch.rand(5, 2)]), dict(ref=[], pred=[])]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(k) + str(i) for i, k in enumerate(BAD)])
def test_value_errors_need_no_gpu(kw, monkeypatch):
    from fs_eend_amd import metrics as M

    def no_gpu(*a, **k):
        raise AssertionError("the GPU path was reached before the argument check")

    monkeypatch.setattr(M._post, "_to_device", no_gpu)
    monkeypatch.setattr(M._lib, "load", no_gpu)
    a = dict(GOOD)
    a.update(kw)
    with pytest.raises(ValueError):
        M.sweep_counters(a["ref"], a["pred"], a["thresholds"], a["medians"], a["sads"], a["collar"], a["subsampling"])
    with pytest.raises(ValueError):
        M.sweep_predictions(a["ref"], a["pred"], a["thresholds"], a["medians"], a["sads"], a["collar"], a["subsampling"])
    with pytest.raises(ValueError):
        M.DerSweep(a["thresholds"], a["medians"], a["collar"], a["subsampling"]).add(a["ref"], a["pred"], a["sads"])
    if set(kw) <= {"thresholds", "medians", "collar", "subsampling"}:
        with pytest.raises(ValueError):
            M.DerSweep(a["thresholds"], a["medians"], a["collar"], a["subsampling"])
        with pytest.raises(ValueError):                               # the packed form checks its numbers before its tensors
            M.collar_der_sweep_packed(None, None, a["thresholds"], a["medians"], a["collar"], a["subsampling"])
    if set(kw) <= {"sads", "ref", "pred"} and "sads" in kw:
        with pytest.raises(ValueError):
            M.pack_predictions(a["pred"], a["sads"])


def test_grid_is_rounded_to_float32_once():
    from fs_eend_amd import metrics as M
    th, med = M._check_grid((0.3, 0.5, 0.7), [1, 11])
    assert th == [float(torch.tensor(v, dtype=torch.float32)) for v in (0.3, 0.5, 0.7)] and th[0] != 0.3 and th[1] == 0.5
    assert med == [1, 11]
    assert M._check_grid(0.5, 11) == ([0.5], [11])
    assert M._check_grid(torch.tensor([0.25, 0.5]), torch.tensor([3])) == ([0.25, 0.5], [3])    # CPU tensors are sequences


def test_empty_sweep_metric_and_no_cpu_fallback():
    from fs_eend_amd import metrics as M
    from fs_eend_amd.lib import EendHipError
    m = M.DerSweep((0.5, 0.25), (1, 11), collar=0, subsampling=1)
    rep = m.report()
    assert rep.recordings == 0 and len(rep.table) == 4 and rep.best == (0.5, 1, 0.0) and rep.details is None
    assert rep.table[3] == {"threshold": 0.25, "median": 11, "total": 0, "correct": 0, "confusion": 0, "false alarm": 0,
                            "missed detection": 0, "diarization error rate": 0.0}
    assert rep.rates() == [[0.0, 0.0], [0.0, 0.0]]
    if not torch.cuda.is_available():
        with pytest.raises(EendHipError):
            M.sweep_predictions(act(5, 2), torch.rand(5, 2), subsampling=1)   # legal arguments: only the device is missing
