"""CPU: the host side of the collar DER -- the two C-ABI entries are declared in include/eend_hip.h and bound in lib.py, the
ABI constant is what it was, the limits entry and the parameter domain of eend_collar_der_u64 answer without a launch, and
every argument error of fs_eend_amd.metrics is a ValueError raised before anything touches the GPU."""
import ctypes
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
    for name, nargs in (("eend_collar_der_u64", 14), ("eend_collar_der_limits", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name])
    assert "LS-EEND/metrics.py:41-108" in txt
    assert L.ABI_VERSION == 5 and re.search(r"#define\s+EEND_ABI_VERSION\s+5\b", txt)


def test_limits_and_domain(hip_lib):
    from fs_eend_amd import metrics as M
    tile, hmax = M.limits()
    assert tile >= 64 and hmax >= 512 and M.MAX_COLLAR == 2 * hmax
    assert hip_lib.eend_collar_der_limits(None, None) == EINVAL
    assert hip_lib.eend_abi_version() == 5                            # the entries are additive
    p = 64                                                            # never dereferenced: every call below is rejected
    ok = dict(ref=p, roff=p, Cr=2, hyp=p, hoff=p, Ch=3, B=1, sub=10, h=25, skip=0, counters=p, cooc=p, mapping=p)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return hip_lib.eend_collar_der_u64(a["ref"], a["roff"], a["Cr"], a["hyp"], a["hoff"], a["Ch"], a["B"], a["sub"], a["h"],
                                           a["skip"], a["counters"], a["cooc"], a["mapping"], None)

    for kw in (dict(ref=None), dict(roff=None), dict(hyp=None), dict(hoff=None), dict(counters=None), dict(cooc=None),
               dict(mapping=None), dict(Cr=0), dict(Cr=17), dict(Ch=0), dict(Ch=17), dict(B=0), dict(B=65536), dict(sub=0),
               dict(h=-1), dict(h=hmax + 1)):
        assert call(**kw) == EINVAL, kw


def act(T, C, dtype=torch.uint8):
    return torch.zeros(T, C, dtype=dtype)


BAD = [dict(collar=3), dict(collar=-2), dict(collar=2.0), dict(collar=True), dict(subsampling=0), dict(subsampling=-1),
       dict(subsampling=2.5), dict(ref=act(5, 17)), dict(hyp=act(5, 17)), dict(ref=torch.zeros(5)), dict(hyp=torch.zeros(5, 2, 1)),
       dict(ref=[act(5, 2), act(6, 2)], hyp=[act(5, 2)]), dict(ref=[], hyp=[]), dict(collar=10 ** 6)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(k) + str(i) for i, k in enumerate(BAD)])
def test_value_errors_need_no_gpu(kw, monkeypatch):
    from fs_eend_amd import metrics as M

    def no_gpu(*a, **k):
        raise AssertionError("the GPU path was reached before the argument check")

    monkeypatch.setattr(M._post, "_to_device", no_gpu)
    monkeypatch.setattr(M._lib, "load", no_gpu)
    a = dict(ref=act(50, 2), hyp=act(5, 3), collar=50, subsampling=10)
    a.update(kw)
    with pytest.raises(ValueError):
        M.collar_der_counters(a["ref"], a["hyp"], a["collar"], a["subsampling"])
    with pytest.raises(ValueError):
        M.score_predictions(a["ref"], a["hyp"], collar=a["collar"], subsampling=a["subsampling"])
    if not isinstance(a["ref"], list):
        with pytest.raises(ValueError):
            M.collar_der(a["ref"], a["hyp"], a["collar"], a["subsampling"])
        if set(kw) <= {"collar", "subsampling"}:
            with pytest.raises(ValueError):
                M.CollarDER(collar=a["collar"], subsampling=a["subsampling"])
        else:
            with pytest.raises(ValueError):
                M.CollarDER()(a["ref"], a["hyp"])
    else:
        with pytest.raises(ValueError):
            M.CollarDER().score_batch(a["ref"], a["hyp"])


def test_out_of_scope_lengths_are_refused_on_the_host():
    from fs_eend_amd import metrics as M
    big = torch.empty(0, 2).expand(0, 2)
    fake = torch.zeros(1, 2).expand(2 ** 28, 2)                       # a view: no memory behind the 2^28 rows
    with pytest.raises(ValueError, match="2\\^31"):
        M.collar_der_counters(act(5, 2), fake, 50, 10)                # Th * subsampling beyond 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        M.collar_der_counters([fake] * 9, [big] * 9, 50, 1)           # the offsets of the batch


def test_empty_metric_and_no_cpu_fallback():
    from fs_eend_amd import metrics as M
    from fs_eend_amd.lib import EendHipError
    m = M.CollarDER(collar=0, subsampling=1, skip_overlap=True)
    assert abs(m) == 0.0 and m.report()["total"] == 0 and m.report()["recordings"] == 0
    assert M.rate(0, 0) == 0.0 and M.rate(0, 3) == 1.0 and M.rate(4, 1) == 0.25
    if not torch.cuda.is_available():
        with pytest.raises(EendHipError):
            M.collar_der(act(5, 2), act(5, 2), 0, 1)                  # legal arguments: only the device is missing
