"""CPU: the chunk form of the LS-EEND retention the prefill kernel implements (tests/ls_prefill_ref.py) equals the per-frame
recurrence in float64 -- the sqrt(t0) hand-over of the old state, the inclusive causal mask, the tail chunk -- and the host
side of LsMultiStreamSession.prefill: the entries in header, bindings and build list, the argument checks that need no GPU."""
import os
import re

import numpy as np
import pytest

from tests.ls_prefill_ref import D, H, ret_chunks64, ret_per_frame64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(N, T, seed):
    """scaled as the GPU tests scale them: k arrives times dk^-0.5, the state times 0.3"""
    r = np.random.default_rng(seed)
    qkvg = r.standard_normal((N, T, 4 * D))
    qkvg[..., D:2 * D] *= 0.125
    return qkvg, r.standard_normal((N, H, 64, 64)) * 0.3


@pytest.mark.parametrize("t0", [0, 1, 63, 35999])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129])
def test_chunk_form_equals_per_frame_recurrence(t0, T):
    qkvg, kv = _inputs(2, T, seed=1000 * T + t0 % 997)
    if t0 == 0:
        kv[:] = np.nan                                                         # an empty state is not read
    want_o, want_s = ret_per_frame64(qkvg, kv, t0)
    got_o, got_s = ret_chunks64(qkvg, kv, t0)
    eo, es = np.abs(got_o - want_o).max(), np.abs(got_s - want_s).max()
    assert np.isfinite(got_o).all() and np.isfinite(got_s).all()
    assert eo < 1e-12 and es < 1e-12, (t0, T, eo, es)


def test_chunk_form_pieces_compose():
    """Two prefills in a row are one: the state handed over carries everything the second piece needs."""
    qkvg, kv = _inputs(1, 150, seed=3)
    o, s = ret_chunks64(qkvg, kv, 7)
    o1, s1 = ret_chunks64(qkvg[:, :70], kv, 7)
    o2, s2 = ret_chunks64(qkvg[:, 70:], s1, 77)
    assert np.abs(np.concatenate([o1, o2], axis=1) - o).max() < 1e-12 and np.abs(s2 - s).max() < 1e-12


def test_entries_in_header_bindings_and_build_list():
    from fs_eend_amd import build
    from fs_eend_amd import lib as L
    txt = open(os.path.join(ROOT, "include", "eend_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("eend_retention_prefill_f32", "eend_dwconv_prefill_f16"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(L.PROTOTYPES[name]) == len(m.group(1).split(",")), name
    assert "ls_prefill.hip" in build.SOURCES
    assert L.ABI_VERSION == 5


def test_workspace_size():
    from fs_eend_amd import ops
    assert ops.retention_prefill_ws(1, 4, 1) == 4 * 4096
    assert ops.retention_prefill_ws(1, 4, 64) == 4 * 4096 and ops.retention_prefill_ws(1, 4, 65) == 2 * 4 * 4096
    assert ops.retention_prefill_ws(10, 4, 1024) == 10 * 4 * 16 * 4096


@pytest.mark.parametrize("bad", [0, -1, 2.0, "8", None, True])
def test_session_validates_prefill_rows_before_touching_the_model(bad):
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.ls_multistream import LsMultiStreamSession
    with pytest.raises(EendHipError, match="prefill_rows"):
        LsMultiStreamSession(None, 2, prefill_rows=bad)
