"""Host-only: the entries of the n-frame LS multi-stream step are declared in the public header, exported by the library and
bound in lib.py; their argument checks return EEND_EINVAL before any launch; the session validates max_frames first."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["eend_retention_chunk_ragged_f32", "eend_dwconv_chunk_ragged_f16", "eend_window_chunk_f32", "eend_spk_attn_rows_f32"]


def test_new_entries_in_header_library_and_bindings(hip_lib):
    from fs_eend_amd import lib
    hdr = open(os.path.join(ROOT, "include", "eend_hip.h")).read()
    L = lib.load()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in lib.PROTOTYPES, name
        assert getattr(L, name) is not None, name
    assert L.eend_abi_version() == 5


def test_entries_reject_null_and_out_of_range_without_launch(hip_lib):
    from fs_eend_amd import lib
    L = lib.load()
    EINVAL = -1
    assert L.eend_retention_chunk_ragged_f32(None, None, None, None, 1, 4, None, None, 8, 4, 1e-6, None) == EINVAL
    a = 4096                                                   # a non-null address that is never dereferenced: checks come first
    assert L.eend_retention_chunk_ragged_f32(a, a, a, a, 1, 0, None, a, 8, 4, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(a, a, a, a, 1, 65, None, a, 8, 4, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(a, a, a, a, 3, 4, None, a, 8, 4, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(a, a, a, a, 1, 4, None, None, 8, 4, 1e-6, None) == EINVAL
    assert L.eend_retention_chunk_ragged_f32(a, a, a, a, 1, 64, None, a, 1 << 21, 4, 1e-6, None) == EINVAL
    assert L.eend_dwconv_chunk_ragged_f16(a, a, a, None, 4, a, a, a, a, a, 1e-5, a, 4, 256, 15, None) == EINVAL
    assert L.eend_dwconv_chunk_ragged_f16(a, a, a, a, 65, a, a, a, a, a, 1e-5, a, 4, 256, 15, None) == EINVAL
    assert L.eend_dwconv_chunk_ragged_f16(a, a, a, a, 4, a, a, a, a, a, 1e-5, a, 4, 256, 1, None) == EINVAL
    assert L.eend_window_chunk_f32(a, a, None, a, a, a, 4, 4, 19, 256, None) == EINVAL
    assert L.eend_window_chunk_f32(a, a, a, a, a, a, 4, 0, 19, 256, None) == EINVAL
    assert L.eend_window_chunk_f32(a, a, a, a, a, a, 1 << 20, 64, 19, 256, None) == EINVAL
    assert L.eend_spk_attn_rows_f32(a, None, 1, 10, 4, 0.125, None) == EINVAL
    assert L.eend_spk_attn_rows_f32(a, a, 1, 17, 4, 0.125, None) == EINVAL
    assert L.eend_spk_attn_rows_f32(a, a, 1, 10, 0, 0.125, None) == EINVAL


@pytest.mark.parametrize("bad", [0, 65, -1, 2.0, "8", True, None])
def test_session_validates_max_frames_before_touching_the_model(bad):
    from fs_eend_amd.lib import EendHipError
    from fs_eend_amd.ls_multistream import LsMultiStreamSession

    class _NoModel:                                            # any use of the model would raise AttributeError instead
        pass

    with pytest.raises(EendHipError, match="max_frames"):
        LsMultiStreamSession(_NoModel(), 4, 10, max_frames=bad)
